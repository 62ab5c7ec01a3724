// augment.hip -- the augmentation chain of a training batch on the device (stardist_amd.augment.Compose.apply_device).
//
//   sd_augment_batch_device   out_x, out_y = FlipRot90 -> Warp -> IntensityScaleShift -> AdditiveNoise of B image / label patches
//
// The arithmetic of one output pixel is csrc/augment.h's, shared with the host harness of the tests.  ONE launch for the whole batch
// and the whole chain: a thread owns one output pixel of one sample (blockIdx.y is the sample, so its parameter row is read with
// wave-uniform loads), computes the warp coordinate once, gathers the 2^nd image corners and the one label through the flip /
// permutation index map, applies intensity and noise to the value in registers and stores both results.  Neighbouring lanes are
// neighbouring output pixels along the last axis: the stores are coalesced, the gathers of a smooth warp fall into neighbouring cache
// lines.  No atomics, no workspace, nothing read back; the result depends on the inputs alone.  A batch is a few MB, so the cost is the
// launch, not the traffic: nothing here is tiled.
#include "common.h"
#include "augment.h"
#include "stardist_hip.h"
#include <limits.h>

using namespace augment;

namespace {

template <int ND>
__global__ void __launch_bounds__(AUG_THREADS) k_augment(Plan P, const Sample* __restrict__ tab, const float* __restrict__ x,
                                                         const int32_t* __restrict__ y, const float* __restrict__ disp,
                                                         float* __restrict__ ox, int32_t* __restrict__ oy) {
  const long long pix = (long long)blockIdx.x * AUG_THREADS + threadIdx.x;
  const unsigned b = blockIdx.y;
  if (pix >= P.npix || b >= (unsigned)P.B) return;
  const long long at = (long long)b * P.npix;
  augment_pixel<ND>(P, tab[b], x + at, y + at, disp ? disp + at * P.na : nullptr, pix, ox + at, oy + at);
}

}  // namespace

extern "C" int sd_augment_batch_device(const float* d_x, const int32_t* d_y, int B, int nd, const int* h_shape, int flags, const void* h_table,
                                       const void* d_table, const float* d_disp, int n_disp, float* d_out_x, int32_t* d_out_y, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "sd_augment_batch";
  if (!d_x || !d_y || !d_out_x || !d_out_y || !h_shape || !h_table || !d_table) { sd::set_error("%s: null pointer", who); return -1; }
  if (d_x == d_out_x || d_y == d_out_y) { sd::set_error("%s: cannot work in place", who); return -1; }
  if (nd != 2 && nd != 3) { sd::set_error("%s: nd must be 2 or 3", who); return -1; }
  if (B < 1 || B > 65535) { sd::set_error("%s: need 1 <= B <= 65535", who); return -1; }
  if (flags < 0 || flags > (AUG_WARP | AUG_REFLECT | AUG_INTENSITY | AUG_NOISE)) { sd::set_error("%s: unknown flags", who); return -1; }
  if (n_disp < 0 || n_disp > nd || (n_disp > 0) != (d_disp != nullptr) || (n_disp > 0 && !(flags & AUG_WARP))) {
    sd::set_error("%s: the displacement field needs 1 .. nd components and a Warp", who);
    return -1;
  }
  Plan P;
  memset(&P, 0, sizeof(P));
  P.nd = nd; P.B = B; P.flags = flags; P.na = n_disp; P.npix = 1;
  for (int d = 0; d < nd; ++d) {
    if (h_shape[d] < 1) { sd::set_error("%s: every extent must be >= 1", who); return -1; }
    P.n[d] = h_shape[d];
    P.npix *= h_shape[d];
    if (P.npix > INT_MAX) { sd::set_error("%s: more than 2^31 - 1 pixels in a sample", who); return -1; }
  }
  if (check_table(P, (const Sample*)h_table)) { sd::set_error("%s: the index map of a sample leaves the patch", who); return -1; }
  const dim3 grid((unsigned)((P.npix + AUG_THREADS - 1) / AUG_THREADS), (unsigned)B), block(AUG_THREADS);
  if (nd == 2)
    hipLaunchKernelGGL(k_augment<2>, grid, block, 0, s, P, (const Sample*)d_table, d_x, d_y, d_disp, d_out_x, d_out_y);
  else
    hipLaunchKernelGGL(k_augment<3>, grid, block, 0, s, P, (const Sample*)d_table, d_x, d_y, d_disp, d_out_x, d_out_y);
  SD_LAUNCH_CHECK();
  return 0;
}
