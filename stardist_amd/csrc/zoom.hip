// zoom.hip -- scipy.ndimage.zoom(x, zoom, order=1) of a contiguous device array of rank <= 4, bit for bit (finite or not).
//
//   sd_zoom_linear_device    dst = zoom(src): one thread per output element in a grid-stride loop, arithmetic of zoom_linear.h
//
// The per-axis tables (first source index, two float64 weights per output index) are built on the host and live on the device; the
// kernel neither divides a coordinate nor rounds one.  A thread reads the 2^rank neighbours of its element -- neighbouring threads
// share most of them, so they come from cache -- and writes once.
#include "common.h"
#include "zoom_linear.h"
#include "../../include/stardist_hip.h"

namespace {

using namespace zoomlin;

enum { ZB = 256, DT_U8 = 0, DT_U16 = 1, DT_F32 = 2 };

template <typename T, int RANK, typename IDX>
__global__ void __launch_bounds__(ZB) k_zoom(const T* __restrict__ src, T* __restrict__ dst, unsigned long long total, Plan P,
                                             const int32_t* __restrict__ i0, const double* __restrict__ w0, const double* __restrict__ w1) {
  for (unsigned long long o = (unsigned long long)blockIdx.x * ZB + threadIdx.x; o < total; o += (unsigned long long)gridDim.x * ZB)
    dst[o] = zoom_element<T, RANK, IDX>(src, (IDX)o, P, i0, w0, w1);
}

int zoom_blocks(unsigned long long total) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    cus = 256;
  const unsigned long long want = (total + ZB - 1) / ZB, cap = (unsigned long long)cus * 16;
  return (int)(want < cap ? want : cap);
}

template <typename T, int RANK>
int launch(const void* src, void* dst, unsigned long long total, const Plan& P, const int32_t* i0, const double* w0, const double* w1,
           hipStream_t s) {
  const int blocks = zoom_blocks(total);
  if (total < (1ull << 32))
    hipLaunchKernelGGL((k_zoom<T, RANK, unsigned>), dim3(blocks), dim3(ZB), 0, s, (const T*)src, (T*)dst, total, P, i0, w0, w1);
  else
    hipLaunchKernelGGL((k_zoom<T, RANK, unsigned long long>), dim3(blocks), dim3(ZB), 0, s, (const T*)src, (T*)dst, total, P, i0, w0, w1);
  SD_LAUNCH_CHECK();
  return 0;
}

template <typename T>
int launch_rank(const void* src, void* dst, unsigned long long total, const Plan& P, const int32_t* i0, const double* w0,
                const double* w1, hipStream_t s) {
  switch (P.rank) {
    case 1: return launch<T, 1>(src, dst, total, P, i0, w0, w1, s);
    case 2: return launch<T, 2>(src, dst, total, P, i0, w0, w1, s);
    case 3: return launch<T, 3>(src, dst, total, P, i0, w0, w1, s);
    default: return launch<T, 4>(src, dst, total, P, i0, w0, w1, s);
  }
}

}  // namespace

extern "C" int sd_zoom_linear_device(const void* d_src, void* d_dst, int dtype, int rank, const int* h_in_shape, const int* h_out_shape,
                                     const int32_t* d_i0, const double* d_w0, const double* d_w1, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (dtype != DT_U8 && dtype != DT_U16 && dtype != DT_F32) { sd::set_error("sd_zoom_linear: dtype must be 0 (uint8), 1 (uint16) or 2 (float32)"); return -1; }
  if (rank < 1 || rank > MAX_RANK) { sd::set_error("sd_zoom_linear: need 1 <= rank <= %d", (int)MAX_RANK); return -1; }
  if (!h_in_shape || !h_out_shape) { sd::set_error("sd_zoom_linear: null shape"); return -1; }
  Plan P;
  memset(&P, 0, sizeof(P));
  P.rank = rank;
  unsigned long long total = 1;
  long long stride = 1, table = 0;
  for (int d = 0; d < rank; ++d) {
    if (h_in_shape[d] < 1 || h_out_shape[d] < 1) { sd::set_error("sd_zoom_linear: every extent must be >= 1"); return -1; }
    P.n[d] = h_in_shape[d];
    P.m[d] = h_out_shape[d];
    P.table[d] = table;
    table += P.m[d];
    total *= (unsigned long long)P.m[d];
  }
  for (int d = rank - 1; d >= 0; --d) { P.stride[d] = stride; stride *= P.n[d]; }
  if (!d_src || !d_dst || !d_i0 || !d_w0 || !d_w1) { sd::set_error("sd_zoom_linear: null pointer"); return -1; }
  if (d_src == (const void*)d_dst) { sd::set_error("sd_zoom_linear: cannot work in place"); return -1; }
  if (dtype == DT_U8) return launch_rank<uint8_t>(d_src, d_dst, total, P, d_i0, d_w0, d_w1, s);
  if (dtype == DT_U16) return launch_rank<uint16_t>(d_src, d_dst, total, P, d_i0, d_w0, d_w1, s);
  return launch_rank<float>(d_src, d_dst, total, P, d_i0, d_w0, d_w1, s);
}
