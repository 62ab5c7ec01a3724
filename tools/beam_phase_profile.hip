// beam_phase_profile.hip -- where do the cycles of ONE bound-slot sweep go?  Compiles stardist_amd/csrc/clip_beam.h with BEAM_PH defined as a
// clock stamp (s_memtime): at every phase boundary of the sweep the ticks since the previous boundary are added to that phase's sum, per
// lane, in LDS behind the sweep's own state (the stamp's own LDS traffic is excluded: the clock is read again after it).  The kernel is the
// tier-1 pair probe of nms2d_full.hip (prepare both polygons, then the K = 8 sweep with 16-bit coordinates), one pair per lane, 64 lanes
// per workgroup.  Driven by tools/beam_phase_profile.py, which builds this file into tools/bin/libbeam_phase.so:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -shared  -Iinclude tools/beam_phase_profile.hip -o tools/bin/libbeam_phase.so
#include <hip/hip_runtime.h>
#include <stdint.h>

enum { PH_S = 64, PH_OFF = 40960, PH_N = 12 };                                 // lanes per workgroup; byte offset of the sums in LDS; rows (PH_N - 1: stamps taken)
__device__ __forceinline__ void beam_ph_stamp(int i) {
  extern __shared__ __attribute__((aligned(16))) char ph_lds[];
  long long* a = (long long*)(ph_lds + PH_OFF);
  const long long t = (long long)__builtin_readcyclecounter();
  const int l = (int)threadIdx.x;
  a[i * PH_S + l] += t - a[PH_N * PH_S + l];
  a[(PH_N - 1) * PH_S + l] += 1;
  a[PH_N * PH_S + l] = (long long)__builtin_readcyclecounter();
}
#define BEAM_PH(i) beam_ph_stamp(i)
#include "../stardist_amd/csrc/clip_beam.h"

static_assert(PH_N > BEAM_PH_COUNT, "one row per phase and one for the stamp count");

template <int MAXV, int K, int BIL, int BREC>
__global__ void __launch_bounds__(PH_S) k_phase(const int* __restrict__ xa, const int* __restrict__ ya, const int* __restrict__ xb, const int* __restrict__ yb,
                                                int n, int R, sdclip::PolyPrep<MAXV>* __restrict__ prepbuf, long long* __restrict__ twice,
                                                int* __restrict__ flags, long long* __restrict__ prof) {
  const int p = blockIdx.x * PH_S + threadIdx.x;
  if (p >= n) return;
  typedef sdclip::LdsStorage<PH_S> LP;
  typedef sdclip::LdsStorage16<PH_S> BP;
  static_assert(sdclip::Beam<MAXV, K, BIL, BREC, BP>::lds_bytes() <= PH_OFF && sdclip::PrepWork<LP, MAXV>::lds_bytes() <= PH_OFF, "the sums lie behind the sweep's state");
  extern __shared__ __attribute__((aligned(16))) char ph_lds[];
  long long* a = (long long*)(ph_lds + PH_OFF);
  for (int i = 0; i < PH_N; ++i) a[i * PH_S + threadIdx.x] = 0;
  const long long t0 = (long long)__builtin_readcyclecounter();
  a[PH_N * PH_S + threadIdx.x] = t0;
  sdclip::PolyPrep<MAXV>* pa = prepbuf + 2 * (size_t)p;
  sdclip::PolyPrep<MAXV>* pb = pa + 1;
  {
    sdclip::PrepWork<LP, MAXV> w;
    w.prepare(xa + (size_t)p * R, ya + (size_t)p * R, R, pa);
    w.prepare(xb + (size_t)p * R, yb + (size_t)p * R, R, pb);
  }
  BEAM_PH(BEAM_PH_PREP);
  sdclip::Beam<MAXV, K, BIL, BREC, BP> bm;
  bm.reset_state(pa, pb);
  const long long t = bm.execute();
  BEAM_PH(BEAM_PH_END);
  twice[p] = t;
  flags[p] = bm.status;
  const long long t1 = (long long)__builtin_readcyclecounter();
  for (int i = 0; i < PH_N; ++i) prof[(size_t)p * (PH_N + 1) + i] = a[i * PH_S + threadIdx.x];
  prof[(size_t)p * (PH_N + 1) + PH_N] = t1 - t0;                               // the lane's whole time, stamps included
}

// prof: n rows of PH_N + 1 ticks {phases..., stamps taken, total}; prepbuf: 2 n PolyPrep<32> records.  Returns the per-pair LDS bytes, < 0 on error.
extern "C" int beam_phase_profile(const int32_t* xa, const int32_t* ya, const int32_t* xb, const int32_t* yb, int n, int R, void* prepbuf,
                                  long long prepbuf_bytes, long long* twice, int32_t* flags, long long* prof, void* stream) {
  if (R < 3 || R > 32 || n <= 0) return -1;
  if ((long long)sizeof(sdclip::PolyPrep<32>) * 2 * n > prepbuf_bytes) return -2;
  const size_t lds = PH_OFF + (PH_N + 1) * PH_S * sizeof(long long);
  hipLaunchKernelGGL((k_phase<32, 8, 6, 4>), dim3((n + PH_S - 1) / PH_S), dim3(PH_S), lds, (hipStream_t)stream, xa, ya, xb, yb, n, R,
                     (sdclip::PolyPrep<32>*)prepbuf, twice, flags, prof);
  if (hipGetLastError() != hipSuccess) return -3;
  return (int)(sdclip::Beam<32, 8, 6, 4, sdclip::LdsStorage16<PH_S>>::lds_bytes() / PH_S);
}
extern "C" int beam_phase_rows(void) { return PH_N + 1; }
extern "C" int beam_phase_prep_bytes(void) { return (int)sizeof(sdclip::PolyPrep<32>); }
