// Host harness of stardist_amd/csrc/zoom_linear.h: the per-element arithmetic of csrc/zoom.hip in a plain loop over the output, with
// the plan built the way sd_zoom_linear_device builds it.  The tables arrive from the caller, as they reach the device.  Built by
// tests/test_cpu_zoom.py (g++ -ffp-contract=off, as the library is).
#include <stdint.h>
#include <string.h>
#include "../../stardist_amd/csrc/zoom_linear.h"

using namespace zoomlin;

namespace {

template <typename T, int RANK, typename IDX>
void run(const T* src, T* dst, unsigned long long total, const Plan& P, const int32_t* i0, const double* w0, const double* w1) {
  for (unsigned long long o = 0; o < total; ++o) dst[o] = zoom_element<T, RANK, IDX>(src, (IDX)o, P, i0, w0, w1);
}

template <typename T, typename IDX>
void run_rank(const T* src, T* dst, unsigned long long total, const Plan& P, const int32_t* i0, const double* w0, const double* w1) {
  switch (P.rank) {
    case 1: run<T, 1, IDX>(src, dst, total, P, i0, w0, w1); break;
    case 2: run<T, 2, IDX>(src, dst, total, P, i0, w0, w1); break;
    case 3: run<T, 3, IDX>(src, dst, total, P, i0, w0, w1); break;
    default: run<T, 4, IDX>(src, dst, total, P, i0, w0, w1); break;
  }
}

}  // namespace

extern "C" {

// dst = zoom of src; dtype 0 = uint8, 1 = uint16, 2 = float32; wide != 0: the 64-bit index arithmetic of outputs beyond 2^32 elements.
// Returns 0, or -1 for arguments sd_zoom_linear_device refuses.
int zl_zoom(const void* src, void* dst, int dtype, int rank, const int* in_shape, const int* out_shape, const int32_t* i0,
            const double* w0, const double* w1, int wide) {
  if (dtype < 0 || dtype > 2 || rank < 1 || rank > MAX_RANK) return -1;
  Plan P;
  memset(&P, 0, sizeof(P));
  P.rank = rank;
  unsigned long long total = 1;
  long long stride = 1, table = 0;
  for (int d = 0; d < rank; ++d) {
    if (in_shape[d] < 1 || out_shape[d] < 1) return -1;
    P.n[d] = in_shape[d];
    P.m[d] = out_shape[d];
    P.table[d] = table;
    table += P.m[d];
    total *= (unsigned long long)P.m[d];
  }
  for (int d = rank - 1; d >= 0; --d) { P.stride[d] = stride; stride *= P.n[d]; }
  if (wide) {
    if (dtype == 0) run_rank<uint8_t, unsigned long long>((const uint8_t*)src, (uint8_t*)dst, total, P, i0, w0, w1);
    else if (dtype == 1) run_rank<uint16_t, unsigned long long>((const uint16_t*)src, (uint16_t*)dst, total, P, i0, w0, w1);
    else run_rank<float, unsigned long long>((const float*)src, (float*)dst, total, P, i0, w0, w1);
  } else {
    if (dtype == 0) run_rank<uint8_t, unsigned>((const uint8_t*)src, (uint8_t*)dst, total, P, i0, w0, w1);
    else if (dtype == 1) run_rank<uint16_t, unsigned>((const uint16_t*)src, (uint16_t*)dst, total, P, i0, w0, w1);
    else run_rank<float, unsigned>((const float*)src, (float*)dst, total, P, i0, w0, w1);
  }
  return 0;
}

}  // extern "C"
