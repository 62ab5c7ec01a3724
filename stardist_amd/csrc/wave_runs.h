// wave_runs.h -- per-label integer sums of a label image without one atomic per pixel: the lanes of a wave hold 64 consecutive pixels,
// the lanes that start a run of equal labels are found with a ballot, every lane's terms are summed towards its run's first lane by a
// segmented shuffle reduction, and that lane sends one 64-bit integer atomic per non-zero term.  Used by k_centroid_sums
// (csrc/relabel_star.hip) and by the two kernels of csrc/measure_shape.hip.
//
// The one invariant: ALL 64 lanes of the wave call runs_of() and every run_add() -- the shuffles read the other lanes -- so the loops
// around them have bounds that are the same for the whole wave, and a lane without a pixel takes part with label 0 and zero terms.
#pragma once
#include <hip/hip_runtime.h>

namespace wave_runs {

enum { WAVE = 64 };

struct Runs {
  unsigned long long heads;   // bit t: lane t starts a run (uniform over the wave)
  int end;                    // one past the last lane of this lane's run
  bool head;                  // this lane starts a run
};

// the runs of equal labels among the 64 lanes; L: this lane's label (0: background, a run like any other)
__device__ __forceinline__ Runs runs_of(int L, int lane) {
  Runs r;
  const int before = __shfl_up(L, 1);
  r.head = lane == 0 || L != before;
  r.heads = __ballot(r.head);
  const unsigned long long later = (r.heads >> lane) >> 1;              // the run starts after this lane
  r.end = later ? lane + __ffsll((long long)later) : (int)WAVE;
  return r;
}

// a wave of background only (uniform: every lane sees the same answer)
__device__ __forceinline__ bool all_background(const Runs& r, int L) { return r.heads == 1ull && L == 0; }

// one step of the segmented reduction, for the offsets o = 1, 2, 4, .. 32 in this order: v += the value of lane + o if that lane
// belongs to this lane's run.  After the six steps the run's first lane holds the run's sum.
template <typename T>
__device__ __forceinline__ void run_add(T& v, int o, int lane, const Runs& r) {
  const T other = __shfl_down(v, o);
  if (lane + o < r.end) v += other;
}

__device__ __forceinline__ void add64(long long* p, long long v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }

}  // namespace wave_runs
