// nms_rounds.h -- what the greedy rounds of the 2D and the 3D NMS have in common (nms2d.hip, nms3d.hip): candidate states and wait
// markers, the small list kernels, the round's triage and list scan, and the host routine that builds the neighbour lists.  The
// dimension-specific parts stay with their file: the cell grid, k_neighbours / k_neighbours3, the emission and pair kernels and the
// tail replays.  The drivers' two event holders (Timer, sd::SideJoin) are here as well.  Everything but sd::SideJoin lives in an
// anonymous namespace: each translation unit gets its own copy with internal linkage.
#pragma once
#include "common.h"
#include <hipcub/hipcub.hpp>

namespace sd {
// A launch forked onto the helper stream (sd::side_stream()): begin() lets `side` continue behind what `s` holds now, end() marks what
// `side` holds then, and the caller's stream joins before it reads the result; the destructor waits for a launch nobody joined (an
// error return: the helper stream still writes into the arena).
struct SideJoin {
  hipEvent_t fork = nullptr, done = nullptr;
  bool pending = false;
  ~SideJoin() { if (pending) (void)hipEventSynchronize(done); if (fork) (void)hipEventDestroy(fork); if (done) (void)hipEventDestroy(done); }
  int begin(hipStream_t s, hipStream_t side) {
    if (!fork) { SD_CHECK(hipEventCreateWithFlags(&fork, hipEventDisableTiming)); SD_CHECK(hipEventCreateWithFlags(&done, hipEventDisableTiming)); }
    SD_CHECK(hipEventRecord(fork, s));
    SD_CHECK(hipStreamWaitEvent(side, fork, 0));
    return 0;
  }
  int end(hipStream_t side) { SD_CHECK(hipEventRecord(done, side)); pending = true; return 0; }
  int join(hipStream_t s) { if (pending) { SD_CHECK(hipStreamWaitEvent(s, done, 0)); pending = false; } return 0; }
};
}  // namespace sd

namespace {

// event pair around a stretch of the stream (the stage and broad-phase times of the statistics); does nothing before init()
struct Timer {
  hipEvent_t a = nullptr, b = nullptr;
  ~Timer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  int init() { SD_CHECK(hipEventCreate(&a)); SD_CHECK(hipEventCreate(&b)); return 0; }
  int start(hipStream_t s) { if (a) SD_CHECK(hipEventRecord(a, s)); return 0; }
  int stop(hipStream_t s) { if (a) SD_CHECK(hipEventRecord(b, s)); return 0; }
  int wait() { if (a) SD_CHECK(hipEventSynchronize(b)); return 0; }
  int ms(float* out) { *out = 0; if (a) SD_CHECK(hipEventElapsedTime(out, a, b)); return 0; }      // after the stream or wait() has reached stop()
};

enum { ST_UNDECIDED = 0, ST_KEPT = 1, ST_SUPPRESSED = 2 };

// waitOn[i]: the better-scored neighbour candidate i was last seen waiting for, or one of
#define WAIT_NONE (-2)   // i has no undecided better-scored neighbour
#define WAIT_SCAN (-1)   // unknown: the list scan has to look

struct NmsFlags { int use_kdtree, use_bbox, thr_nonneg; float thr, max_dist; };

__global__ void k_iota(int* a, int n) { int i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) a[i] = i; }
__global__ void k_keep(const unsigned char* __restrict__ state, unsigned char* __restrict__ keep, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keep[i] = (state[i] != ST_SUPPRESSED);
}

// exact number of list entries of the single-pass form: sum of both halves' sizes (nHigh == nullptr: the lists have no second half),
// one atomic per workgroup (one atomic per candidate on one word serialises at the L2)
__global__ void __launch_bounds__(256) k_sum_halves(const int* __restrict__ nLow, const int* __restrict__ nHigh, int N, unsigned long long* total) {
  __shared__ unsigned long long ws[4];
  unsigned long long v = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) v += (unsigned long long)(nLow[i] + (nHigh ? nHigh[i] : 0));
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(total, ws[0] + ws[1] + ws[2] + ws[3]);
}

// Round kernel A1: thread per undecided candidate, O(1): waitOn[i] is the higher-scored neighbour i was last seen waiting
// for (the neighbour kernel seeds it with the best-scored one).  Most waits persist from round to round, so only the
// candidates whose wait target has just been decided go to the list scan (A2).  Workgroups of 64..1024 threads.
// pend (may be null): pend[i] != 0 = a pair (survivor, i) is still to be evaluated (deferral queues): i cannot be promoted yet,
// and neither can anything that waits for it.
__global__ void __launch_bounds__(1024) k_round_triage(const int* __restrict__ U, int nU, const unsigned char* __restrict__ state,
                                                       const int* __restrict__ waitOn, int* __restrict__ Unext, int* __restrict__ K,
                                                       int* __restrict__ S, int* counters /*0:nUnext 1:nK 2:nS*/,
                                                       const unsigned char* __restrict__ pend) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int kind = 0, i = -1;                       // 0 drop, 1 still waiting, 2 becomes a survivor, 3 needs the list scan
  if (t < nU) {
    i = U[t];
    if (state[i] != ST_SUPPRESSED) {
      const int wo = waitOn[i];
      if (pend && pend[i]) kind = 1;
      else if (wo == WAIT_NONE) kind = 2;
      else if (wo >= 0 && state[wo] == ST_UNDECIDED) kind = 1;
      else kind = 3;
    }
  }
  // ONE atomic per list and workgroup: an atomic per wave (6 500 waves x 3 lists at 2048^2) serialises at the L2 --
  // measured 138 us for this kernel in round 1 of the 2D NMS, most of it waiting for the three counters
  __shared__ int wcnt[3][16];
  __shared__ int bbase[3];
#pragma unroll
  for (int q = 1; q <= 3; ++q) {
    const unsigned long long m = __ballot(kind == q);
    if (lane == 0) wcnt[q - 1][wave] = __popcll(m);
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    int sum = 0;
    for (int w = 0; w < nw; ++w) { const int c = wcnt[threadIdx.x][w]; wcnt[threadIdx.x][w] = sum; sum += c; }
    bbase[threadIdx.x] = sum ? atomicAdd(&counters[threadIdx.x], sum) : 0;
  }
  __syncthreads();
#pragma unroll
  for (int q = 1; q <= 3; ++q) {
    const unsigned long long m = __ballot(kind == q);
    if (kind == q) (q == 1 ? Unext : (q == 2 ? K : S))[bbase[q - 1] + wcnt[q - 1][wave] + __popcll(m & ((1ull << lane) - 1))] = i;
  }
}

// Round kernel A2: wave per candidate of the scan list (persistent grid; the list length is read on the device): is any better-scored
// neighbour still undecided?
__global__ void __launch_bounds__(256) k_round_scan(const int* __restrict__ S, const unsigned char* __restrict__ state,
                                                    const long long* __restrict__ nbrStart, const int* __restrict__ nbrLow, const int* __restrict__ nbr,
                                                    int* __restrict__ waitOn, int* __restrict__ Unext, int* __restrict__ K,
                                                    int* counters /*0:nUnext 1:nK 2:nS*/, const unsigned char* __restrict__ pend) {
  const int lane = threadIdx.x & 63;
  const int nS = counters[2];
  const int nWaves = gridDim.x * (blockDim.x >> 6);
  // a wave visits its candidates one after the other; the outcomes are collected (lane k keeps the k-th) and appended to the two
  // lists with ONE atomic per list and 64 candidates -- an atomicAdd per candidate on a single counter serialises at the L2
  // (10^5 candidates in the second round = 1 ms)
  int myI = -1, myKind = 0, nbuf = 0;
  auto flush = [&]() {
#pragma unroll
    for (int q = 1; q <= 2; ++q) {
      const unsigned long long m = __ballot(lane < nbuf && myKind == q);
      if (!m) continue;
      int base = 0;
      if (lane == 0) base = atomicAdd(&counters[q - 1], __popcll(m));
      base = __shfl(base, 0);
      if (lane < nbuf && myKind == q) (q == 1 ? Unext : K)[base + __popcll(m & ((1ull << lane) - 1))] = myI;
    }
    nbuf = 0;
  };
  // FOUR candidates per wave at a time, 16 lanes each (a list of better-scored neighbours holds ~40 entries): the kernel is a chain of
  // dependent gathers (list bounds -> neighbour -> its state), so candidates in flight are what counts
  const int sub = lane >> 4, sl = lane & 15;
  for (int w0 = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 4; w0 < nS; w0 += nWaves * 4) {
    const int w = w0 + sub;
    const bool valid = w < nS;
    const int i = valid ? S[w] : -1;
    long long t = 0, end = 0;
    if (valid) { t = nbrStart[i]; end = t + nbrLow[i]; }        // the better-scored neighbours
    int found = -1;
    while (__any(found < 0 && t < end)) {
      const long long idx = t + sl;
      int j = -1;
      if (found < 0 && idx < end) { j = nbr[idx]; if (!(j < i && state[j] == ST_UNDECIDED)) j = -1; }
      const unsigned long long m = __ballot(j >= 0);
      const unsigned int m16 = (unsigned int)(m >> (sub << 4)) & 0xffffu;
      const int src = (sub << 4) + (m16 ? __ffs((int)m16) - 1 : 0);
      const int jf = __shfl(j, src);
      if (found < 0 && m16) found = jf;
      t += 16;
    }
    if (valid && sl == 0) waitOn[i] = found >= 0 ? found : WAIT_NONE;
    // (a candidate can have become pending since the triage of this round where a deferral queue is filled between the two)
    const int kind = (found >= 0 || (valid && pend && pend[i])) ? 1 : 2;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int vi = __shfl(i, q << 4), vk = __shfl(kind, q << 4);
      if (vi >= 0) { if (lane == nbuf) { myI = vi; myKind = vk; } ++nbuf; }      // (vi is wave-uniform)
    }
    if (nbuf > 60) flush();
  }
  flush();
}

// The neighbour lists of all candidates in one array: candidate i's entries start at start[i], its low[i] better-scored neighbours
// first -- what the list scan and the tail batches look at -- then its count[i] others -- what a new survivor is paired with.
// lowOnly (2D): the caller's kernel lists the better-scored neighbours only; count[] then holds the slot capacities resp. the counting
// pass's sizes and nothing afterwards, and total counts the entries stored (half of the ordered neighbour relations).
struct NbrLists {
  int* count; int* low; long long* start;      // N + 1 entries each, allocated by the caller
  int* nbr; int* waitOn;                       // allocated here
  long long total, slotTotal;                  // list entries; entries of the slots (single-pass form)
  bool slots;                                  // the single-pass form was used: the lists lie in their slots, with gaps
  bool lowOnly;                                // set by the caller
  bool wantSlotTotal;                          // set by the caller: count[] holds the capacities and slotTotal is reported even where
                                               // the two-pass form is asked for (the statistics)
};

// Exclusive prefix sums of n int counts as 64-bit starts (tmp == nullptr: the query for the temporary bytes).  The sum itself has to run
// in 64 bits: hipcub's ExclusiveSum takes its accumulator from the INPUT's value type, so over int counts it wraps at 2^32 whatever the
// type of the outputs -- a slot total of 2^32 + x came back as x, past every range check.  Here the counts are widened on the way in and
// the initial value, which rocPRIM takes the accumulator type from, is a long long.
struct WidenCount { __host__ __device__ __forceinline__ long long operator()(const int& v) const { return (long long)v; } };
inline hipError_t exclusive_sum_i64(void* tmp, size_t& tmpBytes, const int* count, long long* start, int n, hipStream_t s) {
  hipcub::TransformInputIterator<long long, WidenCount, const int*> in(count, WidenCount());
  return hipcub::DeviceScan::ExclusiveScan(tmp, tmpBytes, in, start, hipcub::Sum(), (long long)0, n, s);
}

// Builds the lists behind the caller's cell grid.  On entry count[] holds every candidate's slot capacity, the population of the cells
// its list is built from (single-pass form or wantSlotTotal; unused otherwise).  Every total is a true 64-bit sum (exclusive_sum_i64).
//   single pass: scan the slots, write the lists into them (launch(2): better-scored neighbours from the slot's front, the others --
//                unless lowOnly -- from its back), sum the exact total on the way;
//   two passes:  count (launch(0)), scan, fill (launch(1)): every candidate test is done twice -- the form for inputs whose slots would
//                exceed 32-bit indices or do not fit the workspace (the slots can be several times the exact list size).
// launch(mode, lists) enqueues the caller's neighbour kernel; beforeLists() runs once, behind the last read-back in front of the
// kernel that writes the lists (work for a helper stream that would delay such a read-back).
// Returns 0: lists written, total known; 1: L.total entries exceed the 32-bit capacity of one call (the caller words the error);
// -1: error set.
template <class LaunchNeighbours, class BeforeLists>
int build_neighbour_lists(sd::Arena& A, hipStream_t s, int N, bool singlePass, void* scanTmp, size_t scanBytes,
                          LaunchNeighbours launch, BeforeLists beforeLists, NbrLists& L) {
  L.nbr = nullptr; L.waitOn = nullptr; L.total = 0; L.slotTotal = 0; L.slots = false;
  if (singlePass || L.wantSlotTotal) {
    SD_CHECK(exclusive_sum_i64(scanTmp, scanBytes, L.count, L.start, N + 1, s));
    SD_CHECK(hipMemcpyAsync(&L.slotTotal, L.start + N, sizeof(long long), hipMemcpyDeviceToHost, s));
    SD_CHECK(hipStreamSynchronize(s));
    L.slots = singlePass && L.slotTotal >= 0 && L.slotTotal < 0x7fffffffll;
  }
  if (L.slots) {
    L.nbr = A.take_n<int>((size_t)L.slotTotal);
    if (!L.nbr) L.slots = false;               // the slots do not fit the workspace: the exact-size lists may
  }
  if (L.slots && beforeLists()) return -1;
  if (!L.slots) {
    SD_CHECK(hipMemsetAsync(L.count, 0, (N + 1) * sizeof(int), s));
    launch(0, L);
    SD_LAUNCH_CHECK();
    SD_CHECK(exclusive_sum_i64(scanTmp, scanBytes, L.count, L.start, N + 1, s));
    SD_CHECK(hipMemcpyAsync(&L.total, L.start + N, sizeof(long long), hipMemcpyDeviceToHost, s));
    SD_CHECK(hipStreamSynchronize(s));
    if (beforeLists()) return -1;
  }
  if (L.total < 0 || L.total >= 0x7fffffffll) return 1;
  if (!L.slots) L.nbr = A.take_n<int>((size_t)L.total);
  L.waitOn = A.take_n<int>(N);
  if (!L.nbr || !L.waitOn) return -1;
  if (L.slots) {
    unsigned long long* d_total = A.take_n<unsigned long long>(1);
    if (!d_total) return -1;
    SD_CHECK(hipMemsetAsync(d_total, 0, sizeof(unsigned long long), s));
    launch(2, L);
    hipLaunchKernelGGL(k_sum_halves, dim3(sd::div_up(N, 256) < 1024 ? sd::div_up(N, 256) : 1024), dim3(256), 0, s, L.low, L.lowOnly ? (const int*)nullptr : L.count, N, d_total);
    SD_LAUNCH_CHECK();
    unsigned long long tot = 0;
    SD_CHECK(hipMemcpyAsync(&tot, d_total, sizeof(tot), hipMemcpyDeviceToHost, s));
    SD_CHECK(hipStreamSynchronize(s));
    L.total = (long long)tot;
  } else {
    launch(1, L);
    SD_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace
