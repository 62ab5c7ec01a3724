// overlap.hip -- sparse overlap of two label images (the table behind stardist/matching.py:45-52 without the dense matrix).
//
//   sd_label_overlap_device         every pair (t, p) != (0, 0) of labels that share a pixel, with its pixel count, ascending by (t, p)
//   sd_label_overlap_stack_device   the same list for every consecutive pair of frames of a stack, in one call (see k_stack_runs)
//
// Pass 1 reads both images once (16-byte loads), counts the runs and takes the min / max of each image.  A run is a stretch of
// consecutive pixels with the same (t, p) inside one 256-pixel chunk of a wave (64 lanes x 4 pixels); its start is found by comparing
// each pixel with its predecessor (the lane's previous pixel, or the previous lane's last one through a shuffle), its end is the next
// start of the chunk (ballot over the lanes that hold a start).  Pass 2 repeats the traversal and appends (key, length) of every run
// except (0, 0), one atomic per wave and chunk.  A radix sort of the keys (t << bits(max p) | p: only the bits the two maxima need)
// and a reduce-by-key turn the runs into the table.  All arithmetic is integer: the table does not depend on the order the runs arrive.
#include "common.h"
#include "../../include/stardist_hip.h"
#include <hipcub/hipcub.hpp>
#include <limits.h>
#include <algorithm>
#include <vector>

namespace {

enum { BLOCK = 256, CHUNK = 256, MAX_BLOCKS = 4096 };

__global__ void k_overlap_init(unsigned long long* counter, int* mm) {
  if (threadIdx.x == 0) { *counter = 0; mm[0] = INT_MAX; mm[1] = INT_MIN; mm[2] = INT_MAX; mm[3] = INT_MIN; }
}

__device__ __forceinline__ void load4(const int* __restrict__ x, long long i0, int v, bool vec, int out[4]) {
  if (vec && v == 4) {
    const int4 q = *reinterpret_cast<const int4*>(x + i0);
    out[0] = q.x; out[1] = q.y; out[2] = q.z; out[3] = q.w;
  } else {
    for (int k = 0; k < 4; ++k) out[k] = k < v ? x[i0 + k] : 0;
  }
}

__device__ __forceinline__ int wave_min(int v) { for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o)); return v; }
__device__ __forceinline__ int wave_max(int v) { for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o)); return v; }

// Run starts of one chunk of a pair of images: bit k of sm = pixel i0 + k starts a run, of em = ... a run other than (0, 0).
__device__ __forceinline__ void run_starts(const int t[4], const int p[4], int v, int lane, unsigned& sm, unsigned& em) {
  const int pt = __shfl(t[3], (lane + 63) & 63), pp = __shfl(p[3], (lane + 63) & 63);
  sm = 0; em = 0;
  for (int k = 0; k < 4; ++k) {
    if (k >= v) break;
    const bool st = k == 0 ? (lane == 0 || t[0] != pt || p[0] != pp) : (t[k] != t[k - 1] || p[k] != p[k - 1]);
    if (st) { sm |= 1u << k; if (t[k] != 0 || p[k] != 0) em |= 1u << k; }
  }
}

// Append (key, length) of the chunk's runs in em: key = prefix | t << bp | p, one atomic per wave.
__device__ __forceinline__ void append_runs(const int t[4], const int p[4], unsigned sm, unsigned em, int lane, long long i0, long long chunkEnd,
                                            unsigned long long prefix, int bp, unsigned long long* __restrict__ counter, long long cap,
                                            unsigned long long* __restrict__ keys, long long* __restrict__ lens) {
  // end of this lane's last run: the first start of the next lane that has one, else the end of the chunk
  const long long firstPos = sm ? i0 + (__ffs(sm) - 1) : 0;
  const unsigned long long has = __ballot(sm != 0);
  const unsigned long long higher = lane == 63 ? 0ull : has & (~0ull << (lane + 1));
  const int nl = higher ? __ffsll((long long)higher) - 1 : lane;
  const long long nf = __shfl(firstPos, nl);
  const long long endAfter = higher ? nf : chunkEnd;
  // exclusive prefix of the emitted runs over the wave, one atomic per wave
  const int e = __popc(em);
  int incl = e;
  for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(incl, o); if (lane >= o) incl += y; }
  const int total = __shfl(incl, 63);
  unsigned long long wbase = 0;
  if (lane == 0 && total) wbase = atomicAdd(counter, (unsigned long long)total);
  wbase = __shfl(wbase, 0);
  long long slot = (long long)wbase + (incl - e);
  for (int k = 0; k < 4; ++k) {
    if (!((em >> k) & 1u)) continue;
    const unsigned later = sm & ~((2u << k) - 1u);
    const long long end = later ? i0 + (__ffs(later) - 1) : endAfter;
    if (slot < cap) {
      keys[slot] = prefix | ((unsigned long long)(unsigned)t[k] << bp) | (unsigned long long)(unsigned)p[k];
      lens[slot] = end - (i0 + k);
    }
    ++slot;
  }
}

// WRITE = false: count runs (pixels of (0, 0) excluded) and min / max of both images.  WRITE = true: append the runs.
template <bool WRITE>
__global__ void __launch_bounds__(BLOCK) k_runs(const int* __restrict__ a, const int* __restrict__ b, long long n, long long nChunks, bool vec,
                                                int bp, unsigned long long* __restrict__ counter, int* __restrict__ mm, long long cap,
                                                unsigned long long* __restrict__ keys, long long* __restrict__ lens) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  const long long nWaves = (long long)gridDim.x * (BLOCK / 64);
  unsigned long long cnt = 0;
  int mnA = INT_MAX, mxA = INT_MIN, mnB = INT_MAX, mxB = INT_MIN;
  for (long long c = wave; c < nChunks; c += nWaves) {
    const long long base = c * CHUNK, i0 = base + lane * 4;
    const long long chunkEnd = min(base + CHUNK, n);
    const int v = (int)max(0ll, min(4ll, n - i0));
    int t[4], p[4];
    load4(a, i0, v, vec, t);
    load4(b, i0, v, vec, p);
    unsigned sm, em;                               // run starts / run starts that are not (0, 0), bit k = pixel i0 + k
    run_starts(t, p, v, lane, sm, em);
    if (!WRITE) {
      for (int k = 0; k < v; ++k) { mnA = min(mnA, t[k]); mxA = max(mxA, t[k]); mnB = min(mnB, p[k]); mxB = max(mxB, p[k]); }
      cnt += __popc(em);
      continue;
    }
    append_runs(t, p, sm, em, lane, i0, chunkEnd, 0ull, bp, counter, cap, keys, lens);
  }
  if (WRITE) return;
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  mnA = wave_min(mnA); mxA = wave_max(mxA); mnB = wave_min(mnB); mxB = wave_max(mxB);
  if (lane == 0) {
    if (cnt) atomicAdd(counter, cnt);
    if (mnA <= mxA) { atomicMin(mm + 0, mnA); atomicMax(mm + 1, mxA); atomicMin(mm + 2, mnB); atomicMax(mm + 3, mxB); }
  }
}

// ---- the stack form: the K - 1 consecutive pairs of a (K, n) stack in one traversal --------------------------------------------------
// A wave owns STACK_CHUNKS chunks (wave + i * nWaves) and walks the frames with them: the chunks of frame f stay in registers as the
// "true" side of pair f while frame f + 1 is loaded, so a pass reads every frame once (two passes: count, append).  The count pass
// also takes min / max of every frame and the number of runs of every pair; the append pass puts the pair index above the id bits.
// Where the ids are so wide that the pairs are worked off in several groups (sd_label_overlap_stack_device), the append pass runs once
// per group, and the frame two groups share -- the last of one, the first of the next -- is read by both: three reads for that frame.
enum { STACK_CHUNKS = 4 };

__global__ void k_stack_init(unsigned long long* pairRuns, int* mm, int F) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < F) { pairRuns[i] = 0; mm[2 * i] = INT_MAX; mm[2 * i + 1] = INT_MIN; }
}

template <bool WRITE>
__global__ void __launch_bounds__(BLOCK) k_stack_runs(const int* __restrict__ ys, int F, long long n, long long nChunks, long long nWaves, bool vec,
                                                      int bits, unsigned long long* __restrict__ pairRuns, int* __restrict__ mm,
                                                      unsigned long long* __restrict__ counter, long long cap,
                                                      unsigned long long* __restrict__ keys, long long* __restrict__ lens) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  if (wave >= nWaves) return;                      // whole waves leave
  long long i0[STACK_CHUNKS], chunkEnd[STACK_CHUNKS];
  int v[STACK_CHUNKS], prev[STACK_CHUNKS][4], cur[STACK_CHUNKS][4];
#pragma unroll
  for (int i = 0; i < STACK_CHUNKS; ++i) {
    const long long c = wave + i * nWaves, base = c * CHUNK;
    i0[i] = base + lane * 4;
    chunkEnd[i] = min(base + CHUNK, n);
    v[i] = c < nChunks ? (int)max(0ll, min(4ll, n - i0[i])) : 0;
  }
  for (int f = 0; f < F; ++f) {
    const int* __restrict__ y = ys + (long long)f * n;
    int mn = INT_MAX, mx = INT_MIN;
    unsigned long long cnt = 0;
#pragma unroll
    for (int i = 0; i < STACK_CHUNKS; ++i) load4(y, i0[i], v[i], vec, cur[i]);
#pragma unroll
    for (int i = 0; i < STACK_CHUNKS; ++i) {
      if (!WRITE) for (int k = 0; k < v[i]; ++k) { mn = min(mn, cur[i][k]); mx = max(mx, cur[i][k]); }
      if (f > 0) {
        unsigned sm, em;
        run_starts(prev[i], cur[i], v[i], lane, sm, em);
        if (WRITE) append_runs(prev[i], cur[i], sm, em, lane, i0[i], chunkEnd[i], (unsigned long long)(f - 1) << (2 * bits), bits, counter, cap, keys, lens);
        else cnt += __popc(em);
      }
      for (int k = 0; k < 4; ++k) prev[i][k] = cur[i][k];
    }
    if (WRITE) continue;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    mn = wave_min(mn); mx = wave_max(mx);
    if (lane == 0) {
      if (cnt) atomicAdd(pairRuns + (f - 1), cnt);
      // min / max only move one way: a stale read can only let a needless atomic through, never drop a needed one
      if (mn < __atomic_load_n(mm + 2 * f, __ATOMIC_RELAXED)) atomicMin(mm + 2 * f, mn);
      if (mx > __atomic_load_n(mm + 2 * f + 1, __ATOMIC_RELAXED)) atomicMax(mm + 2 * f + 1, mx);
    }
  }
}

// first list position of every pair of a group: off[j] = number of table entries of the pairs before j (j = 0 ... nPairs)
__global__ void k_pair_offsets(const unsigned long long* __restrict__ ckeys, const int* __restrict__ nUnique, int shift, int nPairs,
                               long long* __restrict__ off) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long m = *nUnique;
  if (i >= m) return;
  const int pr = (int)(ckeys[i] >> shift), before = i ? (int)(ckeys[i - 1] >> shift) : -1;
  for (int j = before + 1; j <= pr; ++j) off[j] = i;
  if (i == m - 1) for (int j = pr + 1; j <= nPairs; ++j) off[j] = m;
}

__global__ void k_unpack(const unsigned long long* __restrict__ ckeys, const long long* __restrict__ sums, long long m, int bt, int bp,
                         long long* __restrict__ okeys, long long* __restrict__ ocounts) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const unsigned long long k = ckeys[i];
  const unsigned long long t = (k >> bp) & ((1ull << bt) - 1ull), p = k & ((1ull << bp) - 1ull);
  okeys[i] = (long long)((t << 32) | p);
  ocounts[i] = sums[i];
}

int bits_of(int v) { return v <= 0 ? 0 : 32 - __builtin_clz((unsigned)v); }

}  // namespace

extern "C" int sd_label_overlap_device(const int32_t* d_true, const int32_t* d_pred, long long n, long long cap, int64_t* d_keys,
                                       int64_t* d_counts, long long* h_count, int32_t* h_minmax, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!h_count || !h_minmax) { sd::set_error("sd_label_overlap: h_count and h_minmax are required"); return -1; }
  *h_count = 0;
  for (int k = 0; k < 4; ++k) h_minmax[k] = 0;
  if (n <= 0) return 0;
  if (cap < 0 || (cap > 0 && (!d_keys || !d_counts))) { sd::set_error("sd_label_overlap: bad output capacity / buffers"); return -1; }
  const long long nChunks = (n + CHUNK - 1) / CHUNK;
  const int nBlocks = (int)std::min<long long>((nChunks + BLOCK / 64 - 1) / (BLOCK / 64), MAX_BLOCKS);
  const bool vec = ((uintptr_t)d_true % 16 == 0) && ((uintptr_t)d_pred % 16 == 0);
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  unsigned long long* counter = A.take_n<unsigned long long>(1);
  int* mm = A.take_n<int>(4);
  if (!counter || !mm) return -1;
  hipLaunchKernelGGL(k_overlap_init, dim3(1), dim3(64), 0, s, counter, mm);
  SD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_runs<false>, dim3(nBlocks), dim3(BLOCK), 0, s, (const int*)d_true, (const int*)d_pred, n, nChunks, vec, 0, counter, mm,
                     0ll, (unsigned long long*)nullptr, (long long*)nullptr);
  SD_LAUNCH_CHECK();
  unsigned long long runs = 0;
  SD_CHECK(hipMemcpyAsync(&runs, counter, sizeof(runs), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipMemcpyAsync(h_minmax, mm, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipStreamSynchronize(s));
  if (h_minmax[0] < 0 || h_minmax[2] < 0 || runs == 0) return 0;    // negative labels: the caller raises; no pair besides (0, 0)
  if (runs > (unsigned long long)INT_MAX) { sd::set_error("sd_label_overlap: %llu runs exceed the sort's 2^31 - 1 items", runs); return -1; }
  const int R = (int)runs;
  const int bp = bits_of(h_minmax[3]), bt = bits_of(h_minmax[1]);
  const int endBit = bt + bp;                                        // <= 62
  unsigned long long* k0 = A.take_n<unsigned long long>(R);
  unsigned long long* k1 = A.take_n<unsigned long long>(R);
  long long* v0 = A.take_n<long long>(R);
  long long* v1 = A.take_n<long long>(R);
  int* nUnique = A.take_n<int>(1);
  size_t sortBytes = 0, redBytes = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sortBytes, k0, k1, v0, v1, R, 0, endBit, s);
  (void)hipcub::DeviceReduce::ReduceByKey(nullptr, redBytes, k1, k0, v1, v0, nUnique, hipcub::Sum(), R, s);
  void* tmp = A.take(std::max(sortBytes, redBytes) + 256);
  if (!k0 || !k1 || !v0 || !v1 || !nUnique || !tmp) return -1;
  SD_CHECK(hipMemsetAsync(counter, 0, sizeof(unsigned long long), s));
  hipLaunchKernelGGL(k_runs<true>, dim3(nBlocks), dim3(BLOCK), 0, s, (const int*)d_true, (const int*)d_pred, n, nChunks, vec, bp, counter, mm,
                     (long long)R, k0, v0);
  SD_LAUNCH_CHECK();
  SD_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, sortBytes, k0, k1, v0, v1, R, 0, endBit, s));
  SD_CHECK(hipcub::DeviceReduce::ReduceByKey(tmp, redBytes, k1, k0, v1, v0, nUnique, hipcub::Sum(), R, s));
  int m = 0;
  unsigned long long written = 0;
  SD_CHECK(hipMemcpyAsync(&m, nUnique, sizeof(int), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipMemcpyAsync(&written, counter, sizeof(written), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipStreamSynchronize(s));
  if (written != runs) { sd::set_error("sd_label_overlap: the two passes found %llu and %llu runs", runs, written); return -1; }
  *h_count = m;
  const long long w = std::min<long long>(m, cap);
  if (w > 0) {
    hipLaunchKernelGGL(k_unpack, dim3((unsigned)((w + 255) / 256)), dim3(256), 0, s, (const unsigned long long*)k0, (const long long*)v0, w, bt, bp,
                       (long long*)d_keys, (long long*)d_counts);
    SD_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int sd_label_overlap_stack_device(const int32_t* d_ys, int K, long long n, long long cap, int64_t* d_keys, int64_t* d_counts,
                                             long long* h_offsets, long long* h_count, int32_t* h_minmax, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!h_count || !h_minmax || !h_offsets || K < 2) { sd::set_error("sd_label_overlap_stack: K >= 2, h_offsets, h_count and h_minmax are required"); return -1; }
  *h_count = 0;
  for (int k = 0; k < K; ++k) { h_offsets[k] = 0; h_minmax[2 * k] = h_minmax[2 * k + 1] = 0; }
  if (n <= 0) return 0;
  if (cap < 0 || (cap > 0 && (!d_keys || !d_counts))) { sd::set_error("sd_label_overlap_stack: bad output capacity / buffers"); return -1; }
  const long long nChunks = (n + CHUNK - 1) / CHUNK;
  const long long nWaves = (nChunks + STACK_CHUNKS - 1) / STACK_CHUNKS;
  const long long nBlocksLL = (nWaves + BLOCK / 64 - 1) / (BLOCK / 64);
  if (nBlocksLL > INT_MAX) { sd::set_error("sd_label_overlap_stack: frames of %lld elements are too large", n); return -1; }
  const int nBlocks = (int)nBlocksLL;
  const bool vec = ((uintptr_t)d_ys % 16 == 0) && (n % 4 == 0);        // every frame then starts on the 16-byte grid
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  unsigned long long* pairRuns = A.take_n<unsigned long long>(K);
  int* mm = A.take_n<int>(2 * (size_t)K);
  unsigned long long* counter = A.take_n<unsigned long long>(1);
  int* nUnique = A.take_n<int>(1);
  if (!pairRuns || !mm || !counter || !nUnique) return -1;
  hipLaunchKernelGGL(k_stack_init, dim3((K + 255) / 256), dim3(256), 0, s, pairRuns, mm, K);
  SD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_stack_runs<false>, dim3(nBlocks), dim3(BLOCK), 0, s, (const int*)d_ys, K, n, nChunks, nWaves, vec, 0, pairRuns, mm,
                     (unsigned long long*)nullptr, 0ll, (unsigned long long*)nullptr, (long long*)nullptr);
  SD_LAUNCH_CHECK();
  std::vector<unsigned long long> runs(K);
  SD_CHECK(hipMemcpyAsync(runs.data(), pairRuns, (size_t)K * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipMemcpyAsync(h_minmax, mm, 2 * (size_t)K * sizeof(int), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipStreamSynchronize(s));
  int maxId = 0;
  for (int k = 0; k < K; ++k) {
    if (h_minmax[2 * k] < 0) return 0;                                 // negative labels: the caller raises
    maxId = std::max(maxId, h_minmax[2 * k + 1]);
  }
  // groups of consecutive pairs whose index fits above the 2 * bits id bits of a 64-bit key, and whose runs fit one sort
  const int bits = bits_of(maxId);
  const long long maxPairs = 64 - 2 * bits >= 31 ? (long long)INT_MAX : 1ll << (64 - 2 * bits);
  std::vector<int> groupEnd;                                            // one past the last pair of every group
  unsigned long long maxR = 0;
  for (int g0 = 0; g0 < K - 1;) {
    unsigned long long R = 0;
    int g1 = g0;
    while (g1 < K - 1 && g1 - g0 < maxPairs && R + runs[g1] <= (unsigned long long)INT_MAX) R += runs[g1++];
    if (g1 == g0) { sd::set_error("sd_label_overlap_stack: %llu runs of one pair exceed the sort's 2^31 - 1 items", runs[g0]); return -1; }
    groupEnd.push_back(g1);
    maxR = std::max(maxR, R);
    g0 = g1;
  }
  unsigned long long *k0 = nullptr, *k1 = nullptr;
  long long *v0 = nullptr, *v1 = nullptr, *dOff = nullptr;
  void* tmp = nullptr;
  size_t sortBytes = 0, redBytes = 0;
  std::vector<long long> off;
  if (maxR > 0) {
    const int R = (int)maxR;
    int maxGroup = 0;
    for (size_t g = 0, g0 = 0; g < groupEnd.size(); g0 = groupEnd[g++]) maxGroup = std::max(maxGroup, groupEnd[g] - (int)g0);
    k0 = A.take_n<unsigned long long>(R);
    k1 = A.take_n<unsigned long long>(R);
    v0 = A.take_n<long long>(R);
    v1 = A.take_n<long long>(R);
    dOff = A.take_n<long long>((size_t)maxGroup + 1);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sortBytes, k0, k1, v0, v1, R, 0, 64, s);
    (void)hipcub::DeviceReduce::ReduceByKey(nullptr, redBytes, k1, k0, v1, v0, nUnique, hipcub::Sum(), R, s);
    tmp = A.take(std::max(sortBytes, redBytes) + 256);
    if (!k0 || !k1 || !v0 || !v1 || !dOff || !tmp) return -1;
    off.resize((size_t)maxGroup + 1);
  }
  long long total = 0;
  int g0 = 0;
  for (int g1 : groupEnd) {
    const int nPairs = g1 - g0;
    unsigned long long R = 0;
    for (int j = g0; j < g1; ++j) R += runs[j];
    if (R == 0) {
      for (int j = g0; j < g1; ++j) h_offsets[j] = total;
      g0 = g1;
      continue;
    }
    const int32_t* sub = d_ys + (long long)g0 * n;
    const int endBit = 2 * bits + bits_of(nPairs - 1);                 // <= 64 by the choice of maxPairs
    SD_CHECK(hipMemsetAsync(counter, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_stack_runs<true>, dim3(nBlocks), dim3(BLOCK), 0, s, (const int*)sub, nPairs + 1, n, nChunks, nWaves, vec, bits,
                       (unsigned long long*)nullptr, (int*)nullptr, counter, (long long)R, k0, v0);
    SD_LAUNCH_CHECK();
    SD_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, sortBytes, k0, k1, v0, v1, (int)R, 0, endBit, s));
    SD_CHECK(hipcub::DeviceReduce::ReduceByKey(tmp, redBytes, k1, k0, v1, v0, nUnique, hipcub::Sum(), (int)R, s));
    hipLaunchKernelGGL(k_pair_offsets, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s, (const unsigned long long*)k0, (const int*)nUnique,
                       2 * bits, nPairs, dOff);
    SD_LAUNCH_CHECK();
    int m = 0;
    unsigned long long written = 0;
    SD_CHECK(hipMemcpyAsync(&m, nUnique, sizeof(int), hipMemcpyDeviceToHost, s));
    SD_CHECK(hipMemcpyAsync(&written, counter, sizeof(written), hipMemcpyDeviceToHost, s));
    SD_CHECK(hipMemcpyAsync(off.data(), dOff, ((size_t)nPairs + 1) * sizeof(long long), hipMemcpyDeviceToHost, s));
    SD_CHECK(hipStreamSynchronize(s));
    if (written != R) { sd::set_error("sd_label_overlap_stack: the two passes found %llu and %llu runs", R, written); return -1; }
    if (m < 1 || off[nPairs] != m) { sd::set_error("sd_label_overlap_stack: inconsistent pair offsets"); return -1; }
    for (int j = 0; j < nPairs; ++j) h_offsets[g0 + j] = total + off[j];
    const long long w = std::min<long long>(m, std::max(0ll, cap - total));
    if (w > 0) {
      hipLaunchKernelGGL(k_unpack, dim3((unsigned)((w + 255) / 256)), dim3(256), 0, s, (const unsigned long long*)k0, (const long long*)v0, w, bits,
                         bits, (long long*)d_keys + total, (long long*)d_counts + total);
      SD_LAUNCH_CHECK();
    }
    total += m;
    g0 = g1;
  }
  h_offsets[K - 1] = total;
  *h_count = total;
  return 0;
}
