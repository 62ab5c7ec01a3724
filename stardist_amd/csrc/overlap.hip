// overlap.hip -- sparse overlap of two label images (the table behind stardist/matching.py:45-52 without the dense matrix).
//
//   sd_label_overlap_device   every pair (t, p) != (0, 0) of labels that share a pixel, with its pixel count, ascending by (t, p)
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
    const int pt = __shfl(t[3], (lane + 63) & 63), pp = __shfl(p[3], (lane + 63) & 63);
    unsigned sm = 0, em = 0;                       // run starts / run starts that are not (0, 0), bit k = pixel i0 + k
    for (int k = 0; k < 4; ++k) {
      if (k >= v) break;
      const bool st = k == 0 ? (lane == 0 || t[0] != pt || p[0] != pp) : (t[k] != t[k - 1] || p[k] != p[k - 1]);
      if (st) { sm |= 1u << k; if (t[k] != 0 || p[k] != 0) em |= 1u << k; }
      if (!WRITE) { mnA = min(mnA, t[k]); mxA = max(mxA, t[k]); mnB = min(mnB, p[k]); mxB = max(mxB, p[k]); }
    }
    if (!WRITE) { cnt += __popc(em); continue; }
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
        keys[slot] = ((unsigned long long)(unsigned)t[k] << bp) | (unsigned long long)(unsigned)p[k];
        lens[slot] = end - (i0 + k);
      }
      ++slot;
    }
  }
  if (WRITE) return;
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  mnA = wave_min(mnA); mxA = wave_max(mxA); mnB = wave_min(mnB); mxB = wave_max(mxB);
  if (lane == 0) {
    if (cnt) atomicAdd(counter, cnt);
    if (mnA <= mxA) { atomicMin(mm + 0, mnA); atomicMax(mm + 1, mxA); atomicMin(mm + 2, mnB); atomicMax(mm + 3, mxB); }
  }
}

__global__ void k_unpack(const unsigned long long* __restrict__ ckeys, const long long* __restrict__ sums, long long m, int bp,
                         long long* __restrict__ okeys, long long* __restrict__ ocounts) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const unsigned long long k = ckeys[i];
  const unsigned long long t = k >> bp, p = k & ((1ull << bp) - 1ull);
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
    hipLaunchKernelGGL(k_unpack, dim3((unsigned)((w + 255) / 256)), dim3(256), 0, s, (const unsigned long long*)k0, (const long long*)v0, w, bp,
                       (long long*)d_keys, (long long*)d_counts);
    SD_LAUNCH_CHECK();
  }
  return 0;
}
