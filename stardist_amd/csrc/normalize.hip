// normalize.hip -- percentile normalisation of an image on the device (csbdeep.utils.normalize / normalize_mi_ma, bit for bit).
//
//   sd_percentiles_device        exact np.percentile(x, q) (method 'linear') per segment, by radix selection
//   sd_normalize_mi_ma_device    out = (float(x) - mi) / (ma - mi + eps), optionally clipped to [0, 1]
//
// Selection: every element maps to an unsigned key that sorts like its value (select_rank.h).  Each percentile needs the order
// statistics of two neighbouring ranks; every rank is a slot that carries its own key prefix.  One pass = a histogram of the current
// digit over the elements whose higher digits equal a slot's prefix (k_hist_*), then one workgroup per segment that finds, per slot, the
// bin that holds the rank and the rank's offset inside the bin (k_find).  uint8 and uint16 need one pass (256 / 65536 bins), float32
// three (11 + 11 + 10 bits).  After the last pass the prefix is the key of the order statistic; k_find interpolates as numpy does.
//
// Histograms are private to a workgroup in LDS and merged into 64-bit global counters with integer atomics: the sums do not depend on
// the order of arrival, so the result is the same from call to call.  uint16 keeps 65536 counters of 16 bits in 128 KB of LDS and
// merges them after every round of at most 65535 counted elements, so none can overflow.  Equal neighbours in a lane's 16-byte load
// are counted with one add, and a load whose elements are equal across the whole wave (saturated or empty regions) with one add per
// wave: LDS atomics on one address serialise.
//
// Interleaved segments (channels-last images, one percentile pair per channel): blockIdx.y is the segment, each segment's workgroups
// read the whole array and count their own elements only.  n_seg = 1 (the usual case) reads the image once per pass.
#include "common.h"
#include "select_rank.h"
#include "../../include/stardist_hip.h"

namespace {

using namespace selrank;
typedef unsigned long long u64;

enum { HB = 1024, MAX_Q = 3, MAX_SLOTS = 2 * MAX_Q, F32_BINS = 2048, U16_ROUND_LOADS = 7 };

struct QPlan {
  int n_q, f32;
  long long lo[MAX_Q], hi[MAX_Q];
  double t[MAX_Q];
};

// state of one segment between the passes
struct SegState {
  u64 rank[MAX_SLOTS];          // rank of the slot inside the elements that share its prefix
  unsigned prefix[MAX_SLOTS];   // key digits found so far, right-aligned
  int owner[MAX_SLOTS];         // first slot with the same prefix: the one whose histogram is filled
  int has_nan;
};

template <typename T> struct Vec;
template <> struct Vec<uint8_t> { enum { N = 16 }; };
template <> struct Vec<uint16_t> { enum { N = 8 }; };
template <> struct Vec<float> { enum { N = 4 }; };

// the elements i0 .. i0 + N - 1 of x (16 bytes when the whole vector is inside the array and x is 16-byte aligned), count valid
template <typename T>
__device__ __forceinline__ int load_vec(const T* __restrict__ x, long long i0, long long total, bool aligned, T* v) {
  enum { N = Vec<T>::N };
  if (aligned && i0 + N <= total) {
    const uint4 q = *reinterpret_cast<const uint4*>(x + i0);
    memcpy(v, &q, 16);
    return N;
  }
  int c = 0;
  for (int k = 0; k < N; ++k) {
    if (i0 + k < total) { v[k] = x[i0 + k]; c = k + 1; } else v[k] = T(0);
  }
  return c;
}

// index of the histogram whose prefix is p, MAX_SLOTS if none (the prefixes of the filled histograms are distinct)
__device__ __forceinline__ int match(const unsigned (&pre)[MAX_SLOTS], unsigned p) {
  int h = MAX_SLOTS;
#pragma unroll
  for (int j = MAX_SLOTS - 1; j >= 0; --j) if (pre[j] == p) h = j;
  return h;
}

// ---------------------------------------------------------------------------------------------------------------- histograms
// One pass over x for one segment (blockIdx.y).  BINS counters of 32 bits per filled slot in dynamic LDS (uint8: 256, float32: 2048).
// PASS 0 has one histogram and no prefix; later passes count an element in the histogram of the owner slot whose prefix it carries.
template <typename T, int DT, int PASS>
__global__ void __launch_bounds__(HB) k_hist(const T* __restrict__ x, long long total, int n_seg, bool aligned, int n_slots,
                                             SegState* __restrict__ st, u64* __restrict__ ghist) {
  enum { N = Vec<T>::N, BINS = 1 << (DT == DT_U8 ? 8 : (PASS < 2 ? 11 : 10)), GBINS = DT == DT_U8 ? 256 : F32_BINS };
  extern __shared__ unsigned lh[];
  __shared__ unsigned s_prefix[MAX_SLOTS];
  __shared__ int s_hslot[MAX_SLOTS];      // owner slots in order: histogram h belongs to slot s_hslot[h]
  __shared__ int s_nh, s_nan;
  const int seg = blockIdx.y;
  SegState* S = st + seg;
  if (threadIdx.x == 0) {
    int nh = 0;
    if (PASS == 0) { s_hslot[0] = 0; s_prefix[0] = 0; nh = 1; }
    else for (int s = 0; s < n_slots; ++s) if (S->owner[s] == s) { s_hslot[nh] = s; s_prefix[nh] = S->prefix[s]; ++nh; }
    s_nh = nh; s_nan = 0;
  }
  __syncthreads();
  const int nh = s_nh;
  for (int i = threadIdx.x; i < nh * BINS; i += HB) lh[i] = 0;
  __syncthreads();
  unsigned pre[MAX_SLOTS];                     // unused entries never match: a prefix has at most 22 bits
#pragma unroll
  for (int h = 0; h < MAX_SLOTS; ++h) pre[h] = h < nh ? s_prefix[h] : 0xffffffffu;
  bool nan_seen = false;
  const long long nvec = (total + N - 1) / N;
  // the loop runs for whole waves (a lane beyond the end loads nothing) so that the wave votes below are uniform
  for (long long base = (long long)blockIdx.x * HB + (threadIdx.x & ~63); base < nvec; base += (long long)gridDim.x * HB) {
    const long long vi = base + (threadIdx.x & 63);
    const long long i0 = vi * N;
    T v[N];
    const int c = vi < nvec ? load_vec<T>(x, i0, total, aligned, v) : 0;
    const int m0 = n_seg == 1 ? 0 : (int)(i0 % n_seg);
    // one add for a whole wave of equal elements
    if (n_seg == 1) {
      bool same = c == N;
      for (int k = 1; k < N; ++k) same = same && key_of(v[k]) == key_of(v[0]);
      const unsigned k0 = key_of(v[0]);
      same = same && k0 == (unsigned)__shfl((int)k0, 0);
      if (__all(same)) {
        if (DT == DT_F32 && PASS == 0 && k0 > 0xff800000u) nan_seen = true;   // +NaN keys; -NaN: below
        if (DT == DT_F32 && PASS == 0 && k0 < 0x007fffffu) nan_seen = true;
        if ((threadIdx.x & 63) == 0) {
          int h = 0;
          if (PASS > 0) h = match(pre, prefix_of(k0, DT, PASS));
          if (h < nh) atomicAdd(&lh[h * BINS + digit_of(k0, DT, PASS)], 64u * N);
        }
        continue;
      }
    }
    int run_h = -1; unsigned run_d = 0, run_c = 0;
    for (int k = 0; k < N; ++k) {
      if (k >= c) break;
      if (n_seg != 1 && (m0 + k) % n_seg != seg) continue;
      const unsigned key = key_of(v[k]);
      if (DT == DT_F32 && PASS == 0 && (key > 0xff800000u || key < 0x007fffffu)) nan_seen = true;
      int h = 0;
      if (PASS > 0) {
        h = match(pre, prefix_of(key, DT, PASS));
        if (h == MAX_SLOTS) continue;
      }
      const unsigned d = digit_of(key, DT, PASS);
      if (h == run_h && d == run_d) { ++run_c; continue; }
      if (run_c) atomicAdd(&lh[run_h * BINS + run_d], run_c);
      run_h = h; run_d = d; run_c = 1;
    }
    if (run_c) atomicAdd(&lh[run_h * BINS + run_d], run_c);
  }
  if (DT == DT_F32 && PASS == 0 && nan_seen) s_nan = 1;
  __syncthreads();
  for (int i = threadIdx.x; i < nh * BINS; i += HB) {
    const unsigned cnt = lh[i];
    if (cnt) atomicAdd(&ghist[((size_t)seg * MAX_SLOTS + s_hslot[i / BINS]) * GBINS + (i % BINS)], (u64)cnt);
  }
  if (DT == DT_F32 && PASS == 0 && threadIdx.x == 0 && s_nan) atomicOr(&S->has_nan, 1);
}

// uint16: 65536 counters of 16 bits, two per LDS word, merged into the global histogram after every round of U16_ROUND_LOADS loads per
// thread (7 * 1024 * 8 = 57344 <= 65535 elements: no counter can overflow, no add can carry into its neighbour).
__global__ void __launch_bounds__(HB) k_hist_u16(const uint16_t* __restrict__ x, long long total, int n_seg, bool aligned,
                                                 u64* __restrict__ ghist) {
  enum { N = 8, WORDS = 32768 };
  __shared__ unsigned lh[WORDS];
  const int seg = blockIdx.y;
  u64* gh = ghist + (size_t)seg * 65536;
  for (int i = threadIdx.x; i < WORDS; i += HB) lh[i] = 0;
  __syncthreads();
  const long long nvec = (total + N - 1) / N;
  const long long round_vecs = (long long)U16_ROUND_LOADS * HB;
  const long long n_rounds = (nvec + round_vecs - 1) / round_vecs;
  for (long long r = blockIdx.x; r < n_rounds; r += gridDim.x) {
    for (int j = 0; j < U16_ROUND_LOADS; ++j) {
      const long long vi = r * round_vecs + (long long)j * HB + threadIdx.x;    // whole waves run together: the vote below is uniform
      const long long i0 = vi * N;
      uint16_t v[N];
      const int c = vi < nvec ? load_vec<uint16_t>(x, i0, total, aligned, v) : 0;
      const int m0 = n_seg == 1 ? 0 : (int)(i0 % n_seg);
      if (n_seg == 1) {
        bool same = c == N;
        for (int k = 1; k < N; ++k) same = same && v[k] == v[0];
        same = same && (int)v[0] == __shfl((int)v[0], 0);
        if (__all(same)) {
          if ((threadIdx.x & 63) == 0) atomicAdd(&lh[v[0] >> 1], (64u * N) << ((v[0] & 1) * 16));
          continue;
        }
      }
      int run_v = -1; unsigned run_c = 0;
      for (int k = 0; k < N; ++k) {
        if (k >= c) break;
        if (n_seg != 1 && (m0 + k) % n_seg != seg) continue;
        if ((int)v[k] == run_v) { ++run_c; continue; }
        if (run_c) atomicAdd(&lh[run_v >> 1], run_c << ((run_v & 1) * 16));
        run_v = v[k]; run_c = 1;
      }
      if (run_c) atomicAdd(&lh[run_v >> 1], run_c << ((run_v & 1) * 16));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < WORDS; i += HB) {
      const unsigned w = lh[i];
      if (w) {
        if (w & 0xffffu) atomicAdd(&gh[2 * i], (u64)(w & 0xffffu));
        if (w >> 16) atomicAdd(&gh[2 * i + 1], (u64)(w >> 16));
        lh[i] = 0;
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------- rank -> bin
// One workgroup per segment.  For every slot: the bin of the owner's histogram that holds the slot's rank; prefix and rank move one
// digit down.  float32: the histograms are cleared for the next pass once they are read.  LAST: the prefixes are keys; interpolate and write.
template <int DT>
__global__ void __launch_bounds__(HB) k_find(SegState* __restrict__ st, u64* __restrict__ ghist, int pass, int n_slots, QPlan plan,
                                             float* __restrict__ out) {
  __shared__ u64 s_scan[HB];
  __shared__ unsigned s_newpre[MAX_SLOTS];
  __shared__ u64 s_newrank[MAX_SLOTS];
  const int seg = blockIdx.x, t = threadIdx.x;
  SegState* S = st + seg;
  if (t < MAX_SLOTS) { s_newpre[t] = 0; s_newrank[t] = 0; }
  const int gbins = DT == DT_U8 ? 256 : DT == DT_U16 ? 65536 : F32_BINS;
  const int nb = 1 << digit_bits(DT, pass);
  const int per = (nb + HB - 1) / HB;               // consecutive bins per thread
  const int b0 = t * per;
  const int dbits = digit_bits(DT, pass);
  int last_owner = -1;
  for (int s = 0; s < n_slots; ++s) {
    const int own = (DT == DT_F32 && pass > 0) ? S->owner[s] : 0;
    const u64* h = ghist + ((size_t)seg * (DT == DT_U16 ? 1 : MAX_SLOTS) + (DT == DT_U16 ? 0 : own)) * gbins;
    if (own != last_owner) {                        // slots arrive grouped by owner often enough; otherwise the scan is redone
      u64 sum = 0;
      for (int k = 0; k < per; ++k) if (b0 + k < nb) sum += h[b0 + k];
      __syncthreads();
      s_scan[t] = sum;
      __syncthreads();
      for (int o = 1; o < HB; o <<= 1) {            // inclusive scan
        const u64 y = t >= o ? s_scan[t - o] : 0;
        __syncthreads();
        s_scan[t] += y;
        __syncthreads();
      }
      last_owner = own;
    }
    const u64 incl = s_scan[t], excl = t ? s_scan[t - 1] : 0;
    const u64 r = S->rank[s];
    if (b0 < nb && r >= excl && r < incl) {
      u64 rr = r - excl;
      const int nloc = nb - b0 < per ? nb - b0 : per;
      const int b = b0 + find_bin(h + b0, nloc, &rr);
      s_newpre[s] = (DT == DT_F32 && pass > 0 ? (S->prefix[s] << dbits) : 0u) | (unsigned)b;
      s_newrank[s] = rr;
    }
  }
  __syncthreads();
  const bool last = pass == n_passes(DT) - 1;
  if (t < n_slots) { S->prefix[t] = s_newpre[t]; S->rank[t] = s_newrank[t]; }
  __syncthreads();
  if (t == 0) for (int s = 0; s < n_slots; ++s) {
    int o = s;
    for (int j = 0; j < s; ++j) if (s_newpre[j] == s_newpre[s]) { o = j; break; }
    S->owner[s] = o;
  }
  // float32: clear what this pass filled for the next one (the entry point clears the workspace before the first pass)
  if (DT == DT_F32 && !last) {
    const int nh = pass == 0 ? 1 : n_slots;
    u64* hz = ghist + (size_t)seg * MAX_SLOTS * gbins;
    for (int i = t; i < nh * gbins; i += HB) hz[i] = 0;
  }
  if (last && t < plan.n_q) {
    const unsigned ka = s_newpre[2 * t], kb = s_newpre[2 * t + 1];
    float res;
    if (DT == DT_F32) {
      const float a = f32_of_key(ka), b = f32_of_key(kb);
      res = plan.f32 ? lerp_f32(a, b, (float)plan.t[t]) : (float)lerp_f64((double)a, (double)b, plan.t[t]);
      if (S->has_nan) res = __builtin_nanf("");
    } else {
      res = (float)lerp_f64((double)ka, (double)kb, plan.t[t]);
    }
    out[(size_t)seg * plan.n_q + t] = res;
  }
}

__global__ void k_init(SegState* st, int n_seg, QPlan plan) {
  const int seg = blockIdx.x * blockDim.x + threadIdx.x;
  if (seg >= n_seg) return;
  SegState* S = st + seg;
  for (int j = 0; j < MAX_Q; ++j) {
    const bool on = j < plan.n_q;
    S->rank[2 * j] = on ? (u64)plan.lo[j] : 0; S->rank[2 * j + 1] = on ? (u64)plan.hi[j] : 0;
    S->prefix[2 * j] = S->prefix[2 * j + 1] = 0;
    S->owner[2 * j] = S->owner[2 * j + 1] = 0;
  }
  S->has_nan = 0;
}

// ---------------------------------------------------------------------------------------------------------------- rescale
template <typename T>
__global__ void __launch_bounds__(256) k_rescale(const T* x, long long total, int n_seg, bool aligned, const float* __restrict__ mi,
                                                 const float* __restrict__ ma, float eps, int clip, float* out) {   // out may be x (float32)
  enum { N = Vec<T>::N };
  const long long nvec = (total + N - 1) / N;
  float lo0 = 0, den0 = 1;
  if (n_seg == 1) { lo0 = mi[0]; den0 = ma[0] - lo0 + eps; }
  for (long long vi = (long long)blockIdx.x * 256 + threadIdx.x; vi < nvec; vi += (long long)gridDim.x * 256) {
    const long long i0 = vi * N;
    T v[N];
    const int c = load_vec<T>(x, i0, total, aligned, v);
    const int m0 = n_seg == 1 ? 0 : (int)(i0 % n_seg);
    float o[N];
    for (int k = 0; k < N; ++k) {
      float lo = lo0, den = den0;
      if (n_seg != 1) { const int s = (m0 + k) % n_seg; lo = mi[s]; den = ma[s] - lo + eps; }
      float y = ((float)v[k] - lo) / den;             // correctly rounded division (hipcc's default; no reciprocal)
      if (clip) {                                     // np.clip: NaN stays, and so does -0.0 (numpy's clip returns it as it is)
        y = (y >= 0.0f || y != y) ? y : 0.0f;
        y = (y <= 1.0f || y != y) ? y : 1.0f;
      }
      o[k] = y;
    }
    if (aligned && c == N) {
      for (int k = 0; k < N; k += 4) *reinterpret_cast<float4*>(out + i0 + k) = make_float4(o[k], o[k + 1], o[k + 2], o[k + 3]);
    } else {
      for (int k = 0; k < c; ++k) out[i0 + k] = o[k];
    }
  }
}

int cu_count() {
  static int cus[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cus[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}

template <typename T, int DT, int PASS>
int launch_hist(const void* x, long long total, int n_seg, bool aligned, int n_slots, SegState* st, u64* ghist, hipStream_t s) {
  const int bins = 1 << digit_bits(DT, PASS);
  const int nh = PASS == 0 ? 1 : n_slots;
  const size_t lds = (size_t)nh * bins * sizeof(unsigned);
  const long long nvec = (total + Vec<T>::N - 1) / Vec<T>::N;
  const int per_cu = lds <= 32 * 1024 ? 2 : 1;
  const int blocks = (int)std::max<long long>(1, std::min<long long>((nvec + HB - 1) / HB, (long long)cu_count() * per_cu));
  hipLaunchKernelGGL((k_hist<T, DT, PASS>), dim3(blocks, n_seg), dim3(HB), lds, s, (const T*)x, total, n_seg, aligned, n_slots, st, ghist);
  SD_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int sd_percentiles_device(const void* d_x, int dtype, long long n, int n_seg, const double* h_q, int n_q, int interp_f32,
                                     float* d_out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (dtype != DT_U8 && dtype != DT_U16 && dtype != DT_F32) { sd::set_error("sd_percentiles: dtype must be 0 (uint8), 1 (uint16) or 2 (float32)"); return -1; }
  if (!d_x || !d_out || !h_q) { sd::set_error("sd_percentiles: null pointer"); return -1; }
  if (n < 1 || n_seg < 1 || n_seg > 64) { sd::set_error("sd_percentiles: need n >= 1 elements per segment and 1 <= n_seg <= 64"); return -1; }
  if (n_q < 2 || n_q > MAX_Q) { sd::set_error("sd_percentiles: need 2 <= n_q <= %d percentiles", (int)MAX_Q); return -1; }
  QPlan plan;
  memset(&plan, 0, sizeof(plan));
  plan.n_q = n_q;
  plan.f32 = (dtype == DT_F32 && interp_f32) ? 1 : 0;
  for (int j = 0; j < n_q; ++j) {
    if (!(h_q[j] >= 0.0 && h_q[j] <= 100.0)) { sd::set_error("sd_percentiles: percentiles must be in the range [0, 100]"); return -1; }
    const Lerp L = lerp_plan(n, h_q[j], plan.f32 != 0);
    plan.lo[j] = L.lo; plan.hi[j] = L.hi; plan.t[j] = L.t;
  }
  const long long total = n * (long long)n_seg;
  const bool aligned = (uintptr_t)d_x % 16 == 0;
  const int n_slots = 2 * n_q;
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  const size_t hist_words = dtype == DT_U16 ? (size_t)n_seg * 65536 : (size_t)n_seg * MAX_SLOTS * (dtype == DT_U8 ? 256 : F32_BINS);
  SegState* st = A.take_n<SegState>(n_seg);
  u64* ghist = A.take_n<u64>(hist_words);
  if (!st || !ghist) return -1;
  SD_CHECK(hipMemsetAsync(ghist, 0, hist_words * sizeof(u64), s));
  hipLaunchKernelGGL(k_init, dim3((n_seg + 63) / 64), dim3(64), 0, s, st, n_seg, plan);
  SD_LAUNCH_CHECK();
  if (dtype == DT_U8) {
    if (launch_hist<uint8_t, DT_U8, 0>(d_x, total, n_seg, aligned, n_slots, st, ghist, s)) return -1;
    hipLaunchKernelGGL(k_find<DT_U8>, dim3(n_seg), dim3(HB), 0, s, st, ghist, 0, n_slots, plan, d_out);
    SD_LAUNCH_CHECK();
  } else if (dtype == DT_U16) {
    const long long nvec = (total + 7) / 8;
    const long long rounds = (nvec + (long long)U16_ROUND_LOADS * HB - 1) / ((long long)U16_ROUND_LOADS * HB);
    const int blocks = (int)std::max<long long>(1, std::min<long long>(rounds, cu_count()));
    hipLaunchKernelGGL(k_hist_u16, dim3(blocks, n_seg), dim3(HB), 0, s, (const uint16_t*)d_x, total, n_seg, aligned, ghist);
    SD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_find<DT_U16>, dim3(n_seg), dim3(HB), 0, s, st, ghist, 0, n_slots, plan, d_out);
    SD_LAUNCH_CHECK();
  } else {
    if (launch_hist<float, DT_F32, 0>(d_x, total, n_seg, aligned, n_slots, st, ghist, s)) return -1;
    hipLaunchKernelGGL(k_find<DT_F32>, dim3(n_seg), dim3(HB), 0, s, st, ghist, 0, n_slots, plan, d_out);
    SD_LAUNCH_CHECK();
    if (launch_hist<float, DT_F32, 1>(d_x, total, n_seg, aligned, n_slots, st, ghist, s)) return -1;
    hipLaunchKernelGGL(k_find<DT_F32>, dim3(n_seg), dim3(HB), 0, s, st, ghist, 1, n_slots, plan, d_out);
    SD_LAUNCH_CHECK();
    if (launch_hist<float, DT_F32, 2>(d_x, total, n_seg, aligned, n_slots, st, ghist, s)) return -1;
    hipLaunchKernelGGL(k_find<DT_F32>, dim3(n_seg), dim3(HB), 0, s, st, ghist, 2, n_slots, plan, d_out);
    SD_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int sd_normalize_mi_ma_device(const void* d_x, int dtype, long long n, int n_seg, const float* d_mi, const float* d_ma, float eps,
                                         int clip, float* d_out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (dtype != DT_U8 && dtype != DT_U16 && dtype != DT_F32) { sd::set_error("sd_normalize_mi_ma: dtype must be 0 (uint8), 1 (uint16) or 2 (float32)"); return -1; }
  if (n < 0 || n_seg < 1) { sd::set_error("sd_normalize_mi_ma: bad sizes"); return -1; }
  if (n == 0) return 0;
  if (!d_x || !d_out || !d_mi || !d_ma) { sd::set_error("sd_normalize_mi_ma: null pointer"); return -1; }
  const long long total = n * (long long)n_seg;
  const bool aligned = (uintptr_t)d_x % 16 == 0 && (uintptr_t)d_out % 16 == 0;
  const int N = dtype == DT_U8 ? 16 : dtype == DT_U16 ? 8 : 4;
  const long long nvec = (total + N - 1) / N;
  const int blocks = (int)std::max<long long>(1, std::min<long long>((nvec + 255) / 256, (long long)cu_count() * 8));
  if (dtype == DT_U8)
    hipLaunchKernelGGL(k_rescale<uint8_t>, dim3(blocks), dim3(256), 0, s, (const uint8_t*)d_x, total, n_seg, aligned, d_mi, d_ma, eps, clip, d_out);
  else if (dtype == DT_U16)
    hipLaunchKernelGGL(k_rescale<uint16_t>, dim3(blocks), dim3(256), 0, s, (const uint16_t*)d_x, total, n_seg, aligned, d_mi, d_ma, eps, clip, d_out);
  else
    hipLaunchKernelGGL(k_rescale<float>, dim3(blocks), dim3(256), 0, s, (const float*)d_x, total, n_seg, aligned, d_mi, d_ma, eps, clip, d_out);
  SD_LAUNCH_CHECK();
  return 0;
}
