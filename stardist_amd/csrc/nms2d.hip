// nms2d.hip -- greedy non-maximum suppression of star-convex polygons on gfx950.
//
// Replaces stardist.lib.stardist2d.c_non_max_suppression_inds
// (stardist/lib/stardist2d.cpp:390-615).  Same inputs (candidates sorted by score
// descending), same survivor set, different schedule:
//
//   K1 build      one thread per candidate (more than 32 rays: one wave): integer vertices (float math + truncation exactly as
//                 stardist2d.cpp:447-471, sin/cos table computed by the HOST libm so the device
//                 never evaluates sinf/cosf), int bbox, outer radius, float area (:128-138).
//   K2 bin        counting sort of candidates into a uniform grid (replaces the nanoflann
//                 kd-tree, stardist2d.cpp:486-513; result-neutral).
//   K3 neighbours CSR lists of the BETTER-scored candidates whose bounding boxes can touch a candidate's (the predicate is a
//                 symmetric superset of every pair the reference would test; the worse-scored ones are found again by
//                 the few candidates that become survivors, from the cell grid).
//   greedy rounds A: a candidate becomes a survivor once every higher-scored neighbour is
//                    decided and none suppressed it;   (wave ballot over the neighbour list)
//                 B: each new survivor walks its cell window and emits the (i, j) pairs the reference
//                    would evaluate for it (stardist2d.cpp:566-577 predicate, exact) via ballot/prefix-sum
//                    compaction into a pair queue;
//                 C: one thread per pair runs the integer scan-beam intersection
//                    (clip_sweep.h) and applies  overlap > threshold  (:579-585).
//   The fixed point of the rounds is the reference's sequential greedy result: j is
//   suppressed iff some survivor i < j has overlap(i,j) > threshold, and a candidate is only
//   promoted to survivor after all of its possible suppressors are final.
#include <type_traits>

#include "common.h"
#include "clip_sweep.h"
#include "clip_beam.h"
#include "area_bounds.h"
#include "poly_pass.h"
#include "nms_rounds.h"
#include "../../include/stardist_hip.h"
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <stdlib.h>
#include <vector>

namespace {

using sdclip::i64;

__device__ __forceinline__ float wave_min(float v) { for (int o = 32; o; o >>= 1) v = fminf(v, __shfl_xor(v, o)); return v; }
__device__ __forceinline__ float wave_max(float v) { for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o)); return v; }
__device__ __forceinline__ i64 wave_sum(i64 v) { for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o); return v; }

// gstats layout (ints): 0 max radius bits, 1 min y, 2 max y, 3 min x, 4 max x
__global__ void __launch_bounds__(256) k_build(const float* __restrict__ dist, const float* __restrict__ pts,
                                               const float2* __restrict__ sincos, int N, int R,
                                               int* __restrict__ vx, int* __restrict__ vy, int4* __restrict__ bbox,
                                               float* __restrict__ radius, float* __restrict__ area, int* gstats) {
  extern __shared__ int lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * (blockDim.x >> 6) + wave;
  if (i >= N) return;
  int* sx = lds + wave * 2 * R;
  int* sy = sx + R;
  const float py = pts[2 * i], px = pts[2 * i + 1];
  float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY, rmax = 0.f;
  for (int k = lane; k < R; k += 64) {
    const float d = dist[(size_t)i * R + k];
    const float2 sc = sincos[k];
    const float y = py + d * sc.x;   // stardist2d.cpp:454 (compiled with -ffp-contract=off)
    const float x = px + d * sc.y;   // stardist2d.cpp:455
    xmin = fminf(xmin, x); xmax = fmaxf(xmax, x);
    ymin = fminf(ymin, y); ymax = fmaxf(ymax, y);
    const int X = (int)(long long)x, Y = (int)(long long)y;   // IntPoint(cInt(x), cInt(y)) :471
    sx[k] = X; sy[k] = Y;
    vx[(size_t)i * R + k] = X; vy[(size_t)i * R + k] = Y;
    rmax = fmaxf(rmax, d);
  }
  xmin = wave_min(xmin); xmax = wave_max(xmax); ymin = wave_min(ymin); ymax = wave_max(ymax);
  rmax = wave_max(rmax);
  __builtin_amdgcn_wave_barrier();
  // area_from_path :128-138: float accumulation of int64 cross products in path order; this
  // equals the exact integer sum whenever sum|term| < 2^24, else fall back to the serial order.
  i64 s = 0, sa = 0;
  for (int k = lane; k < R; k += 64) {
    const int kn = (k + 1 == R) ? 0 : k + 1;
    const i64 c = (i64)sx[k] * sy[kn] - (i64)sy[k] * sx[kn];
    s += c; sa += (c < 0 ? -c : c);
  }
  s = wave_sum(s); sa = wave_sum(sa);
  if (lane == 0) {
    float a;
    if (sa < (1ll << 24)) a = (float)s;
    else {
      a = 0.f;
      for (int k = 0; k < R; ++k) {
        const int kn = (k + 1 == R) ? 0 : k + 1;
        a += (float)((i64)sx[k] * sy[kn] - (i64)sy[k] * sx[kn]);
      }
    }
    area[i] = (float)(0.5 * (double)fabsf(a));
    radius[i] = rmax;
    bbox[i] = make_int4((int)xmin, (int)xmax, (int)ymin, (int)ymax);   // bbox_intersect takes ints :142-148
    // contended global atomics only when the running extremum actually improves
    const int rb = __float_as_int(rmax);
    const int iy = (int)floorf(py), ix = (int)floorf(px);
    volatile int* gs = gstats;
    if (rb > gs[0]) atomicMax(&gstats[0], rb);
    if (iy < gs[1]) atomicMin(&gstats[1], iy);
    if (iy > gs[2]) atomicMax(&gstats[2], iy);
    if (ix < gs[3]) atomicMin(&gstats[3], ix);
    if (ix > gs[4]) atomicMax(&gstats[4], ix);
  }
}

// k_build for n_rays <= 32: ONE THREAD per candidate, one wave (= one workgroup) per 64 candidates.  Before: half a wave per candidate,
// seven 5-step shuffle reductions (two of them 64-bit) and five guarded atomics per candidate, 0.28 ms for the 418 577 candidates of the
// 2048^2 bench set against 50 us of memory traffic.  Here a thread keeps its candidate's running extremes and the integer cross-product
// sums in registers, the wave reduces the five gstats words once and issues one guarded atomic per word.  The wave's 64 rows of dist, vx
// and vy are contiguous in memory: they are moved with lane-consecutive (16-byte where aligned) accesses and staged in LDS, where a thread
// walks its own row -- starting at ray (its index mod R), so that the lanes of a step hit different banks (R = 32: rows are 32 words apart).
// Same arithmetic: every vertex is the same float expression, min / max and the int64 sums do not depend on the order, and the float area
// of a polygon with sum |term| >= 2^24 is replayed in path order.
// LDS (dynamic): 64 * R words of distances, overwritten in place by x; 64 * R words of y.
__global__ void __launch_bounds__(64) k_build32(const float* __restrict__ dist, const float* __restrict__ pts,
                                                const float2* __restrict__ sincos, int N, int R, int vec4,
                                                int* __restrict__ vx, int* __restrict__ vy, int4* __restrict__ bbox,
                                                float* __restrict__ radius, float* __restrict__ area, int* gstats) {
  extern __shared__ __attribute__((aligned(16))) int rows[];
  __shared__ float2 ssc[32];
  const int c = threadIdx.x;
  const int base = blockIdx.x * 64;
  const int cnt = min(64, N - base);                  // (>= 1: the grid is div_up(N, 64))
  const int nel = cnt * R;                            // elements of this wave's rows, <= 64 * R
  int* sx = rows;
  int* sy = rows + 64 * R;
  if (c < R) ssc[c] = sincos[c];
  {
    const int* g = (const int*)dist + (size_t)base * R;   // (moved as bits: the LDS rows are ints throughout)
    const int nv = vec4 ? nel >> 2 : 0;               // (base * R * 4 bytes is a multiple of 256: the rows are aligned if the array is)
    for (int e = c; e < nv; e += 64) ((int4*)rows)[e] = ((const int4*)g)[e];
    for (int e = 4 * nv + c; e < nel; e += 64) rows[e] = g[e];
  }
  __syncthreads();
  const bool cv = c < cnt;
  float rmax = 0.f;
  int iy = INT32_MAX, ix = INT32_MAX, iyh = INT32_MIN, ixh = INT32_MIN;
  if (cv) {
    const int i = base + c;
    const float py = pts[2 * i], px = pts[2 * i + 1];
    float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    i64 s = 0, sa = 0;
    int X0 = 0, Y0 = 0, Xp = 0, Yp = 0;
    int k = c % R;
    for (int t = 0; t < R; ++t) {
      const float d = __int_as_float(rows[c * R + k]);
      const float2 sc = ssc[k];
      const float y = py + d * sc.x;   // stardist2d.cpp:454 (compiled with -ffp-contract=off)
      const float x = px + d * sc.y;   // stardist2d.cpp:455
      xmin = fminf(xmin, x); xmax = fmaxf(xmax, x);
      ymin = fminf(ymin, y); ymax = fmaxf(ymax, y);
      rmax = fmaxf(rmax, d);
      const int X = (int)(long long)x, Y = (int)(long long)y;   // IntPoint(cInt(x), cInt(y)) :471
      sx[c * R + k] = X; sy[c * R + k] = Y;
      if (t) { const i64 cr = (i64)Xp * Y - (i64)Yp * X; s += cr; sa += (cr < 0 ? -cr : cr); }
      else { X0 = X; Y0 = Y; }
      Xp = X; Yp = Y;
      k = (k + 1 == R) ? 0 : k + 1;
    }
    { const i64 cr = (i64)Xp * Y0 - (i64)Yp * X0; s += cr; sa += (cr < 0 ? -cr : cr); }      // closes the cycle of R edges
    // area_from_path :128-138: float accumulation of int64 cross products in path order; equals the exact integer sum whenever
    // sum|term| < 2^24, else the serial order is replayed (from the thread's own row)
    float a;
    if (sa < (1ll << 24)) a = (float)s;
    else {
      a = 0.f;
      for (int q = 0; q < R; ++q) {
        const int qn = (q + 1 == R) ? 0 : q + 1;
        a += (float)((i64)sx[c * R + q] * sy[c * R + qn] - (i64)sy[c * R + q] * sx[c * R + qn]);
      }
    }
    area[i] = (float)(0.5 * (double)fabsf(a));
    radius[i] = rmax;
    bbox[i] = make_int4((int)xmin, (int)xmax, (int)ymin, (int)ymax);   // bbox_intersect takes ints :142-148
    iy = iyh = (int)floorf(py); ix = ixh = (int)floorf(px);
  }
  for (int o = 32; o; o >>= 1) {
    rmax = fmaxf(rmax, __shfl_xor(rmax, o));
    iy = min(iy, __shfl_xor(iy, o)); iyh = max(iyh, __shfl_xor(iyh, o));
    ix = min(ix, __shfl_xor(ix, o)); ixh = max(ixh, __shfl_xor(ixh, o));
  }
  if (c == 0) {
    // contended global atomics only when the running extremum actually improves
    const int rb = __float_as_int(rmax);
    volatile int* gs = gstats;
    if (rb > gs[0]) atomicMax(&gstats[0], rb);
    if (iy < gs[1]) atomicMin(&gstats[1], iy);
    if (iyh > gs[2]) atomicMax(&gstats[2], iyh);
    if (ix < gs[3]) atomicMin(&gstats[3], ix);
    if (ixh > gs[4]) atomicMax(&gstats[4], ixh);
  }
  __syncthreads();
  {
    int* gx = vx + (size_t)base * R;
    int* gy = vy + (size_t)base * R;
    const int nv = vec4 ? nel >> 2 : 0;
    for (int e = c; e < nv; e += 64) { ((int4*)gx)[e] = ((const int4*)sx)[e]; ((int4*)gy)[e] = ((const int4*)sy)[e]; }
    for (int e = 4 * nv + c; e < nel; e += 64) { gx[e] = sx[e]; gy[e] = sy[e]; }
  }
}

struct GridP { float y0, x0, inv_cs; int ny, nx; };

__device__ __forceinline__ int cell_of(const GridP g, float py, float px, int& cy, int& cx) {
  cy = (int)((py - g.y0) * g.inv_cs); cx = (int)((px - g.x0) * g.inv_cs);
  cy = min(max(cy, 0), g.ny - 1); cx = min(max(cx, 0), g.nx - 1);
  return cy * g.nx + cx;
}

// The cells a candidate's neighbours can lie in (cells are indexed by the CENTRE of a candidate).  With the bbox test in force (threshold >= 0
// or use_bbox: may_interact requires intersecting integer bounding boxes) a neighbour j of i has bbox_j inside [p_j - (r + 1), p_j + (r + 1)],
// r = the largest distance of ANY candidate (a vertex is centre + d (sin, cos) truncated), so its centre lies within bbox_i grown by r + 1:
// a window per candidate (round 6; before: the 5 x 5 cells of size r + 1 around its own cell, 1.5 x the area), with half a pixel of slack
// for the float cell arithmetic.  Without the bbox test (kd-tree radius only) the window is the centre +- (2 r + 1).
struct Window { int ylo, yhi, xlo, xhi; };
__device__ __forceinline__ Window cell_window(const GridP g, bool by_bbox, float reach, const int4 bb, float py, float px) {
  float y0, y1, x0, x1;
  if (by_bbox) { x0 = (float)bb.x - reach; x1 = (float)bb.y + reach; y0 = (float)bb.z - reach; y1 = (float)bb.w + reach; }
  else { const float rr = 2.f * reach; x0 = px - rr; x1 = px + rr; y0 = py - rr; y1 = py + rr; }
  Window w;
  w.ylo = min(max((int)floorf((y0 - 0.5f - g.y0) * g.inv_cs), 0), g.ny - 1); w.yhi = min(max((int)floorf((y1 + 0.5f - g.y0) * g.inv_cs), 0), g.ny - 1);
  w.xlo = min(max((int)floorf((x0 - 0.5f - g.x0) * g.inv_cs), 0), g.nx - 1); w.xhi = min(max((int)floorf((x1 + 0.5f - g.x0) * g.inv_cs), 0), g.nx - 1);
  return w;
}
constexpr int MAX_WIN_ROWS = 32;      // rows of a window (<= 10 with cells of half the reach; the host falls back to coarser cells otherwise)

__global__ void k_cell_count(const float* __restrict__ pts, int N, GridP g, int* __restrict__ cellCount, int* __restrict__ candCell) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  int cy, cx;
  const int c = cell_of(g, pts[2 * i], pts[2 * i + 1], cy, cx);
  candCell[i] = c;
  atomicAdd(&cellCount[c], 1);
}
// candidates re-packed in cell order: the broad phase streams these 32-byte records (coalesced) instead of gathering
// bbox / centre / area of every cell item by candidate index
struct __attribute__((aligned(16))) CellRec { int4 bb; float py, px, area; int j; };
// slotCap (may be null): upper bound of candidate i's neighbour count = the population of the cells of its window (cell_window) its list is built from,
// minus itself -- the capacity of its slot in the single-pass neighbour lists (k_neighbours<2>)
__global__ void k_cell_fill(int N, const int* __restrict__ candCell, const int* __restrict__ cellStart,
                            int* __restrict__ cellFill, const float* __restrict__ pts, const int4* __restrict__ bbox,
                            const float* __restrict__ area, CellRec* __restrict__ rec, GridP g, int by_bbox, float reach, int* __restrict__ slotCap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int c = candCell[i];
  const int pos = atomicAdd(&cellFill[c], 1);
  CellRec r;
  r.bb = bbox[i]; r.py = pts[2 * i]; r.px = pts[2 * i + 1]; r.area = area[i]; r.j = i;
  rec[cellStart[c] + pos] = r;
  if (slotCap) {
    const Window w = cell_window(g, by_bbox != 0, reach, r.bb, r.py, r.px);
    int u = -1;
    for (int yy = w.ylo; yy <= w.yhi; ++yy) u += cellStart[yy * g.nx + w.xhi + 1] - cellStart[yy * g.nx + w.xlo];
    slotCap[i] = u;
    if (i == 0) slotCap[N] = 0;               // (closes the array for the exclusive scan)
  }
}

__device__ __forceinline__ bool bbox_intersect(const int4 a, const int4 b) {   // stardist2d.cpp:142-148
  return (b.x <= a.y && a.x <= b.y && b.z <= a.w && a.z <= b.w);
}

// symmetric "may interact" predicate used for the dependency lists
__device__ __forceinline__ bool may_interact(const NmsFlags f, const int4 bi, const int4 bj, float pyi, float pxi, float pyj, float pxj,
                                             float ai, float aj) {
  if (f.thr_nonneg) {
    // disjoint integer bboxes => area 0 => overlap 0 <= thr; more generally area_inter <= area(bbox_i ∩ bbox_j), so a pair
    // whose bbox-intersection area cannot exceed thr * min(area) can never suppress.  The lists only have to be a SUPERSET of the pairs
    // the emission kernels accept with the exact form of this bound (k_round_emit / k_tail_emit: the double quotient): here it is the
    // division-free float form with a relative margin of 1e-5 (every rounding of either form is below 2e-7).
    if (!bbox_intersect(bi, bj)) return false;
    const float wh = (float)(min(bi.y, bj.y) - max(bi.x, bj.x)) * (float)(min(bi.w, bj.w) - max(bi.z, bj.z));
    return wh * 1.00001f >= f.thr * fminf(ai, aj) * 0.99999f;
  }
  bool ok = true;
  if (f.use_bbox) ok = ok && bbox_intersect(bi, bj);
  if (f.use_kdtree) {
    const float dy = pyi - pyj, dxx = pxi - pxj;
    const float rr = 2.f * f.max_dist + 1.f;
    ok = ok && (dy * dy + dxx * dxx < rr * rr);
  }
  return ok;
}

// The rows of a window are contiguous runs of the cell-ordered records; the runs are walked as ONE list, 64 records per step whatever the
// row lengths -- a row of ~35 records does not cost a step of its own.  Lane r holds row r's start and the exclusive prefix of the row
// lengths; nrows and total are wave-uniform (the whole wave walks ONE candidate's window).
struct WindowRuns { int rbeg, excl, nrows, total; };
__device__ __forceinline__ WindowRuns window_runs(const GridP g, const Window win, const int* __restrict__ cellStart, int lane) {
  WindowRuns w;
  w.nrows = __builtin_amdgcn_readfirstlane(win.yhi - win.ylo + 1);
  int rbeg = 0, rlen = 0;
  if (lane < w.nrows) { rbeg = cellStart[(win.ylo + lane) * g.nx + win.xlo]; rlen = cellStart[(win.ylo + lane) * g.nx + win.xhi + 1] - rbeg; }
  int incl = rlen;
  for (int o = 1; o < MAX_WIN_ROWS; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
  w.total = __builtin_amdgcn_readlane(incl, w.nrows - 1);
  w.rbeg = rbeg; w.excl = incl - rlen;
  return w;
}
// body(index into the cell-ordered records, or -1 past the end) is called by the whole wave, once per step.  The row of virtual index v is
// the last row whose exclusive prefix is <= v (rows may be empty).  A step's 64 indices span few rows: the wave keeps the row of the
// step's first index and advances it, and only the rows that begin inside the step are compared per lane -- scalar reads of the two lane
// arrays (before: every row of the window, two cross-lane reads each, in every step).
template <class Body>
__device__ __forceinline__ void walk_window(const WindowRuns& w, int lane, Body&& body) {
  int r0 = 0;
  for (int t = 0; t < w.total; t += 64) {
    while (r0 + 1 < w.nrows && __builtin_amdgcn_readlane(w.excl, r0 + 1) <= t) ++r0;
    int rb = __builtin_amdgcn_readlane(w.rbeg, r0), re = __builtin_amdgcn_readlane(w.excl, r0);
    const int v = t + lane;
    for (int r = r0 + 1; r < w.nrows; ++r) {
      const int e_r = __builtin_amdgcn_readlane(w.excl, r);
      if (e_r > t + 63) break;
      const int b_r = __builtin_amdgcn_readlane(w.rbeg, r);
      if (e_r <= v) { rb = b_r; re = e_r; }
    }
    body(v < w.total ? rb + (v - re) : -1);
  }
}

// The lists hold a candidate's BETTER-scored (lower-index) neighbours only -- what the greedy scan and the tail batch look at.  The
// worse-scored ones are not listed: a new survivor finds them by walking its own window (k_round_emit), and only 3 % of the candidates
// ever become one.  The predicate is symmetric, so the number of ordered neighbour relations is twice the number of entries.
// MODE 0: count (nbrCount = nbrLow = the list's size), MODE 1: fill CSR (two passes: exact-size lists);
// MODE 2: ONE pass into per-candidate slots whose capacity is the population of the cells scanned (k_cell_fill slotCap; nbrStart = slot
// starts), written from the slot's front; nbrLow tells the consumers where the list ends -- the candidate tests of the counting pass
// are not repeated
template <int MODE>
__global__ void __launch_bounds__(256) k_neighbours(int N, GridP g, NmsFlags f, const CellRec* __restrict__ rec, const int* __restrict__ cellStart,
                                                    int* __restrict__ nbrCount, int* __restrict__ nbrLow, const i64* __restrict__ nbrStart,
                                                    int* __restrict__ nbr, int* __restrict__ waitOn, int by_bbox, float reach) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // wave w handles the w-th candidate IN CELL ORDER, and consecutive workgroups of one XCD (blockIdx % 8) get consecutive
  // cells: the windows of successive waves overlap almost completely and stay in that XCD's L2
  const int per = gridDim.x >> 3;                                   // grid is a multiple of 8
  const int blk = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  const int w = blk * (blockDim.x >> 6) + wave;
  if (w >= N) return;
  const CellRec me = rec[w];
  const int i = me.j;
  const int4 bi = me.bb;
  const float pyi = me.py, pxi = me.px, ai = me.area;
  int nLo = 0;
  int minj = INT32_MAX;                      // best-scored neighbour above i (first wait target of the greedy scan)
  const i64 base = MODE ? nbrStart[i] : 0;
  const WindowRuns runs = window_runs(g, cell_window(g, by_bbox != 0, reach, bi, pyi, pxi), cellStart, lane);
  walk_window(runs, lane, [&](int ri) {
    bool hit = false;
    int j = -1;
    if (ri >= 0) {
      const CellRec r = rec[ri];
      j = r.j;
      if (j < i) hit = may_interact(f, bi, r.bb, pyi, pxi, r.py, r.px, ai, r.area);
    }
    const unsigned long long m = __ballot(hit);
    if (MODE && hit) { nbr[base + nLo + __popcll(m & ((1ull << lane) - 1))] = j; if (j < minj) minj = j; }
    nLo += __popcll(m);
  });
  if (!MODE && lane == 0) nbrCount[i] = nLo;
  if (MODE != 1 && lane == 0) nbrLow[i] = nLo;
  if (MODE) {
    for (int o = 32; o; o >>= 1) minj = min(minj, __shfl_xor(minj, o));
    if (lane == 0) waitOn[i] = (minj < i) ? minj : WAIT_NONE;
  }
}

// Round kernel B: wave per new survivor: mark it, emit the pairs the reference would evaluate.  The survivor walks its own cell window
// over the cell-ordered records (the walk of k_neighbours): the window covers every j the filters below accept -- with the bbox test
// in force j's bounding box meets i's, without it j's centre lies within max_dist + radius[i] < 2 reach of i's -- and the record holds
// everything the filters read of j.
constexpr int EMIT_STAGE = 512;
__global__ void __launch_bounds__(256) k_round_emit(const int* __restrict__ K, const int* __restrict__ nKPtr, unsigned char* __restrict__ state,
                                                    GridP g, const CellRec* __restrict__ rec, const int* __restrict__ cellStart, int by_bbox, float reach,
                                                    NmsFlags f, const float* __restrict__ pts, const int4* __restrict__ bbox,
                                                    const float* __restrict__ radius, const float* __restrict__ area,
                                                    int2* __restrict__ pairs, unsigned long long* pairCount,
                                                    unsigned long long pairCap) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nK = *nKPtr;                               // persistent grid: the survivor count of this round is read on the device
  // pairs are staged per wave in LDS and appended with ONE atomic per EMIT_STAGE pairs: an atomic per 64-record step of a window
  // serialises at the L2
  __shared__ int2 stage[4][EMIT_STAGE];
  int nst = 0;                                         // (wave-uniform)
  auto flush = [&]() {
    if (!nst) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(pairCount, (unsigned long long)nst);
    base = __shfl(base, 0);
    __builtin_amdgcn_wave_barrier();                   // (a wave's LDS accesses are processed in order)
    for (int k = lane; k < nst; k += 64) { const unsigned long long pos = base + k; if (pos < pairCap) pairs[pos] = stage[wave][k]; }
    __builtin_amdgcn_wave_barrier();
    nst = 0;
  };
  for (int w = blockIdx.x * (blockDim.x >> 6) + wave; w < nK; w += gridDim.x * (blockDim.x >> 6)) {
    const int i = K[w];
    if (lane == 0) state[i] = ST_KEPT;
    const int4 bi = bbox[i];
    const float pyi = pts[2 * i], pxi = pts[2 * i + 1];
    const double ai = (double)area[i] + 1.e-10;
    const float rad = f.max_dist + radius[i];
    const float rad2 = rad * rad;                       // stardist2d.cpp:549
    const WindowRuns runs = window_runs(g, cell_window(g, by_bbox != 0, reach, bi, pyi, pxi), cellStart, lane);
    walk_window(runs, lane, [&](int ri) {
      bool emit = false;
      int j = -1;
      if (ri >= 0) {
        const CellRec r = rec[ri];
        j = r.j;
        bool ok = j > i;
        if (ok && f.use_kdtree) {                       // nanoflann L2_Simple, strict '<' (nanoflann.hpp:249-253)
          const float d0 = pyi - r.py, d1 = pxi - r.px;
          float d2 = d0 * d0; d2 += d1 * d1;
          ok = d2 < rad2;
        }
        if (ok && (f.use_bbox || f.thr_nonneg)) {
          const int4 bj = r.bb;
          ok = bbox_intersect(bi, bj);                                               // :576
          if (ok && f.thr_nonneg) {
            // rigorous upper bound: Clipper's output (input vertices + lattice-rounded crossings) stays inside the
            // intersection of the two integer bounding boxes, so area_inter <= w*h; if even that cannot exceed
            // the threshold the reference's  overlap > thr  (:580-581) is false without running the sweep.
            const double w = (double)(min(bi.y, bj.y) - max(bi.x, bj.x)), hgt = (double)(min(bi.w, bj.w) - max(bi.z, bj.z));
            const float ub = (float)((w * hgt) / fmin(ai, (double)r.area + 1.e-10));   // monotone in the area
            if (!(ub > f.thr)) ok = false;
          }
        }
        emit = ok && state[j] == ST_UNDECIDED;          // :572 (read last: the only gather of the walk)
      }
      const unsigned long long m = __ballot(emit);
      if (m) {
        const int c = __popcll(m);
        if (nst + c > EMIT_STAGE) flush();
        if (emit) stage[wave][nst + __popcll(m & ((1ull << lane) - 1))] = make_int2(i, j);
        nst += c;
      }
    });
  }
  flush();
}

// ---- prepared polygons for n_rays > 32: Clipper::AddPath once per candidate (clip_beam.h), one thread per candidate, working arrays
// lane-interleaved in LDS (n_rays <= 32: poly_pass.h)
template <int MAXV, int S>
__global__ void __launch_bounds__(S) k_prepare(const int* __restrict__ vx, const int* __restrict__ vy, int N, int R,
                                               sdclip::PolyPrep<MAXV>* __restrict__ prep) {
  const int i = blockIdx.x * S + threadIdx.x;
  if (i >= N) return;
  sdclip::PrepWork<sdclip::LdsStorage<S>, MAXV> w;
  w.prepare(vx + (size_t)i * R, vy + (size_t)i * R, R, prep + i);
}

// Round kernel C: one thread per pair, bound-slot sweep with the whole per-pair state lane-interleaved in LDS.
// Persistent grid: the pair count is read on the device (no host round trip between emit and this kernel).
//   result 'capacity exceeded'  -> spill queue (next tier with larger K / list capacities, finally the general path)
//   joins recorded / float-order risk / any other flag -> exact queue (clip_sweep_full.h restates JoinCommonEdges)
// queues hold PAIR INDICES (into the round's pair list), so a result can be written per pair (tail batch) as well as applied
struct PairQueues { unsigned int* spill; unsigned int* spillCount; unsigned int* exact; unsigned int* exactCount; unsigned int cap; };
enum { BEAM_CAPFLAGS = sdclip::ST_OVERFLOW_IL | sdclip::ST_OVERFLOW_REC | sdclip::ST_OVERFLOW_AEL | sdclip::ST_OVERFLOW_LM | sdclip::ST_OVERFLOW_GJ };
// idx == nullptr: pairs[0 .. *nPtr);  else pairs[idx[0 .. *nPtr)].   supp == nullptr: a suppressing pair marks state[j]
// (greedy round, i is a survivor); else supp[pair index] = 1 (tail batch: i is still undecided, the result is kept per edge).
// REL16: the sweep state with 16-bit coordinates relative to the pair's origin and recomputed slopes (clip_sweep.h LdsStorage16): 420
// instead of 636 bytes per pair; a pair whose coordinates do not fit raises a capacity flag and spills to the next tier like any other
template <int MAXV, int K, int MAXIL, int MAXREC, int S, typename CNT, bool REL16 = false>
__global__ void __launch_bounds__(S) k_pairs_beam(const int2* __restrict__ pairs, const unsigned int* __restrict__ idx, const CNT* __restrict__ nPtr,
                                                  const unsigned int* __restrict__ firstPtr, const sdclip::PolyPrep<MAXV>* __restrict__ prep,
                                                  const float* __restrict__ area, float thr, unsigned char* __restrict__ state,
                                                  unsigned char* __restrict__ supp, PairQueues q) {
  typedef typename std::conditional<REL16, sdclip::LdsStorage16<S>, sdclip::LdsStorage<S>>::type Storage;
  typedef sdclip::Beam<MAXV, K, MAXIL, MAXREC, Storage> BeamT;
  const unsigned long long n = (unsigned long long)*nPtr;
  const unsigned long long first = firstPtr ? (unsigned long long)*firstPtr : 0ull;      // entries before `first` are already queued for the general path
  // Latency regime (fewer pairs than the launch has lanes: the late rounds, the tail batch): every workgroup takes ONE contiguous chunk of the
  // (offset-ordered) list with its first `chunk` lanes, the others stay idle -- the sweeps of a wave's lanes share no control flow, so a
  // launch lasts as long as the busiest wave's lanes take one after the other; spreading 25 000 pairs over all 1 536 waves at 16 lanes each
  // instead of filling 390 waves halves that.  Otherwise the grid-stride loop over full waves.
  const unsigned long long total = n > first ? n - first : 0ull;
  const unsigned long long chunk = (total + gridDim.x - 1) / gridDim.x;
  const bool spread = chunk <= (unsigned long long)S;
  unsigned long long t = spread ? first + (unsigned long long)blockIdx.x * chunk + threadIdx.x : first + (unsigned long long)blockIdx.x * S + threadIdx.x;
  if (spread && (unsigned long long)threadIdx.x >= chunk) t = n;
  const unsigned long long step = spread ? (1ull << 62) : (unsigned long long)gridDim.x * S;
  for (; t < n; t += step) {
    const unsigned int p = idx ? idx[t] : (unsigned int)t;
    const int2 ij = pairs[p];
    BeamT bm;
    bm.reset_state(prep + ij.x, prep + ij.y);                                  // clip = i (:157), subject = j (:158)
    const i64 twice = bm.execute();
    const int st = bm.status;
    if (st & BEAM_CAPFLAGS) {
      const unsigned int k = atomicAdd(q.spillCount, 1u);
      if (k < q.cap) q.spill[k] = p;
      continue;
    }
    if ((st & ~sdclip::ST_FAIL) || bm.n_joins > 0 || bm.sum_abs_terms >= (1ll << 24)) {
      const unsigned int k = atomicAdd(q.exactCount, 1u);
      if (k < q.cap) q.exact[k] = p;
      continue;
    }
    const float area_inter = 0.5f * (float)twice;
    const float overlap = (float)((double)area_inter / fmin((double)area[ij.x] + 1.e-10, (double)area[ij.y] + 1.e-10));  // :580
    if (overlap > thr) { if (supp) supp[p] = 1; else state[ij.y] = ST_SUPPRESSED; }                // :581-585
  }
}
template <int MAXV, int K, int MAXIL, int MAXREC, int S, bool REL16 = false>
size_t beam_lds_bytes() {
  typedef typename std::conditional<REL16, sdclip::LdsStorage16<S>, sdclip::LdsStorage<S>>::type Storage;
  return (size_t)sdclip::Beam<MAXV, K, MAXIL, MAXREC, Storage>::lds_bytes() + 64;
}

// Round kernel C0 (area_bounds.h): the pairs whose decision follows from an enclosure of the intersection area -- regular arithmetic,
// 32 lanes per pair -- are decided here; decided[t] != 0 removes a pair from the sweep kernels' work list (k_pair_bucket_*).
__global__ void __launch_bounds__(256) k_pairs_decide(const int2* __restrict__ pairs, const unsigned long long* __restrict__ nPtr,
                                                      const unsigned int* __restrict__ firstPtr, const int* __restrict__ vx, const int* __restrict__ vy, int R,
                                                      const sdarea::PolyProps* __restrict__ props, const float* __restrict__ area, float thr,
                                                      unsigned char* __restrict__ state, unsigned char* __restrict__ supp,
                                                      unsigned char* __restrict__ decided, unsigned int* __restrict__ nDecided) {
  __shared__ float4 rec[4][2][sdarea::REC_FLOAT4];
  const int lane = threadIdx.x & 63, half = lane >> 5, l = lane & 31, wv = threadIdx.x >> 6;
  const unsigned long long n = *nPtr, first = firstPtr ? (unsigned long long)*firstPtr : 0ull;
  const unsigned long long step = 2ull * gridDim.x * 4;
  unsigned int mine = 0;
  for (unsigned long long base = first + 2ull * ((unsigned long long)blockIdx.x * 4 + wv); base < n; base += step) {
    const unsigned long long t = base + half;
    const bool active = t < n;
    const int2 ij = active ? pairs[t] : make_int2(0, 0);
    const sdarea::PairOperands o = sdarea::load_operands(vx + (size_t)ij.x * R, vy + (size_t)ij.x * R, vx + (size_t)ij.y * R, vy + (size_t)ij.y * R,
                                                         props + ij.x, props + ij.y, active && l < R, l);   // clip = i, subject = j (:157-158)
    const sdarea::Enclosure E = sdarea::pair_enclosure(o, R, active, rec[wv][half], l, half);
    if (active && l == 0) {
      const int dec = sdarea::decide(E, area[ij.x], area[ij.y], thr);
      decided[t] = (unsigned char)dec;
      if (dec == 2) { if (supp) supp[t] = 1; else state[ij.y] = ST_SUPPRESSED; }                  // :581-585
      if (dec) ++mine;
    }
    __builtin_amdgcn_wave_barrier();
  }
  mine += __shfl_xor(mine, 32);
  if (lane == 0 && mine) atomicAdd(nDecided, mine);
}

// ---- tail batch.  Late greedy rounds hold few pairs but each costs one sweep's serial latency; once few candidates are
// undecided, ALL pairs (i < j, both undecided) the reference could still evaluate are emitted at once, their overlap decisions
// are computed speculatively (supp[edge]), and one workgroup then replays the remaining greedy rounds on the device:
// j is suppressed iff some KEPT i < j has supp(i, j); it is kept once every such i is decided and none suppresses it.
__global__ void __launch_bounds__(256) k_tail_emit(const int* __restrict__ U, int nU, const unsigned char* __restrict__ state,
                                                   const i64* __restrict__ nbrStart, const int* __restrict__ nbrLow, const int* __restrict__ nbr, NmsFlags f,
                                                   const float* __restrict__ pts, const int4* __restrict__ bbox,
                                                   const float* __restrict__ radius, const float* __restrict__ area,
                                                   int2* __restrict__ pairs, unsigned long long* pairCount, unsigned long long pairCap,
                                                   unsigned int* __restrict__ segStart, int* __restrict__ segCnt) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int w = blockIdx.x * (blockDim.x >> 6) + wave; w < nU; w += gridDim.x * (blockDim.x >> 6)) {
    const int j = U[w];
    int cnt = 0;
    unsigned long long base = 0;
    if (state[j] == ST_UNDECIDED) {
      const i64 beg = nbrStart[j], end = beg + nbrLow[j];      // the better-scored neighbours
      const int4 bj = bbox[j];
      const float pyj = pts[2 * j], pxj = pts[2 * j + 1];
      const float aj = area[j];
      for (int pass = 0; pass < 2; ++pass) {
        int k = 0;
        for (i64 t = beg; t < end; t += 64) {
          const i64 id = t + lane;
          bool emit = false;
          int i = -1;
          if (id < end) {
            i = nbr[id];
            if (i < j && state[i] == ST_UNDECIDED) {          // i may become a survivor before j is decided (:572 seen from i)
              bool ok = true;
              if (f.use_kdtree) {                             // nanoflann radius search around i (:546-550)
                const float rad = f.max_dist + radius[i];
                const float d0 = pts[2 * i] - pyj, d1 = pts[2 * i + 1] - pxj;
                float d2 = d0 * d0; d2 += d1 * d1;
                ok = d2 < rad * rad;
              }
              if (ok && (f.use_bbox || f.thr_nonneg)) {
                const int4 bi = bbox[i];
                ok = bbox_intersect(bi, bj);                                             // :576
                if (ok && f.thr_nonneg) {                     // same rigorous bbox-area bound as k_round_emit
                  const double w2 = (double)(min(bi.y, bj.y) - max(bi.x, bj.x)), hgt = (double)(min(bi.w, bj.w) - max(bi.z, bj.z));
                  const float ub = (float)((w2 * hgt) / fmin((double)area[i] + 1.e-10, (double)aj + 1.e-10));
                  if (!(ub > f.thr)) ok = false;
                }
              }
              emit = ok;
            }
          }
          const unsigned long long m = __ballot(emit);
          if (pass == 1 && emit) {
            const unsigned long long pos = base + k + __popcll(m & ((1ull << lane) - 1));
            if (pos < pairCap) pairs[pos] = make_int2(i, j);
          }
          k += __popcll(m);
        }
        if (pass == 0) {
          cnt = k;
          if (cnt == 0) break;
          if (lane == 0) base = atomicAdd(pairCount, (unsigned long long)cnt);
          base = __shfl(base, 0);
        }
      }
    }
    if (lane == 0) { segStart[w] = (unsigned int)base; segCnt[w] = cnt; }
  }
}
// ---- deferral of the general path.  A pair of a normal round that needs the general path (joins / capacities) is NOT evaluated
// in that round: it is appended to the deferred list, j is marked pending (it can still be suppressed by another survivor's pair,
// but cannot be promoted), and all deferred pairs are evaluated by ONE launch of the general kernel in the tail batch -- instead
// of one latency-bound launch per round.  Per candidate the deferred pairs form a linked list (defHead / defNext).
struct Deferred { int2* pairs; int* next; int* head; unsigned char* pend; unsigned int* count; unsigned int cap; };
// (a deferred list that is full cannot take the pair: counted in *nErr, the call then fails loudly instead of dropping a decision)
__global__ void k_defer(const int2* __restrict__ pairs, const unsigned int* __restrict__ exact, const unsigned int* __restrict__ nExact, unsigned int qcap,
                        Deferred d, unsigned int* __restrict__ nErr) {
  unsigned int n = *nExact; if (n > qcap) n = qcap;
  for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
    const int2 ij = pairs[exact[t]];
    const unsigned int k = atomicAdd(d.count, 1u);
    if (k < d.cap) { d.pairs[k] = ij; d.pend[ij.y] = 1; d.next[k] = atomicExch(&d.head[ij.y], (int)k); }
    else atomicAdd(nErr, 1u);
  }
}
// tail batch: the deferred pairs become entries 0 .. nDef-1 of the tail's pair list and of its general-path queue
__global__ void k_tail_init(Deferred d, int2* __restrict__ pairs, unsigned int* __restrict__ exact, unsigned long long* nPairs,
                            unsigned int* nExact, unsigned int* firstNew) {
  unsigned int n = *d.count; if (n > d.cap) n = d.cap;
  for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) { pairs[t] = d.pairs[t]; exact[t] = t; }
  if (blockIdx.x == 0 && threadIdx.x == 0) { *nPairs = n; *nExact = n; *firstNew = n; }
}
// Deferral of the pairs the area enclosure leaves undecided (option "nms2d_defer_undecided" = first round that defers): a sweep launch
// costs one sweep's serial latency (~0.65 ms) however few pairs it holds, so from that round on the undecided pairs are not swept in
// their round but carried to the tail batch like the general-path pairs -- kind[k] = 1 marks them: there they are swept (tier 1 / 2),
// while the kind-0 pairs go to the general kernel as before.  j is pending until then (can be suppressed, cannot be promoted).
__global__ void k_defer_undecided(const int2* __restrict__ pairs, const unsigned long long* __restrict__ nPtr, const unsigned int* __restrict__ nDecided,
                                  unsigned int limit, unsigned char* __restrict__ decided, const unsigned char* __restrict__ state, Deferred d,
                                  unsigned char* __restrict__ kind, unsigned int* __restrict__ nErr) {
  // only a round whose undecided pairs would make a latency-bound sweep launch defers them (many undecided pairs -- a threshold inside
  // the overlap range of one object's candidates -- are swept at once more cheaply than they are carried along); a deferred pair gets
  // decided[t] = 4, so that the bucketing and the sweeps that follow in the stream find nothing to do
  const unsigned long long n = *nPtr;
  if (n - (unsigned long long)*nDecided > (unsigned long long)limit) return;
  for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (unsigned long long)gridDim.x * blockDim.x) {
    if (decided[t]) continue;
    decided[t] = 4;
    const int2 ij = pairs[t];
    if (state[ij.y] == ST_SUPPRESSED) continue;            // a decided pair of this round already suppressed j
    const unsigned int k = atomicAdd(d.count, 1u);
    if (k < d.cap) { d.pairs[k] = ij; d.pend[ij.y] = 1; d.next[k] = atomicExch(&d.head[ij.y], (int)k); kind[k] = 1; }
    else atomicAdd(nErr, 1u);
  }
}
// tail batch with both kinds of deferred pairs: all become entries 0 .. nDef-1 of the pair list; kind 0 -> general-path queue and
// decided[t] = 3 (the sweeps skip them), kind 1 -> decided[t] = 0 (bucketed and swept with the tail's own undecided pairs).
// *nExact must be zero on entry; *nJoin receives the number of kind-0 pairs (the queue's prefix).
// A kind-1 pair whose j another survivor's pair has suppressed since it was deferred is not swept (decided[t] = 4, counted in *nSkipped):
// its supp[] stays 0, j's state is final.
__global__ void k_tail_init2(Deferred d, const unsigned char* __restrict__ kind, int2* __restrict__ pairs, unsigned int* __restrict__ exact,
                             unsigned long long* nPairs, unsigned int* nExact, unsigned int* firstNew, unsigned char* __restrict__ decided,
                             const unsigned char* __restrict__ state, unsigned int* __restrict__ nSkipped) {
  unsigned int n = *d.count; if (n > d.cap) n = d.cap;
  for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
    const int2 ij = d.pairs[t];
    pairs[t] = ij;
    if (kind[t] == 0) { exact[atomicAdd(nExact, 1u)] = t; decided[t] = 3; }
    else if (state[ij.y] == ST_SUPPRESSED) { decided[t] = 4; atomicAdd(nSkipped, 1u); }
    else decided[t] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { *nPairs = n; *firstNew = n; }
}
// the per-candidate arrays of the greedy rounds in their initial state, in one launch (before: an iota kernel and four fill commands)
__global__ void k_round_lists_init(int N, int* __restrict__ U, unsigned char* __restrict__ state, unsigned char* __restrict__ pend,
                                   int* __restrict__ head, unsigned int* __restrict__ dcount) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *dcount = 0;
  if (i >= N) return;
  U[i] = i; state[i] = ST_UNDECIDED; pend[i] = 0; head[i] = -1;
}
__global__ void k_copy_u32(unsigned int* dst, const unsigned int* src) { *dst = *src; }
// a sweep launch over fewer pairs than this is pure latency (98 304 pairs are in flight at once): option "nms2d_defer_max", default 16 384
// deferred pairs of candidate j: true if one of them suppresses it (their survivors i are KEPT by construction)
__device__ __forceinline__ bool deferred_suppresses(int j, const int* __restrict__ defHead, const int* __restrict__ defNext,
                                                    const unsigned char* __restrict__ supp) {
  for (int k = defHead[j]; k >= 0; k = defNext[k]) if (supp[k]) return true;
  return false;
}

// One replayed greedy round for the whole chip (thread per candidate of the tail list).  Decisions only ever go
// UNDECIDED -> final, and a kernel boundary makes the previous step's decisions visible to every CU, so running this a fixed
// number of times needs no host round trip; whatever is still undecided afterwards (dependency chains longer than that) is
// finished by the single-workgroup loop below.
__global__ void __launch_bounds__(256) k_tail_step(const int* __restrict__ U, int nU, unsigned char* state, const int2* __restrict__ pairs,
                                                   const unsigned char* __restrict__ supp, const unsigned int* __restrict__ segStart,
                                                   const int* __restrict__ segCnt, unsigned long long pairCap,
                                                   const int* __restrict__ defHead, const int* __restrict__ defNext) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nU) return;
  const int j = U[t];
  if (state[j] != ST_UNDECIDED) return;
  bool wait = false, sup = deferred_suppresses(j, defHead, defNext, supp);
  const unsigned int e0 = segStart[t];
  const int c = segCnt[t];
  for (int e = 0; e < c && !sup; ++e) {
    if ((unsigned long long)e0 + e >= pairCap) { wait = true; break; }
    const unsigned char si = state[pairs[e0 + e].x];
    if (si == ST_UNDECIDED) wait = true;
    else if (si == ST_KEPT && supp[e0 + e]) sup = true;
  }
  if (sup) state[j] = ST_SUPPRESSED;
  else if (!wait) state[j] = ST_KEPT;
}
// one workgroup; 'left' receives the number of candidates still undecided (0 unless something is inconsistent)
__global__ void __launch_bounds__(1024) k_tail_resolve(const int* __restrict__ U, int nU, volatile unsigned char* state,
                                                       const int2* __restrict__ pairs, const unsigned char* __restrict__ supp,
                                                       const unsigned int* __restrict__ segStart, const int* __restrict__ segCnt,
                                                       unsigned long long pairCap, int* left, const int* __restrict__ defHead,
                                                       const int* __restrict__ defNext) {
  __shared__ int changed, undecided;
  for (int iter = 0; iter <= nU; ++iter) {
    if (threadIdx.x == 0) { changed = 0; undecided = 0; }
    __syncthreads();
    for (int t = threadIdx.x; t < nU; t += blockDim.x) {
      const int j = U[t];
      if (state[j] != ST_UNDECIDED) continue;
      bool wait = false, sup = deferred_suppresses(j, defHead, defNext, supp);
      const unsigned int e0 = segStart[t];
      const int c = segCnt[t];
      for (int e = 0; e < c && !sup; ++e) {
        if ((unsigned long long)e0 + e >= pairCap) { wait = true; break; }
        const unsigned char si = state[pairs[e0 + e].x];
        if (si == ST_UNDECIDED) wait = true;
        else if (si == ST_KEPT && supp[e0 + e]) sup = true;
      }
      if (sup) { state[j] = ST_SUPPRESSED; changed = 1; }
      else if (!wait) { state[j] = ST_KEPT; changed = 1; }
      else undecided = 1;
    }
    __threadfence_block();
    __syncthreads();
    const int ch = changed, un = undecided;
    __syncthreads();
    if (!un || !ch) { if (threadIdx.x == 0) *left = un; break; }
  }
}

// ---- pair order.  The pair kernel runs one sweep per lane; lanes of a wave that sweep geometrically similar pairs take similar
// control paths (the number of scan-beams and where the second polygon enters are functions of the centre offset).  The pair
// list [first, n) is therefore bucketed by the quantised centre offset (dy major, dx minor) before tier 1: histogram, scan,
// scatter of PAIR INDICES -- the kernels behind it already work on index lists.  Decisions are per pair, so the order (and the
// arbitrary order inside a bucket) cannot change any result.
// state != nullptr (normal rounds: decisions are applied to state[j]): a pair whose j the decision kernel of this round has already
// suppressed through another pair is left out of the work list, as the reference does (`if suppressed[j] continue`) -- a sweep launch lasts
// as long as its busiest wave's lanes take one after the other.  Both kernels apply the same predicate and state does not change between
// them; the count kernel counts the pairs left out (*nSkipped).
__device__ __forceinline__ bool pair_j_suppressed(const unsigned char* __restrict__ state, int2 ij) { return state && state[ij.y] == ST_SUPPRESSED; }
constexpr int PAIR_BUCKETS = 4096;
// key = (local-minima class of the two polygons [nl], dy bin [ny], dx bin [nx]); nl * ny * nx <= PAIR_BUCKETS
struct PairKey { const char* prep; size_t prepStride; float inv; int nl, ny, nx; };
__device__ __forceinline__ int pair_bucket(const float* __restrict__ pts, int2 ij, const PairKey& k) {
  const float dy = pts[2 * ij.y] - pts[2 * ij.x], dx = pts[2 * ij.y + 1] - pts[2 * ij.x + 1];
  int by = (int)((dy * k.inv + 0.5f) * (float)k.ny), bx = (int)((dx * k.inv + 0.5f) * (float)k.nx);
  by = by < 0 ? 0 : (by >= k.ny ? k.ny - 1 : by); bx = bx < 0 ? 0 : (bx >= k.nx ? k.nx - 1 : bx);
  int lm = 0;
  if (k.nl > 1) {                                    // n_lm is the second int of a PolyPrep record (clip_beam.h)
    int a = *(const int*)(k.prep + (size_t)ij.x * k.prepStride + 4), b = *(const int*)(k.prep + (size_t)ij.y * k.prepStride + 4);
    a = a < 1 ? 0 : (a > 4 ? 3 : a - 1); b = b < 1 ? 0 : (b > 4 ? 3 : b - 1);
    lm = (a * 4 + b) % k.nl;
  }
  return (lm * k.ny + by) * k.nx + bx;
}
__global__ void __launch_bounds__(256) k_pair_bucket_count(const int2* __restrict__ pairs, const unsigned long long* __restrict__ nPtr,
                                                           const unsigned int* __restrict__ firstPtr, const float* __restrict__ pts, PairKey key,
                                                           unsigned int* __restrict__ hist, const unsigned char* __restrict__ decided,
                                                           const unsigned char* __restrict__ state, unsigned int* __restrict__ nSkipped) {
  __shared__ unsigned int h[PAIR_BUCKETS];
  __shared__ unsigned int skipped;
  for (int b = threadIdx.x; b < PAIR_BUCKETS; b += 256) h[b] = 0;
  if (threadIdx.x == 0) skipped = 0;
  __syncthreads();
  const unsigned long long n = *nPtr, first = firstPtr ? *firstPtr : 0u;
  for (unsigned long long t = first + (unsigned long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (unsigned long long)gridDim.x * 256) {
    if (decided && decided[t]) continue;
    const int2 ij = pairs[t];
    if (pair_j_suppressed(state, ij)) { atomicAdd(&skipped, 1u); continue; }
    atomicAdd(&h[pair_bucket(pts, ij, key)], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < PAIR_BUCKETS; b += 256) if (h[b]) atomicAdd(&hist[b], h[b]);
  if (threadIdx.x == 0 && skipped) atomicAdd(nSkipped, skipped);
}
__global__ void __launch_bounds__(1024) k_pair_bucket_scan(const unsigned int* __restrict__ hist, unsigned int* __restrict__ cursor,
                                                           unsigned long long* __restrict__ nOrdered) {
  __shared__ unsigned int sh[1024];
  const int t = threadIdx.x;
  unsigned int v[PAIR_BUCKETS / 1024], tot = 0;
#pragma unroll
  for (int k = 0; k < PAIR_BUCKETS / 1024; ++k) { v[k] = hist[t * (PAIR_BUCKETS / 1024) + k]; tot += v[k]; }
  sh[t] = tot;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const unsigned int add = t >= o ? sh[t - o] : 0u;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  unsigned int run = sh[t] - tot;
#pragma unroll
  for (int k = 0; k < PAIR_BUCKETS / 1024; ++k) { cursor[t * (PAIR_BUCKETS / 1024) + k] = run; run += v[k]; }
  if (t == 1023) *nOrdered = sh[t];
}
__global__ void __launch_bounds__(256) k_pair_bucket_scatter(const int2* __restrict__ pairs, const unsigned long long* __restrict__ nPtr,
                                                             const unsigned int* __restrict__ firstPtr, const float* __restrict__ pts, PairKey key,
                                                             unsigned int* __restrict__ cursor, unsigned int* __restrict__ order, unsigned int cap,
                                                             const unsigned char* __restrict__ decided, const unsigned char* __restrict__ state) {
  const unsigned long long n = *nPtr, first = firstPtr ? *firstPtr : 0u;
  for (unsigned long long t = first + (unsigned long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (unsigned long long)gridDim.x * 256) {
    if (decided && decided[t]) continue;
    const int2 ij = pairs[t];
    if (pair_j_suppressed(state, ij)) continue;
    const unsigned int k = atomicAdd(&cursor[pair_bucket(pts, ij, key)], 1u);
    if (k < cap) order[k] = (unsigned int)t;
  }
}

__global__ void k_count_after(unsigned int* out, const unsigned int* total, const unsigned int* first) { *out = *total > *first ? *total - *first : 0u; }

}  // namespace

namespace sd {
// general path (nms2d_full.hip): pairs whose result depends on Clipper's JoinCommonEdges, or that exceed the
// capacities of the bound-slot kernels; device-side queue, result applied directly.
int clip_full_pairs(const int2* d_pairs, const unsigned int* d_idx, const unsigned int* d_n, unsigned int cap, int R, const int* d_vx, const int* d_vy,
                    const float* d_area, float thr, unsigned char* d_state, unsigned char* d_supp, unsigned int* d_errCount, hipStream_t stream);
}

namespace {
struct Counters { int nU, nK, nS, left; unsigned long long nPairs; unsigned int nSpill, nExact, nErr, nDecided, nSkipped; };

// prepared polygons + the two tiers of the bound-slot pair kernel for one vertex capacity
template <int MAXV, int SPREP>
struct BeamPath {
  typedef sdclip::PolyPrep<MAXV> Prep;
  static constexpr size_t prep_stride = sizeof(Prep);
  static constexpr bool two_tiers = MAXV == 32;     // n_rays <= 32: tier 1 in front of tier 2
  // props (n_rays <= 32 only; may be null): the polygon properties of the decision shortcut (area_bounds.h), written by the same pass
  static int prepare(const int* vx, const int* vy, int N, int R, sdarea::PolyProps* props, void* prep, hipStream_t s) {
    if constexpr (MAXV == 32) {                     // n_rays <= 32: the per-polygon pass (poly_pass.h)
      if (sdpass::launch_poly_pass(vx, vy, N, R, props, prep, s)) { sd::set_error("sd_nms2d: launch of the per-polygon pass failed"); return -1; }
      return 0;
    } else {
      const size_t lds = sdclip::PrepWork<sdclip::LdsStorage<SPREP>, MAXV>::lds_bytes() + 64;
      hipLaunchKernelGGL((k_prepare<MAXV, SPREP>), dim3(sd::div_up(N, SPREP)), dim3(SPREP), lds, s, vx, vy, N, R, (Prep*)prep);
      SD_LAUNCH_CHECK();
      return 0;
    }
  }
  // tier 1 (K = 8): all pairs of the round; capacity spills -> q.spill
  static int tier1(const int2* pairs, const unsigned int* idx, const unsigned long long* nPairs, const unsigned int* first, const void* prep, const float* area,
                   float thr, unsigned char* state, unsigned char* supp, PairQueues q, hipStream_t s) {
    // One pair per lane, the pair's whole sweep state in LDS.  The kernel is latency-bound under lane divergence (VALU issue 12.5 % at
    // one wave per SIMD, profiles/r03_pmc_mfma.md) and LDS capacity sets how many pairs a CU has in flight: with 32-bit coordinates and
    // stored slopes a pair takes 636 bytes -> 40.7 KB per wave -> FOUR waves per CU; with 16-bit coordinates relative to the pair's origin
    // and recomputed slopes (LdsStorage16, the default since round 4) 420 bytes -> 26.9 KB -> SIX waves per CU, 1.5x the pairs in flight.
    // Same arithmetic (tests/host/beam_check.cpp: 0 mismatches against Clipper in either form); pairs whose coordinates do not fit 16 bits
    // spill to tier 2.  Option "nms2d_pair_lanes": 64 (default) | 32 (half-filled waves: measured no gain) | 6464 (the 32-bit form).
    const int lanes = sd::option(sd::OPT_NMS2D_PAIR_LANES);
    if (lanes == 32) {
      static const size_t lds32 = beam_lds_bytes<MAXV, 8, 6, 4, 32>();
      hipLaunchKernelGGL((k_pairs_beam<MAXV, 8, 6, 4, 32, unsigned long long>), dim3(256 * 8), dim3(32), lds32, s, pairs, idx, nPairs, first, (const Prep*)prep, area, thr, state, supp, q);
    } else if (lanes == 6464) {
      static const size_t lds = beam_lds_bytes<MAXV, 8, 6, 4, 64>();
      hipLaunchKernelGGL((k_pairs_beam<MAXV, 8, 6, 4, 64, unsigned long long>), dim3(256 * 4), dim3(64), lds, s, pairs, idx, nPairs, first, (const Prep*)prep, area, thr, state, supp, q);
    } else {
      static const size_t lds16 = beam_lds_bytes<MAXV, 8, 6, 4, 64, true>();
      static const int per_cu = (int)((160 * 1024) / lds16);
      hipLaunchKernelGGL((k_pairs_beam<MAXV, 8, 6, 4, 64, unsigned long long, true>), dim3(256 * per_cu), dim3(64), lds16, s, pairs, idx, nPairs, first, (const Prep*)prep, area, thr, state, supp, q);
    }
    SD_LAUNCH_CHECK();
    return 0;
  }
  // tier 2 (K = 15, larger lists): the spills of tier 1 (or, for n_rays > 32, all pairs); its spills -> general path
  template <typename CNT>
  static int tier2(const int2* pairs, const unsigned int* idx, const CNT* nPairs, const unsigned int* first, const void* prep, const float* area, float thr,
                   unsigned char* state, unsigned char* supp, PairQueues q, hipStream_t s) {
    static const size_t lds = beam_lds_bytes<MAXV, 15, 16, 8, 32>();
    hipLaunchKernelGGL((k_pairs_beam<MAXV, 15, 16, 8, 32, CNT>), dim3(256 * 3), dim3(32), lds, s, pairs, idx, nPairs, first, (const Prep*)prep, area, thr, state, supp, q);
    SD_LAUNCH_CHECK();
    return 0;
  }
};
// The one place that maps a ray count to its vertex capacity: f(BeamPath<...>{}) -> int
template <class F>
int with_beam_path(int R, F&& f) {
  if (R <= 32) return f(BeamPath<32, 64>{});
  if (R <= 64) return f(BeamPath<64, 64>{});
  if (R <= 128) return f(BeamPath<128, 32>{});
  return f(BeamPath<256, 16>{});
}
size_t prep_stride(int R) { return (size_t)with_beam_path(R, [](auto bp) { return (int)decltype(bp)::prep_stride; }); }
int prepare_polys(const int* vx, const int* vy, int N, int R, sdarea::PolyProps* props, void* prep, hipStream_t s) {
  return with_beam_path(R, [&](auto bp) { return decltype(bp)::prepare(vx, vy, N, R, props, prep, s); });
}

// What one sweep of the pair kernels works on: the polygons, the pair list, the two queues behind the tiers and where the decisions go
// (supp == nullptr: a suppressing pair marks state[j]; else supp[pair index] = 1)
struct Sweep {
  hipStream_t s; int R; const int *vx, *vy; const void* prep; const float* area; float thr;
  const int2* pairs; unsigned int *spillPairs, *exactPairs, qCap; Counters* d_cnt; unsigned char *state, *supp;
};
int general_path(const Sweep& w) {
  return sd::clip_full_pairs(w.pairs, w.exactPairs, &w.d_cnt->nExact, w.qCap, w.R, w.vx, w.vy, w.area, w.thr, w.state, w.supp, &w.d_cnt->nErr, w.s);
}
// The sweep sequence of both drivers over pairs[idx[*first .. *n)] (idx, first: may be null): tier 1 (n_rays <= 32 only; capacity spills
// -> q1.spill) -> tier 2 (what it cannot hold -> the general-path queue) -> general(): the general path over that queue, or what the caller
// does with it instead.  pairTimer stops behind the first tier that runs.
template <class General>
int sweep_tiers(const Sweep& w, const unsigned int* idx, const unsigned long long* n, const unsigned int* first, Timer& pairTimer, General general) {
  const PairQueues q1{w.spillPairs, &w.d_cnt->nSpill, w.exactPairs, &w.d_cnt->nExact, w.qCap};
  const PairQueues q2{w.exactPairs, &w.d_cnt->nExact, w.exactPairs, &w.d_cnt->nExact, w.qCap};   // what tier 2 cannot hold goes to the general path
  const int rc = with_beam_path(w.R, [&](auto bp) -> int {
    typedef decltype(bp) BP;
    if constexpr (BP::two_tiers) {
      if (BP::tier1(w.pairs, idx, n, first, w.prep, w.area, w.thr, w.state, w.supp, q1, w.s) || pairTimer.stop(w.s)) return -1;
      return BP::tier2(w.pairs, w.spillPairs, &w.d_cnt->nSpill, (const unsigned int*)nullptr, w.prep, w.area, w.thr, w.state, w.supp, q2, w.s);
    } else {
      if (BP::tier2(w.pairs, idx, n, first, w.prep, w.area, w.thr, w.state, w.supp, q2, w.s)) return -1;
      return pairTimer.stop(w.s);
    }
  });
  return rc ? -1 : general();
}
// the host's look at the counters a sweep left; who: the driver's prefix in messages, listOverflow: the caller's own pair list overflowed
int check_sweep(const char* who, const Counters& h, unsigned int qCap, bool listOverflow, const char* alsoCounted) {
  if (listOverflow || h.nSpill > qCap || h.nExact > qCap) { sd::set_error("%s: pair queue overflow (internal error)", who); return -1; }
  if (h.nErr) { sd::set_error("%s: %u pairs exceeded the general path's fixed capacities%s", who, h.nErr, alsoCounted); return -1; }
  return 0;
}

// The build step of sd_nms2d_device and of its probe sd_nms2d_build_device: the table of ray directions (host libm: the device never
// evaluates sinf / cosf; stardist2d.cpp:419,454-455) and the initial gstats in ONE block and one copy -- every copy or fill command in front
// of the neighbour lists costs 3-6 us and a gap on the critical path -- then k_build32 (n_rays <= 32) or k_build.  *gstatsOut: 8 ints.
int launch_build(sd::Arena& A, hipStream_t s, const float* d_dist, const float* d_points, int N, int R, int* vx, int* vy, int4* bbox,
                 float* radius, float* area, int** gstatsOut, hipEvent_t evStart) {
  const int gs_init[8] = {0, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, 0, 0, 0};
  std::vector<float> hdr(8 + 2 * (size_t)R);
  memcpy(hdr.data(), gs_init, sizeof(gs_init));
  const float ANGLE_PI = 2 * M_PI / R;
  for (int k = 0; k < R; ++k) { hdr[8 + 2 * k] = sinf(ANGLE_PI * k); hdr[8 + 2 * k + 1] = cosf(ANGLE_PI * k); }
  int* gstats = A.take_n<int>(8 + 2 * (size_t)R);
  if (!gstats) return -1;
  const float2* d_sc = (const float2*)(gstats + 8);
  SD_CHECK(hipMemcpyAsync(gstats, hdr.data(), hdr.size() * sizeof(float), hipMemcpyHostToDevice, s));
  if (evStart) SD_CHECK(hipEventRecord(evStart, s));
  if (R <= 32) {
    const int vec4 = ((((uintptr_t)d_dist | (uintptr_t)vx | (uintptr_t)vy) & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(k_build32, dim3(sd::div_up(N, 64)), dim3(64), 2 * 64 * (size_t)R * sizeof(int), s, d_dist, d_points, d_sc, N, R, vec4,
                       vx, vy, bbox, radius, area, gstats);
  } else
    hipLaunchKernelGGL(k_build, dim3(sd::div_up(N, 4)), dim3(256), 4 * 2 * R * sizeof(int), s, d_dist, d_points, d_sc, N, R,
                       vx, vy, bbox, radius, area, gstats);
  SD_LAUNCH_CHECK();
  *gstatsOut = gstats;
  return 0;
}
}  // namespace

extern "C" int sd_nms2d_build_device(const float* d_dist, const float* d_points, int n_polys, int n_rays, int32_t* d_vx, int32_t* d_vy,
                                     int32_t* d_bbox, float* d_radius, float* d_area, int32_t* d_gstats, void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (n_polys <= 0) return 0;
  if (n_rays < 1 || n_rays > 256) { sd::set_error("sd_nms2d_build: n_rays=%d unsupported (1..256)", n_rays); return -1; }
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  int* gstats = nullptr;
  if (launch_build(A, s, d_dist, d_points, n_polys, n_rays, d_vx, d_vy, (int4*)d_bbox, d_radius, d_area, &gstats, nullptr)) return -1;
  SD_CHECK(hipMemcpyAsync(d_gstats, gstats, 5 * sizeof(int), hipMemcpyDeviceToDevice, s));
  SD_CHECK(hipStreamSynchronize(s));
  return 0;
}

namespace {
// the two events the helper stream records behind the per-polygon work; the caller's stream waits for them at different points
struct SideEvents {
  hipEvent_t props = nullptr, prep = nullptr;
  ~SideEvents() { if (props) (void)hipEventDestroy(props); if (prep) (void)hipEventDestroy(prep); }
  int init() { SD_CHECK(hipEventCreateWithFlags(&props, hipEventDisableTiming)); SD_CHECK(hipEventCreateWithFlags(&prep, hipEventDisableTiming)); return 0; }
};

// One call of sd_nms2d_device: what its phases hand to each other.  Every phase returns 0 or -1 (error set).
struct Nms2d {
  // the call
  hipStream_t s; const float *dist, *pts; int N, R, use_kdtree, use_bbox; float thr; bool wantStats; sd::Arena& A;
  // plan: options and tuning knobs, the helper stream and its events, the times of the statistics (events on the caller's stream)
  bool areaBounds = false, singlePass = false, ordered = false, decide = false, deferOn = false, trace = false;
  int tailT = -1, deferFrom = 0, keyMode = 2; unsigned int deferMax = 0;
  hipStream_t side = nullptr; sd::SideJoin sideJoin; SideEvents sideEv;
  Timer broadTimer, pairTimer, fullTimer, replayTimer;
  double ns_pairs = 0, ns_full = 0, ns_pre = 0; long long n_pair_launches = 0;
  // build: per candidate the integer vertices and what k_build derives from them; gstats: max_dist bits, extent of the centres; the
  // prepared polygons and the properties of the decision shortcut (written by fork_side)
  int *vx = nullptr, *vy = nullptr, *candCell = nullptr, *gstats = nullptr; int4* bbox = nullptr; float *radius = nullptr, *area = nullptr;
  unsigned char* state = nullptr; void* prep = nullptr; size_t prepStride = 0; sdarea::PolyProps* props = nullptr;
  // build_grid: the cell table, the storage of the list builder, the work list of round 1 and the deferred pairs' per-candidate arrays
  GridP g; NmsFlags f; float max_dist = 0, reach = 0;
  int by_bbox = 0, *cellStart = nullptr, *nbrCount = nullptr, *nbrLow = nullptr, *Ucur = nullptr; i64* nbrStart = nullptr; CellRec* cellRec = nullptr;
  void* scanTmp = nullptr; size_t scanBytes = 0; Deferred dfr{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
  // build_lists; totalNbr: ordered neighbour relations (the lists hold each unordered pair once, at its worse-scored end)
  NbrLists L{}; i64 totalNbr = 0;
  // begin_rounds: pair list, queues, counters, deferral storage
  unsigned long long pairCap = 0, *nOrdered = nullptr; int2* pairs = nullptr; unsigned char *decided = nullptr, *defKind = nullptr;
  unsigned int qCap = 0, *spillPairs = nullptr, *exactPairs = nullptr, *pairOrder = nullptr, *bucketHist = nullptr, *firstNew = nullptr, *nNewExact = nullptr, *nJoinDef = nullptr;
  int *Unext = nullptr, *K = nullptr, *Sl = nullptr, decideGrid = 0; Counters *d_cnt = nullptr, h;
  // the rounds; nDeferred: general-path pairs deferred so far; nUndecDeferredUpper: upper bound of the kind-1 deferred pairs so far (those
  // whose j was suppressed meanwhile are skipped); totalDecided: pairs decided by the area enclosure; totalSkipped: pairs not swept
  // because j was suppressed meanwhile
  int nU = 0, rounds = 0; bool forceTail = false;
  i64 nDeferred = 0, nUndecDeferredUpper = 0, totalPairs = 0, totalExact = 0, totalSpill = 0, totalUndecDeferred = 0, totalDecided = 0, totalSkipped = 0;
  // tail_batch (taken on first use)
  unsigned char* supp = nullptr; unsigned int* segStart = nullptr; int* segCnt = nullptr;

  Nms2d(hipStream_t s_, const float* dist_, const float* pts_, int N_, int R_, int use_kdtree_, int use_bbox_, float thr_, bool wantStats_)
      : s(s_), dist(dist_), pts(pts_), N(N_), R(R_), use_kdtree(use_kdtree_), use_bbox(use_bbox_), thr(thr_), wantStats(wantStats_), A(sd::arena()) {}

  // validation, options and tuning knobs (read once); begins the arena pass
  int plan() {
    if (R < 1 || R > 256) { sd::set_error("sd_nms2d: n_rays=%d unsupported (1..256)", R); return -1; }
    if (A.begin(s)) return -1;
    if (wantStats && (broadTimer.init() || pairTimer.init() || fullTimer.init())) return -1;
    trace = wantStats && sd::option(sd::OPT_TRACE) != 0;
    // polygon properties of the decision shortcut (area_bounds.h)
    areaBounds = R <= 32 && R >= 3 && sd::option(sd::OPT_NMS2D_AREA_BOUNDS) != 0 && sd::option(sd::OPT_NMS2D_STRICT) == 0;
    // Neighbour lists in ONE pass (option "nms2d_neighbours_single_pass", default 1): every candidate gets a slot as large as the population
    // of the cells its list is built from (known from the cell table: no candidate test needed), the lists -- the better-scored neighbours
    // only -- are written into the slots from their front and the exact total is counted on the way.  The two-pass form
    // (count, scan, fill: every candidate test done twice, 1.2 + 0.8 ms at 2048^2) remains for inputs whose slots would exceed 32-bit indices or the workspace.
    singlePass = sd::option(sd::OPT_NMS2D_NBR_SINGLE) != 0;
    // pair order (see k_pair_bucket_*): SD_NMS_PAIR_SORT=0 keeps emission order
    static const bool pairSort = sd::tuning_env("SD_NMS_PAIR_SORT", 1) != 0;
    static const int pairKey = sd::tuning_env("SD_NMS_PAIR_KEY", 2);
    ordered = pairSort && R <= 32;
    keyMode = pairKey;
    decide = areaBounds && ordered;             // (the shortcut filters through the ordered index list)
    // tail batch threshold: undecided candidates at or below which the remaining rounds are replayed on the device
    static const int tailDiv = sd::tuning_env("SD_NMS_TAIL_DIV", 6);
    static const int tailMax = sd::tuning_env("SD_NMS_TAIL_MAX", 65536);
    tailT = tailDiv > 0 ? ((N / tailDiv) < tailMax ? (N / tailDiv) : tailMax) : -1;
    // deferral of the general path to the tail batch (only with a tail batch to run it in)
    static const bool deferEnv = sd::tuning_env("SD_NMS_DEFER", 1) != 0;
    deferOn = tailT >= 0 && deferEnv;
    // deferral of the enclosure's undecided pairs (see k_defer_undecided): from round 2 on by default (option nms2d_defer_undecided)
    deferFrom = (deferOn && decide) ? sd::option(sd::OPT_NMS2D_DEFER_UNDECIDED) : 0;
    deferMax = (unsigned int)(sd::option(sd::OPT_NMS2D_DEFER_MAX) > 0 ? sd::option(sd::OPT_NMS2D_DEFER_MAX) : 0);
    side = sd::side_stream();
    if (!side || sideEv.init()) return -1;
    return 0;
  }

  // per candidate: integer vertices, bounding box, radius, area; the extent of the centres (launch_build); starts the broad-phase time
  int build() {
    vx = A.take_n<int>((size_t)N * R);
    vy = A.take_n<int>((size_t)N * R);
    bbox = A.take_n<int4>(N);
    radius = A.take_n<float>(N);
    area = A.take_n<float>(N);
    state = A.take_n<unsigned char>(N);
    candCell = A.take_n<int>(N);
    prepStride = prep_stride(R);
    prep = A.take((size_t)N * prepStride);
    if (areaBounds) props = (sdarea::PolyProps*)A.take((size_t)N * sizeof(sdarea::PolyProps));
    if (!vx || !vy || !bbox || !radius || !area || !state || !candCell || !prep || (areaBounds && !props)) return -1;
    return launch_build(A, s, dist, pts, N, R, vx, vy, bbox, radius, area, &gstats, broadTimer.a);
  }

  // ---- prepared polygons (Clipper::AddPath once per candidate), on a second stream: they depend on the integer vertices only, the
  // grid and the neighbour lists that follow on the caller's stream do not need them (0.84 ms of independent work at 2048^2).
  // The polygon properties of the decision shortcut with them: they also depend on the integer vertices only, and the decision kernel of
  // the first round needs them before any sweep needs a prepared polygon (sideEv.props / sideEv.prep).
  // The helper stream's work is enqueued once the LAST read-back of the grid set-up is behind us (build_neighbour_lists calls this): it
  // fills every wave slot of the chip, and an 8-byte device -> host copy of the caller's stream issued while it runs waits for a slot
  // until it drains (measured: 0.69 ms for that copy, the neighbour-list kernel started 0.7 ms late; profiles/r05_step_timeline_2d.txt).
  // n_rays <= 32: ONE pass writes the properties and the prepared polygons (poly_pass.h); more rays: k_prepare alone (no shortcut).
  int fork_side() {
    if (sideJoin.begin(s, side) || prepare_polys(vx, vy, N, R, props, prep, side)) return -1;
    SD_CHECK(hipEventRecord(sideEv.props, side));
    SD_CHECK(hipEventRecord(sideEv.prep, side));
    return 0;
  }

  // ---- uniform grid: cell size from the largest radius, cell table, the slot capacities of the single-pass lists
  int build_grid() {
    int gs[8];
    SD_CHECK(hipMemcpyAsync(gs, gstats, sizeof(gs), hipMemcpyDeviceToHost, s));
    SD_CHECK(hipStreamSynchronize(s));
    memcpy(&max_dist, &gs[0], 4);
    // cells of HALF the reach (max_dist + 1): a candidate's window (cell_window: its bounding box grown by the reach) then spans at most
    // (2 (max_dist + 1) + 2 (max_dist + 1)) / cs + 2 = 10 rows; a grid that would exceed 2^26 cells gets coarser cells (fewer rows still)
    reach = (max_dist + 1.f) * 1.0001f + 1e-3f;
    by_bbox = (thr >= 0.f || use_bbox) ? 1 : 0;
    float cs = 0.5f * reach;
    if (!(cs >= 1.f)) cs = 1.f;
    for (;;) {
      g.ny = (int)(((double)gs[2] - gs[1]) / cs) + 1;
      g.nx = (int)(((double)gs[4] - gs[3]) / cs) + 1;
      if ((long long)g.ny * g.nx <= (1ll << 26)) break;
      cs *= 2.f;
    }
    g.y0 = (float)gs[1]; g.x0 = (float)gs[3]; g.inv_cs = 1.f / cs;
    const int nCells = g.ny * g.nx;
    int* cellCount = A.take_n<int>(2 * ((size_t)nCells + 1));          // the two arrays that start at zero in one block: one fill
    int* cellFill = cellCount ? cellCount + nCells + 1 : nullptr;
    cellStart = A.take_n<int>(nCells + 1);
    cellRec = (CellRec*)A.take((size_t)N * sizeof(CellRec));
    nbrCount = A.take_n<int>(N + 1);
    nbrStart = A.take_n<i64>(N + 1);
    nbrLow = A.take_n<int>(N + 1);
    if (!cellCount || !cellStart || !cellRec || !nbrCount || !nbrStart || !nbrLow) return -1;
    SD_CHECK(hipMemsetAsync(cellCount, 0, 2 * ((size_t)nCells + 1) * sizeof(int), s));
    hipLaunchKernelGGL(k_cell_count, dim3(sd::div_up(N, 256)), dim3(256), 0, s, pts, N, g, cellCount, candCell);
    SD_LAUNCH_CHECK();
    size_t scanBytes2 = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scanBytes, cellCount, cellStart, nCells + 1, s);
    (void)exclusive_sum_i64(nullptr, scanBytes2, nbrCount, nbrStart, N + 1, s);
    if (scanBytes2 > scanBytes) scanBytes = scanBytes2;
    scanTmp = A.take(scanBytes + 256);
    if (!scanTmp) return -1;
    SD_CHECK(hipcub::DeviceScan::ExclusiveSum(scanTmp, scanBytes, cellCount, cellStart, nCells + 1, s));
    // (k_cell_fill writes every slot capacity and the closing zero; the two-pass form clears nbrCount itself)
    hipLaunchKernelGGL(k_cell_fill, dim3(sd::div_up(N, 256)), dim3(256), 0, s, N, candCell, cellStart, cellFill, pts, bbox, area, cellRec, g, by_bbox, reach,
                       (singlePass || wantStats) ? nbrCount : (int*)nullptr);      // (the statistics report the slot total of either form)
    SD_LAUNCH_CHECK();
    // The N-sized work lists of the greedy rounds are set up HERE, in front of the neighbour lists: behind the read-back of the list total
    // their four small launches sat on the critical path in front of round 1 (~60 us of 5-us kernels and gaps)
    Ucur = A.take_n<int>(N);
    dfr.pend = A.take_n<unsigned char>(N);
    dfr.head = A.take_n<int>(N);
    dfr.count = A.take_n<unsigned int>(1);
    if (!Ucur || !dfr.pend || !dfr.head || !dfr.count) return -1;
    hipLaunchKernelGGL(k_round_lists_init, dim3(sd::div_up(N, 256)), dim3(256), 0, s, N, Ucur, state, dfr.pend, dfr.head, dfr.count);
    f.use_kdtree = use_kdtree; f.use_bbox = use_bbox; f.thr_nonneg = (thr >= 0.f); f.thr = thr; f.max_dist = max_dist;
    return 0;
  }

  // ---- neighbour CSR (build_neighbour_lists, nms_rounds.h), the helper stream's work forked from inside it; ends the broad-phase time
  int build_lists() {
    const int nbBlocks = (sd::div_up(N, 4) + 7) & ~7;
    L.count = nbrCount; L.low = nbrLow; L.start = nbrStart; L.lowOnly = true; L.wantSlotTotal = wantStats;
    auto launch_neighbours = [&](int mode, const NbrLists& l) {      // (the counting pass gets no lists)
      auto go = [&](auto kern, const i64* start, int* nbr, int* waitOn) {
        hipLaunchKernelGGL(kern, dim3(nbBlocks), dim3(256), 0, s, N, g, f, cellRec, cellStart, nbrCount, nbrLow, start, nbr, waitOn, by_bbox, reach);
      };
      if (mode == 0) go(k_neighbours<0>, nullptr, nullptr, nullptr);
      else if (mode == 1) go(k_neighbours<1>, nbrStart, l.nbr, l.waitOn);
      else go(k_neighbours<2>, nbrStart, l.nbr, l.waitOn);
    };
    const int rc = build_neighbour_lists(A, s, N, singlePass, scanTmp, scanBytes, launch_neighbours, [&]() { return fork_side(); }, L);
    // capacity of one call: neighbour lists and pair queues are indexed with 32 bits.  Beyond it (about 13 M candidates at the density
    // of the 2048^2 bench set) the input has to be sharded -- predict_instances_sharded / predict_instances_big do exactly that.
    if (rc > 0)
      sd::set_error("sd_nms2d: %lld neighbour entries for %d candidates exceed the capacity of one call (2^31 - 1): shard the input "
                    "(predict_instances_sharded / predict_instances_big)", (long long)L.total, N);
    if (rc) return -1;
    totalNbr = 2 * L.total;
    // (the prepared polygons are being written on the side stream meanwhile; the sweep kernels are their first readers and wait for
    // sideEv.prep in sweep_pairs -- with the shortcut on, the decision kernel of round 1 runs before that and only needs the properties)
    SD_CHECK(hipStreamWaitEvent(s, sideEv.props, 0));
    float ms = 0;
    if (broadTimer.stop(s) || broadTimer.wait() || broadTimer.ms(&ms)) return -1;
    ns_pre = ms * 1e6;
    return 0;
  }

  // ---- greedy rounds: every kernel of a round takes its work-list length from device memory; ONE host round trip per
  // round (the undecided / survivor counts that end the loop)
  int begin_rounds() {
    pairCap = (unsigned long long)(totalNbr / 2 + 64);
    qCap = (unsigned int)(pairCap < (1ull << 30) ? pairCap : (1ull << 30));
    Unext = A.take_n<int>(N);
    K = A.take_n<int>(N);
    pairs = A.take_n<int2>(pairCap);
    spillPairs = A.take_n<unsigned int>(qCap);
    exactPairs = A.take_n<unsigned int>(qCap);
    Sl = A.take_n<int>(N);
    d_cnt = (Counters*)A.take(sizeof(Counters));
    if (ordered) pairOrder = A.take_n<unsigned int>(qCap);
    bucketHist = A.take_n<unsigned int>(2 * PAIR_BUCKETS);
    nOrdered = A.take_n<unsigned long long>(1);
    if (decide) decided = A.take_n<unsigned char>(pairCap);
    firstNew = A.take_n<unsigned int>(1);
    nNewExact = A.take_n<unsigned int>(1);
    if (!Unext || !K || !pairs || !spillPairs || !exactPairs || !Sl || !d_cnt || !bucketHist || !nOrdered || !firstNew || !nNewExact || (ordered && !pairOrder) ||
        (decide && !decided)) return -1;
    static int decideGridOf[sd::kMaxDevices] = {};
    decideGrid = decide ? sd::resident_grid((const void*)k_pairs_decide, 256, decideGridOf) : 0;   // every launched wave resident, equal work
    if (decide && decideGrid <= 0) return -1;
    dfr.cap = qCap;
    if (deferOn) {
      dfr.pairs = A.take_n<int2>(qCap);
      dfr.next = A.take_n<int>(qCap);
      if (!dfr.pairs || !dfr.next) return -1;
    }
    if (deferFrom > 0) {
      defKind = A.take_n<unsigned char>(qCap); nJoinDef = A.take_n<unsigned int>(1);
      if (!defKind || !nJoinDef) return -1;
      SD_CHECK(hipMemsetAsync(defKind, 0, qCap, s));
    }
    nU = N;
    return 0;
  }

  // The ordered-pair path in front of a sweep (n_rays <= 32): the decision shortcut, the deferral of what it leaves undecided, and the
  // offset-ordered index list of the pairs that remain (pairOrder[0 .. *nOrdered)).
  int order_pairs(unsigned char* suppOut, const unsigned int* first) {
    // measured on the 2048^2 bench set (pair kernels incl. the bucketing, ms): emission order 9.9 | 32x32 7.85 | 64x16 7.38 | 64x64 6.70 |
    // 16 local-minima classes x 16x16 8.53: resolution of the offset is what counts (64x64 = whole pixels at radius 10)
    static const int modes[6][3] = {{1, 32, 32}, {1, 64, 16}, {1, 64, 64}, {16, 16, 16}, {16, 32, 8}, {4, 32, 32}};
    const int* md = modes[keyMode >= 0 && keyMode < 6 ? keyMode : 2];
    const PairKey key{(const char*)prep, prepStride, 1.f / (4.f * (max_dist + 1.f)), md[0], md[1], md[2]};   // offsets lie in (-2 max_dist, 2 max_dist)
    SD_CHECK(hipMemsetAsync(bucketHist, 0, PAIR_BUCKETS * sizeof(unsigned int), s));
    if (decided)
      hipLaunchKernelGGL(k_pairs_decide, dim3(decideGrid), dim3(256), 0, s, pairs, &d_cnt->nPairs, first, vx, vy, R, props, area, thr, state, suppOut,
                         decided, &d_cnt->nDecided);
    if (!suppOut && deferFrom > 0 && rounds >= deferFrom)      // few undecided pairs: they wait for the tail batch's sweep launch
      hipLaunchKernelGGL(k_defer_undecided, dim3(256), dim3(256), 0, s, pairs, &d_cnt->nPairs, &d_cnt->nDecided, deferMax, decided, state, dfr, defKind, &d_cnt->nErr);
    // tail batch with deferred undecided pairs: they sit in the list's prefix with decided[] = 0 and are bucketed with the rest
    const unsigned int* bfirst = (suppOut && deferFrom > 0) ? nullptr : first;
    SD_CHECK(hipStreamWaitEvent(s, sideEv.prep, 0));          // the prepared polygons (side stream; complete long before, except in round 1)
    const unsigned char* liveState = suppOut ? nullptr : state;      // normal round: pairs whose j is suppressed by now are not swept
    hipLaunchKernelGGL(k_pair_bucket_count, dim3(512), dim3(256), 0, s, pairs, &d_cnt->nPairs, bfirst, pts, key, bucketHist, decided, liveState,
                       &d_cnt->nSkipped);
    hipLaunchKernelGGL(k_pair_bucket_scan, dim3(1), dim3(1024), 0, s, bucketHist, bucketHist + PAIR_BUCKETS, nOrdered);
    hipLaunchKernelGGL(k_pair_bucket_scatter, dim3(512), dim3(256), 0, s, pairs, &d_cnt->nPairs, bfirst, pts, key, bucketHist + PAIR_BUCKETS,
                       pairOrder, qCap, decided, liveState);
    SD_LAUNCH_CHECK();
    return 0;
  }

  // one beam-path pass over the current pair list (tier 1, tier 2, then the general path -- or its deferral); suppOut == nullptr
  // applies decisions to state (normal round), else records them per pair (tail batch, whose first *firstNew entries are the
  // deferred pairs, already queued for the general path)
  int sweep_pairs(unsigned char* suppOut) {
    const unsigned int* first = suppOut ? firstNew : nullptr;
    if (pairTimer.start(s)) return -1;
    if (!ordered) SD_CHECK(hipStreamWaitEvent(s, sideEv.prep, 0));
    else if (order_pairs(suppOut, first)) return -1;
    const Sweep w{s, R, vx, vy, prep, area, thr, pairs, spillPairs, exactPairs, qCap, d_cnt, state, suppOut};
    auto general = [&]() -> int {
      if (fullTimer.start(s)) return -1;
      if (!suppOut && deferOn) {
        hipLaunchKernelGGL(k_defer, dim3(64), dim3(256), 0, s, pairs, exactPairs, &d_cnt->nExact, qCap, dfr, &d_cnt->nErr);
        SD_LAUNCH_CHECK();
      } else if (suppOut && sideJoin.pending) {
        // tail batch: the deferred pairs (the first nDeferred queue entries) are being evaluated on the helper stream since the batch
        // began; here only what the two tiers added behind them, then join
        hipLaunchKernelGGL(k_count_after, dim3(1), dim3(1), 0, s, nNewExact, &d_cnt->nExact, deferFrom > 0 ? nJoinDef : firstNew);
        SD_LAUNCH_CHECK();
        if (sd::clip_full_pairs(pairs, exactPairs + nDeferred, nNewExact, qCap - (unsigned int)nDeferred, R, vx, vy, area, thr, state, suppOut, &d_cnt->nErr, s)) return -1;
        if (sideJoin.join(s)) return -1;
      } else if (general_path(w)) return -1;
      return fullTimer.stop(s);
    };
    if (ordered) return sweep_tiers(w, pairOrder, nOrdered, nullptr, pairTimer, general);
    return sweep_tiers(w, nullptr, &d_cnt->nPairs, first, pairTimer, general);
  }

  // the counters of a round or of the tail batch, read back: refuse overflows, add to the totals and the times
  int account(const char* what) {
    if (check_sweep("sd_nms2d", h, qCap, h.nPairs > pairCap,
                    " or the deferred-pair list (with more than 64 rays: at least that many; the launch stops at the first)")) return -1;
    totalPairs += (i64)h.nPairs; totalExact += h.nExact; totalSpill += h.nSpill; totalDecided += h.nDecided; totalSkipped += h.nSkipped;
    if (wantStats) {
      float ms = 0, ms2 = 0;
      if (pairTimer.ms(&ms) || fullTimer.ms(&ms2)) return -1;
      if (h.nPairs) { ns_pairs += ms * 1e6; ++n_pair_launches; }
      ns_full += ms2 * 1e6;
      if (trace) printf("%s %d: nU=%d nK=%d pairs=%llu decided by the area enclosure=%u j already suppressed=%u spill=%u exact=%u pair_kernel=%.3f ms general_path=%.3f ms\n", what, rounds, h.nU, h.nK, h.nPairs, h.nDecided, h.nSkipped, h.nSpill, h.nExact, ms, ms2);
    }
    return 0;
  }

  // one greedy round: triage and list scan of the undecided, the new survivors' pairs, their sweep -- or, once few enough candidates
  // are left (or all of them wait for deferred pairs), the tail batch
  int run_round() {
    ++rounds;
    if (tailT >= 0 && ((nU <= tailT && rounds > 1) || forceTail)) return tail_batch();
    SD_CHECK(hipMemsetAsync(d_cnt, 0, sizeof(Counters), s));
    hipLaunchKernelGGL(k_round_triage, dim3(sd::div_up(nU, 1024)), dim3(1024), 0, s, Ucur, nU, state, L.waitOn, Unext, K, Sl, (int*)d_cnt, dfr.pend);
    const int wgrid = sd::div_up(nU, 4) < 2048 ? sd::div_up(nU, 4) : 2048;
    hipLaunchKernelGGL(k_round_scan, dim3(wgrid), dim3(256), 0, s, Sl, state, nbrStart, nbrLow, L.nbr, L.waitOn, Unext, K, (int*)d_cnt, dfr.pend);
    hipLaunchKernelGGL(k_round_emit, dim3(wgrid), dim3(256), 0, s, K, &d_cnt->nK, state, g, cellRec, cellStart, by_bbox, reach, f, pts, bbox,
                       radius, area, pairs, &d_cnt->nPairs, pairCap);
    SD_LAUNCH_CHECK();
    if (sweep_pairs(nullptr)) return -1;
    SD_CHECK(hipMemcpyAsync(&h, d_cnt, sizeof(Counters), hipMemcpyDeviceToHost, s));
    SD_CHECK(hipStreamSynchronize(s));
    if (h.nK == 0 && h.nU > 0) {
      if (deferOn && (nDeferred > 0 || nUndecDeferredUpper > 0) && !forceTail) forceTail = true;      // everything left waits on deferred pairs: run the tail batch now
      else { sd::set_error("sd_nms2d: greedy scan made no progress (internal error)"); return -1; }
    }
    if (deferOn) nDeferred += h.nExact;
    if (deferFrom > 0 && rounds >= deferFrom && h.nPairs > h.nDecided && h.nPairs - h.nDecided <= deferMax) nUndecDeferredUpper += (i64)(h.nPairs - h.nDecided);
    if (account("round")) return -1;
    nU = h.nU;
    int* t = Ucur; Ucur = Unext; Unext = t;
    return 0;
  }

  // ---- tail batch: every remaining (undecided, undecided) pair at once, then the greedy rounds replayed on the device; ends the rounds
  int tail_batch() {
    if (!supp) { supp = A.take_n<unsigned char>(pairCap); segStart = A.take_n<unsigned int>(N); segCnt = A.take_n<int>(N); }
    if (!supp || !segStart || !segCnt) return -1;
    SD_CHECK(hipMemsetAsync(d_cnt, 0, sizeof(Counters), s));
    SD_CHECK(hipMemsetAsync(supp, 0, pairCap, s));
    if (deferFrom > 0) {
      hipLaunchKernelGGL(k_tail_init2, dim3(64), dim3(256), 0, s, dfr, defKind, pairs, exactPairs, &d_cnt->nPairs, &d_cnt->nExact, firstNew, decided, state,
                         &d_cnt->nSkipped);
      hipLaunchKernelGGL(k_copy_u32, dim3(1), dim3(1), 0, s, nJoinDef, &d_cnt->nExact);
    } else
      hipLaunchKernelGGL(k_tail_init, dim3(64), dim3(256), 0, s, dfr, pairs, exactPairs, &d_cnt->nPairs, &d_cnt->nExact, firstNew);
    // The deferred pairs all need the general path (a latency-bound launch of ~1 ms over a few thousand pairs, a fraction of the
    // chip): it starts NOW on the helper stream, next to the emission of the remaining pairs and the two bound-slot tiers; decisions
    // are recorded per pair (supp[]), so the two streams write disjoint bytes.  Joined in sweep_pairs.
    if (deferOn && nDeferred > 0 && nDeferred < (i64)qCap) {
      if (sideJoin.begin(s, side)) return -1;
      if (sd::clip_full_pairs(pairs, exactPairs, deferFrom > 0 ? nJoinDef : firstNew, qCap, R, vx, vy, area, thr, state, supp, &d_cnt->nErr, side)) return -1;
      if (sideJoin.end(side)) return -1;
    }
    const int wg = sd::div_up(nU, 4) < 2048 ? sd::div_up(nU, 4) : 2048;
    hipLaunchKernelGGL(k_tail_emit, dim3(wg), dim3(256), 0, s, Ucur, nU, state, nbrStart, nbrLow, L.nbr, f, pts, bbox, radius, area, pairs,
                       &d_cnt->nPairs, pairCap, segStart, segCnt);
    SD_LAUNCH_CHECK();
    if (sweep_pairs(supp)) return -1;
    if (trace && (replayTimer.init() || replayTimer.start(s))) return -1;
    for (int it = 0; it < 10; ++it)
      hipLaunchKernelGGL(k_tail_step, dim3(sd::div_up(nU, 256)), dim3(256), 0, s, Ucur, nU, state, pairs, supp, segStart, segCnt, pairCap, dfr.head, dfr.next);
    hipLaunchKernelGGL(k_tail_resolve, dim3(1), dim3(1024), 0, s, Ucur, nU, state, pairs, supp, segStart, segCnt, pairCap, &d_cnt->left, dfr.head, dfr.next);
    SD_LAUNCH_CHECK();
    if (trace) {
      float ms = 0;
      if (replayTimer.stop(s) || replayTimer.wait() || replayTimer.ms(&ms)) return -1;
      printf("tail replay (10 steps + resolve loop): %.3f ms\n", ms);
    }
    unsigned int hDefTotal = (unsigned int)nDeferred;      // all deferred pairs, the undecided ones included
    SD_CHECK(hipMemcpyAsync(&h, d_cnt, sizeof(Counters), hipMemcpyDeviceToHost, s));
    if (deferFrom > 0) SD_CHECK(hipMemcpyAsync(&hDefTotal, dfr.count, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    SD_CHECK(hipStreamSynchronize(s));
    h.nU = nU; h.nK = 0;
    if (deferFrom > 0) totalUndecDeferred = (i64)hDefTotal - nDeferred;
    // pairs: the deferred ones in the list's prefix were counted in their rounds -- every deferred pair where the undecided ones are
    // deferred too (hDefTotal), the general-path ones otherwise
    const unsigned long long counted = deferFrom > 0 ? (unsigned long long)hDefTotal : (unsigned long long)nDeferred;
    if (counted <= h.nPairs) h.nPairs -= counted;
    // general-path pairs: the queue's deferred prefix was counted in its rounds, whatever else was deferred
    if ((i64)h.nExact >= nDeferred) h.nExact -= (unsigned int)nDeferred;
    if (account("tail batch after round")) return -1;
    if (h.left) { sd::set_error("sd_nms2d: tail batch left candidates undecided (internal error)"); return -1; }
    nU = 0;
    return 0;
  }

  int report(uint8_t* d_keep, int64_t* stats, int verbose) {
    hipLaunchKernelGGL(k_keep, dim3(sd::div_up(N, 256)), dim3(256), 0, s, state, d_keep, N);
    SD_LAUNCH_CHECK();
    SD_CHECK(hipStreamSynchronize(s));
    if (stats) { stats[0] = totalPairs; stats[1] = totalExact; stats[2] = rounds; stats[3] = totalNbr;
                 stats[4] = (int64_t)ns_pairs; stats[5] = n_pair_launches; stats[6] = (int64_t)ns_full; stats[7] = (int64_t)ns_pre;
                 stats[8] = totalSpill; stats[9] = totalDecided; stats[10] = totalUndecDeferred; stats[11] = totalSkipped;
                 stats[12] = L.slotTotal; stats[13] = L.slots ? 1 : 0; }
    if (verbose) {
      printf("NMS: %lld pair intersections (%lld on the exact-join path), %d greedy rounds, %lld neighbour entries\n",
             (long long)totalPairs, (long long)totalExact, rounds, (long long)totalNbr);
      fflush(stdout);
    }
    return 0;
  }
};
}  // namespace

extern "C" int sd_nms2d_device(const float* d_dist, const float* d_points, int n_polys, int n_rays, int use_kdtree,
                               int use_bbox, int verbose, float threshold, uint8_t* d_keep, int64_t* stats,
                               void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (stats) memset(stats, 0, 16 * sizeof(int64_t));
  if (n_polys <= 0) return 0;
  Nms2d c(s, d_dist, d_points, n_polys, n_rays, use_kdtree, use_bbox, threshold, stats != nullptr);
  if (c.plan()) return -1;
  if (verbose) {
    printf("Non Maximum Suppression (2D) ++++ \n");
    printf("NMS: n_polys    = %d \nNMS: n_rays     = %d  \nNMS: thresh     = %.3f \nNMS: use_bbox   = %d\nNMS: use_kdtree = %d\n",
           n_polys, n_rays, threshold, use_bbox, use_kdtree);
    printf("NMS: using HIP (gfx950), uniform-grid broad phase + scan-beam pair kernel\n");
  }
  // all-pairs configuration with a negative threshold: every pair (0, j) passes the reference's
  // filters and overlap >= 0 > thr, so polygon 0 suppresses everything else.
  if (!use_kdtree && !use_bbox && threshold < 0) {
    SD_CHECK(hipMemsetAsync(d_keep, 0, n_polys, s));
    SD_CHECK(hipMemsetAsync(d_keep, 1, 1, s));
    SD_CHECK(hipStreamSynchronize(s));
    return 0;
  }
  if (c.build() || c.build_grid() || c.build_lists() || c.begin_rounds()) return -1;
  while (c.nU > 0)
    if (c.run_round()) return -1;
  return c.report(d_keep, stats, verbose);
}

// ---- the legacy variant: c_non_max_suppression_inds_old (stardist2d.cpp:173-386; caller stardist/nms.py:20-74, reference test
// tests/test_nms2D.py:78-110 "old == new").  Input = integer polygons (n, 2, R) (row 0 = y, row 1 = x) sorted by score descending and,
// with max_bbox_search, the map pixel -> polygon id: polygon i is only compared with the polygons j > i found in a window of the map
// around i's bounding box (:285-301); without it, with every j > i (:337).  Not on predict_instances(): kept as the reference keeps it,
// a second statement of the same NMS.  Every pair the reference could evaluate is evaluated once (Clipper-exact sweep, decisions per
// pair), then the greedy order is replayed by one workgroup in index order -- exactly the reference's outer loop.
namespace {
__global__ void __launch_bounds__(256) k_old_build(const int* __restrict__ polys, int N, int R, int* __restrict__ vx, int* __restrict__ vy,
                                                   int4* __restrict__ bbox, float* __restrict__ area, int* __restrict__ gmax) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int* py = polys + (size_t)i * 2 * R;
  const int* px = py + R;
  int x1 = 0, x2 = 0, y1 = 0, y2 = 0;
  float a = 0.f;
  for (int k = 0; k < R; ++k) {
    const int y = py[k], x = px[k];
    if (k == 0) { x1 = x2 = x; y1 = y2 = y; }
    else { x1 = x < x1 ? x : x1; x2 = x > x2 ? x : x2; y1 = y < y1 ? y : y1; y2 = y > y2 ? y : y2; }   // :229-239
    vx[(size_t)i * R + k] = x; vy[(size_t)i * R + k] = y;
    const int kn = (k + 1 == R) ? 0 : k + 1;
    a += (float)((i64)x * py[kn] - (i64)y * px[kn]);                       // area_from_path :128-138
  }
  area[i] = (float)(0.5 * (double)fabsf(a));
  bbox[i] = make_int4(x1, x2, y1, y2);
  atomicMax(&gmax[0], x2 - x1); atomicMax(&gmax[1], y2 - y1);            // :242-253
}
struct OldSearch { int max_bbox_search, grid_y, grid_x, height, width; };
// wave per polygon i; MODE 0 counts the pairs (i, j) the reference would test, MODE 1 writes them
template <int MODE>
__global__ void __launch_bounds__(256) k_old_pairs(int N, OldSearch o, const int* __restrict__ mapping, const int4* __restrict__ bbox,
                                                   const int* __restrict__ gmax, int* __restrict__ cnt, const i64* __restrict__ start,
                                                   int2* __restrict__ pairs) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (i >= N) return;
  const int4 bi = bbox[i];
  const i64 base = MODE ? start[i] : 0;
  int n = 0;
  auto visit = [&](bool in, int j) {
    const bool hit = in && j > i && j < N && bbox_intersect(bi, bbox[j]);   // :305-311 (j <= i: higher score or no candidate)
    const unsigned long long m = __ballot(hit);
    if (MODE && hit) pairs[base + n + __popcll(m & ((1ull << lane) - 1))] = make_int2(i, j);
    n += __popcll(m);
  };
  if (o.max_bbox_search) {
    const int mx = gmax[0], my = gmax[1];
    const int xs = max((bi.x - mx) / o.grid_x, 0), xe = min((bi.y + mx) / o.grid_x, o.width);       // :285-288 (C division, exclusive end)
    const int ys = max((bi.z - my) / o.grid_y, 0), ye = min((bi.w + my) / o.grid_y, o.height);
    const int w = xe - xs, h = ye - ys;
    if (w > 0 && h > 0) {
      const i64 tot = (i64)w * h;
      for (i64 t = 0; t < tot; t += 64) {
        const i64 q = t + lane;
        const bool in = q < tot;
        int j = -1;
        if (in) { const int jj = ys + (int)(q / w), ii = xs + (int)(q % w); j = mapping[(size_t)jj * o.width + ii]; }
        visit(in, j);
      }
    }
  } else {
    for (int t = i + 1; t < N; t += 64) visit(t + lane < N, t + lane);   // :337
  }
  if (!MODE && lane == 0) cnt[i] = n;
}
// the reference's outer loop (:273-323): i ascending; an unsuppressed i suppresses the j of its pairs with overlap > threshold
__global__ void __launch_bounds__(1024) k_old_replay(int N, const i64* __restrict__ start, const int2* __restrict__ pairs,
                                                     const unsigned char* __restrict__ supp, volatile unsigned char* state) {
  for (int i = 0; i < N; ++i) {
    const i64 beg = start[i], end = start[i + 1];
    if (beg == end) continue;
    if (state[i] != ST_SUPPRESSED)
      for (i64 t = beg + threadIdx.x; t < end; t += blockDim.x) if (supp[t]) state[pairs[t].y] = ST_SUPPRESSED;
    __threadfence_block();
    __syncthreads();
  }
}
}  // namespace

extern "C" int sd_nms2d_old_device(const int32_t* d_polys, int n_polys, int n_rays, const int32_t* d_mapping, int height, int width,
                                   float threshold, int max_bbox_search, int grid_y, int grid_x, int verbose, uint8_t* d_keep,
                                   void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  const int N = n_polys, R = n_rays;
  if (N <= 0) return 0;
  if (R < 1 || R > 256) { sd::set_error("sd_nms2d_old: n_rays=%d unsupported (1..256)", R); return -1; }
  if (max_bbox_search && (!d_mapping || height <= 0 || width <= 0 || grid_y <= 0 || grid_x <= 0)) {
    sd::set_error("sd_nms2d_old: max_bbox_search needs a (height, width) mapping and positive grid steps"); return -1;
  }
  if (verbose) {
    printf("Non Maximum Suppression (2D) ++++ \n");
    printf("NMS: n_polys  = %d \nNMS: n_rays   = %d  \nNMS: thresh   = %.3f \nNMS: max_bbox_search = %d \n", N, R, threshold, max_bbox_search);
    printf("NMS: using HIP (gfx950), every candidate pair by the scan-beam pair kernel, greedy order replayed on the device\n");
  }
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  int* vx = A.take_n<int>((size_t)N * R);
  int* vy = A.take_n<int>((size_t)N * R);
  int4* bbox = A.take_n<int4>(N);
  float* area = A.take_n<float>(N);
  int* gmax = A.take_n<int>(2);
  unsigned char* state = A.take_n<unsigned char>(N);
  int* cnt = A.take_n<int>(N + 1);
  i64* start = A.take_n<i64>(N + 1);
  Counters* d_cnt = (Counters*)A.take(sizeof(Counters));
  if (!vx || !vy || !bbox || !area || !gmax || !state || !cnt || !start || !d_cnt) return -1;
  SD_CHECK(hipMemsetAsync(gmax, 0, 2 * sizeof(int), s));
  SD_CHECK(hipMemsetAsync(state, 0, N, s));
  SD_CHECK(hipMemsetAsync(cnt, 0, (N + 1) * sizeof(int), s));
  SD_CHECK(hipMemsetAsync(d_cnt, 0, sizeof(Counters), s));
  hipLaunchKernelGGL(k_old_build, dim3(sd::div_up(N, 256)), dim3(256), 0, s, d_polys, N, R, vx, vy, bbox, area, gmax);
  SD_LAUNCH_CHECK();
  const OldSearch o{max_bbox_search, grid_y, grid_x, height, width};
  hipLaunchKernelGGL((k_old_pairs<0>), dim3(sd::div_up(N, 4)), dim3(256), 0, s, N, o, d_mapping, bbox, gmax, cnt, (const i64*)nullptr, (int2*)nullptr);
  SD_LAUNCH_CHECK();
  size_t tmpBytes = 0;
  (void)exclusive_sum_i64(nullptr, tmpBytes, cnt, start, N + 1, s);
  void* scanTmp = A.take(tmpBytes + 256);
  if (!scanTmp) return -1;
  SD_CHECK(exclusive_sum_i64(scanTmp, tmpBytes, cnt, start, N + 1, s));
  i64 total = 0;
  SD_CHECK(hipMemcpyAsync(&total, start + N, sizeof(i64), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipStreamSynchronize(s));
  if (total < 0 || total >= (i64)(1ll << 30)) {
    sd::set_error("sd_nms2d_old: %lld candidate pairs exceed the capacity of one call (2^30)", (long long)total); return -1;
  }
  if (total > 0) {
    const unsigned int qCap = (unsigned int)total + 64u;
    int2* pairs = A.take_n<int2>((size_t)total + 64);
    unsigned char* supp = A.take_n<unsigned char>((size_t)total + 64);
    unsigned int* spillPairs = A.take_n<unsigned int>(qCap);
    unsigned int* exactPairs = A.take_n<unsigned int>(qCap);
    void* prep = A.take((size_t)N * prep_stride(R));
    if (!pairs || !supp || !spillPairs || !exactPairs || !prep) return -1;
    SD_CHECK(hipMemsetAsync(supp, 0, (size_t)total + 64, s));
    hipLaunchKernelGGL((k_old_pairs<1>), dim3(sd::div_up(N, 4)), dim3(256), 0, s, N, o, d_mapping, bbox, gmax, cnt, (const i64*)start, pairs);
    SD_LAUNCH_CHECK();
    const unsigned long long nP = (unsigned long long)total;
    SD_CHECK(hipMemcpyAsync(&d_cnt->nPairs, &nP, sizeof(nP), hipMemcpyHostToDevice, s));
    const Sweep w{s, R, vx, vy, prep, area, threshold, pairs, spillPairs, exactPairs, qCap, d_cnt, state, supp};
    Timer untimed;
    if (prepare_polys(vx, vy, N, R, nullptr, prep, s)) return -1;
    if (sweep_tiers(w, nullptr, &d_cnt->nPairs, nullptr, untimed, [&]() { return general_path(w); })) return -1;
    hipLaunchKernelGGL(k_old_replay, dim3(1), dim3(1024), 0, s, N, (const i64*)start, (const int2*)pairs, (const unsigned char*)supp, state);
    SD_LAUNCH_CHECK();
    Counters h;
    SD_CHECK(hipMemcpyAsync(&h, d_cnt, sizeof(Counters), hipMemcpyDeviceToHost, s));
    SD_CHECK(hipStreamSynchronize(s));
    if (check_sweep("sd_nms2d_old", h, qCap, false, "")) return -1;
  }
  hipLaunchKernelGGL(k_keep, dim3(sd::div_up(N, 256)), dim3(256), 0, s, state, d_keep, N);
  SD_LAUNCH_CHECK();
  SD_CHECK(hipStreamSynchronize(s));
  if (verbose) { printf("NMS: %lld candidate pairs evaluated\n", (long long)total); fflush(stdout); }
  return 0;
}

// Test hook: the 64-bit exclusive sum of the neighbour-list builder and of sd_nms2d_old_device (exclusive_sum_i64, nms_rounds.h) on its own
extern "C" int sd_exclusive_sum_i32_i64_device(const int32_t* d_in, int n, int64_t* d_out, void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (n <= 0) return 0;
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  size_t tmpBytes = 0;
  (void)exclusive_sum_i64(nullptr, tmpBytes, (const int*)d_in, (long long*)d_out, n, s);
  void* tmp = A.take(tmpBytes + 256);
  if (!tmp) return -1;
  SD_CHECK(exclusive_sum_i64(tmp, tmpBytes, (const int*)d_in, (long long*)d_out, n, s));
  SD_CHECK(hipStreamSynchronize(s));
  return 0;
}

extern "C" int sd_nms2d_old_host(const int32_t* polys, int n_polys, int n_rays, const int32_t* mapping, int height, int width,
                                 float threshold, int max_bbox_search, int grid_y, int grid_x, int verbose, uint8_t* keep) {
  if (n_polys <= 0) return 0;
  int32_t *d_polys = nullptr, *d_map = nullptr;
  uint8_t* d_keep = nullptr;
  const size_t pb = (size_t)n_polys * 2 * n_rays * sizeof(int32_t), mb = max_bbox_search ? (size_t)height * width * sizeof(int32_t) : 0;
  SD_CHECK(hipMalloc(&d_polys, pb));
  if (mb) SD_CHECK(hipMalloc(&d_map, mb));
  SD_CHECK(hipMalloc(&d_keep, n_polys));
  int rc = -1;
  do {
    if (hipMemcpy(d_polys, polys, pb, hipMemcpyHostToDevice) != hipSuccess) { sd::set_error("H2D failed"); break; }
    if (mb && hipMemcpy(d_map, mapping, mb, hipMemcpyHostToDevice) != hipSuccess) { sd::set_error("H2D failed"); break; }
    if (sd_nms2d_old_device(d_polys, n_polys, n_rays, d_map, height, width, threshold, max_bbox_search, grid_y, grid_x, verbose, d_keep, nullptr)) break;
    if (hipMemcpy(keep, d_keep, n_polys, hipMemcpyDeviceToHost) != hipSuccess) { sd::set_error("D2H failed"); break; }
    rc = 0;
  } while (0);
  (void)hipFree(d_polys); if (d_map) (void)hipFree(d_map); (void)hipFree(d_keep);
  return rc;
}

extern "C" int sd_nms2d_host(const float* dist, const float* points, int n_polys, int n_rays, int use_kdtree, int use_bbox,
                             int verbose, float threshold, uint8_t* keep, int64_t* stats) {
  if (n_polys <= 0) return 0;
  float *d_dist = nullptr, *d_pts = nullptr;
  uint8_t* d_keep = nullptr;
  SD_CHECK(hipMalloc(&d_dist, (size_t)n_polys * n_rays * sizeof(float)));
  SD_CHECK(hipMalloc(&d_pts, (size_t)n_polys * 2 * sizeof(float)));
  SD_CHECK(hipMalloc(&d_keep, n_polys));
  int rc = -1;
  do {
    if (hipMemcpy(d_dist, dist, (size_t)n_polys * n_rays * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { sd::set_error("H2D failed"); break; }
    if (hipMemcpy(d_pts, points, (size_t)n_polys * 2 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { sd::set_error("H2D failed"); break; }
    if (sd_nms2d_device(d_dist, d_pts, n_polys, n_rays, use_kdtree, use_bbox, verbose, threshold, d_keep, stats, nullptr)) break;
    if (hipMemcpy(keep, d_keep, n_polys, hipMemcpyDeviceToHost) != hipSuccess) { sd::set_error("D2H failed"); break; }
    rc = 0;
  } while (0);
  (void)hipFree(d_dist); (void)hipFree(d_pts); (void)hipFree(d_keep);
  return rc;
}
