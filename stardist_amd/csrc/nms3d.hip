// nms3d.hip -- greedy non-maximum suppression of star-convex polyhedra on gfx950.
//
// Replaces _COMMON_non_maximum_suppression_sparse (stardist/lib/stardist3d_impl.cpp:956-1385),
// reached through the reference's C ABI name _LIB_non_maximum_suppression_sparse
// (stardist3d_lib.h:52-66) and the CPython c_non_max_suppression_inds (stardist3d.cpp:13-62).
//
//   P1  per candidate: signed-tetrahedra volume (sequential fp32 sum over faces, :257-291),
//       integer bbox (lrint, :536-567)
//   P1b anisotropy = max_k(mean bbox extent) / mean bbox extent_k  (:1008-1023) -- the reference
//       accumulates it inside an OpenMP loop without synchronisation; the defined value is the
//       sequential fp32 sum over candidates, which is what is computed here (on the host, from
//       the device bboxes, n_polys float additions)
//   P2  per candidate: outer radius, outer/inner isotropic radii (:343-467)
//   P3  uniform-grid broad phase (replaces nanoflann, :1056-1085, :1167-1171)
//   greedy rounds (same fixed point as the sequential loop :1121-1338, see nms2d.hip):
//       emit:  exact neighbour predicate, then the two cheap cascade stages inline
//              (1) sphere/bbox upper bound  -> keep      :1213-1228
//              (2) inscribed-sphere lower bound -> suppress :1232-1248
//       (3) kernel-kernel intersection volume -> suppress   :1261-1277
//           Qhull's half-space intersection is replaced by an exact-geometry routine: one wave
//           per pair, one half-space per lane, the face polygon of each plane obtained by
//           clipping against all other half-spaces in fp64, volume = 1/3 sum(area * height).
//       (4) hull-hull intersection volume -> keep           :1282-1295
//           convex hulls by exhaustive facet search (one wave per polyhedron: every vertex triple whose
//           plane has all other vertices on one side), then the same half-space volume routine.
//       (5) voxel rendering: count lattice points inside both polyhedra -> suppress :1305-1330
#include <algorithm>

#include "common.h"
#include "geom3d.h"
#include "nms_rounds.h"
#include "../../include/stardist_hip.h"
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <vector>

namespace {

typedef long long i64;

// ------------------------------------------------------------------ P1 / P2
// The per-candidate kernels walk a candidate's R distances in face order (gathers).  A workgroup's rows are contiguous in memory: they are
// read once, coalesced, into LDS (row pitch R + 1: the lanes of a wave, one row each, hit distinct banks) -- one pass over the 4 R bytes
// of every candidate instead of line-by-line re-fetches of 128 interleaved rows (FETCH_SIZE was 12x the rows' size).
__device__ __forceinline__ const float* stage_rows(const float* __restrict__ dist, int N, int R, float* lds, int staged) {
  if (!staged) return dist + (size_t)min((int)(blockIdx.x * blockDim.x + threadIdx.x), N - 1) * R;     // several hundred rays: rows stay in memory
  const int i0 = blockIdx.x * blockDim.x;
  const int rows = min((int)blockDim.x, N - i0);
  const float* src = dist + (size_t)i0 * R;
  for (int e = threadIdx.x; e < rows * R; e += blockDim.x) { const int r = e / R; lds[r * (R + 1) + (e - r * R)] = src[e]; }
  __syncthreads();
  return lds + threadIdx.x * (R + 1);
}

__global__ void k_pre1(const float* __restrict__ dist, const float* __restrict__ pts, const float* __restrict__ verts,
                       const int* __restrict__ faces, int N, int R, int F, float* __restrict__ volume, int* __restrict__ bbox, int staged) {
  extern __shared__ float rows_lds[];
  const float* d = stage_rows(dist, N, R, rows_lds, staged);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float vol = 0.f;                                                            // polyhedron_volume :257-291
  for (int f = 0; f < F; ++f) {
    const int iA = faces[3 * f], iB = faces[3 * f + 1], iC = faces[3 * f + 2];
    const float dA = d[iA], dB = d[iB], dC = d[iC];
    vol += sd3::tetrahedron_volume0(dA * verts[3 * iA], dA * verts[3 * iA + 1], dA * verts[3 * iA + 2],
                                    dB * verts[3 * iB], dB * verts[3 * iB + 1], dB * verts[3 * iB + 2],
                                    dC * verts[3 * iC], dC * verts[3 * iC + 1], dC * verts[3 * iC + 2]);
  }
  volume[i] = vol;
  const float cz = pts[3 * i], cy = pts[3 * i + 1], cx = pts[3 * i + 2];
  int z1 = INT_MAX, z2 = -1, y1 = INT_MAX, y2 = -1, x1 = INT_MAX, x2 = -1;   // polyhedron_bbox :536-567
  for (int j = 0; j < R; ++j) {
    const float z = cz + d[j] * verts[3 * j], y = cy + d[j] * verts[3 * j + 1], x = cx + d[j] * verts[3 * j + 2];
    const int rz = sd3::round_to_int(z), ry = sd3::round_to_int(y), rx = sd3::round_to_int(x);
    z1 = min(z1, rz); z2 = max(z2, rz); y1 = min(y1, ry); y2 = max(y2, ry); x1 = min(x1, rx); x2 = max(x2, rx);
  }
  int* b = bbox + 6 * (size_t)i;
  b[0] = z1; b[1] = z2; b[2] = y1; b[3] = y2; b[4] = x1; b[5] = x2;
}

struct Aniso { float a[3]; };

__global__ void k_pre2(const float* __restrict__ dist, const float* __restrict__ verts, const int* __restrict__ faces, int N, int R,
                       int F, Aniso an, float* __restrict__ r_outer, float* __restrict__ r_outer_iso, float* __restrict__ r_inner_iso,
                       int* gmax /* max outer radius bits */, int staged) {
  extern __shared__ float rows_lds[];
  const float* d = stage_rows(dist, N, R, rows_lds, staged);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float r = 0;                                                                // bounding_radius_outer :343-350
  float r2max = 0;                                                            // bounding_radius_outer_isotropic :401-418
  for (int k = 0; k < R; ++k) {
    r = fmaxf(r, d[k]);
    const float z = an.a[0] * d[k] * verts[3 * k], y = an.a[1] * d[k] * verts[3 * k + 1], x = an.a[2] * d[k] * verts[3 * k + 2];
    r2max = fmaxf(z * z + y * y + x * x, r2max);
  }
  r_outer[i] = r;
  r_outer_iso[i] = sqrtf(r2max);
  float rmin = INFINITY;                                                      // bounding_radius_inner_isotropic :420-467
  for (int f = 0; f < F; ++f) {
    const int iA = faces[3 * f], iB = faces[3 * f + 1], iC = faces[3 * f + 2];
    const float Az = an.a[0] * d[iA] * verts[3 * iA], Ay = an.a[1] * d[iA] * verts[3 * iA + 1], Ax = an.a[2] * d[iA] * verts[3 * iA + 2];
    const float Bz = an.a[0] * d[iB] * verts[3 * iB], By = an.a[1] * d[iB] * verts[3 * iB + 1], Bx = an.a[2] * d[iB] * verts[3 * iB + 2];
    const float Cz = an.a[0] * d[iC] * verts[3 * iC], Cy = an.a[1] * d[iC] * verts[3 * iC + 1], Cx = an.a[2] * d[iC] * verts[3 * iC + 2];
    const float pz = Bz - Az, py = By - Ay, px = Bx - Ax;
    const float qz = Cz - Az, qy = Cy - Ay, qx = Cx - Ax;
    float Nz = (px * qy - py * qx);
    float Ny = (pz * qx - px * qz);
    float Nx = (py * qz - pz * qy);
    const float normz = (float)(1.f / ((double)sqrtf(Nz * Nz + Ny * Ny + Nx * Nx) + 1.e-10));
    Nz *= normz; Ny *= normz; Nx *= normz;
    const float rr = Az * Nz + Ay * Ny + Ax * Nx;
    rmin = fminf(rmin, rr);
  }
  r_inner_iso[i] = rmin;
  const int rb = __float_as_int(r);
  volatile int* gm = gmax;
  if (rb > gm[0]) atomicMax(gmax, rb);
}

// ------------------------------------------------------------------ grid
struct Grid3 { float z0, y0, x0, inv_cs; int nz, ny, nx; };
__device__ __forceinline__ int cell3(const Grid3 g, const float* p, int& cz, int& cy, int& cx) {
  cz = min(max((int)((p[0] - g.z0) * g.inv_cs), 0), g.nz - 1);
  cy = min(max((int)((p[1] - g.y0) * g.inv_cs), 0), g.ny - 1);
  cx = min(max((int)((p[2] - g.x0) * g.inv_cs), 0), g.nx - 1);
  return (cz * g.ny + cy) * g.nx + cx;
}
__global__ void k_minmax3(const float* __restrict__ pts, int N, int* mm /* zmin zmax ymin ymax xmin xmax */) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  volatile int* m = mm;
  for (int d = 0; d < 3; ++d) {
    const int v = (int)floorf(pts[3 * i + d]);
    if (v < m[2 * d]) atomicMin(&mm[2 * d], v);
    if (v > m[2 * d + 1]) atomicMax(&mm[2 * d + 1], v);
  }
}
__global__ void k_cell_count3(const float* __restrict__ pts, int N, Grid3 g, int* __restrict__ cellCount, int* __restrict__ candCell) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  int a, b, c;
  const int cell = cell3(g, pts + 3 * (size_t)i, a, b, c);
  candCell[i] = cell;
  atomicAdd(&cellCount[cell], 1);
}
// what the broad phase needs of a candidate, stored in CELL ORDER: a wave that scans the rows of cells around its candidate reads
// contiguous 40-byte records (mostly L2 hits: neighbouring candidates scan the same rows) instead of gathering 36 bytes per test
// through an index list
struct CellRec3 { float p[3]; int idx; int bb[6]; };
// slotCap (may be null): upper bound of candidate i's neighbour count = the population of the (2 W + 1)^3 cells its list is built from, minus
// itself: the capacity of its slot in the single-pass neighbour lists (k_neighbours3<2>)
__global__ void k_cell_fill3(int N, const int* __restrict__ candCell, const int* __restrict__ cellStart, int* __restrict__ cellFill,
                             const float* __restrict__ pts, const int* __restrict__ bbox, CellRec3* __restrict__ cellRec, Grid3 g, int W,
                             int* __restrict__ slotCap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int c = candCell[i];
  if (slotCap) {
    const int cz = c / (g.ny * g.nx), cy = (c / g.nx) % g.ny, cx = c % g.nx;
    const int x_lo = max(cx - W, 0), x_hi = min(cx + W, g.nx - 1);
    int u = -1;
    for (int zz = max(cz - W, 0); zz <= min(cz + W, g.nz - 1); ++zz)
      for (int yy = max(cy - W, 0); yy <= min(cy + W, g.ny - 1); ++yy) {
        const int row = (zz * g.ny + yy) * g.nx;
        u += cellStart[row + x_hi + 1] - cellStart[row + x_lo];
      }
    slotCap[i] = u;
  }
  CellRec3 r;
  r.p[0] = pts[3 * (size_t)i]; r.p[1] = pts[3 * (size_t)i + 1]; r.p[2] = pts[3 * (size_t)i + 2];
  r.idx = i;
#pragma unroll
  for (int k = 0; k < 6; ++k) r.bb[k] = bbox[6 * (size_t)i + k];
  cellRec[cellStart[c] + atomicAdd(&cellFill[c], 1)] = r;
}

__device__ __forceinline__ bool bbox_pos_overlap(const int* a, const int* b) {
  return (min(a[1], b[1]) - max(a[0], b[0]) > 0) && (min(a[3], b[3]) - max(a[2], b[2]) > 0) && (min(a[5], b[5]) - max(a[4], b[4]) > 0);
}

// symmetric superset of the pairs that can interact
__device__ __forceinline__ bool may_interact3(const NmsFlags f, const float* pi, const float* pj, const int* bi, const int* bj) {
  const float dz = pi[0] - pj[0], dy = pi[1] - pj[1], dx = pi[2] - pj[2];
  const float rr = 2.f * f.max_dist + 1.f;
  if (f.use_kdtree && !(dz * dz + dy * dy + dx * dx < rr * rr)) return false;
  // with use_bbox and thr >= 0 a pair is dropped at stage 1 unless the boxes overlap with positive extent
  if (f.use_bbox && f.thr_nonneg && !bbox_pos_overlap(bi, bj)) return false;
  return true;
}

// one wave per candidate, taken in cell order; consecutive workgroups go round-robin over the 8 XCDs, so block b is given the
// (b % 8)-th eighth of the cell-ordered list: the candidates of one region of space stay on one XCD's L2
template <int MODE>
__global__ void __launch_bounds__(256) k_neighbours3(int N, Grid3 g, NmsFlags f, const CellRec3* __restrict__ cellRec,
                                                     const int* __restrict__ candCell, const int* __restrict__ cellStart,
                                                     int* __restrict__ nbrCount, int* __restrict__ nbrLow,
                                                     const i64* __restrict__ nbrStart, int* __restrict__ nbr, int* __restrict__ waitOn, int W) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int blk = ((int)blockIdx.x & 7) * ((int)gridDim.x >> 3) + ((int)blockIdx.x >> 3);
  const int slot = blk * (blockDim.x >> 6) + wave;
  if (slot >= N) return;
  const CellRec3 me = cellRec[slot];
  const int i = me.idx;
  const int c = candCell[i];
  const int cz = c / (g.ny * g.nx), cy = (c / g.nx) % g.ny, cx = c % g.nx;
  const float* pi = me.p;
  const int* bi = me.bb;
  // a candidate's list holds its lower-index neighbours first (what the greedy scan looks at: is a better candidate still undecided?),
  // then the higher-index ones (what a survivor is paired with): each consumer reads its half only
  int nLo = 0, nHi = 0;
  int minj = INT_MAX;                      // MODE 1: the best-scored neighbour above i = the first wait target of the greedy scan
  const i64 baseLo = MODE ? nbrStart[i] : 0;
  // MODE 2 (one pass into slots sized from the cell table, nms2d.hip k_neighbours<2>): the higher-index half is written downwards from
  // the slot's last entry
  const i64 baseHi = MODE == 1 ? baseLo + nbrLow[i] : (MODE == 2 ? nbrStart[i + 1] - 1 : 0);
  const int x_lo = max(cx - W, 0), x_hi = min(cx + W, g.nx - 1);
  for (int zz = max(cz - W, 0); zz <= min(cz + W, g.nz - 1); ++zz)
    for (int yy = max(cy - W, 0); yy <= min(cy + W, g.ny - 1); ++yy) {
      const int row = (zz * g.ny + yy) * g.nx;
      const int beg = cellStart[row + x_lo], end = cellStart[row + x_hi + 1];
      for (int t = beg; t < end; t += 64) {
        const int idx = t + lane;
        bool hit = false;
        int j = -1;
        if (idx < end) {
          const CellRec3 o = cellRec[idx];
          j = o.idx;
          if (j != i) hit = may_interact3(f, pi, o.p, bi, o.bb);
        }
        const unsigned long long mLo = __ballot(hit && j < i), mHi = __ballot(hit && j > i);
        const unsigned long long below = (1ull << lane) - 1;
        if (MODE && hit) {
          if (j < i) { nbr[baseLo + nLo + __popcll(mLo & below)] = j; minj = min(minj, j); }
          else if (MODE == 1) nbr[baseHi + nHi + __popcll(mHi & below)] = j;
          else nbr[baseHi - (nHi + __popcll(mHi & below))] = j;
        }
        nLo += __popcll(mLo); nHi += __popcll(mHi);
      }
    }
  if (!MODE && lane == 0) { nbrCount[i] = nLo + nHi; nbrLow[i] = nLo; }
  if (MODE == 2 && lane == 0) nbrLow[i] = nLo;
  if (MODE && lane == 0) nbrCount[i] = nHi;            // from here on nbrCount holds the size of the higher-index half (k_round_emit3)
  if (MODE) {
    for (int o = 32; o; o >>= 1) minj = min(minj, __shfl_xor(minj, o));
    if (lane == 0) waitOn[i] = (minj < i) ? minj : WAIT_NONE;
  }
}

struct Stats { unsigned long long upper, lower, kernel, render, kept_pre, sup_pre, sup_kernel, sup_render, convex, kept_convex, overflow, hiv_faces, hiv_fallback, hiv_list, hiv_clips, hiv_rest, lb_decided, ub_decided, near_thr;
               unsigned long long cyc[6]; };   // SD_TRACE: stage-3 wave cycles spent in load+half-spaces / cull / bounds / exact volume / total
#define SD_PROF_BIT 0x40000000u
#define SD_NOREUSE_BIT 0x20000000u   // bounds passes: cast every direction of the refined mesh (A/B switch of "nms3d_bounds_reuse")
#define SD_LEAN_BIT 0x10000000u      // bounds-ONLY launch without the seed table; pos / orig (written by the cull, read by nobody) lie in the workspace ("nms3d_bounds_lean")
#define SD_WS_MASK 0x0FFFFFFFu

// Where a cascade stage records "i suppresses j".  Normal round (i is already KEPT): straight into the state array.  Tail batch
// (i is still undecided, the pair is evaluated speculatively): appended to an edge list; the greedy order is replayed over those
// edges afterwards (k_tail3_mark / k_tail3_promote).
struct SuppSink {
  unsigned char* state; int2* edges; unsigned int* count; unsigned int cap;
  __device__ __forceinline__ void suppress(int i, int j) const {
    if (edges) { const unsigned int pos = atomicAdd(count, 1u); if (pos < cap) edges[pos] = make_int2(i, j); }
    else state[j] = ST_SUPPRESSED;
  }
};

// Exact volumes carried into the tail batch ("nms3d_defer_exact"): a late round's launch of the exact-volume kernel costs the latency
// of one exact volume (~0.5 ms) for a few dozen pairs.  From round r on, the pairs (i kept, j) the bounds of stage 3 / stage 4 leave
// undecided are queued instead; j is marked pending (k_round_triage keeps it undecided) and the tail batch evaluates the queue in
// its one pass, in front of its own pairs (k_seed3).  The queue re-enters the cascade at stage 3 (a pair queued by stage 4 passes
// stage 3's bounds again, with the same outcome).  Same fixed point: the tail replay suppresses j iff a KEPT i has a suppressing edge.
__global__ void k_defer3(const int2* __restrict__ pairsX, const unsigned int* __restrict__ nX, int2* __restrict__ dfr, unsigned int* dfrCount,
                         unsigned int cap, unsigned char* __restrict__ pend, unsigned long long* overflow) {
  const unsigned int n = *nX;
  for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
    const int2 ij = pairsX[t];
    const unsigned int pos = atomicAdd(dfrCount, 1u);
    if (pos < cap) dfr[pos] = ij; else atomicAdd(overflow, 1ull);           // the host keeps the total below cap: cannot happen
    pend[ij.y] = 1;
  }
}
__global__ void k_seed3(const int2* __restrict__ dfr, const unsigned int* __restrict__ dfrCount, unsigned int cap, int2* __restrict__ pairs, unsigned int* pairCount) {
  const unsigned int n = *dfrCount < cap ? *dfrCount : cap;
  for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) pairs[t] = dfr[t];
  if (blockIdx.x == 0 && threadIdx.x == 0) *pairCount = n;                  // the tail's emit appends behind the queue
}

// Tail replay: the fixed point of the sequential loop over the remaining candidates -- j is suppressed iff some KEPT i < j has a
// suppressing edge (i, j).  One sweep over the edges marks what the decided sources imply, one sweep over the candidates promotes
// every j none of whose sources is still undecided; decisions only move UNDECIDED -> final, so sweeps can simply be repeated.
__global__ void k_tail3_mark(const int2* __restrict__ edges, unsigned int n, unsigned char* __restrict__ state, unsigned char* __restrict__ blocked) {
  const unsigned int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int2 ij = edges[e];
  const unsigned char si = ((volatile unsigned char*)state)[ij.x];
  if (si == ST_KEPT) state[ij.y] = ST_SUPPRESSED;
  else if (si == ST_UNDECIDED) blocked[ij.y] = 1;
}
__global__ void k_tail3_promote(const int* __restrict__ U, int nU, unsigned char* __restrict__ state, unsigned char* __restrict__ blocked, int* left) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nU) return;
  const int j = U[t];
  if (state[j] != ST_UNDECIDED) return;
  if (blocked[j]) { blocked[j] = 0; atomicAdd(left, 1); }
  else state[j] = ST_KEPT;
}

// emit: exact neighbour predicate + cascade stages 1 and 2 (:1199-1248).  tail != 0: K is the list of the still undecided candidates,
// none of which is marked kept; every pair of undecided candidates the sequential loop could still evaluate is emitted.
__global__ void __launch_bounds__(256) k_round_emit3(const int* __restrict__ K, int nK, const int* __restrict__ nKPtr, SuppSink sink, int tail,
                                                     const i64* __restrict__ nbrStart, const int* __restrict__ nbrHigh, const int* __restrict__ nbr, NmsFlags f, Aniso an,
                                                     const float* __restrict__ pts, const int* __restrict__ bbox,
                                                     const float* __restrict__ volume, const float* __restrict__ r_outer,
                                                     const float* __restrict__ r_outer_iso, const float* __restrict__ r_inner_iso,
                                                     int2* __restrict__ pairs, unsigned int* pairCount, unsigned int pairCap, Stats* st) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (nKPtr) nK = *nKPtr;                            // normal round: the survivor count of this round is read on the device (persistent grid)
  unsigned char* state = sink.state;
  int n_upper = 0, n_lower = 0, n_keep = 0, n_sup = 0;
  for (int w = blockIdx.x * (blockDim.x >> 6) + wave; w < nK; w += gridDim.x * (blockDim.x >> 6)) {
  const int i = K[w];
  if (tail) { if (state[i] != ST_UNDECIDED) continue; }
  else if (lane == 0) state[i] = ST_KEPT;
  const i64 end = nbrStart[i + 1], beg = end - nbrHigh[i];          // the higher-index neighbours (the back of i's slot)
  const float* pi = pts + 3 * (size_t)i;
  const float rad = f.max_dist + r_outer[i];
  const float rad2 = rad * rad;                                                // :1170
  for (i64 t = beg; t < end; t += 64) {
    const i64 idx = t + lane;
    bool emit = false;
    int j = -1;
    int c_upper = 0, c_lower = 0, c_keep = 0, c_sup = 0;
    if (idx < end) {
      j = nbr[idx];
      if (j > i && state[j] == ST_UNDECIDED) {
        const float* pj = pts + 3 * (size_t)j;
        bool ok = true;
        if (f.use_kdtree) {                                                    // nanoflann L2_Simple, strict '<'
          const float d0 = pi[0] - pj[0], d1 = pi[1] - pj[1], d2_ = pi[2] - pj[2];
          float d2 = d0 * d0; d2 += d1 * d1; d2 += d2_ * d2_;
          ok = d2 < rad2;
        }
        if (ok) {
          const float A_min = fminf(volume[i], volume[j]);                     // :1206
          float A_inter = fminf(sd3::intersect_sphere_isotropic(r_outer_iso[i], pi, r_outer_iso[j], pj, an.a),
                                sd3::intersect_bbox(bbox + 6 * (size_t)i, bbox + 6 * (size_t)j));   // :1213-1219
          c_upper = 1;
          float iou = (float)fmin(1.0, (double)A_inter / ((double)A_min + 1e-10));                // :1223
          if (f.use_bbox && (((double)A_inter < 1.e-10) || (iou <= f.thr))) { c_keep = 1; }
          else {
            A_inter = sd3::intersect_sphere_isotropic(r_inner_iso[i], pi, r_inner_iso[j], pj, an.a);   // :1232-1237
            c_lower = 1;
            iou = (float)fmax(0.0, (double)A_inter / ((double)A_min + 1e-10));                    // :1241
            if (iou > f.thr) { c_sup = 1; sink.suppress(i, j); }
            else emit = true;
          }
        }
      }
    }
    const unsigned long long m = __ballot(emit);
    if (m) {
      unsigned int base = 0;
      if (lane == 0) base = atomicAdd(pairCount, (unsigned int)__popcll(m));
      base = __shfl(base, 0);
      if (emit) {
        const unsigned int pos = base + __popcll(m & ((1ull << lane) - 1));
        if (pos < pairCap) pairs[pos] = make_int2(i, j);
      }
    }
    n_upper += __popcll(__ballot(c_upper)); n_lower += __popcll(__ballot(c_lower)); n_keep += __popcll(__ballot(c_keep)); n_sup += __popcll(__ballot(c_sup));
  }
  }
  if (lane == 0 && (n_upper | n_lower | n_keep | n_sup)) {          // (once per wave, not once per 64 neighbours)
    if (n_upper) atomicAdd(&st->upper, (unsigned long long)n_upper);
    if (n_lower) atomicAdd(&st->lower, (unsigned long long)n_lower);
    if (n_keep) atomicAdd(&st->kept_pre, (unsigned long long)n_keep);
    if (n_sup) atomicAdd(&st->sup_pre, (unsigned long long)n_sup);
  }
}

// ------------------------------------------------------------------ stage 3: kernel ∩ kernel volume
// One wave per pair.  Half-spaces h = (n, d): inside <=> n.p + d <= 0 (build_halfspace :744-764,
// interleaved poly1/poly2 per face as qhull_overlap_kernel :840-853 does).
// Qhull's feasibility rule (qh_sethalfspace): the interior point must satisfy offset + n.c <= 0 for
// every half-space (evaluated in that order in fp64), otherwise the reference gets a QhullError and
// uses err_value (0).
#define HIV_MAXP 64
struct HivPoly { double ps[HIV_MAXP], pt[HIV_MAXP], qs[HIV_MAXP], qt[HIV_MAXP]; int n; };
// Sutherland-Hodgman against the half-plane a*s + b*t + e <= 0; returns false on capacity overflow
__device__ __forceinline__ bool hiv_clip(HivPoly& P, double a, double b, double e) {
  int nq = 0;
  const int n = P.n;
  double s_prev = P.ps[n - 1], t_prev = P.pt[n - 1];
  double f_prev = a * s_prev + b * t_prev + e;
  for (int v = 0; v < n; ++v) {
    const double s_cur = P.ps[v], t_cur = P.pt[v];
    const double f_cur = a * s_cur + b * t_cur + e;
    if ((f_prev <= 0) != (f_cur <= 0)) {
      const double w = f_prev / (f_prev - f_cur);
      if (nq >= HIV_MAXP) return false;
      P.qs[nq] = s_prev + w * (s_cur - s_prev); P.qt[nq] = t_prev + w * (t_cur - t_prev); ++nq;
    }
    if (f_cur <= 0) { if (nq >= HIV_MAXP) return false; P.qs[nq] = s_cur; P.qt[nq] = t_cur; ++nq; }
    s_prev = s_cur; t_prev = t_cur; f_prev = f_cur;
  }
  P.n = nq;
  for (int v = 0; v < nq; ++v) { P.ps[v] = P.qs[v]; P.pt[v] = P.qt[v]; }
  return true;
}
struct HivFrame { double uz, uy, ux, vz, vy, vx, oz, oy, ox, h; bool ok; };
// in-plane frame of half-space k: origin = foot point of c, (u, v) orthonormal in the plane
__device__ __forceinline__ HivFrame hiv_frame(const double* __restrict__ hs, int k, const double c[3]) {
  HivFrame fr;
  const double nz = hs[4 * k], ny = hs[4 * k + 1], nx = hs[4 * k + 2], d = hs[4 * k + 3];
  const double nn = sqrt(nz * nz + ny * ny + nx * nx);
  fr.ok = nn > 0;
  if (!fr.ok) { fr.uz = fr.uy = fr.ux = fr.vz = fr.vy = fr.vx = fr.oz = fr.oy = fr.ox = fr.h = 0; return fr; }
  fr.h = -(nz * c[0] + ny * c[1] + nx * c[2] + d) / nn;                        // distance from c to the plane (>= 0)
  const double uz0 = nz / nn, uy0 = ny / nn, ux0 = nx / nn;                    // unit normal
  fr.oz = c[0] + fr.h * uz0; fr.oy = c[1] + fr.h * uy0; fr.ox = c[2] + fr.h * ux0;
  double az = 0, ay = 0, ax = 0;
  const double fz = fabs(uz0), fy = fabs(uy0), fx = fabs(ux0);
  if (fz <= fy && fz <= fx) az = 1; else if (fy <= fx) ay = 1; else ax = 1;
  double uz = ay * ux0 - ax * uy0, uy = ax * uz0 - az * ux0, ux = az * uy0 - ay * uz0;   // u = normalize(a x n), v = n x u
  const double un = sqrt(uz * uz + uy * uy + ux * ux);
  uz /= un; uy /= un; ux /= un;
  fr.uz = uz; fr.uy = uy; fr.ux = ux;
  fr.vz = uy0 * ux - ux0 * uy; fr.vy = ux0 * uz - uz0 * ux; fr.vx = uz0 * uy - uy0 * uz;
  return fr;
}
#define HIV_LINE(fr, hs, m, a, b, e)                                                                         \
  const double mz_ = hs[4 * (m)], my_ = hs[4 * (m) + 1], mx_ = hs[4 * (m) + 2], md_ = hs[4 * (m) + 3];       \
  const double a = mz_ * fr.uz + my_ * fr.uy + mx_ * fr.ux, b = mz_ * fr.vz + my_ * fr.vy + mx_ * fr.vx,     \
               e = mz_ * fr.oz + my_ * fr.oy + mx_ * fr.ox + md_;

// COINCIDENT half-spaces (round 6).  Two polyhedra of the same shape whose centres differ along a direction that lies IN a facet plane have
// that plane twice, bit for bit (Rays_Cartesian's vertical band under a shift along the pole axis, an octahedron under a shift (1, 1, 0)):
// each of the twins cuts the other's face with a trace "line" a = b = 0, e = +-1 ulp, so that rounding decided whether a face was counted
// twice, once or not at all (found with tools/diag_cartesian3.py: 285.8 instead of 321.7).  The twins bound the intersection ONCE: the
// lower index keeps its face, the higher one drops out.  +1: m is a twin of k and wins (face k is empty); -1: m is a twin and loses (m
// does not cut k); 0: not a twin.  Unit normals; tol: rounding of an offset at the size of the objects.
__device__ __forceinline__ int hiv_twin(const double* __restrict__ hs, int k, int m, double a, double b, double e, double L) {
  if (!(a * a + b * b <= 1e-24) || !(fabs(e) <= 1e-12 * L)) return 0;
  if (hs[4 * m] * hs[4 * k] + hs[4 * m + 1] * hs[4 * k + 1] + hs[4 * m + 2] * hs[4 * k + 2] <= 0) return 0;      // opposite: a slab of zero width, not a twin
  return m < k ? 1 : -1;
}

// Scratch-resident fallback (arbitrary polygons up to HIV_MAXP vertices); only used for the rare faces that exceed
// the LDS capacities below.  Returns area * height (height from c); NaN on overflow.
__device__ __noinline__ double hiv_face_term(const double* __restrict__ hs, int M, int k, const double c[3], double L) {
  const HivFrame fr = hiv_frame(hs, k, c);
  if (!fr.ok) return 0;
  HivPoly P;
  P.n = 4;
  P.ps[0] = -L; P.pt[0] = -L; P.ps[1] = L; P.pt[1] = -L; P.ps[2] = L; P.pt[2] = L; P.ps[3] = -L; P.pt[3] = L;
  // pass 0: distance of every other plane's trace line from the origin; the nearest ones bound the face.
  // Clipping with the near lines first keeps the intermediate polygons small (the result is order independent).
  double dmin = 1e300;
  for (int m = 0; m < M; ++m) {
    if (m == k) continue;
    HIV_LINE(fr, hs, m, a, b, e)
    if (hiv_twin(hs, k, m, a, b, e, L) > 0) return 0;
    const double nrm = sqrt(a * a + b * b);
    if (nrm > 0) dmin = fmin(dmin, fabs(e) / nrm);
  }
  const double near_lim = 4.0 * dmin + 1e-9 * L;
  double rad2 = 2.0 * L * L;                      // squared circum-radius of the current polygon about the origin
  for (int pass = 0; pass < 2 && P.n > 0; ++pass) {
    for (int m = 0; m < M && P.n > 0; ++m) {
      if (m == k) continue;
      HIV_LINE(fr, hs, m, a, b, e)
      const double n2 = a * a + b * b;
      const bool is_near = (n2 > 0) && (e * e <= near_lim * near_lim * n2);
      if (is_near != (pass == 0)) continue;
      if (hiv_twin(hs, k, m, a, b, e, L) < 0) continue;
      // the origin is inside (e <= 0) and the whole polygon is closer to the origin than the line: nothing to cut
      if (e <= 0 && e * e >= rad2 * n2 * (1.0 + 1e-12)) continue;
      if (!hiv_clip(P, a, b, e)) return NAN;
      double r2 = 0;
      for (int v = 0; v < P.n; ++v) r2 = fmax(r2, P.ps[v] * P.ps[v] + P.pt[v] * P.pt[v]);
      rad2 = r2;
    }
  }
  if (P.n < 3) return 0;
  double area2 = 0;
  for (int v = 0; v < P.n; ++v) { const int w = (v + 1 == P.n) ? 0 : v + 1; area2 += P.ps[v] * P.pt[w] - P.ps[w] * P.pt[v]; }
  return 0.5 * fabs(area2) * fr.h;
}

// LDS-resident fast path.  Each lane owns one face; its polygon (<= HIV_CAPL vertices, lane-interleaved doubles) lives
// in LDS, nothing in scratch.  Half-spaces are expected with UNIT normals (zero normals stay zero).  The polygon is
// seeded by the (up to three) half-spaces of the faces that share an edge with this face -- known from the mesh topology
// (kernels) or from the cached hull adjacency -- which localises it immediately; it is then re-centred and every other
// half-space is rejected with one dot product (polygon inside the ball around its centre inside the half-space) before
// the exact in-plane test.  A convex polygon cut by a line loses ONE cyclic run of vertices and gains two, which is
// done in place.  Anything unusual (capacity, more than one run because of rounding) sets `fallback` and the caller
// recomputes this face with the routine above.  The result does not depend on the clipping order (up to rounding).
#define HIV_CAPL 16
#define HIV_LCAP 56
#define HIV_NONE 0xFFFFu
struct HivLds {
  double* S; double* T;                 // polygon vertices [HIV_CAPL][64]
  unsigned short* list;                 // [HIV_LCAP][64] per-lane list of half-spaces that may cut the polygon
  const unsigned short* seed;           // [M_orig][3]: original indices of the edge-adjacent half-spaces (HIV_NONE: unknown)
  const unsigned short* pos;            // [M_orig]: original index -> index after culling (HIV_NONE: culled)
  const unsigned short* orig;           // [M]: index after culling -> original index
};
static inline size_t hiv_poly_bytes() { return (size_t)2 * HIV_CAPL * 64 * sizeof(double) + (size_t)HIV_LCAP * 64 * sizeof(unsigned short); }
__device__ __forceinline__ size_t hiv_poly_bytes_dev() { return (size_t)2 * HIV_CAPL * 64 * sizeof(double) + (size_t)HIV_LCAP * 64 * sizeof(unsigned short); }

// returns false when the fallback is needed
__device__ __forceinline__ bool hiv_clip_lds(const HivLds& W, int lane, int& n, double a, double b, double e) {
  unsigned int in_mask = 0;
  for (int v = 0; v < n; ++v) {
    const double f = a * W.S[v * 64 + lane] + b * W.T[v * 64 + lane] + e;
    if (f <= 0) in_mask |= 1u << v;
  }
  const unsigned int full = (1u << n) - 1u;
  if (in_mask == full) return true;
  if (in_mask == 0) { n = 0; return true; }
  const unsigned int out = ~in_mask & full;
  const unsigned int prev_out = ((out << 1) | (out >> (n - 1))) & full;     // bit i = out[i-1 cyclic]
  const unsigned int starts = out & ~prev_out;
  if (__popc(starts) != 1) return false;
  const int i = __ffs((int)starts) - 1;        // first vertex of the outside run
  const int k = __popc(out);                   // its length
  const int nn = n - k + 2;
  if (nn > HIV_CAPL) return false;
  const int im1 = (i == 0) ? n - 1 : i - 1;
  int j1 = i + k - 1; if (j1 >= n) j1 -= n;
  int j2 = i + k; if (j2 >= n) j2 -= n;
  double As, At, Bs, Bt;
  {
    const double sp = W.S[im1 * 64 + lane], tp = W.T[im1 * 64 + lane], sc = W.S[i * 64 + lane], tc = W.T[i * 64 + lane];
    const double fp = a * sp + b * tp + e, fc = a * sc + b * tc + e;
    const double w = fp / (fp - fc);
    As = sp + w * (sc - sp); At = tp + w * (tc - tp);
  }
  {
    const double sp = W.S[j1 * 64 + lane], tp = W.T[j1 * 64 + lane], sc = W.S[j2 * 64 + lane], tc = W.T[j2 * 64 + lane];
    const double fp = a * sp + b * tp + e, fc = a * sc + b * tc + e;
    const double w = fp / (fp - fc);
    Bs = sp + w * (sc - sp); Bt = tp + w * (tc - tp);
  }
  if (i + k <= n) {                             // run does not wrap: [0,i) stays, A, B, then the tail [i+k, n)
    const int shift = 2 - k;
    if (shift < 0) { for (int v = i + k; v < n; ++v) { W.S[(v + shift) * 64 + lane] = W.S[v * 64 + lane]; W.T[(v + shift) * 64 + lane] = W.T[v * 64 + lane]; } }
    else if (shift > 0) { for (int v = n - 1; v >= i + k; --v) { W.S[(v + 1) * 64 + lane] = W.S[v * 64 + lane]; W.T[(v + 1) * 64 + lane] = W.T[v * 64 + lane]; } }
    W.S[i * 64 + lane] = As; W.T[i * 64 + lane] = At; W.S[(i + 1) * 64 + lane] = Bs; W.T[(i + 1) * 64 + lane] = Bt;
  } else {                                      // run wraps: inside vertices are [w0, i)
    const int w0 = i + k - n;
    if (w0 > 0) for (int v = w0; v < i; ++v) { W.S[(v - w0) * 64 + lane] = W.S[v * 64 + lane]; W.T[(v - w0) * 64 + lane] = W.T[v * 64 + lane]; }
    W.S[(n - k) * 64 + lane] = As; W.T[(n - k) * 64 + lane] = At; W.S[(n - k + 1) * 64 + lane] = Bs; W.T[(n - k + 1) * 64 + lane] = Bt;
  }
  n = nn;
  return true;
}

__device__ __forceinline__ double hiv_rad2(const HivLds& W, int lane, int n) {
  double r2 = 0;
  for (int v = 0; v < n; ++v) { const double s = W.S[v * 64 + lane], t = W.T[v * 64 + lane]; r2 = fmax(r2, s * s + t * t); }
  return r2;
}

__device__ __forceinline__ double hiv_face_term_lds(const double* __restrict__ hs, int M, int k, const double c[3], double L, const HivLds& W,
                                                    int lane, bool& fallback, int* dbg, const double* __restrict__ balls = nullptr) {
#pragma clang fp contract(fast)
  fallback = false;
  HivFrame fr = hiv_frame(hs, k, c);
  if (!fr.ok) return 0;
  int sd[3];
  {
    const int o_ = W.orig[k];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const unsigned int t = W.seed[3 * o_ + q];
      const unsigned int pp = (t == HIV_NONE) ? HIV_NONE : (unsigned int)W.pos[t];
      sd[q] = (pp == HIV_NONE) ? -1 : (int)pp;
    }
  }
  int n = 4;
  // initial polygon: the intersection region lies inside the outer balls of BOTH polyhedra, so this face's polygon lies inside
  // the discs in which its plane cuts them: start from the intersection of the discs' bounding squares instead of the +-L box
  // (a tight start makes the cutter lists short: most half-spaces cannot reach a polygon of the objects' own size)
  double s_lo = -L, s_hi = L, t_lo = -L, t_hi = L;
  if (balls) {
#pragma unroll
    for (int bq = 0; bq < 2; ++bq) {
      const double qz = balls[4 * bq] - fr.oz, qy = balls[4 * bq + 1] - fr.oy, qx = balls[4 * bq + 2] - fr.ox, r = balls[4 * bq + 3];
      const double dn = qz * hs[4 * k] + qy * hs[4 * k + 1] + qx * hs[4 * k + 2];      // signed distance of the ball centre to the plane (unit normal)
      const double rho2 = r * r - dn * dn;
      if (!(rho2 > 0)) return 0;                                                        // the plane misses the ball: empty face
      const double rho = sqrt(rho2) * (1.0 + 1e-9) + 1e-9;
      const double s0 = qz * fr.uz + qy * fr.uy + qx * fr.ux, t0 = qz * fr.vz + qy * fr.vy + qx * fr.vx;
      s_lo = fmax(s_lo, s0 - rho); s_hi = fmin(s_hi, s0 + rho); t_lo = fmax(t_lo, t0 - rho); t_hi = fmin(t_hi, t0 + rho);
    }
    if (!(s_lo < s_hi && t_lo < t_hi)) return 0;
  }
  W.S[0 * 64 + lane] = s_lo; W.T[0 * 64 + lane] = t_lo; W.S[1 * 64 + lane] = s_hi; W.T[1 * 64 + lane] = t_lo;
  W.S[2 * 64 + lane] = s_hi; W.T[2 * 64 + lane] = t_hi; W.S[3 * 64 + lane] = s_lo; W.T[3 * 64 + lane] = t_hi;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    if (sd[q] < 0 || n == 0) continue;
    HIV_LINE(fr, hs, sd[q], a, b, e)
    if (!hiv_clip_lds(W, lane, n, a, b, e)) { fallback = true; return 0; }
  }
  if (n < 3) return 0;
  {                                              // re-centre the in-plane frame on the polygon
    double ms = 0, mt = 0;
    for (int v = 0; v < n; ++v) { ms += W.S[v * 64 + lane]; mt += W.T[v * 64 + lane]; }
    ms /= n; mt /= n;
    for (int v = 0; v < n; ++v) { W.S[v * 64 + lane] -= ms; W.T[v * 64 + lane] -= mt; }
    fr.oz += ms * fr.uz + mt * fr.vz; fr.oy += ms * fr.uy + mt * fr.vy; fr.ox += ms * fr.ux + mt * fr.vx;
  }
  double rad2 = hiv_rad2(W, lane, n);
  const double radm = sqrt(rad2) * (1.0 + 1e-12);
  // phase 1 (no divergence): half-spaces whose TRACE LINE in this face's plane reaches the disc around the polygon go to this
  // lane's list.  (The 3D ball test alone -- half-space does not contain the ball around the polygon -- let through every
  // half-space that is steep against this face: 77 % of the faces overflowed the list into the divergent loop below.  The
  // in-plane test is the one phase 2 applies anyway; here it runs for all half-spaces in lock step.)
  int nl = 0, m_rest = M;
  for (int m0 = 0; m0 < M; m0 += 4) {
    double e4[4], n4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = (m0 + q < M) ? m0 + q : M - 1;
      const double mz_ = hs[4 * m], my_ = hs[4 * m + 1], mx_ = hs[4 * m + 2];
      e4[q] = mz_ * fr.oz + my_ * fr.oy + mx_ * fr.ox + hs[4 * m + 3];
      const double a_ = mz_ * fr.uz + my_ * fr.uy + mx_ * fr.ux, b_ = mz_ * fr.vz + my_ * fr.vy + mx_ * fr.vx;
      n4[q] = a_ * a_ + b_ * b_;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = m0 + q;
      bool misses = (e4[q] + radm <= 0) || (e4[q] <= 0 && e4[q] * e4[q] >= rad2 * n4[q] * (1.0 + 1e-12));
      if (m < M && m != k && n4[q] <= 1e-24 && fabs(e4[q]) <= 1e-12 * L) {            // coincident twin (hiv_twin)
        const int tw = hiv_twin(hs, k, m, 0.0, 0.0, e4[q], L);
        if (tw > 0) return 0;
        if (tw < 0) misses = true;
      }
      const bool cand = (m < M) && !misses && m != k && m != sd[0] && m != sd[1] && m != sd[2];
      if (cand) {
        if (nl < HIV_LCAP) { W.list[nl * 64 + lane] = (unsigned short)m; ++nl; }
        else if (m < m_rest) m_rest = m;
      }
    }
  }
  dbg[0] += nl; if (m_rest < M) dbg[2] += 1;
  // phase 2: every lane walks its own short list -- twice.  The first pass only clips with DEEP cutters (trace line closer to the
  // polygon centre than half its radius, or centre outside): they shrink the polygon quickly, so that in the second pass most of
  // the shallow cutters no longer reach it and are rejected by the one-comparison test instead of a clip (the result does not
  // depend on the clipping order).
  for (int pass = 0; pass < 2; ++pass) {
    for (int t = 0; t < nl && n > 0; ++t) {
      const int m = W.list[t * 64 + lane];
      if (m == (int)HIV_NONE) continue;
      HIV_LINE(fr, hs, m, a, b, e)
      const double n2 = a * a + b * b;
      if (e <= 0 && e * e >= rad2 * n2 * (1.0 + 1e-12)) { W.list[t * 64 + lane] = (unsigned short)HIV_NONE; continue; }   // does not reach the polygon (it only shrinks)
      if (pass == 0 && e <= 0 && e * e >= 0.25 * rad2 * n2) continue;                                                       // shallow: second pass
      W.list[t * 64 + lane] = (unsigned short)HIV_NONE;
      dbg[1] += 1;
      if (!hiv_clip_lds(W, lane, n, a, b, e)) { fallback = true; return 0; }
      rad2 = hiv_rad2(W, lane, n);
    }
  }
  // list overflow (rare): the remaining half-spaces one by one
  for (int m = m_rest; m < M && n > 0; ++m) {
    if (m == k || m == sd[0] || m == sd[1] || m == sd[2]) continue;
    HIV_LINE(fr, hs, m, a, b, e)
    const double n2 = a * a + b * b;
    if (e <= 0 && e * e >= rad2 * n2 * (1.0 + 1e-12)) continue;
    if (hiv_twin(hs, k, m, a, b, e, L) < 0) continue;
    if (!hiv_clip_lds(W, lane, n, a, b, e)) { fallback = true; return 0; }
    rad2 = hiv_rad2(W, lane, n);
  }
  if (n < 3) return 0;
  double area2 = 0;
  const double s0 = W.S[lane], t0 = W.T[lane];
  double sp = s0, tp = t0;
  for (int v = 1; v < n; ++v) { const double sc = W.S[v * 64 + lane], tc = W.T[v * 64 + lane]; area2 += sp * tc - sc * tp; sp = sc; tp = tc; }
  area2 += sp * t0 - s0 * tp;
  return 0.5 * fabs(area2) * fr.h;
}

// sum of the face terms of the M half-spaces in hs (one wave); NaN when a face exceeded even the fallback capacity
__device__ __forceinline__ double hiv_volume_wave(const double* __restrict__ hs, int M, const double c[3], double L, const HivLds& W, int lane,
                                                  Stats* st, const double* __restrict__ balls = nullptr) {
  double acc = 0;
  int nfb = 0;
  int dbg[3] = {0, 0, 0};
  for (int k0 = 0; k0 < M; k0 += 64) {
    const int k = k0 + lane;
    if (k < M) {
      bool fb;
      double term = hiv_face_term_lds(hs, M, k, c, L, W, lane, fb, dbg, balls);
      if (fb) { term = hiv_face_term(hs, M, k, c, L); ++nfb; }
      acc += term;
    }
  }
  for (int o = 32; o; o >>= 1) {
    acc += __shfl_xor(acc, o); nfb += __shfl_xor(nfb, o);
    dbg[0] += __shfl_xor(dbg[0], o); dbg[1] += __shfl_xor(dbg[1], o); dbg[2] += __shfl_xor(dbg[2], o);
  }
  if (lane == 0) {
    atomicAdd(&st->hiv_faces, (unsigned long long)M); if (nfb) atomicAdd(&st->hiv_fallback, (unsigned long long)nfb);
    atomicAdd(&st->hiv_list, (unsigned long long)dbg[0]); atomicAdd(&st->hiv_clips, (unsigned long long)dbg[1]);
    if (dbg[2]) atomicAdd(&st->hiv_rest, (unsigned long long)dbg[2]);
  }
  return acc / 3.0;
}

// The same sum by a workgroup of NW waves (k_stage3x / k_stage4x): wave w takes the faces k0 + 64 w + lane, every term goes to
// terms[k] (LDS), and wave 0 adds them up in exactly the order of the one-wave routine (lane l: faces l, l + 64, ...; then the xor
// butterfly) -- the result is bit-identical, only the latency of a pair is 1/NW.  W = THIS wave's polygon workspace.  The value is
// returned in wave 0; every wave must call (workgroup barrier inside).
template <int NW>
__device__ __forceinline__ double hiv_volume_block(const double* __restrict__ hs, int M, const double c[3], double L, const HivLds& W, int lane, int wave,
                                                   double* __restrict__ terms, Stats* st, const double* __restrict__ balls) {
  int nfb = 0;
  int dbg[3] = {0, 0, 0};
  for (int k0 = 0; k0 < M; k0 += 64 * NW) {
    const int k = k0 + 64 * wave + lane;
    if (k < M) {
      bool fb;
      double term = hiv_face_term_lds(hs, M, k, c, L, W, lane, fb, dbg, balls);
      if (fb) { term = hiv_face_term(hs, M, k, c, L); ++nfb; }
      terms[k] = term;
    }
  }
  for (int o = 32; o; o >>= 1) {
    nfb += __shfl_xor(nfb, o);
    dbg[0] += __shfl_xor(dbg[0], o); dbg[1] += __shfl_xor(dbg[1], o); dbg[2] += __shfl_xor(dbg[2], o);
  }
  if (lane == 0) {
    if (wave == 0) atomicAdd(&st->hiv_faces, (unsigned long long)M);
    if (nfb) atomicAdd(&st->hiv_fallback, (unsigned long long)nfb);
    atomicAdd(&st->hiv_list, (unsigned long long)dbg[0]); atomicAdd(&st->hiv_clips, (unsigned long long)dbg[1]);
    if (dbg[2]) atomicAdd(&st->hiv_rest, (unsigned long long)dbg[2]);
  }
  __syncthreads();
  double acc = 0;
  if (wave == 0) {
    for (int k0 = 0; k0 < M; k0 += 64) { const int k = k0 + lane; if (k < M) acc += terms[k]; }
    for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o);
  }
  return acc / 3.0;
}

// Cull + compact + normalise the M half-spaces in hs (one wave, in place).  A half-space of one polyhedron that contains
// the whole outer ball of the OTHER polyhedron cannot bound the intersection (exact, 1e-6 safety margin).
// `second(k)` tells whether original half-space k belongs to polyhedron 2.  Fills pos/orig; returns the kept count.
// The kept half-spaces are also translated so that the interior point c becomes the origin (offset = n.c + d < 0).
// BS = false: called by ONE wave of a larger workgroup (k_stage3x / k_stage4x): no workgroup barrier -- a wave's own LDS accesses are
// processed in order and all its lanes read a chunk before any of them writes, which is all the compaction needs.
template <class Second, bool BS = true>
__device__ __forceinline__ int hiv_cull_wave(double* hs, int M, const double b1[4], const double b2[4], const double c[3], unsigned short* pos,
                                             unsigned short* orig, int lane, Second second) {
  int kept = 0;
  for (int k0 = 0; k0 < M; k0 += 64) {
    const int k = k0 + lane;
    bool keep = false;
    double h0 = 0, h1 = 0, h2 = 0, h3 = 0;
    if (k < M) {
      h0 = hs[4 * k]; h1 = hs[4 * k + 1]; h2 = hs[4 * k + 2]; h3 = hs[4 * k + 3];
      const double* ob = second(k) ? b1 : b2;      // plane of polyhedron 2 vs ball of polyhedron 1 and vice versa
      const double nn = sqrt(h0 * h0 + h1 * h1 + h2 * h2);
      keep = !(h0 * ob[0] + h1 * ob[1] + h2 * ob[2] + h3 + nn * ob[3] <= 0);
      h3 += h0 * c[0] + h1 * c[1] + h2 * c[2];
      if (nn > 0) { h0 /= nn; h1 /= nn; h2 /= nn; h3 /= nn; }
    }
    const unsigned long long mk = __ballot(keep);
    if (BS) __syncthreads(); else __builtin_amdgcn_wave_barrier();      // all reads of this chunk done before compacted writes land
    if (k < M) {
      if (keep) {
        const int p_ = kept + __popcll(mk & ((1ull << lane) - 1));
        hs[4 * p_] = h0; hs[4 * p_ + 1] = h1; hs[4 * p_ + 2] = h2; hs[4 * p_ + 3] = h3;
        pos[k] = (unsigned short)p_; orig[p_] = (unsigned short)k;
      } else pos[k] = (unsigned short)HIV_NONE;
    }
    kept += __popcll(mk);
    if (BS) __syncthreads(); else __builtin_amdgcn_wave_barrier();
  }
  return kept;
}

// Rigorous lower AND upper bound of the volume of the convex region K = {x : n_m.x + d_m <= 0 for all m} (origin strictly
// inside) from one ray cast per ray direction u_y (boundary point w_y = t_y u_y on half-space m_y):
//   lower: K is convex, so every tetrahedron (0, w_a, w_b, w_c) over a triangle of the ray mesh lies in K; these are cones
//          over a triangulation of the sphere of directions and do not overlap (the ray mesh is the hull of the ray
//          directions and contains the origin, rays.py);
//   upper: K lies inside each of its half-spaces, so (cone over the triangle) n K is inside (cone) n half-space m_x for each
//          corner x, a tetrahedron with volume |det(w_a,w_b,w_c)|/6 * prod_y s_y, s_y = -d_x / (n_x.w_y) >= 1; take the
//          smallest of the three.
// ~100x cheaper than the exact volume and decisive unless the ratio to the threshold is within the gap between the two
// (a few percent).  wv: LDS 3R doubles, hit: LDS R shorts.  ub = +inf when no bound could be formed.
template <int NB>
__device__ __forceinline__ void hiv_bounds_wave(const double* __restrict__ hs, int M, const float* __restrict__ verts,
                                                const int* __restrict__ faces, int R, int F, double* wv, unsigned short* hit, int lane,
                                                double& lb, double& ub, int kdone = 0, const unsigned short* hitDone = nullptr) {
#pragma clang fp contract(fast)
  // kdone != 0: the caller has just evaluated a coarser mesh whose kdone directions are the first kdone of this one (k_refine_mesh
  // keeps the parent's vertices in front), over the same planes: wv[0 .. 3 kdone) holds their boundary points already (the same
  // arithmetic on the same operands: bit for bit what this loop would store) and hitDone their planes, which only move to this mesh's
  // table -- a quarter of the once-refined mesh's directions is not cast twice
  if (kdone) {
    for (int k = lane; k < kdone; k += 64) hit[k] = hitDone[k];
    __syncthreads();                                            // hitDone lies where wv[3 kdone ..) is about to be written
  }
  // ray cast: the plane loop is the outer one and a lane keeps up to NB directions in registers -- one LDS read of a plane serves
  // NB independent compare chains (a loop over planes per direction is bound by LDS latency + its loop-carried dependency:
  // 358k cycles per pair measured with the refined mesh, 80 % of stage 3)
  for (int k0 = kdone; k0 < R; k0 += 64 * NB) {
    double dz[NB], dy[NB], dx[NB], ne_b[NB], q_b[NB];
    int m_b[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int k = k0 + j * 64 + lane;
      const bool v = k < R;
      dz[j] = v ? (double)verts[3 * k] : 0.0; dy[j] = v ? (double)verts[3 * k + 1] : 0.0; dx[j] = v ? (double)verts[3 * k + 2] : 0.0;
      ne_b[j] = 1.0; q_b[j] = 0.0; m_b[j] = 0;          // boundary distance t = ne_b / q_b, kept as a fraction
    }
#pragma unroll 2
    for (int m = 0; m < M; ++m) {
      const double h0 = hs[4 * m], h1 = hs[4 * m + 1], h2 = hs[4 * m + 2], ne = -hs[4 * m + 3];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const double q = h0 * dz[j] + h1 * dy[j] + h2 * dx[j];
        if (q > 0 && ne * q_b[j] < ne_b[j] * q) { ne_b[j] = ne; q_b[j] = q; m_b[j] = m; }
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int k = k0 + j * 64 + lane;
      if (k < R) {
        const double t = (q_b[j] > 0) ? ne_b[j] / q_b[j] : 0.0;
        wv[3 * k] = t * dz[j]; wv[3 * k + 1] = t * dy[j]; wv[3 * k + 2] = t * dx[j];
        hit[k] = (unsigned short)((q_b[j] > 0) ? m_b[j] : HIV_NONE);
      }
    }
  }
  __syncthreads();
  double accl = 0, accu = 0;
  bool bad = false;
  for (int f = lane; f < F; f += 64) {
    const int iv[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    double w[3][3];
#pragma unroll
    for (int y = 0; y < 3; ++y) { w[y][0] = wv[3 * iv[y]]; w[y][1] = wv[3 * iv[y] + 1]; w[y][2] = wv[3 * iv[y] + 2]; }
    const double det = fabs(w[0][0] * (w[1][1] * w[2][2] - w[1][2] * w[2][1]) + w[0][1] * (w[1][2] * w[2][0] - w[1][0] * w[2][2]) +
                            w[0][2] * (w[1][0] * w[2][1] - w[1][1] * w[2][0]));
    accl += det;
    double best = 1e300;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      const unsigned int m = hit[iv[x]];
      if (m == HIV_NONE) continue;
      const double nz = hs[4 * m], ny = hs[4 * m + 1], nx = hs[4 * m + 2], ne = -hs[4 * m + 3];
      double qp = 1.0;
      bool ok = true;
#pragma unroll
      for (int y = 0; y < 3; ++y) {
        const double q = nz * w[y][0] + ny * w[y][1] + nx * w[y][2];
        if (!(q > 0)) ok = false;
        qp *= q;
      }
      if (ok) best = fmin(best, (ne * ne * ne) / qp);            // prod_y s_y = prod_y ne / q_y
    }
    if (best >= 1e300) bad = true;
    accu += det * fmax(best, 1.0);
  }
  for (int o = 32; o; o >>= 1) { accl += __shfl_xor(accl, o); accu += __shfl_xor(accu, o); }
  bad = __any(bad);
  __syncthreads();
  lb = accl / 6.0;
  ub = bad ? 1e300 : accu / 6.0;
}

// The same bounds by the NW waves of a workgroup over a finer direction mesh (k_stage3x / k_stage4x, before they integrate: the
// mesh refined twice has 16x the triangles of the ray mesh, its gap between the bounds is ~1/4 of the once-refined mesh's, and a ray
// cast over it costs ~1/10 of the exact volume it makes unnecessary for most of the pairs that reach these kernels).  Any summation
// order gives rigorous bounds (the callers' 1e-9 margins cover the rounding).  red: 2 NW doubles of LDS.  Workgroup barriers inside.
template <int NW, int NB>
__device__ __forceinline__ void hiv_bounds_block(const double* __restrict__ hs, int M, const float* __restrict__ verts,
                                                 const int* __restrict__ faces, int R, int F, double* wv, unsigned short* hit, double* red,
                                                 int tid, double& lb, double& ub) {
#pragma clang fp contract(fast)
  constexpr int NT = 64 * NW;
  for (int k0 = 0; k0 < R; k0 += NT * NB) {
    double dz[NB], dy[NB], dx[NB], ne_b[NB], q_b[NB];
    int m_b[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int k = k0 + j * NT + tid;
      const bool v = k < R;
      dz[j] = v ? (double)verts[3 * k] : 0.0; dy[j] = v ? (double)verts[3 * k + 1] : 0.0; dx[j] = v ? (double)verts[3 * k + 2] : 0.0;
      ne_b[j] = 1.0; q_b[j] = 0.0; m_b[j] = 0;
    }
#pragma unroll 2
    for (int m = 0; m < M; ++m) {
      const double h0 = hs[4 * m], h1 = hs[4 * m + 1], h2 = hs[4 * m + 2], ne = -hs[4 * m + 3];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const double q = h0 * dz[j] + h1 * dy[j] + h2 * dx[j];
        if (q > 0 && ne * q_b[j] < ne_b[j] * q) { ne_b[j] = ne; q_b[j] = q; m_b[j] = m; }
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int k = k0 + j * NT + tid;
      if (k < R) {
        const double t = (q_b[j] > 0) ? ne_b[j] / q_b[j] : 0.0;
        wv[3 * k] = t * dz[j]; wv[3 * k + 1] = t * dy[j]; wv[3 * k + 2] = t * dx[j];
        hit[k] = (unsigned short)((q_b[j] > 0) ? m_b[j] : HIV_NONE);
      }
    }
  }
  __syncthreads();
  double accl = 0, accu = 0;
  int bad = 0;
  for (int f = tid; f < F; f += NT) {
    const int iv[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    double w[3][3];
#pragma unroll
    for (int y = 0; y < 3; ++y) { w[y][0] = wv[3 * iv[y]]; w[y][1] = wv[3 * iv[y] + 1]; w[y][2] = wv[3 * iv[y] + 2]; }
    const double det = fabs(w[0][0] * (w[1][1] * w[2][2] - w[1][2] * w[2][1]) + w[0][1] * (w[1][2] * w[2][0] - w[1][0] * w[2][2]) +
                            w[0][2] * (w[1][0] * w[2][1] - w[1][1] * w[2][0]));
    accl += det;
    double best = 1e300;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      const unsigned int m = hit[iv[x]];
      if (m == HIV_NONE) continue;
      const double nz = hs[4 * m], ny = hs[4 * m + 1], nx = hs[4 * m + 2], ne = -hs[4 * m + 3];
      double qp = 1.0;
      bool ok = true;
#pragma unroll
      for (int y = 0; y < 3; ++y) {
        const double q = nz * w[y][0] + ny * w[y][1] + nx * w[y][2];
        if (!(q > 0)) ok = false;
        qp *= q;
      }
      if (ok) best = fmin(best, (ne * ne * ne) / qp);
    }
    if (best >= 1e300) bad = 1;
    accu += det * fmax(best, 1.0);
  }
  for (int o = 32; o; o >>= 1) { accl += __shfl_xor(accl, o); accu += __shfl_xor(accu, o); }
  if ((tid & 63) == 0) { red[2 * (tid >> 6)] = accl; red[2 * (tid >> 6) + 1] = accu; }
  const bool anybad = __syncthreads_or(bad) != 0;
  accl = 0; accu = 0;
#pragma unroll
  for (int w_ = 0; w_ < NW; ++w_) { accl += red[2 * w_]; accu += red[2 * w_ + 1]; }
  __syncthreads();
  lb = accl / 6.0;
  ub = anybad ? 1e300 : accu / 6.0;
}

// edge adjacency of the ray mesh: adj[3f + e] = face sharing edge e = (v_e, v_{e+1}) of face f (the lowest-numbered one), or -1.
// One wave per face, the lanes share the scan over the other faces (the meshes of the finer bounds have 4 F and 16 F faces).
__global__ void __launch_bounds__(64) k_face_adj(const int* __restrict__ faces, int F, int* __restrict__ adj) {
  const int f = blockIdx.x, lane = threadIdx.x;
  if (f >= F) return;
  const int v[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
  int found[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff};
  for (int g = lane; g < F; g += 64) {
    if (g == f) continue;
    const int a = faces[3 * g], b = faces[3 * g + 1], c = faces[3 * g + 2];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const int x = v[e], y = v[(e + 1) % 3];
      if ((a == x || b == x || c == x) && (a == y || b == y || c == y) && g < found[e]) found[e] = g;
    }
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    int m = found[e];
    for (int o = 32; o; o >>= 1) { const int t = __shfl_xor(m, o); m = t < m ? t : m; }
    if (lane == 0) adj[3 * f + e] = m == 0x7fffffff ? -1 : m;
  }
}

// Direction mesh for the volume bounds: the ray mesh with every triangle split in four at its edge midpoints (directions
// R + edge id).  The cones over the sub-triangles tile the cone of their parent, so the arguments above hold unchanged, and the
// gap between the two bounds shrinks ~4x: the exact volume (100x the cost) is needed for ~4x fewer pairs.
__global__ void k_refine_edges(const int* __restrict__ faces, const int* __restrict__ adj, int F, int* __restrict__ edgeId, int* counter) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * F) return;
  const int f = t / 3, g = adj[t];
  edgeId[t] = (g < 0 || f < g) ? atomicAdd(counter, 1) : -1;            // the face with the smaller index owns the shared edge
}
__global__ void k_refine_mesh(const float* __restrict__ verts, const int* __restrict__ faces, const int* __restrict__ adj, int R, int F,
                              const int* __restrict__ edgeId, float* __restrict__ verts2, int* __restrict__ faces2) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < R) { verts2[3 * f] = verts[3 * f]; verts2[3 * f + 1] = verts[3 * f + 1]; verts2[3 * f + 2] = verts[3 * f + 2]; }
  if (f >= F) return;
  const int v[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
  int mid[3];
  for (int e = 0; e < 3; ++e) {
    const int x = v[e], y = v[(e + 1) % 3];
    int id = edgeId[3 * f + e];
    if (id < 0) {                                                       // owned by the neighbour: its edge with the same end points
      const int g = adj[3 * f + e];
      for (int e2 = 0; e2 < 3; ++e2) {
        const int a = faces[3 * g + e2], b = faces[3 * g + (e2 + 1) % 3];
        if ((a == x && b == y) || (a == y && b == x)) id = edgeId[3 * g + e2];
      }
    } else {
      const int m = R + id;
      verts2[3 * m] = 0.5f * (verts[3 * x] + verts[3 * y]); verts2[3 * m + 1] = 0.5f * (verts[3 * x + 1] + verts[3 * y + 1]);
      verts2[3 * m + 2] = 0.5f * (verts[3 * x + 2] + verts[3 * y + 2]);
    }
    mid[e] = R + id;
  }
  int* o = faces2 + 12 * f;                                             // same orientation as the parent
  o[0] = v[0]; o[1] = mid[0]; o[2] = mid[2];
  o[3] = mid[0]; o[4] = v[1]; o[5] = mid[1];
  o[6] = mid[2]; o[7] = mid[1]; o[8] = v[2];
  o[9] = mid[0]; o[10] = mid[1]; o[11] = mid[2];
}

// The volume bounds above need the ray mesh to be a closed surface that is star-shaped about the origin (cones over its
// triangles tile the sphere of directions exactly once).  mesh[0] |= 1: an edge without a partner, |= 2: degenerate or
// degenerate face; mesh_sa = sum of the absolute solid angles (Van Oosterom & Strackee): exactly 4 pi iff the radial
// projection of the closed mesh covers the sphere once without folds.
__global__ void k_mesh_check(const float* __restrict__ verts, const int* __restrict__ faces, const int* __restrict__ adj, int F, int* mesh,
                             double* mesh_sa) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  double u[3][3];
  for (int y = 0; y < 3; ++y) {
    const int v = faces[3 * f + y];
    const double z = verts[3 * v], yy = verts[3 * v + 1], x = verts[3 * v + 2];
    const double nn = sqrt(z * z + yy * yy + x * x);
    u[y][0] = z / nn; u[y][1] = yy / nn; u[y][2] = x / nn;
  }
  const double det = u[0][0] * (u[1][1] * u[2][2] - u[1][2] * u[2][1]) + u[0][1] * (u[1][2] * u[2][0] - u[1][0] * u[2][2]) +
                     u[0][2] * (u[1][0] * u[2][1] - u[1][1] * u[2][0]);
  const double d01 = u[0][0] * u[1][0] + u[0][1] * u[1][1] + u[0][2] * u[1][2];
  const double d12 = u[1][0] * u[2][0] + u[1][1] * u[2][1] + u[1][2] * u[2][2];
  const double d20 = u[2][0] * u[0][0] + u[2][1] * u[0][1] + u[2][2] * u[0][2];
  const double sa = 2.0 * atan2(det, 1.0 + d01 + d12 + d20);
  int bad = 0;
  if (adj[3 * f] < 0 || adj[3 * f + 1] < 0 || adj[3 * f + 2] < 0) bad |= 1;
  if (!(fabs(det) > 1e-12)) bad |= 2;
  if (bad) atomicOr(&mesh[0], bad);
  atomicAdd(&mesh[det > 0 ? 1 : 2], 1);
  atomicAdd(mesh_sa, fabs(sa));
}

__global__ void __launch_bounds__(64) k_stage3(const int2* __restrict__ pairs, unsigned int nPairs, const float* __restrict__ dist,
                                               const float* __restrict__ pts, const float* __restrict__ verts,
                                               const int* __restrict__ faces, const int* __restrict__ faceAdj, int R, int F,
                                               const float* __restrict__ volume, float thr, SuppSink sink,
                                               int2* __restrict__ pairs5, unsigned int* pair5Count, Stats* st, unsigned int wsBytes,
                                               const float* __restrict__ bverts, const int* __restrict__ bfaces, int bR, int bF,
                                               double* __restrict__ volOut = nullptr, int2* __restrict__ pairsX = nullptr,
                                               unsigned int* __restrict__ nX = nullptr) {
  // pairsX != nullptr: a pair the bounds leave undecided is queued for k_stage3x (NW waves per pair) instead of being integrated here
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* hs = (double*)smem;                 // 2F * 4
  float* pv1 = (float*)(hs + 8 * F);          // 3R   (dead once hs is built: aliased by the polygon workspace)
  float* pv2 = pv1 + 3 * R;                   // 3R
  // lean (a bounds-only launch, pairsX != nullptr): the adjacency seeds are only read by the exact routine, and the cull's pos / orig
  // tables by nobody -- no seed table, pos / orig at the start of the workspace (free between the half-space build and the ray cast):
  // 21.9 instead of 25.6 KB per wave, seven waves per CU instead of six
  const bool lean = (wsBytes & SD_LEAN_BIT) != 0;
  unsigned short* seed = (unsigned short*)(smem + (size_t)8 * F * sizeof(double) + (wsBytes & SD_WS_MASK));   // 2F * 3
  unsigned short* pos = lean ? (unsigned short*)(hs + 8 * F) : seed + 6 * F;         // 2F
  unsigned short* orig = pos + 2 * F;         // 2F
  HivLds W;
  W.S = hs + 8 * F; W.T = W.S + HIV_CAPL * 64; W.list = (unsigned short*)(W.T + HIV_CAPL * 64); W.seed = seed; W.pos = pos; W.orig = orig;
  const int lane = threadIdx.x;
  if (!lean)
  for (int idx = lane; idx < 6 * F; idx += 64) {            // half-space 2f+w belongs to face f of polyhedron w (interleaved)
    const int o_ = idx / 3, e_ = idx - 3 * o_;
    const int a_ = faceAdj[3 * (o_ >> 1) + e_];
    seed[idx] = (unsigned short)(a_ < 0 ? HIV_NONE : (unsigned int)(2 * a_ + (o_ & 1)));
  }
  const bool prof = (wsBytes & SD_PROF_BIT) != 0;
  for (unsigned int p = blockIdx.x; p < nPairs; p += gridDim.x) {
    const long long t0 = prof ? clock64() : 0;
    long long t1 = 0, t2 = 0, t3 = 0;
    const int2 ij = pairs[p];
    __syncthreads();
    const float* c1 = pts + 3 * (size_t)ij.x;
    const float* c2 = pts + 3 * (size_t)ij.y;
    for (int k = lane; k < R; k += 64) {
      const float d1 = dist[(size_t)ij.x * R + k], d2 = dist[(size_t)ij.y * R + k];
      pv1[3 * k] = c1[0] + d1 * verts[3 * k]; pv1[3 * k + 1] = c1[1] + d1 * verts[3 * k + 1]; pv1[3 * k + 2] = c1[2] + d1 * verts[3 * k + 2];
      pv2[3 * k] = c2[0] + d2 * verts[3 * k]; pv2[3 * k + 1] = c2[1] + d2 * verts[3 * k + 1]; pv2[3 * k + 2] = c2[2] + d2 * verts[3 * k + 2];
    }
    __syncthreads();
    for (int f = lane; f < F; f += 64) {
      const int iA = faces[3 * f], iB = faces[3 * f + 1], iC = faces[3 * f + 2];
      sd3::build_halfspace(&pv1[3 * iA], &pv1[3 * iB], &pv1[3 * iC], &hs[4 * (2 * f)]);
      sd3::build_halfspace(&pv2[3 * iA], &pv2[3 * iB], &pv2[3 * iC], &hs[4 * (2 * f + 1)]);
    }
    __syncthreads();
    if (prof) t1 = clock64();
    const int M = 2 * F;
    double c[3];
    c[0] = .5 * (c1[0] + c2[0]); c[1] = .5 * (c1[1] + c2[1]); c[2] = .5 * (c1[2] + c2[2]);   // :857-859 (float add, then *.5 in double)
    bool infeasible = false;
    for (int k = lane; k < M; k += 64) {
      double dd = hs[4 * k + 3];
      dd += hs[4 * k] * c[0]; dd += hs[4 * k + 1] * c[1]; dd += hs[4 * k + 2] * c[2];
      if (dd > 0 || !(dd < 0)) infeasible = true;     // dist > 0 -> error; dist == 0 -> division by zero -> error
    }
    infeasible = __any(infeasible);
    double vol = 0;
    int Mc = M;
    bool deferred = false;
    if (!infeasible) {
      double ext = 0, ext1 = 0, ext2 = 0;
      for (int k = lane; k < R; k += 64) {
        const float e1 = dist[(size_t)ij.x * R + k], e2 = dist[(size_t)ij.y * R + k];
        ext1 = fmax(ext1, (double)e1); ext2 = fmax(ext2, (double)e2);
      }
      for (int o = 32; o; o >>= 1) { ext1 = fmax(ext1, __shfl_xor(ext1, o)); ext2 = fmax(ext2, __shfl_xor(ext2, o)); }
      ext = fmax(ext1, ext2);
      __syncthreads();
      {
        const double b1[4] = {(double)c1[0], (double)c1[1], (double)c1[2], ext1 * (1.0 + 1e-6) + 1e-6};
        const double b2[4] = {(double)c2[0], (double)c2[1], (double)c2[2], ext2 * (1.0 + 1e-6) + 1e-6};
        Mc = hiv_cull_wave(hs, M, b1, b2, c, pos, orig, lane, [](int k) { return (k & 1) != 0; });
      }
      if (prof) t2 = clock64();
      const double A_min_d = (double)fminf(volume[ij.x], volume[ij.y]) + 1e-10;
      const double thr_hi = (double)thr + 1e-5 * fabs((double)thr) + 1e-7;
      const double zero3[3] = {0, 0, 0};
      const double thr_lo = (double)thr - 1e-5 * fabs((double)thr) - 1e-7;
      double lb, ub;
      // coarse direction mesh (the rays) first; the refined one (4x the cost) only for the pairs it leaves undecided
      hiv_bounds_wave<2>(hs, Mc, verts, faces, R, F, W.S, (unsigned short*)(W.S + 3 * R), lane, lb, ub);
      if (bR != R && !(lb * (1.0 - 1e-9) / A_min_d > thr_hi) && !(ub * (1.0 + 1e-9) / A_min_d < thr_lo)) {
        const double lb0 = lb, ub0 = ub;
        if (wsBytes & SD_NOREUSE_BIT) hiv_bounds_wave<6>(hs, Mc, bverts, bfaces, bR, bF, W.S, (unsigned short*)(W.S + 3 * bR), lane, lb, ub);
        else hiv_bounds_wave<5>(hs, Mc, bverts, bfaces, bR, bF, W.S, (unsigned short*)(W.S + 3 * bR), lane, lb, ub, R, (const unsigned short*)(W.S + 3 * R));
        lb = fmax(lb, lb0); ub = fmin(ub, ub0);
      }
      if (prof) t3 = clock64();
      if (lb * (1.0 - 1e-9) / A_min_d > thr_hi && !(wsBytes >> 31)) {
        vol = lb;                                       // certainly above the threshold: same decision as the exact volume
        if (lane == 0) atomicAdd(&st->lb_decided, 1ull);
      } else if (ub * (1.0 + 1e-9) / A_min_d < thr_lo && !(wsBytes >> 31)) {
        vol = ub;                                       // certainly not above the threshold
        if (lane == 0) atomicAdd(&st->ub_decided, 1ull);
      } else if (pairsX) {
        deferred = true;
        if (lane == 0) pairsX[atomicAdd(nX, 1u)] = ij;
      } else {
        const double sep = sqrt((double)(c1[0] - c2[0]) * (c1[0] - c2[0]) + (double)(c1[1] - c2[1]) * (c1[1] - c2[1]) + (double)(c1[2] - c2[2]) * (c1[2] - c2[2]));
        const double L = 4.0 * (2.0 * ext + sep + 1.0);
        const double balls[8] = {(double)c1[0] - c[0], (double)c1[1] - c[1], (double)c1[2] - c[2], ext1 * (1.0 + 1e-6) + 1e-6,
                                 (double)c2[0] - c[0], (double)c2[1] - c[1], (double)c2[2] - c[2], ext2 * (1.0 + 1e-6) + 1e-6};
        vol = hiv_volume_wave(hs, Mc, zero3, L, W, lane, st, balls);
      }
    }
    if (prof && lane == 0 && t3) {
      const long long t4 = clock64();
      atomicAdd(&st->cyc[0], (unsigned long long)(t1 - t0)); atomicAdd(&st->cyc[1], (unsigned long long)(t2 - t1));
      atomicAdd(&st->cyc[2], (unsigned long long)(t3 - t2)); atomicAdd(&st->cyc[3], (unsigned long long)(t4 - t3));
      atomicAdd(&st->cyc[4], (unsigned long long)(t4 - t0)); atomicAdd(&st->cyc[5], 1ull);
    }
    if (deferred) continue;
    if (volOut) { if (lane == 0) volOut[p] = vol; continue; }     // pair-level probe (sd_hiv_pairs_device): the volume itself
    if (lane == 0) {
      atomicAdd(&st->kernel, 1ull);
      if (vol != vol) atomicAdd(&st->overflow, 1ull);   // polygon capacity overflow (reported as an error by the host)
      const float A_inter_kernel = (float)vol;                                  // function returns float :679
      const float A_min = fminf(volume[ij.x], volume[ij.y]);
      const float iou = (float)((double)A_inter_kernel / ((double)A_min + 1e-10));   // :1269
      if (fabsf(iou - thr) < 1e-6f) atomicAdd(&st->near_thr, 1ull);      // (a flip by the <= 1e-9 volume deviation from Qhull would need |iou - thr| ~ 1e-9)
      if (iou > thr) { sink.suppress(ij.x, ij.y); atomicAdd(&st->sup_kernel, 1ull); }
      else pairs5[atomicAdd(pair5Count, 1u)] = ij;
    }
  }
}

// Exact kernel ∩ kernel volume of the pairs the bounds left undecided (queued by k_stage3), NW waves per pair.  An exact volume is
// ~2 M wave cycles (one lane per face: six passes over the 2F half-spaces), ~1 ms: with one wave per pair every launch of a round
// lasted at least that long, however few pairs it held.  Here the faces of a pair are spread over 64 NW lanes (the culled
// half-spaces usually fit one pass), the terms are added in the one-wave order (hiv_volume_block: bit-identical volume).
// LDS: hs | wave 0's workspace (aliases the vertex staging) | seed pos orig | terms | the other waves' workspaces.
struct OddIsSecond { __device__ bool operator()(int k) const { return (k & 1) != 0; } };
template <int NW>
__global__ void __launch_bounds__(64 * NW) k_stage3x(const int2* __restrict__ pairs, const unsigned int* __restrict__ nPairsPtr, unsigned int nPairsImm,
                                                     const float* __restrict__ dist, const float* __restrict__ pts, const float* __restrict__ verts,
                                                     const int* __restrict__ faces, const int* __restrict__ faceAdj, int R, int F,
                                                     const float* __restrict__ volume, float thr, SuppSink sink, int2* __restrict__ pairs5,
                                                     unsigned int* pair5Count, Stats* st, unsigned int wsBytes, double* __restrict__ volOut,
                                                     const float* __restrict__ b3verts = nullptr, const int* __restrict__ b3faces = nullptr,
                                                     int b3R = 0, int b3F = 0) {
  // b3R != 0: direction mesh (refined twice) of one more pair of volume bounds, evaluated by the whole workgroup before the exact volume
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* hs = (double*)smem;
  float* pv1 = (float*)(hs + 8 * F);
  float* pv2 = pv1 + 3 * R;
  unsigned short* seed = (unsigned short*)(smem + (size_t)8 * F * sizeof(double) + wsBytes);
  unsigned short* pos = seed + 6 * F;
  unsigned short* orig = pos + 2 * F;
  double* terms = (double*)(smem + (((size_t)8 * F * sizeof(double) + wsBytes + (size_t)10 * F * sizeof(unsigned short) + 15) & ~(size_t)15));   // 2F
  int* shared = (int*)(terms + 2 * F);                    // [0] = half-spaces kept by the cull
  char* extra = (char*)(shared + 4);                      // NW - 1 further polygon workspaces
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  HivLds W;
  W.S = wave == 0 ? hs + 8 * F : (double*)(extra + (size_t)(wave - 1) * hiv_poly_bytes_dev());
  W.T = W.S + HIV_CAPL * 64; W.list = (unsigned short*)(W.T + HIV_CAPL * 64); W.seed = seed; W.pos = pos; W.orig = orig;
  for (int idx = tid; idx < 6 * F; idx += 64 * NW) {
    const int o_ = idx / 3, e_ = idx - 3 * o_;
    const int a_ = faceAdj[3 * (o_ >> 1) + e_];
    seed[idx] = (unsigned short)(a_ < 0 ? HIV_NONE : (unsigned int)(2 * a_ + (o_ & 1)));
  }
  const unsigned int nPairs = nPairsPtr ? *nPairsPtr : nPairsImm;
  for (unsigned int p = blockIdx.x; p < nPairs; p += gridDim.x) {
    const int2 ij = pairs[p];
    __syncthreads();
    const float* c1 = pts + 3 * (size_t)ij.x;
    const float* c2 = pts + 3 * (size_t)ij.y;
    for (int k = tid; k < R; k += 64 * NW) {
      const float d1 = dist[(size_t)ij.x * R + k], d2 = dist[(size_t)ij.y * R + k];
      pv1[3 * k] = c1[0] + d1 * verts[3 * k]; pv1[3 * k + 1] = c1[1] + d1 * verts[3 * k + 1]; pv1[3 * k + 2] = c1[2] + d1 * verts[3 * k + 2];
      pv2[3 * k] = c2[0] + d2 * verts[3 * k]; pv2[3 * k + 1] = c2[1] + d2 * verts[3 * k + 1]; pv2[3 * k + 2] = c2[2] + d2 * verts[3 * k + 2];
    }
    __syncthreads();
    for (int f = tid; f < F; f += 64 * NW) {
      const int iA = faces[3 * f], iB = faces[3 * f + 1], iC = faces[3 * f + 2];
      sd3::build_halfspace(&pv1[3 * iA], &pv1[3 * iB], &pv1[3 * iC], &hs[4 * (2 * f)]);
      sd3::build_halfspace(&pv2[3 * iA], &pv2[3 * iB], &pv2[3 * iC], &hs[4 * (2 * f + 1)]);
    }
    __syncthreads();
    const int M = 2 * F;
    double c[3];
    c[0] = .5 * (c1[0] + c2[0]); c[1] = .5 * (c1[1] + c2[1]); c[2] = .5 * (c1[2] + c2[2]);   // :857-859 (float add, then *.5 in double)
    int bad = 0;
    for (int k = tid; k < M; k += 64 * NW) {
      double dd = hs[4 * k + 3];
      dd += hs[4 * k] * c[0]; dd += hs[4 * k + 1] * c[1]; dd += hs[4 * k + 2] * c[2];
      if (dd > 0 || !(dd < 0)) bad = 1;
    }
    const bool infeasible = __syncthreads_or(bad) != 0;
    double vol = 0;
    if (!infeasible) {
      double ext = 0, ext1 = 0, ext2 = 0;                  // (every wave computes the same values)
      for (int k = lane; k < R; k += 64) {
        const float e1 = dist[(size_t)ij.x * R + k], e2 = dist[(size_t)ij.y * R + k];
        ext1 = fmax(ext1, (double)e1); ext2 = fmax(ext2, (double)e2);
      }
      for (int o = 32; o; o >>= 1) { ext1 = fmax(ext1, __shfl_xor(ext1, o)); ext2 = fmax(ext2, __shfl_xor(ext2, o)); }
      ext = fmax(ext1, ext2);
      if (wave == 0) {
        const double b1[4] = {(double)c1[0], (double)c1[1], (double)c1[2], ext1 * (1.0 + 1e-6) + 1e-6};
        const double b2[4] = {(double)c2[0], (double)c2[1], (double)c2[2], ext2 * (1.0 + 1e-6) + 1e-6};
        const int kept = hiv_cull_wave<OddIsSecond, false>(hs, M, b1, b2, c, pos, orig, lane, OddIsSecond());      // half-space 2f + w: polyhedron w
        if (lane == 0) shared[0] = kept;
      }
      __syncthreads();
      const int Mc = shared[0];
      const double zero3[3] = {0, 0, 0};
      const double sep = sqrt((double)(c1[0] - c2[0]) * (c1[0] - c2[0]) + (double)(c1[1] - c2[1]) * (c1[1] - c2[1]) + (double)(c1[2] - c2[2]) * (c1[2] - c2[2]));
      const double L = 4.0 * (2.0 * ext + sep + 1.0);
      const double balls[8] = {(double)c1[0] - c[0], (double)c1[1] - c[1], (double)c1[2] - c[2], ext1 * (1.0 + 1e-6) + 1e-6,
                               (double)c2[0] - c[0], (double)c2[1] - c[1], (double)c2[2] - c[2], ext2 * (1.0 + 1e-6) + 1e-6};
      bool decided = false;
      if (b3R > 0 && !volOut) {
        const double A_min_d = (double)fminf(volume[ij.x], volume[ij.y]) + 1e-10;
        const double thr_hi = (double)thr + 1e-5 * fabs((double)thr) + 1e-7, thr_lo = (double)thr - 1e-5 * fabs((double)thr) - 1e-7;
        double lb, ub;
        hiv_bounds_block<NW, 6>(hs, Mc, b3verts, b3faces, b3R, b3F, (double*)extra, (unsigned short*)((double*)extra + 3 * b3R), terms, tid, lb, ub);
        if (lb * (1.0 - 1e-9) / A_min_d > thr_hi) { vol = lb; decided = true; if (tid == 0) atomicAdd(&st->lb_decided, 1ull); }            // as in k_stage3
        else if (ub * (1.0 + 1e-9) / A_min_d < thr_lo) { vol = ub; decided = true; if (tid == 0) atomicAdd(&st->ub_decided, 1ull); }
      }
      if (!decided) vol = hiv_volume_block<NW>(hs, Mc, zero3, L, W, lane, wave, terms, st, balls);
    }
    if (tid == 0) {
      if (volOut) volOut[p] = vol;
      else {
        atomicAdd(&st->kernel, 1ull);
        if (vol != vol) atomicAdd(&st->overflow, 1ull);
        const float A_inter_kernel = (float)vol;                                  // function returns float :679
        const float A_min = fminf(volume[ij.x], volume[ij.y]);
        const float iou = (float)((double)A_inter_kernel / ((double)A_min + 1e-10));   // :1269
        if (fabsf(iou - thr) < 1e-6f) atomicAdd(&st->near_thr, 1ull);      // (a flip by the <= 1e-9 volume deviation from Qhull would need |iou - thr| ~ 1e-9)
      if (iou > thr) { sink.suppress(ij.x, ij.y); atomicAdd(&st->sup_kernel, 1ull); }
        else pairs5[atomicAdd(pair5Count, 1u)] = ij;
      }
    }
  }
}
static inline size_t stage3x_lds(int F, size_t ws3, int nw) {
  return (((size_t)8 * F * sizeof(double) + ws3 + (size_t)10 * F * sizeof(unsigned short) + 15) & ~(size_t)15) + (size_t)2 * F * sizeof(double) + 16 +
         (size_t)(nw - 1) * hiv_poly_bytes();
}

// ------------------------------------------------------------------ stage 4: hull ∩ hull volume (:872-939)
// Convex hull facets of the R vertices of one polyhedron by exhaustive search, computed ONCE per candidate that
// reaches stage 4 and cached in HBM: (a<b<c) is a facet iff every other vertex lies on one side of its plane and
// (a,b,c) are the three lowest-indexed vertices on that plane (one plane per facet).  One wave per polyhedron:
// each lane owns a triple, rejects it against 8 extreme "probe" vertices, survivors are verified by the whole wave.
// ---- fast hull: gift wrapping, breadth first (one lane per open edge), for non-degenerate point sets.
// Each open edge (u,v) of a known facet (u,v,t) is pivoted: the neighbouring facet's third vertex w is the point that is
// angularly extreme about the edge (all points lie in a wedge < pi; 2D cross-product order in the plane normal to the edge).
// Every facet is verified by the whole wave with the criterion of the exhaustive search below; anything unusual (more than
// three points on a supporting plane, an edge used three times, a facet that is not supporting) returns false and the caller
// runs the exhaustive search, so both paths emit the same facet set; the facets are sorted so that they are also emitted
// in the same order.
#define HULL_FAST_MAXR 192
// Partial pivot: the angular extreme about the edge among the points q = q0, q0 + qstep, ... (best = -1: none); (bx, by) are its
// coordinates in the plane normal to the edge.  hull_pivot_merge combines two partial results; all points lie in a wedge < pi about a
// hull edge, so the cross-product order is a total order there and the combination is associative (exact ties = four coplanar
// points, which the facet verification turns into the exhaustive search anyway).
struct PivotFrame { double u[3], x[3], y[3]; bool ok; };
// (x, y): axes of the plane normal to the edge direction e, x towards dref, y towards the side of the interior point g.  Only the
// SIGN of a 2D cross product in this frame is ever used, and that is invariant under a positive scaling of either axis: nothing is
// normalised (no square root, no division -- the f64 forms of both are long dependent instruction chains).
__device__ __forceinline__ PivotFrame hull_pivot_frame(const double u[3], const double e[3], const double dref[3], const double g[3]) {
  PivotFrame F;
  F.ok = false;
  F.u[0] = u[0]; F.u[1] = u[1]; F.u[2] = u[2];
  const double ee = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
  if (!(ee > 0)) return F;
  const double dr = dref[0] * e[0] + dref[1] * e[1] + dref[2] * e[2];
  const double x0 = ee * dref[0] - dr * e[0], x1 = ee * dref[1] - dr * e[1], x2 = ee * dref[2] - dr * e[2];     // |e|^2 (dref - its part along e)
  if (!(x0 * x0 + x1 * x1 + x2 * x2 > 0)) return F;
  double y0 = e[1] * x2 - e[2] * x1, y1 = e[2] * x0 - e[0] * x2, y2 = e[0] * x1 - e[1] * x0;
  if ((g[0] - u[0]) * y0 + (g[1] - u[1]) * y1 + (g[2] - u[2]) * y2 < 0) { y0 = -y0; y1 = -y1; y2 = -y2; }
  F.x[0] = x0; F.x[1] = x1; F.x[2] = x2; F.y[0] = y0; F.y[1] = y1; F.y[2] = y2;
  F.ok = true;
  return F;
}
__device__ __forceinline__ void hull_pivot_part(const double* __restrict__ pv, int R, int iu, int iv, int it, const PivotFrame& F, int q0, int qstep,
                                                int& best, double& bx, double& by) {
  // Branch-free, with a wave-uniform trip count (a lane past the end re-reads the last point and discards it) so that the unrolled
  // body's LDS reads are issued together: the loop is a chain of LDS reads and dependent f64 operations, and its only product is
  // the CHOICE of a vertex (the facet is verified afterwards with the exhaustive search's arithmetic), so the projections may be fused.
  best = -1; bx = 0; by = 0;
  const double ux = F.u[0] * F.x[0] + F.u[1] * F.x[1] + F.u[2] * F.x[2], uy = F.u[0] * F.y[0] + F.u[1] * F.y[1] + F.u[2] * F.y[2];
  const int niter = (R + qstep - 1) / qstep;
  int q = q0;
#pragma unroll 4
  for (int k = 0; k < niter; ++k, q += qstep) {
    const int qq = q < R ? q : R - 1;
    const double p0 = pv[3 * qq], p1 = pv[3 * qq + 1], p2 = pv[3 * qq + 2];
    const double xq = __builtin_fma(p0, F.x[0], __builtin_fma(p1, F.x[1], __builtin_fma(p2, F.x[2], -ux)));
    const double yq = __builtin_fma(p0, F.y[0], __builtin_fma(p1, F.y[1], __builtin_fma(p2, F.y[2], -uy)));
    const bool take = (q < R) & (q != iu) & (q != iv) & (q != it) & ((best < 0) | (bx * yq > by * xq));     // q is counter-clockwise of the current extreme
    best = take ? q : best; bx = take ? xq : bx; by = take ? yq : by;
  }
}
__device__ __forceinline__ void hull_pivot_merge(int& best, double& bx, double& by, int obest, double obx, double oby) {
  if (obest < 0) return;
  if (best < 0) { best = obest; bx = obx; by = oby; return; }
  const double cr = bx * oby - by * obx;
  if (cr > 0 || (cr == 0 && obest < best)) { best = obest; bx = obx; by = oby; }
}
// the extreme over all points, computed by `grp` consecutive lanes (a power of two) that share the edge; every lane of the group
// returns the same vertex
__device__ __forceinline__ int hull_pivot_group(const double* __restrict__ pv, int R, int iu, int iv, int it, const PivotFrame& F, int sub, int grp) {
  int best; double bx, by;
  hull_pivot_part(pv, R, iu, iv, it, F, sub, grp, best, bx, by);
  for (int o = grp >> 1; o; o >>= 1) {
    const int ob = __shfl_xor(best, o); const double ox = __shfl_xor(bx, o), oy = __shfl_xor(by, o);
    hull_pivot_merge(best, bx, by, ob, ox, oy);
  }
  return best;
}

// Edge use counts of the wrap: two bits per vertex pair lo * R + hi, sixteen to a word, incremented with a word atomic.  A field
// that would pass 2 makes the increment that sees 2 report it and the construction is abandoned before anything reads the
// (then possibly carried-into) neighbouring fields.  R * R / 4 bytes instead of R * R: 10 instead of 17 KB of LDS per polyhedron.
__device__ __forceinline__ unsigned int hull_cnt_get(const unsigned int* cntw, int idx) { return (cntw[idx >> 4] >> ((idx & 15) * 2)) & 3u; }
__device__ __forceinline__ unsigned int hull_cnt_inc(unsigned int* cntw, int idx) {
  const unsigned int sh = (unsigned int)(idx & 15) * 2u;
  return (atomicAdd(&cntw[idx >> 4], 1u << sh) >> sh) & 3u;
}

// tri: facets packed a << 20 | b << 10 | c with a < b < c, bit 30 = flip the normal; returns the facet count or -1.
// One batch = up to 64 open edges, `grp` lanes each: the group pivots its edge, VERIFIES the facet it found against all R points
// (criterion and arithmetic of the exhaustive search) and its first lane inserts it -- every step of a batch runs on all edges at
// once (round 3 verified and inserted the facets one after the other with the whole wave: 2 R-point passes, a square root and a
// barrier per facet, ~190 times per polyhedron).  A facet is reached from each of its open edges; the proposal through the
// SMALLEST open edge inserts it (all open edges are in the frontier, so that edge is pivoted in this round too; its batch may be a
// later one -- then the facet is inserted there).  If the point set is degenerate the proposals disagree: an edge gets a third
// facet or stays open, both are detected (use counts) and the caller falls back to the exhaustive search.
__device__ int hull_giftwrap(const double* __restrict__ pv, int R, int cap, int p0, double ext, unsigned int* tri, unsigned int* cntw,
                             unsigned int* frA, unsigned int* frB, int* s_cnt, int lane) {
  for (int k = lane; k < (R * R + 15) / 16; k += 64) cntw[k] = 0u;
  double g[3] = {0, 0, 0};
  for (int k = lane; k < R; k += 64) { g[0] += pv[3 * k]; g[1] += pv[3 * k + 1]; g[2] += pv[3 * k + 2]; }
  for (int o = 32; o; o >>= 1) { g[0] += __shfl_xor(g[0], o); g[1] += __shfl_xor(g[1], o); g[2] += __shfl_xor(g[2], o); }
  g[0] /= R; g[1] /= R; g[2] /= R;
  if (lane == 0) { s_cnt[0] = 0; s_cnt[1] = 0; s_cnt[2] = 0; }
  __syncthreads();
  // first facet: p0 has the lowest z, so the plane z = z(p0) supports the hull; pivot about the line through p0 parallel
  // to y, then about the edge (p0, p1).  Every lane computes the same thing.
  int p1, p2;
  {
    const double u[3] = {pv[3 * p0], pv[3 * p0 + 1], pv[3 * p0 + 2]};
    const double ey[3] = {0, 1, 0}, ex[3] = {0, 0, 1};
    const PivotFrame F1 = hull_pivot_frame(u, ey, ex, g);
    if (!F1.ok) return -1;
    p1 = hull_pivot_group(pv, R, p0, -1, -1, F1, lane, 64);
    if (p1 < 0) return -1;
    const double e[3] = {pv[3 * p1] - u[0], pv[3 * p1 + 1] - u[1], pv[3 * p1 + 2] - u[2]};
    const PivotFrame F2 = hull_pivot_frame(u, e, ey, g);
    if (!F2.ok) return -1;
    p2 = hull_pivot_group(pv, R, p0, p1, -1, F2, lane, 64);
    if (p2 < 0) return -1;
  }
  int nfr = 0;            // entries in the current frontier (uniform)
  unsigned int* frCur = frA; unsigned int* frNext = frB;
  int nf = 0;             // facets so far (uniform, mirror of s_cnt[0])
  bool failed = false;
  int round_start = 0;
  for (int round = 0; round < 8 * R && !failed; ++round) {
    // round 0 is a "batch" with the first facet as its only proposal, verified by the whole wave.  Later: the open edges of the
    // frontier, `per` at a time; the 64 / per lanes of an edge's group split the R points among them (a small frontier -- the first
    // and the last rounds of the breadth-first wrap -- costs R / grp steps instead of R)
    const int nitems = round == 0 ? 1 : nfr;
    int per = 64, grp = 1;
    while (per > 1 && (per >> 1) >= nitems) { per >>= 1; grp <<= 1; }
    for (int base = 0; base < nitems && !failed; base += per) {
      const int slot = lane / grp, sub = lane - slot * grp;
      int eu = -1, ev = -1, w = -1;
      bool bad = false;
      // (every lane of a group takes the same branches: the conditions depend on the edge only)
      if (round == 0) { eu = p0; ev = p1; w = p2; }
      else if (base + slot < nitems) {
        const unsigned int item = frCur[base + slot];
        eu = (int)(item & 1023u); ev = (int)((item >> 10) & 1023u);
        const int t = (int)((item >> 20) & 1023u);
        const int lo = eu < ev ? eu : ev, hi = eu < ev ? ev : eu;
        if (hull_cnt_get(cntw, lo * R + hi) == 1u) {               // still open (not closed by an earlier batch of this round)
          const double u[3] = {pv[3 * eu], pv[3 * eu + 1], pv[3 * eu + 2]};
          const double e[3] = {pv[3 * ev] - u[0], pv[3 * ev + 1] - u[1], pv[3 * ev + 2] - u[2]};
          const double dref[3] = {pv[3 * t] - u[0], pv[3 * t + 1] - u[1], pv[3 * t + 2] - u[2]};
          const PivotFrame F = hull_pivot_frame(u, e, dref, g);
          if (!F.ok) bad = true;
          else {
            w = hull_pivot_group(pv, R, eu, ev, t, F, sub, grp);
            if (w < 0) bad = true;
          }
        }
      }
      // verification by the edge's group (same arithmetic and tolerance as the exhaustive search)
      int a = eu, b = ev, c = w;
      unsigned int key = 0u;
      bool okf = false;
      if (w >= 0) {
        if (a > b) { const int t_ = a; a = b; b = t_; }
        if (b > c) { const int t_ = b; b = c; c = t_; }
        if (a > b) { const int t_ = a; a = b; b = t_; }
        if (a == b || b == c) bad = true;
        else {
          const double az = pv[3 * a], ay = pv[3 * a + 1], ax = pv[3 * a + 2];
          const double ez = pv[3 * b] - az, ey_ = pv[3 * b + 1] - ay, ex_ = pv[3 * b + 2] - ax;
          const double fz = pv[3 * c] - az, fy = pv[3 * c + 1] - ay, fx = pv[3 * c + 2] - ax;
          const double nz = ey_ * fx - ex_ * fy, ny = ex_ * fz - ez * fx, nx = ez * fy - ey_ * fz;
          const double nn = sqrt(nz * nz + ny * ny + nx * nx);
          const double te = 1e-10 * nn * (ext + 1e-30);
          if (!(nn > 1e-12 * ext * ext)) bad = true;
          else {
            int fl = 0;                                            // 1: a point above, 2: below, 4: on the plane
            const int niter = (R + grp - 1) / grp;
            int q = sub;
#pragma unroll 4
            for (int k = 0; k < niter; ++k, q += grp) {
              const int qq = q < R ? q : R - 1;
              const double sd_ = nz * (pv[3 * qq] - az) + ny * (pv[3 * qq + 1] - ay) + nx * (pv[3 * qq + 2] - ax);
              const int f = sd_ > te ? 1 : (sd_ < -te ? 2 : 4);
              fl |= ((q >= R) | (q == a) | (q == b) | (q == c)) ? 0 : f;
            }
            for (int o = grp >> 1; o; o >>= 1) fl |= __shfl_xor(fl, o);
            if ((fl & 3) == 3 || (fl & 4)) bad = true;
            else { okf = true; key = ((unsigned int)a << 20) | ((unsigned int)b << 10) | (unsigned int)c | ((fl & 1) ? (1u << 30) : 0u); }
          }
        }
      }
      if (__any(bad)) { failed = true; break; }
      // insertion: one lane per facet
      const int iab = a * R + b, iac = a * R + c, ibc = b * R + c;     // iab < iac < ibc
      bool win = okf && sub == 0;
      if (win && round > 0) {
        const int my = (eu < ev ? eu : ev) * R + (eu < ev ? ev : eu);
        if (iab < my && hull_cnt_get(cntw, iab) == 1u) win = false;
        if (iac < my && hull_cnt_get(cntw, iac) == 1u) win = false;
      }
      __builtin_amdgcn_wave_barrier();                               // every lane has read the counts of the batch's start
      if (win) {
        const int pos = atomicAdd(&s_cnt[0], 1);
        if (pos < cap) tri[pos] = key;
        const unsigned int o0 = hull_cnt_inc(cntw, iab), o1 = hull_cnt_inc(cntw, ibc), o2 = hull_cnt_inc(cntw, iac);
        if (pos >= cap || o0 >= 2u || o1 >= 2u || o2 >= 2u) s_cnt[2] = 1;
      }
      __syncthreads();
      if (s_cnt[2]) failed = true;
      nf = s_cnt[0];
    }
    if (failed) break;
    // next frontier: edges of this round's facets that are still used once
    if (lane == 0) s_cnt[1] = 0;
    __syncthreads();
    for (int t = round_start + lane; t < nf; t += 64) {
      const unsigned int key = tri[t];
      const int a = (int)((key >> 20) & 1023u), b = (int)((key >> 10) & 1023u), c = (int)(key & 1023u);
      if (hull_cnt_get(cntw, a * R + b) == 1u) frNext[atomicAdd(&s_cnt[1], 1)] = (unsigned int)a | ((unsigned int)b << 10) | ((unsigned int)c << 20);
      if (hull_cnt_get(cntw, b * R + c) == 1u) frNext[atomicAdd(&s_cnt[1], 1)] = (unsigned int)b | ((unsigned int)c << 10) | ((unsigned int)a << 20);
      if (hull_cnt_get(cntw, a * R + c) == 1u) frNext[atomicAdd(&s_cnt[1], 1)] = (unsigned int)a | ((unsigned int)c << 10) | ((unsigned int)b << 20);
    }
    __syncthreads();
    nfr = s_cnt[1];
    round_start = nf;
    { unsigned int* t_ = frCur; frCur = frNext; frNext = t_; }
    if (nfr == 0) break;
    if (nfr > 6 * R) { failed = true; break; }
  }
  __syncthreads();
  if (failed || nfr != 0 || nf < 4) return -1;
  // a closed surface: every edge of every facet is used exactly twice (an edge whose proposal was left to a smaller edge that then
  // found another facet would still be open)
  {
    bool open = false;
    for (int t = lane; t < nf; t += 64) {
      const unsigned int key = tri[t];
      const int a = (int)((key >> 20) & 1023u), b = (int)((key >> 10) & 1023u), c = (int)(key & 1023u);
      if (hull_cnt_get(cntw, a * R + b) != 2u || hull_cnt_get(cntw, b * R + c) != 2u || hull_cnt_get(cntw, a * R + c) != 2u) open = true;
    }
    if (__any(open)) return -1;
  }
  // sort the facets lexicographically by (a, b, c) (rank sort; keys are distinct)
  for (int t = lane; t < nf; t += 64) {
    const unsigned int key = tri[t] & 0x3FFFFFFFu;
    int rank = 0;
    for (int q = 0; q < nf; ++q) rank += ((tri[q] & 0x3FFFFFFFu) < key) ? 1 : 0;
    frCur[rank] = tri[t];
  }
  __syncthreads();
  for (int t = lane; t < nf; t += 64) tri[t] = frCur[t];
  __syncthreads();
  return nf;
}

// arg-extreme vertices along the probe directions d0 <= d < d1 (lowest index among equals) -> s_probe[d]
__device__ __forceinline__ void hull_probes(const double* __restrict__ pv, int R, int lane, int* s_probe, int d0, int d1) {
  const double dirs[8][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}, {1, 1, 1}, {-1, -1, -1}};
  for (int d = d0; d < d1; ++d) {
    double best = -1e300; int bi = 0;
    for (int k = lane; k < R; k += 64) {
      const double v = dirs[d][0] * pv[3 * k] + dirs[d][1] * pv[3 * k + 1] + dirs[d][2] * pv[3 * k + 2];
      if (v > best) { best = v; bi = k; }
    }
    for (int o = 32; o; o >>= 1) {
      const double ob = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) s_probe[d] = bi;
  }
}

__global__ void __launch_bounds__(64) k_hull(const int* __restrict__ hullList, unsigned int nList, const float* __restrict__ dist,
                                             const float* __restrict__ pts, const float* __restrict__ verts, int R, int cap,
                                             double* __restrict__ hullPlanes, unsigned short* __restrict__ hullAdj, int* __restrict__ hullCount,
                                             const unsigned int* __restrict__ nListPtr = nullptr) {
  if (nListPtr) nList = *nListPtr;       // the list length read on the device (the grid is sized from an upper bound)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* pv = (double*)smem;            // 3R doubles
  unsigned int* tri = (unsigned int*)(pv + 3 * R);   // cap packed facets a | b << 10 | c << 20
  unsigned int* frA = tri + cap;                     // fast path only: 6R + 6R open edges, R*R edge use counts
  unsigned int* frB = frA + 6 * R;
  unsigned int* cnt = frB + 6 * R;                   // R*R edge use counts, two bits each
  __shared__ int s_probe[8];
  __shared__ int s_n;
  __shared__ int s_cnt[3];
  __shared__ unsigned int s_dup[32];      // exhaustive search: bit k = vertex k coincides with a lower-indexed vertex (R <= 800 < 1024)
  const int lane = threadIdx.x;
  for (unsigned int it = blockIdx.x; it < nList; it += gridDim.x) {
    const int cand = hullList[it];
    __syncthreads();
    const float* c1 = pts + 3 * (size_t)cand;
    for (int k = lane; k < R; k += 64) {
      const float d1 = dist[(size_t)cand * R + k];
      pv[3 * k] = (double)(c1[0] + d1 * verts[3 * k]); pv[3 * k + 1] = (double)(c1[1] + d1 * verts[3 * k + 1]); pv[3 * k + 2] = (double)(c1[2] + d1 * verts[3 * k + 2]);
    }
    if (lane == 0) s_n = 0;
    __syncthreads();
    // probes: arg-extremes along 8 directions (all are hull vertices).  The gift wrapping starts from probe 1 (lowest z); the other
    // seven are the exhaustive search's quick rejection and are only computed when it runs.
    double ext = 0;
    hull_probes(pv, R, lane, s_probe, 1, 2);
    for (int k = lane; k < R; k += 64) ext = fmax(ext, fmax(fabs(pv[3 * k] - pv[0]), fmax(fabs(pv[3 * k + 1] - pv[1]), fabs(pv[3 * k + 2] - pv[2]))));
    for (int o = 32; o; o >>= 1) ext = fmax(ext, __shfl_xor(ext, o));
    __syncthreads();
    double* out = hullPlanes + (size_t)cand * cap * 4;
    int nfast = -1;
    if (R <= HULL_FAST_MAXR) nfast = hull_giftwrap(pv, R, cap, s_probe[1], ext, tri, cnt, frA, frB, s_cnt, lane);
    if (nfast > 0) {
      for (int t = lane; t < nfast; t += 64) {
        const unsigned int key = tri[t];
        const int a = (int)((key >> 20) & 1023u), b = (int)((key >> 10) & 1023u), c = (int)(key & 1023u);
        const double az = pv[3 * a], ay = pv[3 * a + 1], ax = pv[3 * a + 2];
        const double ez = pv[3 * b] - az, ey = pv[3 * b + 1] - ay, ex = pv[3 * b + 2] - ax;
        const double fz = pv[3 * c] - az, fy = pv[3 * c + 1] - ay, fx = pv[3 * c + 2] - ax;
        const double tz = ey * fx - ex * fy, ty = ex * fz - ez * fx, tx = ez * fy - ey * fz;
        const double sg = (key >> 30) & 1u ? -1.0 : 1.0;
        out[4 * t] = sg * tz; out[4 * t + 1] = sg * ty; out[4 * t + 2] = sg * tx;
        out[4 * t + 3] = -(sg * tz * az + sg * ty * ay + sg * tx * ax);
      }
      __syncthreads();
      for (int t = lane; t < nfast; t += 64) {          // repack as the adjacency code below expects
        const unsigned int key = tri[t];
        tri[t] = ((key >> 20) & 1023u) | (((key >> 10) & 1023u) << 10) | ((key & 1023u) << 20);
      }
      if (lane == 0) s_n = nfast;
    } else {
    hull_probes(pv, R, lane, s_probe, 0, 8);
    // Degenerate vertex sets (round 6; Rays_Cartesian: its eight pole rays end in ONE float32 point).  One triple stands for a facet plane:
    // the lexicographically first NON-DEGENERATE one among the plane's points -- a point that coincides with a lower-indexed point is
    // left out altogether (s_dup), and a point on the line through (a, b) cannot complete them.  (Until round 6 the rule was "the three
    // lowest indices on the plane": a plane whose three lowest points coincide or are collinear lost its facet, the hull was open there and
    // the intersection volume too large -- found with tools/diag_cartesian.py against the reference's Qhull volumes.)
    if (lane < 32) s_dup[lane] = 0u;
    __syncthreads();
    for (int k = lane; k < R; k += 64) {
      bool dp = false;
      for (int j = 0; j < k && !dp; ++j) dp = pv[3 * j] == pv[3 * k] && pv[3 * j + 1] == pv[3 * k + 1] && pv[3 * j + 2] == pv[3 * k + 2];
      if (dp) atomicOr(&s_dup[k >> 5], 1u << (k & 31));
    }
    __syncthreads();
    for (int a = 0; a < R - 2; ++a) {
      if ((s_dup[a >> 5] >> (a & 31)) & 1u) continue;
      const double az = pv[3 * a], ay = pv[3 * a + 1], ax = pv[3 * a + 2];
      for (int b = a + 1; b < R - 1; ++b) {
        if ((s_dup[b >> 5] >> (b & 31)) & 1u) continue;
        const double ez = pv[3 * b] - az, ey = pv[3 * b + 1] - ay, ex = pv[3 * b + 2] - ax;
        for (int c0 = b + 1; c0 < R; c0 += 64) {
          const int c = c0 + lane;
          bool ok = c < R && !((s_dup[(c < R ? c : 0) >> 5] >> ((c < R ? c : 0) & 31)) & 1u);
          double nz = 0, ny = 0, nx = 0, eps = 0;
          if (ok) {
            const double fz = pv[3 * c] - az, fy = pv[3 * c + 1] - ay, fx = pv[3 * c + 2] - ax;
            nz = ey * fx - ex * fy; ny = ex * fz - ez * fx; nx = ez * fy - ey * fz;
            const double nn = sqrt(nz * nz + ny * ny + nx * nx);
            eps = 1e-10 * nn * (ext + 1e-30);
            if (!(nn > 1e-12 * ext * ext)) ok = false;
            int sign = 0;
            for (int d = 0; d < 8 && ok; ++d) {
              const int q = s_probe[d];
              const double sd_ = nz * (pv[3 * q] - az) + ny * (pv[3 * q + 1] - ay) + nx * (pv[3 * q + 2] - ax);
              if (sd_ > eps) { if (sign < 0) ok = false; sign = 1; }
              else if (sd_ < -eps) { if (sign > 0) ok = false; sign = -1; }
            }
          }
          unsigned long long m = __ballot(ok);
          while (m) {                                   // verify each surviving triple with the whole wave
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int cc = c0 + src;
            const double tz = __shfl(nz, src), ty = __shfl(ny, src), tx = __shfl(nx, src), te = __shfl(eps, src);
            bool pos = false, neg = false, low = false;
            for (int q = lane; q < R; q += 64) {
              if (q == a || q == b || q == cc || ((s_dup[q >> 5] >> (q & 31)) & 1u)) continue;
              const double gz = pv[3 * q] - az, gy = pv[3 * q + 1] - ay, gx = pv[3 * q + 2] - ax;
              const double sd_ = tz * gz + ty * gy + tx * gx;
              if (sd_ > te) pos = true; else if (sd_ < -te) neg = true;
              else if (q < b) low = true;                       // (a, b) are not the plane's two lowest points
              else if (q < cc) {                                // a lower point that completes (a, b) as well -- unless it lies on their line
                const double kz = ey * gx - ex * gy, ky = ex * gz - ez * gx, kx = ez * gy - ey * gz;
                if (sqrt(kz * kz + ky * ky + kx * kx) > 1e-12 * ext * ext) low = true;
              }
            }
            const bool anyp = __any(pos), anyn = __any(neg), anyl = __any(low);
            if (!(anyp && anyn) && !anyl && lane == 0) {
              const int pos_i = s_n;
              if (pos_i < cap) {
                const double sg = anyp ? -1.0 : 1.0;   // outward normal: every vertex satisfies n.(p-a) <= 0
                out[4 * pos_i] = sg * tz; out[4 * pos_i + 1] = sg * ty; out[4 * pos_i + 2] = sg * tx;
                out[4 * pos_i + 3] = -(sg * tz * az + sg * ty * ay + sg * tx * ax);
                tri[pos_i] = (unsigned int)a | ((unsigned int)b << 10) | ((unsigned int)cc << 20);
              }
              s_n = pos_i + 1;
            }
          }
        }
      }
    }
    }
    __syncthreads();
    // edge adjacency of the facets (seeds of the intersection-volume routine; a hint, not needed for correctness)
    if (s_n >= 4 && s_n <= cap) {
      const int nf = s_n;
      unsigned short* adj = hullAdj + (size_t)cand * cap * 3;
      // facets per vertex (a hull vertex of a near-spherical point set has ~6): the neighbour across edge (x, y) is looked up among the
      // facets of x instead of among all facets.  The table lives in the frontier buffers of the gift wrapping (R <= HULL_FAST_MAXR).
      const bool table = R <= HULL_FAST_MAXR;
      unsigned short* vf = (unsigned short*)frA;      // [R][VF_CAP]
      int* vcnt = (int*)frB;                          // [R]
      constexpr int VF_CAP = 12;
      if (table) {
        for (int k = lane; k < R; k += 64) vcnt[k] = 0;
        __syncthreads();
        for (int t = lane; t < nf; t += 64) {
          const unsigned int tt = tri[t];
          const unsigned int v[3] = {tt & 1023u, (tt >> 10) & 1023u, (tt >> 20) & 1023u};
          for (int e = 0; e < 3; ++e) { const int pos = atomicAdd(&vcnt[v[e]], 1); if (pos < VF_CAP) vf[v[e] * VF_CAP + pos] = (unsigned short)t; }
        }
        __syncthreads();
      }
      for (int t = lane; t < nf; t += 64) {
        const unsigned int tt = tri[t];
        const unsigned int v[3] = {tt & 1023u, (tt >> 10) & 1023u, (tt >> 20) & 1023u};
        for (int e = 0; e < 3; ++e) {
          const unsigned int x = v[e], y = v[(e + 1) % 3];
          unsigned int found = HIV_NONE;
          if (table && vcnt[x] <= VF_CAP) {
            // (the lowest facet index, like the scan over all facets below)
            for (int k = 0; k < vcnt[x]; ++k) {
              const unsigned int u = vf[x * VF_CAP + k];
              if ((int)u == t) continue;
              const unsigned int uu = tri[u];
              const unsigned int a_ = uu & 1023u, b_ = (uu >> 10) & 1023u, c_ = (uu >> 20) & 1023u;
              if ((a_ == y || b_ == y || c_ == y) && (found == HIV_NONE || u < found)) found = u;
            }
          } else
          for (int u = 0; u < nf && found == HIV_NONE; ++u) {
            if (u == t) continue;
            const unsigned int uu = tri[u];
            const unsigned int a_ = uu & 1023u, b_ = (uu >> 10) & 1023u, c_ = (uu >> 20) & 1023u;
            if ((a_ == x || b_ == x || c_ == x) && (a_ == y || b_ == y || c_ == y)) found = (unsigned int)u;
          }
          adj[3 * t + e] = (unsigned short)found;
        }
      }
    }
    __syncthreads();
    if (lane == 0) hullCount[cand] = (s_n >= 4 && s_n <= cap) ? s_n : -2;   // -2: failed (Qhull error -> 1e10, :933-936)
  }
}

// hullState: 0 = not requested, 1 = requested/computed
__global__ void k_hull_mark(const int2* __restrict__ pairs, unsigned int nPairs, int* __restrict__ hullState, int* __restrict__ hullList,
                            unsigned int* hullListCount) {
  const unsigned int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nPairs) return;
  const int2 ij = pairs[p];
  if (atomicExch(&hullState[ij.x], 1) == 0) hullList[atomicAdd(hullListCount, 1u)] = ij.x;
  if (atomicExch(&hullState[ij.y], 1) == 0) hullList[atomicAdd(hullListCount, 1u)] = ij.y;
}

__global__ void __launch_bounds__(64) k_stage4(const int2* __restrict__ pairs, unsigned int nPairs, const float* __restrict__ dist,
                                               const float* __restrict__ pts, const float* __restrict__ verts,
                                               const int* __restrict__ faces, int R, int F, int cap, const double* __restrict__ hullPlanes,
                                               const unsigned short* __restrict__ hullAdj, const int* __restrict__ hullCount,
                                               const float* __restrict__ volume, float thr,
                                               int2* __restrict__ pairs5, unsigned int* pair5Count, Stats* st, int no_lb,
                                               const float* __restrict__ bverts, const int* __restrict__ bfaces, int bR, int bF,
                                               double* __restrict__ volOut = nullptr, int2* __restrict__ pairsX = nullptr,
                                               unsigned int* __restrict__ nX = nullptr, unsigned int wsBytes = 0) {
  // pairsX != nullptr: undecided pairs are queued for k_stage4x (as in k_stage3).  wsBytes != 0: the workspace between the half-spaces
  // and the seed / pos / orig lists is only that large (a bounds-only launch: the polygon workspace of the exact routine is not needed,
  // the smaller footprint lets six waves share a CU instead of four)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* hs = (double*)smem;                   // 2*cap*4
  const bool lean = (wsBytes & SD_LEAN_BIT) != 0;                 // as in k_stage3: no seed table, pos / orig in the workspace
  unsigned short* seed = (unsigned short*)(smem + (size_t)8 * cap * sizeof(double) + ((wsBytes & SD_WS_MASK) ? (size_t)(wsBytes & SD_WS_MASK) : hiv_poly_bytes_dev()));   // 2*cap*3
  unsigned short* pos = lean ? (unsigned short*)(hs + 8 * cap) : seed + 6 * cap;         // 2*cap
  unsigned short* orig = pos + 2 * cap;         // 2*cap
  HivLds W;
  W.S = hs + 8 * cap; W.T = W.S + HIV_CAPL * 64; W.list = (unsigned short*)(W.T + HIV_CAPL * 64); W.seed = seed; W.pos = pos; W.orig = orig;
  const int lane = threadIdx.x;
  for (unsigned int p = blockIdx.x; p < nPairs; p += gridDim.x) {
    const int2 ij = pairs[p];
    __syncthreads();
    const float* c1 = pts + 3 * (size_t)ij.x;
    const float* c2 = pts + 3 * (size_t)ij.y;
    const int n1 = hullCount[ij.x], n2 = hullCount[ij.y];
    const bool failed = (n1 < 4 || n2 < 4);
    const int M = failed ? 0 : n1 + n2;
    if (!failed) {
      const double* h1 = hullPlanes + (size_t)ij.x * cap * 4;
      const double* h2 = hullPlanes + (size_t)ij.y * cap * 4;
      for (int k = lane; k < 4 * n1; k += 64) hs[k] = h1[k];
      for (int k = lane; k < 4 * n2; k += 64) hs[4 * n1 + k] = h2[k];
      if (!lean) {
        const unsigned short* a1 = hullAdj + (size_t)ij.x * cap * 3;
        const unsigned short* a2 = hullAdj + (size_t)ij.y * cap * 3;
        for (int k = lane; k < 3 * n1; k += 64) seed[k] = a1[k];
        for (int k = lane; k < 3 * n2; k += 64) { const unsigned int t = a2[k]; seed[3 * n1 + k] = (unsigned short)(t == HIV_NONE ? HIV_NONE : t + n1); }
      }
    }
    __syncthreads();
    double c[3];
    c[0] = .5 * ((double)c1[0] + (double)c2[0]); c[1] = .5 * ((double)c1[1] + (double)c2[1]); c[2] = .5 * ((double)c1[2] + (double)c2[2]);   // :919-921
    bool infeasible = false;
    for (int k = lane; k < M; k += 64) {
      double dd = hs[4 * k + 3];
      dd += hs[4 * k] * c[0]; dd += hs[4 * k + 1] * c[1]; dd += hs[4 * k + 2] * c[2];
      if (dd > 0 || !(dd < 0)) infeasible = true;
    }
    infeasible = __any(infeasible) || failed;
    double vol = 1.e10;                                             // err_value :927
    bool deferred = false;
    if (!infeasible) {
      double ext = 0, ext1 = 0, ext2 = 0;
      for (int k = lane; k < R; k += 64) { ext1 = fmax(ext1, (double)dist[(size_t)ij.x * R + k]); ext2 = fmax(ext2, (double)dist[(size_t)ij.y * R + k]); }
      for (int o = 32; o; o >>= 1) { ext1 = fmax(ext1, __shfl_xor(ext1, o)); ext2 = fmax(ext2, __shfl_xor(ext2, o)); }
      ext = fmax(ext1, ext2);
      const double sep = sqrt((double)(c1[0] - c2[0]) * (c1[0] - c2[0]) + (double)(c1[1] - c2[1]) * (c1[1] - c2[1]) + (double)(c1[2] - c2[2]) * (c1[2] - c2[2]));
      const double L = 4.0 * (2.0 * ext + sep + 1.0);
      // cull half-spaces of one hull that contain the other polyhedron's outer ball (which contains its hull)
      int Mc;
      {
        const double b1[4] = {(double)c1[0], (double)c1[1], (double)c1[2], ext1 * (1.0 + 1e-6) + 1e-6};
        const double b2[4] = {(double)c2[0], (double)c2[1], (double)c2[2], ext2 * (1.0 + 1e-6) + 1e-6};
        Mc = hiv_cull_wave(hs, M, b1, b2, c, pos, orig, lane, [n1](int k) { return k >= n1; });
      }
      const double A_min_d = (double)fminf(volume[ij.x], volume[ij.y]) + 1e-10;
      const double thr_hi = (double)thr + 1e-5 * fabs((double)thr) + 1e-7;
      const double zero3[3] = {0, 0, 0};
      const double thr_lo = (double)thr - 1e-5 * fabs((double)thr) - 1e-7;
      double lb, ub;
      hiv_bounds_wave<2>(hs, Mc, verts, faces, R, F, W.S, (unsigned short*)(W.S + 3 * R), lane, lb, ub);
      if (bR != R && !(lb * (1.0 - 1e-9) / A_min_d > thr_hi) && !(ub * (1.0 + 1e-9) / A_min_d < thr_lo)) {
        const double lb0 = lb, ub0 = ub;
        if (wsBytes & SD_NOREUSE_BIT) hiv_bounds_wave<6>(hs, Mc, bverts, bfaces, bR, bF, W.S, (unsigned short*)(W.S + 3 * bR), lane, lb, ub);
        else hiv_bounds_wave<5>(hs, Mc, bverts, bfaces, bR, bF, W.S, (unsigned short*)(W.S + 3 * bR), lane, lb, ub, R, (const unsigned short*)(W.S + 3 * R));
        lb = fmax(lb, lb0); ub = fmin(ub, ub0);
      }
      if (lb * (1.0 - 1e-9) / A_min_d > thr_hi && !no_lb) {
        vol = lb;                                       // certainly above the threshold -> render stage, as with the exact volume
        if (lane == 0) atomicAdd(&st->lb_decided, 1ull);
      } else if (ub * (1.0 + 1e-9) / A_min_d < thr_lo && !no_lb) {
        vol = ub;                                       // certainly not above the threshold -> pair kept
        if (lane == 0) atomicAdd(&st->ub_decided, 1ull);
      } else if (pairsX) {
        deferred = true;
        if (lane == 0) pairsX[atomicAdd(nX, 1u)] = ij;
      } else {
        const double balls[8] = {(double)c1[0] - c[0], (double)c1[1] - c[1], (double)c1[2] - c[2], ext1 * (1.0 + 1e-6) + 1e-6,
                                 (double)c2[0] - c[0], (double)c2[1] - c[1], (double)c2[2] - c[2], ext2 * (1.0 + 1e-6) + 1e-6};
        vol = hiv_volume_wave(hs, Mc, zero3, L, W, lane, st, balls);
      }
    }
    if (deferred) continue;
    if (volOut) { if (lane == 0) volOut[p] = vol; continue; }     // pair-level probe
    if (lane == 0) {
      atomicAdd(&st->convex, 1ull);
      if (vol != vol) atomicAdd(&st->overflow, 1ull);
      const float A_inter_convex = (float)vol;
      const float A_min = fminf(volume[ij.x], volume[ij.y]);
      const float iou = (float)((double)A_inter_convex / ((double)A_min + 1e-10));     // :1289
      if (fabsf(iou - thr) < 1e-6f) atomicAdd(&st->near_thr, 1ull);
      if (iou <= thr) atomicAdd(&st->kept_convex, 1ull);                                // :1291-1295
      else pairs5[atomicAdd(pair5Count, 1u)] = ij;
    }
  }
}

// Exact hull ∩ hull volume of the pairs k_stage4 queued, NW waves per pair (see k_stage3x).
// LDS: hs | wave 0's workspace | seed pos orig | terms | the other waves' workspaces.
struct FromIndex { int n1; __device__ bool operator()(int k) const { return k >= n1; } };
template <int NW>
__global__ void __launch_bounds__(64 * NW) k_stage4x(const int2* __restrict__ pairs, const unsigned int* __restrict__ nPairsPtr, unsigned int nPairsImm,
                                                     const float* __restrict__ dist, const float* __restrict__ pts, int R, int cap,
                                                     const double* __restrict__ hullPlanes, const unsigned short* __restrict__ hullAdj,
                                                     const int* __restrict__ hullCount, const float* __restrict__ volume, float thr,
                                                     int2* __restrict__ pairs5, unsigned int* pair5Count, Stats* st, double* __restrict__ volOut,
                                                     const float* __restrict__ b3verts = nullptr, const int* __restrict__ b3faces = nullptr,
                                                     int b3R = 0, int b3F = 0) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* hs = (double*)smem;
  unsigned short* seed = (unsigned short*)(smem + (size_t)8 * cap * sizeof(double) + hiv_poly_bytes_dev());
  unsigned short* pos = seed + 6 * cap;
  unsigned short* orig = pos + 2 * cap;
  double* terms = (double*)(smem + (((size_t)8 * cap * sizeof(double) + hiv_poly_bytes_dev() + (size_t)10 * cap * sizeof(unsigned short) + 15) & ~(size_t)15));   // 2 cap
  int* shared = (int*)(terms + 2 * cap);
  char* extra = (char*)(shared + 4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  HivLds W;
  W.S = wave == 0 ? hs + 8 * cap : (double*)(extra + (size_t)(wave - 1) * hiv_poly_bytes_dev());
  W.T = W.S + HIV_CAPL * 64; W.list = (unsigned short*)(W.T + HIV_CAPL * 64); W.seed = seed; W.pos = pos; W.orig = orig;
  const unsigned int nPairs = nPairsPtr ? *nPairsPtr : nPairsImm;
  for (unsigned int p = blockIdx.x; p < nPairs; p += gridDim.x) {
    const int2 ij = pairs[p];
    __syncthreads();
    const float* c1 = pts + 3 * (size_t)ij.x;
    const float* c2 = pts + 3 * (size_t)ij.y;
    const int n1 = hullCount[ij.x], n2 = hullCount[ij.y];
    const bool failed = (n1 < 4 || n2 < 4);
    const int M = failed ? 0 : n1 + n2;
    if (!failed) {
      const double* h1 = hullPlanes + (size_t)ij.x * cap * 4;
      const double* h2 = hullPlanes + (size_t)ij.y * cap * 4;
      for (int k = tid; k < 4 * n1; k += 64 * NW) hs[k] = h1[k];
      for (int k = tid; k < 4 * n2; k += 64 * NW) hs[4 * n1 + k] = h2[k];
      const unsigned short* a1 = hullAdj + (size_t)ij.x * cap * 3;
      const unsigned short* a2 = hullAdj + (size_t)ij.y * cap * 3;
      for (int k = tid; k < 3 * n1; k += 64 * NW) seed[k] = a1[k];
      for (int k = tid; k < 3 * n2; k += 64 * NW) { const unsigned int t = a2[k]; seed[3 * n1 + k] = (unsigned short)(t == HIV_NONE ? HIV_NONE : t + n1); }
    }
    __syncthreads();
    double c[3];
    c[0] = .5 * ((double)c1[0] + (double)c2[0]); c[1] = .5 * ((double)c1[1] + (double)c2[1]); c[2] = .5 * ((double)c1[2] + (double)c2[2]);   // :919-921
    int bad = 0;
    for (int k = tid; k < M; k += 64 * NW) {
      double dd = hs[4 * k + 3];
      dd += hs[4 * k] * c[0]; dd += hs[4 * k + 1] * c[1]; dd += hs[4 * k + 2] * c[2];
      if (dd > 0 || !(dd < 0)) bad = 1;
    }
    const bool infeasible = (__syncthreads_or(bad) != 0) || failed;
    double vol = 1.e10;                                             // err_value :927
    if (!infeasible) {
      double ext = 0, ext1 = 0, ext2 = 0;
      for (int k = lane; k < R; k += 64) { ext1 = fmax(ext1, (double)dist[(size_t)ij.x * R + k]); ext2 = fmax(ext2, (double)dist[(size_t)ij.y * R + k]); }
      for (int o = 32; o; o >>= 1) { ext1 = fmax(ext1, __shfl_xor(ext1, o)); ext2 = fmax(ext2, __shfl_xor(ext2, o)); }
      ext = fmax(ext1, ext2);
      const double sep = sqrt((double)(c1[0] - c2[0]) * (c1[0] - c2[0]) + (double)(c1[1] - c2[1]) * (c1[1] - c2[1]) + (double)(c1[2] - c2[2]) * (c1[2] - c2[2]));
      const double L = 4.0 * (2.0 * ext + sep + 1.0);
      if (wave == 0) {
        const double b1[4] = {(double)c1[0], (double)c1[1], (double)c1[2], ext1 * (1.0 + 1e-6) + 1e-6};
        const double b2[4] = {(double)c2[0], (double)c2[1], (double)c2[2], ext2 * (1.0 + 1e-6) + 1e-6};
        const int kept = hiv_cull_wave<FromIndex, false>(hs, M, b1, b2, c, pos, orig, lane, FromIndex{n1});
        if (lane == 0) shared[0] = kept;
      }
      __syncthreads();
      const int Mc = shared[0];
      const double zero3[3] = {0, 0, 0};
      const double balls[8] = {(double)c1[0] - c[0], (double)c1[1] - c[1], (double)c1[2] - c[2], ext1 * (1.0 + 1e-6) + 1e-6,
                               (double)c2[0] - c[0], (double)c2[1] - c[1], (double)c2[2] - c[2], ext2 * (1.0 + 1e-6) + 1e-6};
      bool decided = false;
      if (b3R > 0 && !volOut) {
        const double A_min_d = (double)fminf(volume[ij.x], volume[ij.y]) + 1e-10;
        const double thr_hi = (double)thr + 1e-5 * fabs((double)thr) + 1e-7, thr_lo = (double)thr - 1e-5 * fabs((double)thr) - 1e-7;
        double lb, ub;
        hiv_bounds_block<NW, 6>(hs, Mc, b3verts, b3faces, b3R, b3F, (double*)extra, (unsigned short*)((double*)extra + 3 * b3R), terms, tid, lb, ub);
        if (lb * (1.0 - 1e-9) / A_min_d > thr_hi) { vol = lb; decided = true; if (tid == 0) atomicAdd(&st->lb_decided, 1ull); }            // as in k_stage4
        else if (ub * (1.0 + 1e-9) / A_min_d < thr_lo) { vol = ub; decided = true; if (tid == 0) atomicAdd(&st->ub_decided, 1ull); }
      }
      if (!decided) vol = hiv_volume_block<NW>(hs, Mc, zero3, L, W, lane, wave, terms, st, balls);
    }
    if (tid == 0) {
      if (volOut) volOut[p] = vol;
      else {
        atomicAdd(&st->convex, 1ull);
        if (vol != vol) atomicAdd(&st->overflow, 1ull);
        const float A_inter_convex = (float)vol;
        const float A_min = fminf(volume[ij.x], volume[ij.y]);
        const float iou = (float)((double)A_inter_convex / ((double)A_min + 1e-10));     // :1289
        if (fabsf(iou - thr) < 1e-6f) atomicAdd(&st->near_thr, 1ull);
      if (iou <= thr) atomicAdd(&st->kept_convex, 1ull);                                // :1291-1295
        else pairs5[atomicAdd(pair5Count, 1u)] = ij;
      }
    }
  }
}
static inline size_t stage4x_lds(int cap, int nw) {
  return (((size_t)8 * cap * sizeof(double) + hiv_poly_bytes() + (size_t)10 * cap * sizeof(unsigned short) + 15) & ~(size_t)15) + (size_t)2 * cap * sizeof(double) + 16 +
         (size_t)(nw - 1) * hiv_poly_bytes();
}

// ------------------------------------------------------------------ stage 5: voxel rendering (:587-636, 1305-1330)
__global__ void __launch_bounds__(256) k_stage5(const int2* __restrict__ pairs, unsigned int nPairs, const float* __restrict__ dist,
                                                const float* __restrict__ pts, const float* __restrict__ verts,
                                                const int* __restrict__ faces, int R, int F, const int* __restrict__ bbox,
                                                const float* __restrict__ volume, float thr, SuppSink sink, Stats* st,
                                                sd3::ConeMap cm, int whole_box) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* pv1 = (float*)smem;       // 3R
  float* pv2 = pv1 + 3 * R;        // 3R
  int* fc = (int*)(pv2 + 3 * R);   // 3F
  __shared__ unsigned int s_count;
  __shared__ int s_unsafe[2];      // cone map preconditions violated (geom3d.h): some dist < 1 or a coordinate beyond 8192
  for (int k = threadIdx.x; k < 3 * F; k += blockDim.x) fc[k] = faces[k];
  for (unsigned int p = blockIdx.x; p < nPairs; p += gridDim.x) {
    const int2 ij = pairs[p];
    __syncthreads();
    const float* c1 = pts + 3 * (size_t)ij.x;
    const float* c2 = pts + 3 * (size_t)ij.y;
    for (int k = threadIdx.x; k < R; k += blockDim.x) {
      const float d1 = dist[(size_t)ij.x * R + k], d2 = dist[(size_t)ij.y * R + k];
      pv1[3 * k] = c1[0] + d1 * verts[3 * k]; pv1[3 * k + 1] = c1[1] + d1 * verts[3 * k + 1]; pv1[3 * k + 2] = c1[2] + d1 * verts[3 * k + 2];
      pv2[3 * k] = c2[0] + d2 * verts[3 * k]; pv2[3 * k + 1] = c2[1] + d2 * verts[3 * k + 1]; pv2[3 * k + 2] = c2[2] + d2 * verts[3 * k + 2];
    }
    if (threadIdx.x == 0) { s_count = 0; s_unsafe[0] = cm.list ? 0 : 1; s_unsafe[1] = cm.list ? 0 : 1; }
    __syncthreads();
    if (cm.list) {
      for (int k = threadIdx.x; k < R; k += blockDim.x) {
        const float d1 = dist[(size_t)ij.x * R + k], d2 = dist[(size_t)ij.y * R + k];
        const float m1 = fmaxf(fmaxf(fabsf(pv1[3 * k]), fabsf(pv1[3 * k + 1])), fabsf(pv1[3 * k + 2]));
        const float m2 = fmaxf(fmaxf(fabsf(pv2[3 * k]), fabsf(pv2[3 * k + 1])), fabsf(pv2[3 * k + 2]));
        if (!(d1 >= 1.f) || !(m1 < 8192.f)) s_unsafe[0] = 1;
        if (!(d2 >= 1.f) || !(m2 < 8192.f)) s_unsafe[1] = 1;
      }
      __syncthreads();
    }
    const bool safe1 = !s_unsafe[0] && fabsf(c1[0]) < 8192.f && fabsf(c1[1]) < 8192.f && fabsf(c1[2]) < 8192.f;
    const bool safe2 = !s_unsafe[1] && fabsf(c2[0]) < 8192.f && fabsf(c2[1]) < 8192.f && fabsf(c2[2]) < 8192.f;
    // the reference sweeps the whole bbox of i; lattice points outside j's (rounded) bbox cannot be inside j -- unless the ray mesh has a
    // DEGENERATE face (whole_box; Rays_Cartesian: pole rays on one line): a tetrahedron (centre, A, B, C) of zero volume passes
    // inside_tetrahedron's four `det >= 0` tests (:89-150) on its whole PLANE, lattice points far outside j's box included, and the reference
    // counts those that fall into i's box.  Then the sweep is the reference's (round 6, found with tools/diag_cartesian2.py).
    const int* b1 = bbox + 6 * (size_t)ij.x;
    const int* b2 = bbox + 6 * (size_t)ij.y;
    const int zlo = whole_box ? b1[0] : max(b1[0], b2[0] - 1), zhi = whole_box ? b1[1] : min(b1[1], b2[1] + 1);
    const int ylo = whole_box ? b1[2] : max(b1[2], b2[2] - 1), yhi = whole_box ? b1[3] : min(b1[3], b2[3] + 1);
    const int xlo = whole_box ? b1[4] : max(b1[4], b2[4] - 1), xhi = whole_box ? b1[5] : min(b1[5], b2[5] + 1);
    unsigned int local = 0;
    if (zhi >= zlo && yhi >= ylo && xhi >= xlo) {
      const i64 bz = zhi - zlo + 1, by = yhi - ylo + 1, bx = xhi - xlo + 1;
      const i64 nvox = bz * by * bx;
      for (i64 t = threadIdx.x; t < nvox; t += blockDim.x) {
        const float x = (float)(xlo + (int)(t % bx));
        const i64 r = t / bx;
        const float y = (float)(ylo + (int)(r % by)), z = (float)(zlo + (int)(r / by));
        if (sd3::inside_polyhedron_mapped(z, y, x, c1[0], c1[1], c1[2], pv1, fc, F, cm, safe1) &&
            sd3::inside_polyhedron_mapped(z, y, x, c2[0], c2[1], c2[2], pv2, fc, F, cm, safe2)) ++local;
      }
    }
    for (int o = 32; o; o >>= 1) local += __shfl_xor(local, o);
    if ((threadIdx.x & 63) == 0 && local) atomicAdd(&s_count, local);
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned int C = s_count;
      const float A_min = fminf(volume[ij.x], volume[ij.y]);
      const float overlap_maximal = (float)(((double)A_min + 1e-10) * (double)thr);      // :1321
      // overlap_render_polyhedron returns as soon as res > overlap_maximal (:629-631): the returned value is
      // the first integer exceeding it, or the full count if that is never reached.
      unsigned int res = C;
      if ((float)C > overlap_maximal) {
        // smallest n in [1, C] with (float)n > overlap_maximal
        unsigned int lo = 1, hi = C;
        while (lo < hi) { const unsigned int mid = lo + (hi - lo) / 2; if ((float)mid > overlap_maximal) hi = mid; else lo = mid + 1; }
        res = lo;
      }
      const float A_inter_render = (float)(int)res;
      const float iou = (float)((double)A_inter_render / ((double)A_min + 1e-10));       // :1325
      atomicAdd(&st->render, 1ull);
      if (iou > thr) { sink.suppress(ij.x, ij.y); atomicAdd(&st->sup_render, 1ull); }
    }
  }
}

__global__ void k_cone_map(const float* __restrict__ verts, const int* __restrict__ faces, int F, unsigned short* __restrict__ list,
                           signed char* __restrict__ count) {
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell < SD_CM_CELLS) sd3::cone_map_build_cell(cell, verts, faces, F, list, count);
}

}  // namespace

namespace sd {
// Convex hulls of n polyhedra (the half-spaces Qhull gives the reference in halfspaces_convex, stardist3d_impl.cpp:767-795):
// planes[(i*cap + f)*4 .. +3] = (nz, ny, nx, offset) with inside <=> n.p + offset <= 0, count[i] facets (cap = 2*n_rays),
// count[i] == -2 if the hull could not be built.  Buffers come from the CURRENT arena pass (caller has called begin()).
static unsigned short* g_last_hull_adj = nullptr;
unsigned short* last_hull_adj() { return g_last_hull_adj; }
int hull_planes(const float* d_dist, const float* d_points, const float* d_verts, int n, int R, double** planes, int** count, int* cap_out,
                hipStream_t s);
int hull_planes_adj(const float* d_dist, const float* d_points, const float* d_verts, int n, int R, double** planes, int** count, int* cap_out,
                    hipStream_t s) { return hull_planes(d_dist, d_points, d_verts, n, R, planes, count, cap_out, s); }
int hull_planes(const float* d_dist, const float* d_points, const float* d_verts, int n, int R, double** planes, int** count, int* cap_out,
                hipStream_t s) {
  if (R < 4 || R > 800) { sd::set_error("hull_planes: n_rays=%d unsupported (4..800)", R); return -1; }
  const int cap = 2 * R;
  const size_t ldsH = (size_t)3 * R * sizeof(double) + (size_t)2 * R * sizeof(unsigned int) +
                      (R <= HULL_FAST_MAXR ? (size_t)12 * R * sizeof(unsigned int) + (size_t)((R * R + 15) / 16) * 4 : 0);
  if (ldsH > 150 * 1024) { sd::set_error("hull_planes: n_rays too large for LDS staging"); return -1; }
  if (ldsH > 64 * 1024) SD_CHECK(hipFuncSetAttribute((const void*)k_hull, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsH));
  sd::Arena& A = sd::arena();
  double* pl = A.take_n<double>((size_t)n * cap * 4);
  unsigned short* adj = A.take_n<unsigned short>((size_t)n * cap * 3);
  int* cnt = A.take_n<int>(n);
  int* list = A.take_n<int>(n);
  if (!pl || !adj || !cnt || !list) return -1;
  hipLaunchKernelGGL(k_iota, dim3(sd::div_up(n, 256)), dim3(256), 0, s, list, n);
  const unsigned int bh = n < 32768 ? (unsigned int)n : 32768u;
  hipLaunchKernelGGL(k_hull, dim3(bh), dim3(64), ldsH, s, list, (unsigned int)n, d_dist, d_points, d_verts, R, cap, pl, adj, cnt);
  SD_LAUNCH_CHECK();
  *planes = pl; *count = cnt; *cap_out = cap; g_last_hull_adj = adj;
  return 0;
}
// cone map of a ray mesh (geom3d.h) in buffers of the CURRENT arena pass; *out stays {nullptr, nullptr} when the map is switched off
// (sd_set_option("nms3d_cone_map", 0)) or the mesh has too many faces for its 16-bit face ids
int cone_map(const float* d_verts, const int* d_faces, int F, sd3::ConeMap* out, hipStream_t s) {
  out->list = nullptr; out->count = nullptr;
  if (F > 65535 || sd::option(sd::OPT_NMS3D_CONE_MAP) == 0) return 0;
  sd::Arena& A = sd::arena();
  unsigned short* cmList = A.take_n<unsigned short>((size_t)SD_CM_CELLS * SD_CM_CAP);
  signed char* cmCount = A.take_n<signed char>(SD_CM_CELLS);
  if (!cmList || !cmCount) return -1;
  hipLaunchKernelGGL(k_cone_map, dim3(sd::div_up(SD_CM_CELLS, 64)), dim3(64), 0, s, d_verts, d_faces, F, cmList, cmCount);
  SD_LAUNCH_CHECK();
  out->list = cmList; out->count = cmCount;
  return 0;
}
}  // namespace sd

// Pair-level probe of the two volume stages (tests): for every pair (i, j) the EXACT intersection volume of the two kernels
// (reference: qhull_overlap_kernel :830-869, error value 0) and of the two convex hulls (qhull_overlap_convex_hulls :872-939,
// error value 1e10), computed by the same wave-cooperative fp64 routines the NMS cascade runs, with the bound shortcuts off.
extern "C" int sd_hiv_pairs_device(const float* d_dist, const float* d_points, int n_polys, int n_rays, int n_faces, const float* d_verts,
                                   const int* d_faces, const int32_t* d_pairs, int n_pairs, double* d_vol_kernel, double* d_vol_hull, void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  const int N = n_polys, R = n_rays, F = n_faces;
  if (n_pairs <= 0) return 0;
  if (R < 4 || F < 4 || R > 800) { sd::set_error("sd_hiv_pairs: need 4 <= n_rays <= 800 and n_faces >= 4"); return -1; }
  const size_t hivBytes = hiv_poly_bytes();
  const size_t ws3 = ((size_t)3 * R * sizeof(double) + 2 * R > hivBytes ? (((size_t)3 * R * sizeof(double) + 2 * R + 15) & ~(size_t)15) : hivBytes);
  const size_t lds3 = (size_t)8 * F * sizeof(double) + ws3 + (size_t)10 * F * sizeof(unsigned short);
  const size_t lds4 = (size_t)16 * R * sizeof(double) + hivBytes + (size_t)20 * R * sizeof(unsigned short);
  if (lds3 > 150 * 1024 || lds4 > 150 * 1024) { sd::set_error("sd_hiv_pairs: n_rays/n_faces too large for LDS staging"); return -1; }
  if (lds3 > 64 * 1024) SD_CHECK(hipFuncSetAttribute((const void*)k_stage3, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3));
  if (lds4 > 64 * 1024) SD_CHECK(hipFuncSetAttribute((const void*)k_stage4, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds4));
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  float* volume = A.take_n<float>(N);                       // only read by the (disabled) bound shortcuts
  int* faceAdj = A.take_n<int>((size_t)3 * F);
  Stats* d_st = (Stats*)A.take(sizeof(Stats));
  unsigned int* dummyCount = A.take_n<unsigned int>(1);
  unsigned char* state = A.take_n<unsigned char>(N);
  if (!volume || !faceAdj || !d_st || !dummyCount || !state) return -1;
  SD_CHECK(hipMemsetAsync(volume, 0, (size_t)N * sizeof(float), s));
  SD_CHECK(hipMemsetAsync(d_st, 0, sizeof(Stats), s));
  hipLaunchKernelGGL(k_face_adj, dim3(F), dim3(64), 0, s, d_faces, F, faceAdj);
  const int2* pairs = (const int2*)d_pairs;
  const unsigned int nb = (unsigned int)n_pairs < 16384u ? (unsigned int)n_pairs : 16384u;
  const size_t lds3x = stage3x_lds(F, ws3, 4);
  if (d_vol_kernel && sd::option(sd::OPT_NMS3D_SPLIT_EXACT) && lds3x <= 150 * 1024) {      // the routine the cascade uses: four waves per pair
    if (lds3x > 64 * 1024) SD_CHECK(hipFuncSetAttribute((const void*)k_stage3x<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3x));
    hipLaunchKernelGGL(k_stage3x<4>, dim3((unsigned int)n_pairs < 1024u ? (unsigned int)n_pairs : 1024u), dim3(256), lds3x, s, pairs, (const unsigned int*)nullptr,
                       (unsigned int)n_pairs, d_dist, d_points, d_verts, d_faces, faceAdj, R, F, volume, 0.f, SuppSink{state, nullptr, nullptr, 0u}, (int2*)nullptr,
                       dummyCount, d_st, (unsigned int)ws3, d_vol_kernel);
    SD_LAUNCH_CHECK();
  } else if (d_vol_kernel) {
    hipLaunchKernelGGL(k_stage3, dim3(nb), dim3(64), lds3, s, pairs, (unsigned int)n_pairs, d_dist, d_points, d_verts, d_faces, faceAdj, R, F, volume,
                       0.f, SuppSink{state, nullptr, nullptr, 0u}, (int2*)nullptr, dummyCount, d_st, (unsigned int)ws3 | 0x80000000u, d_verts, d_faces, R, F, d_vol_kernel);
    SD_LAUNCH_CHECK();
  }
  if (d_vol_hull) {
    double* planes = nullptr; int* count = nullptr; int cap = 0;
    if (sd::hull_planes_adj(d_dist, d_points, d_verts, N, R, &planes, &count, &cap, s)) return -1;
    const size_t lds4x = stage4x_lds(cap, 4);
    if (sd::option(sd::OPT_NMS3D_SPLIT_EXACT) && lds4x <= 150 * 1024) {
      if (lds4x > 64 * 1024) SD_CHECK(hipFuncSetAttribute((const void*)k_stage4x<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds4x));
      hipLaunchKernelGGL(k_stage4x<4>, dim3((unsigned int)n_pairs < 1024u ? (unsigned int)n_pairs : 1024u), dim3(256), lds4x, s, pairs, (const unsigned int*)nullptr,
                         (unsigned int)n_pairs, d_dist, d_points, R, cap, planes, sd::last_hull_adj(), count, volume, 0.f, (int2*)nullptr, dummyCount, d_st, d_vol_hull);
    } else
      hipLaunchKernelGGL(k_stage4, dim3(nb), dim3(64), lds4, s, pairs, (unsigned int)n_pairs, d_dist, d_points, d_verts, d_faces, R, F, cap, planes,
                         sd::last_hull_adj(), count, volume, 0.f, (int2*)nullptr, dummyCount, d_st, 1, d_verts, d_faces, R, F, d_vol_hull);
    SD_LAUNCH_CHECK();
  }
  Stats hst;
  SD_CHECK(hipMemcpyAsync(&hst, d_st, sizeof(Stats), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipStreamSynchronize(s));
  if (hst.overflow) { sd::set_error("sd_hiv_pairs: %llu pairs exceeded the polygon capacity of the volume routine", hst.overflow); return -1; }
  return 0;
}

// point-level probe of the voxel test of stage 5 / the rasteriser (inside_polyhedron, stardist3d_impl.cpp:153-191): out[t] = 1
// if point t lies in the union of the tetrahedra (centre, face) of ONE polyhedron; use_cone_map selects the face lists of
// geom3d.h instead of the loop over every face -- both must agree on every point (tests/test_gpu_parity3d.py).
namespace {
__global__ void __launch_bounds__(256) k_inside_probe(const float* __restrict__ dist, const float* __restrict__ centre, int R, int F,
                                                      const float* __restrict__ verts, const int* __restrict__ faces,
                                                      const float* __restrict__ points, long long n, sd3::ConeMap cm, unsigned char* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* pv = (float*)smem;
  __shared__ int s_unsafe;
  const float cz = centre[0], cy = centre[1], cx = centre[2];
  if (threadIdx.x == 0) s_unsafe = cm.list ? 0 : 1;
  __syncthreads();
  for (int k = threadIdx.x; k < R; k += blockDim.x) {
    const float d = dist[k];
    pv[3 * k] = cz + d * verts[3 * k]; pv[3 * k + 1] = cy + d * verts[3 * k + 1]; pv[3 * k + 2] = cx + d * verts[3 * k + 2];
    const float m = fmaxf(fmaxf(fabsf(pv[3 * k]), fabsf(pv[3 * k + 1])), fabsf(pv[3 * k + 2]));
    if (!(d >= 1.f) || !(m < 8192.f)) s_unsafe = 1;
  }
  __syncthreads();
  const bool safe = !s_unsafe && fabsf(cz) < 8192.f && fabsf(cy) < 8192.f && fabsf(cx) < 8192.f;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x)
    out[t] = sd3::inside_polyhedron_mapped(points[3 * t], points[3 * t + 1], points[3 * t + 2], cz, cy, cx, pv, faces, F, cm, safe) ? 1 : 0;
}
}  // namespace
extern "C" int sd_inside_polyhedron_device(const float* d_dist, const float* d_centre, int n_rays, int n_faces, const float* d_verts,
                                           const int* d_faces, const float* d_points, long long n, int use_cone_map, uint8_t* d_out,
                                           void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (n <= 0) return 0;
  if (n_rays < 4 || n_faces < 4 || n_rays > 800 || n_faces > 65535) { sd::set_error("sd_inside_polyhedron: need 4 <= n_rays <= 800, 4 <= n_faces <= 65535"); return -1; }
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  sd3::ConeMap cm{nullptr, nullptr};
  if (use_cone_map) {
    unsigned short* l = A.take_n<unsigned short>((size_t)SD_CM_CELLS * SD_CM_CAP);
    signed char* c = A.take_n<signed char>(SD_CM_CELLS);
    if (!l || !c) return -1;
    hipLaunchKernelGGL(k_cone_map, dim3(sd::div_up(SD_CM_CELLS, 64)), dim3(64), 0, s, d_verts, d_faces, n_faces, l, c);
    SD_LAUNCH_CHECK();
    cm.list = l; cm.count = c;
  }
  long long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_inside_probe, dim3((unsigned int)blocks), dim3(256), (size_t)3 * n_rays * sizeof(float), s, d_dist, d_centre, n_rays, n_faces, d_verts,
                     d_faces, d_points, n, cm, d_out);
  SD_LAUNCH_CHECK();
  return 0;
}

extern "C" int sd_nms3d_device(const float* d_scores, const float* d_dist, const float* d_points, int n_polys, int n_rays, int n_faces,
                               const float* d_verts, const int* d_faces, float threshold, int use_bbox, int use_kdtree, int verbose,
                               uint8_t* d_keep, int64_t* stats, void* stream_) {
  (void)d_scores;   // unused by the reference's arithmetic as well
  hipStream_t s = (hipStream_t)stream_;
  const int N = n_polys, R = n_rays, F = n_faces;
  if (stats) memset(stats, 0, 16 * sizeof(int64_t));
  if (verbose) {
    printf("Non Maximum Suppression (3D) ++++ \n");
    printf("NMS: n_polys  = %d \nNMS: n_rays   = %d  \nNMS: n_faces  = %d \nNMS: thresh   = %.3f \nNMS: use_bbox = %d \nNMS: use_kdtree = %d \n",
           N, R, F, threshold, use_bbox, use_kdtree);
    printf("NMS: using HIP (gfx950)\n");
    fflush(stdout);
  }
  if (N <= 0) return 0;
  if (R < 4 || F < 4) { sd::set_error("sd_nms3d: need n_rays >= 4 and n_faces >= 4"); return -1; }
  if (R > 800) { sd::set_error("sd_nms3d: n_rays must be <= 800"); return -1; }
  const size_t hivBytes = hiv_poly_bytes();
  const size_t ws3 = ((size_t)3 * R * sizeof(double) + 2 * R > hivBytes ? (((size_t)3 * R * sizeof(double) + 2 * R + 15) & ~(size_t)15) : hivBytes);   // >= 6R floats
  const size_t lds3 = (size_t)8 * F * sizeof(double) + ws3 + (size_t)10 * F * sizeof(unsigned short);
  const size_t lds5 = (size_t)6 * R * sizeof(float) + (size_t)3 * F * sizeof(int);
  const size_t lds4 = (size_t)16 * R * sizeof(double) + hivBytes + (size_t)20 * R * sizeof(unsigned short);   // cap = 2R
  if (lds3 > 150 * 1024 || lds5 > 150 * 1024 || lds4 > 150 * 1024) { sd::set_error("sd_nms3d: n_rays/n_faces too large for LDS staging"); return -1; }
  const size_t ldsH = (size_t)3 * R * sizeof(double) + (size_t)2 * R * sizeof(unsigned int) +
                      (R <= HULL_FAST_MAXR ? (size_t)12 * R * sizeof(unsigned int) + (size_t)((R * R + 15) / 16) * 4 : 0);
  // more than 64 KiB of dynamic LDS needs an explicit opt-in (only reached with several hundred rays)
  if (lds3 > 64 * 1024) SD_CHECK(hipFuncSetAttribute((const void*)k_stage3, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3));
  if (lds4 > 64 * 1024) SD_CHECK(hipFuncSetAttribute((const void*)k_stage4, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds4));
  if (lds5 > 64 * 1024) SD_CHECK(hipFuncSetAttribute((const void*)k_stage5, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds5));
  // exact volumes of the undecided pairs by four waves per pair (k_stage3x): when the four workspaces fit
  // (the launches of the later rounds hold few pairs and lasted as long as their slowest pair, an exact volume of ~1 ms by one wave;
  // in the first round the one-wave form is faster: thousands of exact volumes keep every SIMD busy either way)
  const size_t lds3x = stage3x_lds(F, ws3, 4), lds4x = stage4x_lds(2 * R, 4);
  // option nms3d_split_exact: 0 exact volumes in place; 1 second pass (k_stage3x / k_stage4x: four waves per pair) for the smaller launches
  // (round 3); 2 (default): stage 3 ALWAYS splits, and a bounds-only first pass is launched with the small LDS footprint (no polygon
  // workspace: 25.6 instead of 39.3 KB per wave = six waves per CU instead of four) -- measured on the 256^3 bench set: stage 3
  // 12.9 -> 10.7 ms; stage 4 keeps its threshold (always splitting it: 12.6 -> 13.1 ms, the hull construction dominates there);
  // 3: both stages always split
  const int splitOpt = sd::option(sd::OPT_NMS3D_SPLIT_EXACT);
  const bool split3 = splitOpt && lds3x <= 150 * 1024;
  const bool split4 = splitOpt && lds4x <= 150 * 1024;
  const unsigned int split3Max = splitOpt >= 2 ? 0x7fffffffu : 32768u, split4Max = splitOpt >= 3 ? 0x7fffffffu : 16384u;   // pairs per launch up to which the second pass pays
  if (split3 && lds3x > 64 * 1024) SD_CHECK(hipFuncSetAttribute((const void*)k_stage3x<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3x));
  if (split4 && lds4x > 64 * 1024) SD_CHECK(hipFuncSetAttribute((const void*)k_stage4x<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds4x));
  if (ldsH > 64 * 1024) SD_CHECK(hipFuncSetAttribute((const void*)k_hull, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsH));
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (stats) { SD_CHECK(hipEventCreate(&ev0)); SD_CHECK(hipEventCreate(&ev1)); }
  struct EvGuard { hipEvent_t a, b; ~EvGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } evguard{ev0, ev1};
  hipEvent_t evb0 = nullptr, evb1 = nullptr;          // broad phase (per-candidate precompute, grid, neighbour lists): the HBM-bound scan
  if (stats) { SD_CHECK(hipEventCreate(&evb0)); SD_CHECK(hipEventCreate(&evb1)); SD_CHECK(hipEventRecord(evb0, s)); }
  EvGuard evguardb{evb0, evb1};
  double ns3 = 0, ns4 = 0, ns5 = 0;
  const bool trace = sd::option(sd::OPT_TRACE) != 0;
  if (!use_kdtree && !use_bbox && threshold < 0) {   // every (0, j) passes and iou >= 0 > thr at stage 2
    SD_CHECK(hipMemsetAsync(d_keep, 0, N, s));
    SD_CHECK(hipMemsetAsync(d_keep, 1, 1, s));
    SD_CHECK(hipStreamSynchronize(s));
    return 0;
  }
  float* volume = A.take_n<float>(N);
  int* bbox = A.take_n<int>((size_t)6 * N);
  float* r_outer = A.take_n<float>(N);
  float* r_outer_iso = A.take_n<float>(N);
  float* r_inner_iso = A.take_n<float>(N);
  int* gi = A.take_n<int>(8);
  unsigned char* state = A.take_n<unsigned char>(N);
  int* candCell = A.take_n<int>(N);
  if (!volume || !bbox || !r_outer || !r_outer_iso || !r_inner_iso || !gi || !state || !candCell) return -1;
  const int gi_init[8] = {0, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, 0};
  SD_CHECK(hipMemcpyAsync(gi, gi_init, sizeof(gi_init), hipMemcpyHostToDevice, s));
  SD_CHECK(hipMemsetAsync(state, 0, N, s));
  size_t ldsRows = (size_t)128 * (R + 1) * sizeof(float);
  const int staged = ldsRows <= 150 * 1024 ? 1 : 0;
  if (!staged) ldsRows = 0;
  if (ldsRows > 64 * 1024) {
    SD_CHECK(hipFuncSetAttribute((const void*)k_pre1, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsRows));
    SD_CHECK(hipFuncSetAttribute((const void*)k_pre2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsRows));
  }
  hipLaunchKernelGGL(k_pre1, dim3(sd::div_up(N, 128)), dim3(128), ldsRows, s, d_dist, d_points, d_verts, d_faces, N, R, F, volume, bbox, staged);
  SD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_minmax3, dim3(sd::div_up(N, 256)), dim3(256), 0, s, d_points, N, gi + 1);
  // cone map for the voxel tests of stage 5 (geom3d.h); option "nms3d_cone_map" = 0 tests every face as the reference does.  It depends on
  // the ray mesh only and is a latency-bound launch of a few workgroups (0.23 ms at 96 rays): it runs on a helper stream NEXT TO the
  // read-back of the bounding boxes and the host's sequential anisotropy sum below (0.3 ms of otherwise idle device), joined before the rounds
  sd3::ConeMap cmap{nullptr, nullptr};
  struct ConeJoin { hipEvent_t fork = nullptr, done = nullptr; bool pending = false;
                    ~ConeJoin() { if (pending) (void)hipEventSynchronize(done);       // (an error return: the helper stream still writes into the arena)
                                  if (fork) (void)hipEventDestroy(fork); if (done) (void)hipEventDestroy(done); } } coneJoin;
  if (F <= 65535 && sd::option(sd::OPT_NMS3D_CONE_MAP) != 0) {
    unsigned short* cmList = A.take_n<unsigned short>((size_t)SD_CM_CELLS * SD_CM_CAP);
    signed char* cmCount = A.take_n<signed char>(SD_CM_CELLS);
    if (!cmList || !cmCount) return -1;
    hipStream_t side = sd::side_stream();          // (nullptr: everything stays on the caller's stream)
    if (side) {
      SD_CHECK(hipEventCreateWithFlags(&coneJoin.fork, hipEventDisableTiming));
      SD_CHECK(hipEventCreateWithFlags(&coneJoin.done, hipEventDisableTiming));
      SD_CHECK(hipEventRecord(coneJoin.fork, s));
      SD_CHECK(hipStreamWaitEvent(side, coneJoin.fork, 0));
    }
    hipLaunchKernelGGL(k_cone_map, dim3(sd::div_up(SD_CM_CELLS, 64)), dim3(64), 0, side ? side : s, d_verts, d_faces, F, cmList, cmCount);
    SD_LAUNCH_CHECK();
    if (side) { SD_CHECK(hipEventRecord(coneJoin.done, side)); coneJoin.pending = true; }
    cmap.list = cmList; cmap.count = cmCount;
  }
  // anisotropy: sequential fp32 accumulation over candidates (:1008-1010) on the host
  std::vector<int> hb((size_t)6 * N);
  SD_CHECK(hipMemcpyAsync(hb.data(), bbox, (size_t)6 * N * sizeof(int), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipStreamSynchronize(s));
  Aniso an;
  {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int i = 0; i < N; ++i) {
      a0 += (float)(hb[6 * (size_t)i + 1] - hb[6 * (size_t)i]) / N;
      a1 += (float)(hb[6 * (size_t)i + 3] - hb[6 * (size_t)i + 2]) / N;
      a2 += (float)(hb[6 * (size_t)i + 5] - hb[6 * (size_t)i + 4]) / N;
    }
    const float tmp = fmaxf(fmaxf(a0, a1), a2);
    an.a[0] = tmp / a0; an.a[1] = tmp / a1; an.a[2] = tmp / a2;
  }
  if (verbose) { printf("NMS: calculated anisotropy: %.2f \t %.2f \t %.2f \n", an.a[0], an.a[1], an.a[2]); fflush(stdout); }
  hipLaunchKernelGGL(k_pre2, dim3(sd::div_up(N, 128)), dim3(128), ldsRows, s, d_dist, d_verts, d_faces, N, R, F, an, r_outer, r_outer_iso, r_inner_iso, gi, staged);
  SD_LAUNCH_CHECK();
  int g[8];
  SD_CHECK(hipMemcpyAsync(g, gi, sizeof(g), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipStreamSynchronize(s));
  float max_dist;
  memcpy(&max_dist, &g[0], 4);

  Grid3 gr;
  float cs = (2.f * max_dist + 1.f) * 0.5f * 1.0001f + 1e-3f;
  if (!(cs >= 1.f)) cs = 1.f;
  const int W = 2;
  if (!use_kdtree) {
    // the reference then tests every j > i (:1172-1176): one grid cell = all pairs
    if (N > 16384) { sd::set_error("sd_nms3d: use_kdtree=0 is only supported up to 16384 candidates (all-pairs)"); return -1; }
    cs = 4.f * (fmaxf(fmaxf((float)g[2] - g[1], (float)g[4] - g[3]), (float)g[6] - g[5]) + 2.f);
  }
  for (;;) {
    gr.nz = (int)(((double)g[2] - g[1]) / cs) + 1;
    gr.ny = (int)(((double)g[4] - g[3]) / cs) + 1;
    gr.nx = (int)(((double)g[6] - g[5]) / cs) + 1;
    if ((i64)gr.nz * gr.ny * gr.nx <= (1ll << 26)) break;
    cs *= 2.f;
  }
  gr.z0 = (float)g[1]; gr.y0 = (float)g[3]; gr.x0 = (float)g[5]; gr.inv_cs = 1.f / cs;
  const int nCells = gr.nz * gr.ny * gr.nx;
  int* cellCount = A.take_n<int>(nCells + 1);
  int* cellStart = A.take_n<int>(nCells + 1);
  int* cellFill = A.take_n<int>(nCells + 1);
  CellRec3* cellRec = A.take_n<CellRec3>(N);
  int* nbrCount = A.take_n<int>(N + 1);
  int* nbrLow = A.take_n<int>(N + 1);
  i64* nbrStart = A.take_n<i64>(N + 1);
  if (!cellCount || !cellStart || !cellFill || !cellRec || !nbrCount || !nbrLow || !nbrStart) return -1;
  SD_CHECK(hipMemsetAsync(cellCount, 0, (nCells + 1) * sizeof(int), s));
  SD_CHECK(hipMemsetAsync(cellFill, 0, (nCells + 1) * sizeof(int), s));
  hipLaunchKernelGGL(k_cell_count3, dim3(sd::div_up(N, 256)), dim3(256), 0, s, d_points, N, gr, cellCount, candCell);
  size_t tb1 = 0, tb2 = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb1, cellCount, cellStart, nCells + 1, s);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, nbrCount, nbrStart, N + 1, s);
  if (tb2 > tb1) tb1 = tb2;
  void* scanTmp = A.take(tb1 + 256);
  if (!scanTmp) return -1;
  SD_CHECK(hipcub::DeviceScan::ExclusiveSum(scanTmp, tb1, cellCount, cellStart, nCells + 1, s));
  // neighbour lists in ONE pass (option "nms3d_neighbours_single_pass", default 1; nms2d.hip has the 2D twin): slots sized from the cell
  // table, better-scored neighbours from the slot's front, the others from its back, the exact total summed afterwards; the two-pass form
  // (count, scan, fill: every candidate test done twice) remains for inputs whose slots would exceed 32-bit indices or the workspace
  const bool singlePass = sd::option(sd::OPT_NMS3D_NBR_SINGLE) != 0;
  SD_CHECK(hipMemsetAsync(nbrCount, 0, (N + 1) * sizeof(int), s));
  hipLaunchKernelGGL(k_cell_fill3, dim3(sd::div_up(N, 256)), dim3(256), 0, s, N, candCell, cellStart, cellFill, d_points, bbox, cellRec, gr, W,
                     singlePass ? nbrCount : (int*)nullptr);
  SD_LAUNCH_CHECK();
  const int nbBlocks = (sd::div_up(N, 4) + 7) & ~7;
  NmsFlags f;
  f.use_kdtree = use_kdtree; f.use_bbox = use_bbox; f.thr_nonneg = (threshold >= 0.f); f.thr = threshold; f.max_dist = max_dist;
  // ray mesh: edge adjacency (seeds of the exact volume routine) and validity (precondition of the volume bounds)
  int* faceAdj = A.take_n<int>((size_t)3 * F);
  int* d_mesh = A.take_n<int>(4);
  double* d_mesh_sa = A.take_n<double>(1);
  if (!faceAdj || !d_mesh || !d_mesh_sa) return -1;
  SD_CHECK(hipMemsetAsync(d_mesh, 0, 4 * sizeof(int), s));
  SD_CHECK(hipMemsetAsync(d_mesh_sa, 0, sizeof(double), s));
  hipLaunchKernelGGL(k_face_adj, dim3(F), dim3(64), 0, s, d_faces, F, faceAdj);
  hipLaunchKernelGGL(k_mesh_check, dim3(sd::div_up(F, 64)), dim3(64), 0, s, d_verts, d_faces, faceAdj, F, d_mesh, d_mesh_sa);
  SD_LAUNCH_CHECK();
  int h_mesh[4]; double h_mesh_sa = 0;
  SD_CHECK(hipMemcpyAsync(h_mesh, d_mesh, sizeof(h_mesh), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipMemcpyAsync(&h_mesh_sa, d_mesh_sa, sizeof(double), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipStreamSynchronize(s));
  const bool mesh_ok = h_mesh[0] == 0 && fabs(h_mesh_sa - 4.0 * M_PI) < 1e-6;
  const bool use_bounds = mesh_ok && sd::option(sd::OPT_NMS3D_VOLUME_BOUNDS) != 0;
  if (trace) printf("ray mesh: open/degenerate flags %d, orientation +%d/-%d, solid angle %.9f -> volume bounds %s\n", h_mesh[0], h_mesh[1], h_mesh[2],
                    h_mesh_sa, use_bounds ? "on" : "off");
  // direction mesh of the volume bounds: refined once (k_refine_mesh) when its ray-cast workspace fits the LDS the stages have anyway
  const float* bverts = d_verts; const int* bfaces = d_faces; int bR = R, bF = F;
  {
    const int R2 = R + 3 * F / 2, F2 = 4 * F;
    const size_t need = (size_t)3 * R2 * sizeof(double) + (size_t)2 * R2;
    if (use_bounds && F % 2 == 0 && need <= hivBytes && need <= ws3 && R2 < 65535 && sd::option(sd::OPT_NMS3D_REFINE_MESH) != 0) {
      float* v2 = A.take_n<float>((size_t)3 * R2);
      int* f2 = A.take_n<int>((size_t)3 * F2);
      int* edgeId = A.take_n<int>((size_t)3 * F);
      int* ecount = A.take_n<int>(1);
      if (!v2 || !f2 || !edgeId || !ecount) return -1;
      SD_CHECK(hipMemsetAsync(ecount, 0, sizeof(int), s));
      hipLaunchKernelGGL(k_refine_edges, dim3(sd::div_up(3 * F, 64)), dim3(64), 0, s, d_faces, faceAdj, F, edgeId, ecount);
      hipLaunchKernelGGL(k_refine_mesh, dim3(sd::div_up(F > R ? F : R, 64)), dim3(64), 0, s, d_verts, d_faces, faceAdj, R, F, edgeId, v2, f2);
      SD_LAUNCH_CHECK();
      bverts = v2; bfaces = f2; bR = R2; bF = F2;
    }
  }
  // refined once more for the pairs that reach the exact-volume kernels (k_stage3x / k_stage4x evaluate it with the whole workgroup;
  // its ray-cast vectors live in the polygon workspaces of waves 1..3, which are idle until the integration starts)
  const float* b3verts = nullptr; const int* b3faces = nullptr; int b3R = 0, b3F = 0;
  if (bR != R && splitOpt && sd::option(sd::OPT_NMS3D_REFINE_MESH) >= 2) {
    const int R3 = bR + 3 * bF / 2, F3 = 4 * bF;
    const size_t need = (size_t)3 * R3 * sizeof(double) + (size_t)2 * R3;
    if (need <= (size_t)3 * hivBytes && R3 < 65535) {
      int* adj2 = A.take_n<int>((size_t)3 * bF);
      float* v3 = A.take_n<float>((size_t)3 * R3);
      int* f3 = A.take_n<int>((size_t)3 * F3);
      int* edgeId = A.take_n<int>((size_t)3 * bF);
      int* ecount = A.take_n<int>(1);
      if (!adj2 || !v3 || !f3 || !edgeId || !ecount) return -1;
      SD_CHECK(hipMemsetAsync(ecount, 0, sizeof(int), s));
      hipLaunchKernelGGL(k_face_adj, dim3(bF), dim3(64), 0, s, bfaces, bF, adj2);
      hipLaunchKernelGGL(k_refine_edges, dim3(sd::div_up(3 * bF, 64)), dim3(64), 0, s, bfaces, adj2, bF, edgeId, ecount);
      hipLaunchKernelGGL(k_refine_mesh, dim3(sd::div_up(bF > bR ? bF : bR, 64)), dim3(64), 0, s, bverts, bfaces, adj2, bR, bF, edgeId, v3, f3);
      SD_LAUNCH_CHECK();
      b3verts = v3; b3faces = f3; b3R = R3; b3F = F3;
    }
  }
  // neighbour lists (build_neighbour_lists, nms_rounds.h)
  NbrLists L{};
  L.count = nbrCount; L.low = nbrLow; L.start = nbrStart;
  auto launch_neighbours = [&](int mode, const NbrLists& l) {
    if (mode == 0)
      hipLaunchKernelGGL((k_neighbours3<0>), dim3(nbBlocks), dim3(256), 0, s, N, gr, f, cellRec, candCell, cellStart,
                         nbrCount, nbrLow, (const i64*)nullptr, (int*)nullptr, (int*)nullptr, W);
    else if (mode == 1)
      hipLaunchKernelGGL((k_neighbours3<1>), dim3(nbBlocks), dim3(256), 0, s, N, gr, f, cellRec, candCell, cellStart,
                         nbrCount, nbrLow, (const i64*)nbrStart, l.nbr, l.waitOn, W);
    else
      hipLaunchKernelGGL((k_neighbours3<2>), dim3(nbBlocks), dim3(256), 0, s, N, gr, f, cellRec, candCell, cellStart,
                         nbrCount, nbrLow, (const i64*)nbrStart, l.nbr, l.waitOn, W);
  };
  const int rcLists = build_neighbour_lists(A, s, N, singlePass, scanTmp, tb1, launch_neighbours, []() { return 0; }, L);
  // capacity of one call (32-bit indices into the neighbour lists and pair queues, N * n_rays * 4 bytes of distances): beyond it the
  // input has to be sharded -- predict_instances_sharded / predict_instances_big do exactly that
  if (rcLists > 0 || (rcLists == 0 && (i64)N * R >= (i64)0x3fffffff)) {
    sd::set_error("sd_nms3d: %d candidates (%lld neighbour entries) exceed the capacity of one call (2^30 distance values, 2^31 - 1 "
                  "neighbour entries): shard the input (predict_instances_sharded / predict_instances_big)", N, (long long)L.total);
    return -1;
  }
  if (rcLists) return -1;
  const int* nbr = L.nbr;
  int* waitOn = L.waitOn;
  const i64 totalNbr = L.total;
  if (stats) SD_CHECK(hipEventRecord(evb1, s));

  // (the cone map of stage 5 was started on the helper stream in front of the anisotropy sum; from here on the caller's stream waits for it)
  if (coneJoin.pending) { SD_CHECK(hipStreamWaitEvent(s, coneJoin.done, 0)); coneJoin.pending = false; }
  const unsigned int pairCap = (unsigned int)((totalNbr / 2 + 64) < (1ll << 31) ? (totalNbr / 2 + 64) : ((1ll << 31) - 1));
  int* U0 = A.take_n<int>(N);
  int* U1 = A.take_n<int>(N);
  int* Kl = A.take_n<int>(N);
  int* Sl = A.take_n<int>(N);
  int2* pairs3 = A.take_n<int2>(pairCap);
  int2* pairs4 = A.take_n<int2>(pairCap);
  int2* pairs5 = A.take_n<int2>(pairCap);
  int2* pairsX = (split3 || split4) ? A.take_n<int2>(pairCap) : nullptr;          // pairs whose exact volume is needed
  struct Counters { int nU, nK, nS; unsigned int nP3, nP4, nP5, nHull, nX3, nX4; };     // (the first three: k_round_triage / k_round_scan)
  Counters* d_cnt = (Counters*)A.take(sizeof(Counters));
  Stats* d_st = (Stats*)A.take(sizeof(Stats));
  if (!U0 || !U1 || !Kl || !Sl || !pairs3 || !pairs4 || !pairs5 || !d_cnt || !d_st || ((split3 || split4) && !pairsX)) return -1;
  const int hullCap = 2 * R;                       // a hull of R points has at most 2R-4 facets
  int* hullState = A.take_n<int>(N);
  int* hullCount = A.take_n<int>(N);
  int* hullList = A.take_n<int>(N);
  double* hullPlanes = nullptr;                    // N * hullCap * 4 doubles, allocated on first use
  unsigned short* hullAdj = nullptr;               // N * hullCap * 3

  if (!hullState || !hullCount || !hullList) return -1;
  SD_CHECK(hipMemsetAsync(hullState, 0, (size_t)N * sizeof(int), s));
  SD_CHECK(hipMemsetAsync(d_st, 0, sizeof(Stats), s));
  hipLaunchKernelGGL(k_iota, dim3(sd::div_up(N, 256)), dim3(256), 0, s, U0, N);
  int nU = N, rounds = 0;
  int* Ucur = U0; int* Unext = U1;
  Counters h;
  // Tail batch: the late rounds hold few pairs, but every stage launch costs the latency of its slowest pair (an exact volume: ~1.5 ms).
  // Once few candidates are undecided (N/128, at least 512), the cascade is run ONCE over every pair of undecided candidates the
  // sequential loop could still evaluate (speculatively: i need not end up kept), suppressions are recorded as edges, and the remaining
  // greedy order is replayed on the device over those edges (k_tail3_mark / k_tail3_promote).  Same fixed point: j is suppressed iff
  // some KEPT i < j suppresses it.  The threshold is late on purpose: undecided candidates sit in dense clusters, so the speculative
  // pair count grows quickly with them (measured on the 256^3 bench set: at N/8 = 16 404 undecided candidates 71 674 stage-3 pairs
  // instead of the 2 397 the plain rounds evaluate -- slower than the rounds it replaces; at N/128 the three last rounds, ~7 ms of
  // launch latency, become one pass).  sd_set_option("nms3d_tail_batch", 0) keeps the plain rounds (the parity suite runs both).
  const int tailOpt = sd::option(sd::OPT_NMS3D_TAIL_BATCH), tailDiv = tailOpt >= 2 ? tailOpt : 32;       // option value >= 2: the divisor itself (tuning)
  const int tailT = tailOpt ? (N / tailDiv > 512 ? N / tailDiv : 512) : -1;
  int2* supEdges = nullptr; unsigned int* supCount = nullptr; unsigned char* blocked = nullptr; int* d_left = nullptr;
  // exact volumes of the late rounds carried into the tail batch (k_defer3): from round deferFrom on, while the queue has room for
  // the round's pairs.  Needs the tail batch and the split exact-volume passes (the bounds passes hand over the undecided pairs).
  const int deferFrom = (tailOpt && use_bounds && (split3 || split4)) ? sd::option(sd::OPT_NMS3D_DEFER_EXACT) : 0;
  const unsigned int dfrCap = 262144u;
  int2* dfr = nullptr; unsigned int* dfrCount = nullptr; unsigned char* pend = nullptr;
  unsigned int hDef = 0;                                   // pairs queued so far (host mirror: the counters of every round are read anyway)
  if (deferFrom > 0) {
    dfr = A.take_n<int2>(dfrCap); dfrCount = A.take_n<unsigned int>(1); pend = A.take_n<unsigned char>(N);
    if (!dfr || !dfrCount || !pend) return -1;
    SD_CHECK(hipMemsetAsync(dfrCount, 0, sizeof(unsigned int), s));
    SD_CHECK(hipMemsetAsync(pend, 0, N, s));
  }
  const unsigned int noReuse = sd::option(sd::OPT_NMS3D_BOUNDS_REUSE) ? 0u : SD_NOREUSE_BIT;
  const bool leanOpt = use_bounds && sd::option(sd::OPT_NMS3D_BOUNDS_LEAN) != 0;
  bool forceTail = false;
  while (nU > 0) {
    ++rounds;
    const bool tail = rounds > 1 && (nU <= tailT || forceTail);
    SD_CHECK(hipMemsetAsync(d_cnt, 0, sizeof(Counters), s));
    if (tail) {
      if (!supEdges) {
        supEdges = A.take_n<int2>(pairCap); supCount = A.take_n<unsigned int>(1); blocked = A.take_n<unsigned char>(N); d_left = A.take_n<int>(1);
        if (!supEdges || !supCount || !blocked || !d_left) return -1;
      }
      SD_CHECK(hipMemsetAsync(supCount, 0, sizeof(unsigned int), s));
      SD_CHECK(hipMemsetAsync(blocked, 0, N, s));
      if (hDef) hipLaunchKernelGGL(k_seed3, dim3(sd::div_up(hDef, 256)), dim3(256), 0, s, dfr, dfrCount, dfrCap, pairs3, &d_cnt->nP3);
      h.nK = nU; h.nU = 0;
    } else {
      hipLaunchKernelGGL(k_round_triage, dim3(sd::div_up(nU, 256)), dim3(256), 0, s, Ucur, nU, state, waitOn, Unext, Kl, Sl, (int*)d_cnt, (const unsigned char*)pend);
      const int wgrid = sd::div_up(nU, 4) < 2048 ? sd::div_up(nU, 4) : 2048;
      hipLaunchKernelGGL(k_round_scan, dim3(wgrid), dim3(256), 0, s, Sl, state, nbrStart, nbrLow, nbr, waitOn, Unext, Kl, (int*)d_cnt, (const unsigned char*)pend);
      SD_LAUNCH_CHECK();
    }
    const SuppSink sink = tail ? SuppSink{state, supEdges, supCount, pairCap} : SuppSink{state, nullptr, nullptr, 0u};
    {
      // ONE read-back for the survivors, the undecided and the stage-3 pairs of the round: the emission takes the survivor count from
      // device memory (a persistent grid sized from the undecided candidates), as the 2D rounds do
      const int egrid = sd::div_up(nU, 4) < 2048 ? sd::div_up(nU, 4) : 2048;
      hipLaunchKernelGGL(k_round_emit3, dim3(egrid), dim3(256), 0, s, tail ? Ucur : Kl, tail ? nU : 0, tail ? (const int*)nullptr : (const int*)&d_cnt->nK, sink, tail ? 1 : 0,
                         nbrStart, nbrCount, nbr, f, an, d_points, bbox, volume, r_outer, r_outer_iso, r_inner_iso, pairs3, &d_cnt->nP3, pairCap, d_st);
      SD_LAUNCH_CHECK();
      SD_CHECK(hipMemcpyAsync(&h, d_cnt, sizeof(Counters), hipMemcpyDeviceToHost, s));
      SD_CHECK(hipStreamSynchronize(s));
    }
    if (!tail && h.nK == 0 && h.nU > 0) {
      if (!hDef) { sd::set_error("sd_nms3d: greedy scan made no progress (internal error)"); return -1; }
      // every remaining candidate is pending or waits for a pending one: the tail batch takes over from here
      forceTail = true;
      nU = h.nU;
      int* t = Ucur; Ucur = Unext; Unext = t;
      continue;
    }
    const int nUndecided = tail ? 0 : h.nU;
    {
      if (h.nP3 > pairCap) { sd::set_error("sd_nms3d: pair queue overflow (internal error)"); return -1; }
      if (h.nP3 > 0) {
        const unsigned int b3 = h.nP3 < 16384u ? h.nP3 : 16384u;
        if (stats) SD_CHECK(hipEventRecord(ev0, s));
        const bool sp3 = split3 && h.nP3 <= split3Max;
        // bounds-only pass: the workspace only holds the ray-cast vectors (3 bR doubles + bR shorts; at least the 6 R floats of the vertex staging)
        const size_t ws3s = (std::max((size_t)6 * R * sizeof(float), (size_t)3 * bR * sizeof(double) + (size_t)2 * bR) + 15) & ~(size_t)15;
        const bool small3 = sp3 && splitOpt >= 2 && ws3s < ws3;
        const size_t ws3l = small3 ? ws3s : ws3;
        const bool lean3 = small3 && leanOpt;            // bounds-only launch: no seed / pos / orig tables behind the workspace
        const size_t lds3l = (size_t)8 * F * sizeof(double) + ws3l + (lean3 ? (size_t)0 : (size_t)10 * F * sizeof(unsigned short));
        hipLaunchKernelGGL(k_stage3, dim3(b3), dim3(64), lds3l, s, pairs3, h.nP3, d_dist, d_points, d_verts, d_faces, faceAdj, R, F, volume,
                           threshold, sink, pairs4, &d_cnt->nP4, d_st, (unsigned int)ws3l | (use_bounds ? 0u : 0x80000000u) | (trace ? SD_PROF_BIT : 0u) | noReuse | (lean3 ? SD_LEAN_BIT : 0u), bverts, bfaces, bR, bF,
                           (double*)nullptr, sp3 ? pairsX : (int2*)nullptr, &d_cnt->nX3);
        const bool defer3 = sp3 && !tail && deferFrom > 0 && rounds >= deferFrom && hDef + h.nP3 <= dfrCap;
        if (defer3)
          hipLaunchKernelGGL(k_defer3, dim3(h.nP3 < 16384u ? sd::div_up(h.nP3, 256) : 64), dim3(256), 0, s, pairsX, &d_cnt->nX3, dfr, dfrCount, dfrCap, pend, &d_st->overflow);
        else if (sp3)
          hipLaunchKernelGGL(k_stage3x<4>, dim3(h.nP3 < 256u ? h.nP3 : 256u), dim3(256), lds3x, s, pairsX, &d_cnt->nX3, 0u, d_dist, d_points, d_verts, d_faces, faceAdj,
                             R, F, volume, threshold, sink, pairs4, &d_cnt->nP4, d_st, (unsigned int)ws3, (double*)nullptr, b3verts, b3faces, b3R, b3F);
        SD_LAUNCH_CHECK();
        if (stats) SD_CHECK(hipEventRecord(ev1, s));
        SD_CHECK(hipMemcpyAsync(&h, d_cnt, sizeof(Counters), hipMemcpyDeviceToHost, s));
        SD_CHECK(hipStreamSynchronize(s));
        if (defer3) hDef += h.nX3;
        if (stats) { float ms = 0; SD_CHECK(hipEventElapsedTime(&ms, ev0, ev1)); ns3 += ms * 1e6;
                     if (trace) printf("round %d: nU=%d nK=%d stage3 pairs=%u %.3f ms -> stage4 pairs=%u\n", rounds, h.nU, h.nK, h.nP3, ms, h.nP4); }
        if (h.nP4 > 0) {
          const unsigned int b4 = h.nP4 < 16384u ? h.nP4 : 16384u;
          if (stats) SD_CHECK(hipEventRecord(ev0, s));
          if (!hullPlanes) {
            hullPlanes = A.take_n<double>((size_t)N * hullCap * 4);
            hullAdj = A.take_n<unsigned short>((size_t)N * hullCap * 3);
            if (!hullPlanes || !hullAdj) return -1;
          }
          SD_CHECK(hipMemsetAsync(&d_cnt->nHull, 0, sizeof(unsigned int), s));
          hipLaunchKernelGGL(k_hull_mark, dim3(sd::div_up(h.nP4, 256)), dim3(256), 0, s, pairs4, h.nP4, hullState, hullList, &d_cnt->nHull);
          {
            // no read-back of the hull count (~40 us of idle device per round): a pair asks for at most two hulls, the kernel reads the
            // length of its list on the device; the count reaches the host with the counters behind stage 4
            const unsigned long long ub = 2ull * h.nP4;
            const unsigned int bh = ub < 32768ull ? (unsigned int)ub : 32768u;
            hipLaunchKernelGGL(k_hull, dim3(bh), dim3(64), ldsH, s, hullList,
                               0u, d_dist, d_points, d_verts, R, hullCap, hullPlanes, hullAdj, hullCount, (const unsigned int*)&d_cnt->nHull);
            SD_LAUNCH_CHECK();
          }
          const bool sp4 = split4 && h.nP4 <= split4Max;
          const size_t ws4s = (((size_t)3 * bR * sizeof(double) + (size_t)2 * bR) + 15) & ~(size_t)15;
          const bool small4 = sp4 && splitOpt >= 2 && ws4s < hivBytes;
          const bool lean4 = small4 && leanOpt;
          const size_t lds4l = small4 ? (size_t)16 * R * sizeof(double) + ws4s + (lean4 ? (size_t)0 : (size_t)20 * R * sizeof(unsigned short)) : lds4;
          hipLaunchKernelGGL(k_stage4, dim3(b4), dim3(64), lds4l, s, pairs4, h.nP4, d_dist, d_points, d_verts, d_faces, R, F, hullCap, hullPlanes, hullAdj, hullCount,
                             volume, threshold, pairs5, &d_cnt->nP5, d_st, use_bounds ? 0 : 1, bverts, bfaces, bR, bF, (double*)nullptr,
                             sp4 ? pairsX : (int2*)nullptr, &d_cnt->nX4, (small4 ? (unsigned int)ws4s : 0u) | noReuse | (lean4 ? SD_LEAN_BIT : 0u));
          const bool defer4 = sp4 && !tail && deferFrom > 0 && rounds >= deferFrom && hDef + h.nP4 <= dfrCap;
          if (defer4)
            hipLaunchKernelGGL(k_defer3, dim3(h.nP4 < 16384u ? sd::div_up(h.nP4, 256) : 64), dim3(256), 0, s, pairsX, &d_cnt->nX4, dfr, dfrCount, dfrCap, pend, &d_st->overflow);
          else if (sp4)
            hipLaunchKernelGGL(k_stage4x<4>, dim3(h.nP4 < 256u ? h.nP4 : 256u), dim3(256), lds4x, s, pairsX, &d_cnt->nX4, 0u, d_dist, d_points, R, hullCap, hullPlanes, hullAdj,
                               hullCount, volume, threshold, pairs5, &d_cnt->nP5, d_st, (double*)nullptr, b3verts, b3faces, b3R, b3F);
          SD_LAUNCH_CHECK();
          if (stats) SD_CHECK(hipEventRecord(ev1, s));
          SD_CHECK(hipMemcpyAsync(&h, d_cnt, sizeof(Counters), hipMemcpyDeviceToHost, s));
          SD_CHECK(hipStreamSynchronize(s));
          if (defer4) hDef += h.nX4;
          if (stats) { float ms = 0; SD_CHECK(hipEventElapsedTime(&ms, ev0, ev1)); ns4 += ms * 1e6;
                       if (trace) printf("         stage4 pairs=%u hulls=%u %.3f ms -> stage5 pairs=%u\n", h.nP4, h.nHull, ms, h.nP5); }
        }
        if (h.nP4 > 0 && h.nP5 > 0) {
          const unsigned int b5 = h.nP5 < 16384u ? h.nP5 : 16384u;
          if (stats) SD_CHECK(hipEventRecord(ev0, s));
          hipLaunchKernelGGL(k_stage5, dim3(b5), dim3(256), lds5, s, pairs5, h.nP5, d_dist, d_points, d_verts, d_faces, R, F, bbox, volume,
                             threshold, sink, d_st, cmap, mesh_ok ? 0 : 1);
          SD_LAUNCH_CHECK();
          if (stats) { SD_CHECK(hipEventRecord(ev1, s)); SD_CHECK(hipEventSynchronize(ev1)); float ms = 0; SD_CHECK(hipEventElapsedTime(&ms, ev0, ev1)); ns5 += ms * 1e6; }
        }
      }
    }
    if (tail) {
      unsigned int nEdges = 0;
      SD_CHECK(hipMemcpyAsync(&nEdges, supCount, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
      SD_CHECK(hipStreamSynchronize(s));
      if (nEdges > pairCap) { sd::set_error("sd_nms3d: tail edge list overflow (internal error)"); return -1; }
      if (trace) printf("tail batch after round %d: %d undecided candidates, %u suppressing edges, %u pairs carried over from the rounds%s\n", rounds - 1, nU, nEdges, hDef,
                        forceTail ? " (started early: every remaining candidate waits for one of them)" : "");
      int left = 1, sweeps = 0;
      while (left) {
        for (int it = 0; it < 8; ++it) {
          SD_CHECK(hipMemsetAsync(d_left, 0, sizeof(int), s));
          if (nEdges) hipLaunchKernelGGL(k_tail3_mark, dim3(sd::div_up(nEdges, 256)), dim3(256), 0, s, supEdges, nEdges, state, blocked);
          hipLaunchKernelGGL(k_tail3_promote, dim3(sd::div_up(nU, 256)), dim3(256), 0, s, Ucur, nU, state, blocked, d_left);
        }
        SD_LAUNCH_CHECK();
        SD_CHECK(hipMemcpyAsync(&left, d_left, sizeof(int), hipMemcpyDeviceToHost, s));
        SD_CHECK(hipStreamSynchronize(s));
        if (++sweeps > N / 8 + 4) { sd::set_error("sd_nms3d: tail replay does not converge (internal error)"); return -1; }
      }
      nU = 0;
      break;
    }
    nU = nUndecided;
    int* t = Ucur; Ucur = Unext; Unext = t;
  }
  hipLaunchKernelGGL(k_keep, dim3(sd::div_up(N, 256)), dim3(256), 0, s, state, d_keep, N);
  SD_LAUNCH_CHECK();
  Stats hs_;
  SD_CHECK(hipMemcpyAsync(&hs_, d_st, sizeof(Stats), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipStreamSynchronize(s));
  if (hs_.overflow) { sd::set_error("sd_nms3d: half-space intersection capacity exceeded (%llu pairs)", hs_.overflow); return -1; }
  if (stats) {
    stats[0] = (int64_t)hs_.upper; stats[1] = (int64_t)hs_.lower; stats[2] = (int64_t)hs_.kernel; stats[3] = (int64_t)hs_.render;
    stats[4] = rounds; stats[5] = totalNbr; stats[6] = (int64_t)hs_.sup_kernel; stats[7] = (int64_t)hs_.sup_render;
    stats[8] = (int64_t)ns3; stats[9] = (int64_t)ns4; stats[10] = (int64_t)ns5; stats[11] = (int64_t)hs_.convex; stats[12] = (int64_t)hs_.kept_convex;
    stats[13] = (int64_t)hs_.near_thr; stats[14] = (int64_t)hs_.hiv_fallback;
    { float msb = 0; SD_CHECK(hipEventElapsedTime(&msb, evb0, evb1)); stats[15] = (int64_t)(msb * 1e6); }
    if (trace) printf("hiv: faces %llu list entries %llu clips %llu list overflows %llu fallbacks %llu\n", hs_.hiv_faces, hs_.hiv_list, hs_.hiv_clips, hs_.hiv_rest, hs_.hiv_fallback);
    if (trace && hs_.cyc[5]) printf("stage 3 wave cycles per pair (clock64): load+half-spaces %.0f, cull %.0f, bounds %.0f, decide/exact %.0f, total %.0f (%llu pairs)\n",
                                    (double)hs_.cyc[0] / hs_.cyc[5], (double)hs_.cyc[1] / hs_.cyc[5], (double)hs_.cyc[2] / hs_.cyc[5], (double)hs_.cyc[3] / hs_.cyc[5],
                                    (double)hs_.cyc[4] / hs_.cyc[5], hs_.cyc[5]);
    if (trace) printf("hiv: pairs decided by the lower bound %llu, by the upper bound %llu, of %llu\n", hs_.lb_decided, hs_.ub_decided, hs_.kernel + hs_.convex);
  }
  if (verbose) {
    printf("NMS: Function calls:\nNMS: ~ bbox+out: %8llu\nNMS: ~ inner:    %8llu\nNMS: ~ kernel:   %8llu\nNMS: ~ convex:   %8llu\nNMS: ~ render:   %8llu\n",
           hs_.upper, hs_.lower, hs_.kernel, hs_.convex, hs_.render);
    printf("NMS: Excluded intersection:\nNMS: + pretest:  %8llu\nNMS: + convex:   %8llu\n", hs_.kept_pre, hs_.kept_convex);
    printf("NMS: Suppressed polyhedra:\nNMS: # inner:    %8llu / %d\nNMS: # kernel:   %8llu / %d\nNMS: # render:   %8llu / %d\n", hs_.sup_pre, N,
           hs_.sup_kernel, N, hs_.sup_render, N);
    printf("NMS: greedy rounds: %d, neighbour entries: %lld\n", rounds, (long long)totalNbr);
    fflush(stdout);
  }
  if (trace) fflush(stdout);
  return 0;
}

extern "C" void _LIB_non_maximum_suppression_sparse(const float* scores, const float* dist, const float* points, const int n_polys,
                                                    const int n_rays, const int n_faces, const float* verts, const int* faces,
                                                    const float threshold, const int use_bbox, const int use_kdtree, const int verbose,
                                                    bool* result) {
  if (n_polys <= 0) return;
  float *d_dist = nullptr, *d_pts = nullptr, *d_verts = nullptr, *d_scores = nullptr;
  int* d_faces = nullptr;
  uint8_t* d_keep = nullptr;
  bool ok = hipMalloc(&d_dist, (size_t)n_polys * n_rays * 4) == hipSuccess && hipMalloc(&d_pts, (size_t)n_polys * 12) == hipSuccess &&
            hipMalloc(&d_verts, (size_t)n_rays * 12) == hipSuccess && hipMalloc(&d_faces, (size_t)n_faces * 12) == hipSuccess &&
            hipMalloc(&d_scores, (size_t)n_polys * 4) == hipSuccess && hipMalloc(&d_keep, n_polys) == hipSuccess;
  if (ok) {
    ok = hipMemcpy(d_dist, dist, (size_t)n_polys * n_rays * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_pts, points, (size_t)n_polys * 12, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_verts, verts, (size_t)n_rays * 12, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_faces, faces, (size_t)n_faces * 12, hipMemcpyHostToDevice) == hipSuccess &&
         (scores == nullptr || hipMemcpy(d_scores, scores, (size_t)n_polys * 4, hipMemcpyHostToDevice) == hipSuccess);
    if (!ok) sd::set_error("_LIB_non_maximum_suppression_sparse: H2D failed");
  } else sd::set_error("_LIB_non_maximum_suppression_sparse: hipMalloc failed");
  std::vector<uint8_t> keep(n_polys);
  if (ok) ok = sd_nms3d_device(d_scores, d_dist, d_pts, n_polys, n_rays, n_faces, d_verts, d_faces, threshold, use_bbox, use_kdtree, verbose,
                               d_keep, nullptr, nullptr) == 0;
  if (ok) ok = hipMemcpy(keep.data(), d_keep, n_polys, hipMemcpyDeviceToHost) == hipSuccess;
  (void)hipFree(d_dist); (void)hipFree(d_pts); (void)hipFree(d_verts); (void)hipFree(d_faces); (void)hipFree(d_scores); (void)hipFree(d_keep);
  if (!ok) {   // the reference ABI has no return code: fail loudly
    fprintf(stderr, "_LIB_non_maximum_suppression_sparse failed: %s\n", sd::err_buf());
    abort();
  }
  for (int i = 0; i < n_polys; ++i) result[i] = keep[i] != 0;
}
