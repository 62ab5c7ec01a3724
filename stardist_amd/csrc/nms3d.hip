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
//
// This file: the broad phase, the stage kernels, the driver and the C entry points.  Around it: nms3d_lds.h (the LDS layout of every
// kernel), nms3d_hiv.h (half-space-intersection volumes and volume bounds), nms3d_hull.h (convex hulls), nms3d_mesh.h (ray-mesh
// adjacency, validity, refinement), nms_rounds.h (round scheduler and neighbour lists, shared with the 2D NMS), nms3d_shared.h (what
// raster3d.hip uses of this file).
#include <algorithm>

#include "common.h"
#include "geom3d.h"
#include "nms_rounds.h"
#include "nms3d_shared.h"
#include "nms3d_lds.h"
#include "nms3d_hiv.h"
#include "nms3d_mesh.h"
#include "nms3d_hull.h"
#include "../../include/stardist_hip.h"
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <vector>

namespace {

typedef long long i64;

// ------------------------------------------------------------------ P1 / P2
// The per-candidate kernels walk a candidate's R distances in face order (gathers).  A workgroup's rows are contiguous in memory: they are
// read once, coalesced, into LDS (sdl::RowsLds, row pitch R + 1: the lanes of a wave, one row each, hit distinct banks) -- one pass over the 4 R bytes
// of every candidate instead of line-by-line re-fetches of 128 interleaved rows (FETCH_SIZE was 12x the rows' size).
__device__ __forceinline__ const float* stage_rows(const float* __restrict__ dist, int N, int R, float* lds, int staged) {
  if (!staged) return dist + (size_t)min((int)(blockIdx.x * blockDim.x + threadIdx.x), N - 1) * R;     // several hundred rays: rows stay in memory
  const int i0 = blockIdx.x * blockDim.x;
  const int rows = min((int)blockDim.x, N - i0);
  const float* src = dist + (size_t)i0 * R;
  const int pitch = sdl::RowsLds{R}.pitch();
  for (int e = threadIdx.x; e < rows * R; e += blockDim.x) { const int r = e / R; lds[r * pitch + (e - r * R)] = src[e]; }
  __syncthreads();
  return lds + threadIdx.x * pitch;
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

// ------------------------------------------------------------------ stages 3 and 4: intersection volume of a pair
// Stage 3 intersects the two kernels, stage 4 the two convex hulls.  Half-spaces h = (n, d): inside <=> n.p + d <= 0
// (build_halfspace :744-764, interleaved poly1/poly2 per face as qhull_overlap_kernel :840-853 does; the hulls' planes one polyhedron
// after the other).  Qhull's feasibility rule (qh_sethalfspace): the interior point must satisfy offset + n.c <= 0 for every
// half-space (evaluated in that order in fp64), otherwise the reference gets a QhullError and uses err_value (0 / 1e10).
// Each stage has a kernel of one wave per pair (k_stage3, k_stage4: cull, volume bounds, then the exact volume or the queue of the
// second kernel) and one of NW waves per pair (k_stage3x, k_stage4x: the exact volumes of the pairs the bounds left undecided).  They
// differ in where the half-spaces come from, in how the interior point is rounded and in what becomes of the volume; the rest is the
// routines below, templated on the thread stride NT (64: one wave; 64 NW: the workgroup, barriers inside).  LDS: sdl::PairLds.

// adjacency seeds of the kernel form: half-space 2f + w belongs to face f of polyhedron w, its neighbours across the face's edges likewise
template <int NT>
__device__ __forceinline__ void kernel_seeds(unsigned short* seed, const int* __restrict__ faceAdj, int F, int tid) {
  for (int idx = tid; idx < 6 * F; idx += NT) {
    const int o_ = idx / 3, e_ = idx - 3 * o_;
    const int a_ = faceAdj[3 * (o_ >> 1) + e_];
    seed[idx] = (unsigned short)(a_ < 0 ? HIV_NONE : (unsigned int)(2 * a_ + (o_ & 1)));
  }
}
// the half-spaces of the two kernels of pair ij; pv: vertex staging of 6 R floats (dead afterwards)
template <int NT>
__device__ __forceinline__ void kernel_halfspaces(double* hs, float* pv1, int2 ij, const float* c1, const float* c2, const float* __restrict__ dist,
                                                  const float* __restrict__ verts, const int* __restrict__ faces, int R, int F, int tid) {
  float* pv2 = pv1 + 3 * R;
  __syncthreads();
  for (int k = tid; k < R; k += NT) {
    const float d1 = dist[(size_t)ij.x * R + k], d2 = dist[(size_t)ij.y * R + k];
    pv1[3 * k] = c1[0] + d1 * verts[3 * k]; pv1[3 * k + 1] = c1[1] + d1 * verts[3 * k + 1]; pv1[3 * k + 2] = c1[2] + d1 * verts[3 * k + 2];
    pv2[3 * k] = c2[0] + d2 * verts[3 * k]; pv2[3 * k + 1] = c2[1] + d2 * verts[3 * k + 1]; pv2[3 * k + 2] = c2[2] + d2 * verts[3 * k + 2];
  }
  __syncthreads();
  for (int f = tid; f < F; f += NT) {
    const int iA = faces[3 * f], iB = faces[3 * f + 1], iC = faces[3 * f + 2];
    sd3::build_halfspace(&pv1[3 * iA], &pv1[3 * iB], &pv1[3 * iC], &hs[4 * (2 * f)]);
    sd3::build_halfspace(&pv2[3 * iA], &pv2[3 * iB], &pv2[3 * iC], &hs[4 * (2 * f + 1)]);
  }
  __syncthreads();
}
// the cached hull planes of pair ij (n1, then n2 of them) and, with seed != nullptr, their facet adjacency; failed: a hull is missing
template <int NT>
__device__ __forceinline__ void hull_halfspaces(double* hs, unsigned short* seed, int2 ij, int cap, const double* __restrict__ hullPlanes,
                                                const unsigned short* __restrict__ hullAdj, int n1, int n2, bool failed, int tid) {
  __syncthreads();
  if (!failed) {
    const double* h1 = hullPlanes + (size_t)ij.x * cap * 4;
    const double* h2 = hullPlanes + (size_t)ij.y * cap * 4;
    for (int k = tid; k < 4 * n1; k += NT) hs[k] = h1[k];
    for (int k = tid; k < 4 * n2; k += NT) hs[4 * n1 + k] = h2[k];
    if (seed) {
      const unsigned short* a1 = hullAdj + (size_t)ij.x * cap * 3;
      const unsigned short* a2 = hullAdj + (size_t)ij.y * cap * 3;
      for (int k = tid; k < 3 * n1; k += NT) seed[k] = a1[k];
      for (int k = tid; k < 3 * n2; k += NT) { const unsigned int t = a2[k]; seed[3 * n1 + k] = (unsigned short)(t == HIV_NONE ? HIV_NONE : t + n1); }
    }
  }
  __syncthreads();
}
// Qhull's feasibility rule for the interior point c
template <int NT>
__device__ __forceinline__ bool interior_infeasible(const double* hs, int M, const double c[3], int tid) {
  bool bad = false;
  for (int k = tid; k < M; k += NT) {
    double dd = hs[4 * k + 3];
    dd += hs[4 * k] * c[0]; dd += hs[4 * k + 1] * c[1]; dd += hs[4 * k + 2] * c[2];
    if (dd > 0 || !(dd < 0)) bad = true;     // dist > 0 -> error; dist == 0 -> division by zero -> error
  }
  if constexpr (NT == 64) return __any(bad);
  else return __syncthreads_or(bad ? 1 : 0) != 0;
}
// largest distance of each polyhedron of the pair (every wave computes the same values)
struct PairExt { double ext1, ext2; };
__device__ __forceinline__ PairExt pair_extents(const float* __restrict__ dist, int2 ij, int R, int lane) {
  double ext1 = 0, ext2 = 0;
  for (int k = lane; k < R; k += 64) {
    const float e1 = dist[(size_t)ij.x * R + k], e2 = dist[(size_t)ij.y * R + k];
    ext1 = fmax(ext1, (double)e1); ext2 = fmax(ext2, (double)e2);
  }
  for (int o = 32; o; o >>= 1) { ext1 = fmax(ext1, __shfl_xor(ext1, o)); ext2 = fmax(ext2, __shfl_xor(ext2, o)); }
  return PairExt{ext1, ext2};
}
// Cull (hiv_cull_wave) against the outer balls of the two polyhedra: centre, largest distance with a 1e-6 safety margin
template <class Second, bool BS>
__device__ __forceinline__ int pair_cull(double* hs, int M, const float* c1, const float* c2, const PairExt& e, const double c[3], const HivLds& W, int lane, Second second) {
  const double b1[4] = {(double)c1[0], (double)c1[1], (double)c1[2], e.ext1 * (1.0 + 1e-6) + 1e-6};
  const double b2[4] = {(double)c2[0], (double)c2[1], (double)c2[2], e.ext2 * (1.0 + 1e-6) + 1e-6};
  return hiv_cull_wave<Second, BS>(hs, M, b1, b2, c, W.pos, W.orig, lane, second);
}
// for the exact volume: the balls relative to the interior point c, and the half-width L of the box every face polygon starts from
__device__ __forceinline__ double pair_box(const float* c1, const float* c2, const double c[3], const PairExt& e, double balls[8]) {
  const double sep = sqrt((double)(c1[0] - c2[0]) * (c1[0] - c2[0]) + (double)(c1[1] - c2[1]) * (c1[1] - c2[1]) + (double)(c1[2] - c2[2]) * (c1[2] - c2[2]));
  balls[0] = (double)c1[0] - c[0]; balls[1] = (double)c1[1] - c[1]; balls[2] = (double)c1[2] - c[2]; balls[3] = e.ext1 * (1.0 + 1e-6) + 1e-6;
  balls[4] = (double)c2[0] - c[0]; balls[5] = (double)c2[1] - c[1]; balls[6] = (double)c2[2] - c[2]; balls[7] = e.ext2 * (1.0 + 1e-6) + 1e-6;
  return 4.0 * (2.0 * fmax(e.ext1, e.ext2) + sep + 1.0);
}
// Is a bound on the intersection volume on one side of the threshold for certain?  Then the exact volume would give the same decision.
struct BoundsTest {
  double A_min_d, thr_hi, thr_lo;
  __device__ __forceinline__ BoundsTest(const float* __restrict__ volume, int2 ij, float thr)
      : A_min_d((double)fminf(volume[ij.x], volume[ij.y]) + 1e-10), thr_hi((double)thr + 1e-5 * fabs((double)thr) + 1e-7),
        thr_lo((double)thr - 1e-5 * fabs((double)thr) - 1e-7) {}
  __device__ __forceinline__ bool above(double lb) const { return lb * (1.0 - 1e-9) / A_min_d > thr_hi; }
  __device__ __forceinline__ bool below(double ub) const { return ub * (1.0 + 1e-9) / A_min_d < thr_lo; }
};
// vol = the bound that settles the pair (counted by the thread `first`); false: neither does
__device__ __forceinline__ bool bounds_decide(const BoundsTest& bt, double lb, double ub, double& vol, Stats* st, bool first) {
  if (bt.above(lb)) { vol = lb; if (first) atomicAdd(&st->lb_decided, 1ull); return true; }      // certainly above the threshold
  if (bt.below(ub)) { vol = ub; if (first) atomicAdd(&st->ub_decided, 1ull); return true; }      // certainly not above the threshold
  return false;
}

// One wave, the feasible pair's M half-spaces in hs: cull, bounds over the ray mesh and -- where they leave the decision open -- over
// the refined mesh (4x the cost), then the exact volume, or with pairsX the queue of the NW-wave kernel (returns false: no volume).
// clk (stage 3 with flags.prof): the clock after the cull and after the bounds.
template <class Second>
__device__ __forceinline__ bool pair_volume_wave(double* hs, int M, const HivLds& W, const PairExt& fr, const float* c1, const float* c2, const double c[3],
                                                 Second second, const float* __restrict__ verts, const int* __restrict__ faces, int R, int F,
                                                 const float* __restrict__ bverts, const int* __restrict__ bfaces, int bR, int bF,
                                                 const float* __restrict__ volume, int2 ij, float thr, const sdl::PairFlags& flags,
                                                 int2* __restrict__ pairsX, unsigned int* __restrict__ nX, Stats* st, int lane, double& vol, long long* clk) {
  const int Mc = pair_cull<Second, true>(hs, M, c1, c2, fr, c, W, lane, second);
  if (clk && flags.prof) clk[0] = clock64();
  const BoundsTest bt(volume, ij, thr);
  double lb, ub;
  hiv_bounds_wave<2>(hs, Mc, verts, faces, R, F, W.S, (unsigned short*)(W.S + 3 * R), lane, lb, ub);
  if (bR != R && !bt.above(lb) && !bt.below(ub)) {
    const double lb0 = lb, ub0 = ub;
    if (flags.recast) hiv_bounds_wave<6>(hs, Mc, bverts, bfaces, bR, bF, W.S, (unsigned short*)(W.S + 3 * bR), lane, lb, ub);
    else hiv_bounds_wave<5>(hs, Mc, bverts, bfaces, bR, bF, W.S, (unsigned short*)(W.S + 3 * bR), lane, lb, ub, R, (const unsigned short*)(W.S + 3 * R));
    lb = fmax(lb, lb0); ub = fmin(ub, ub0);
  }
  if (clk && flags.prof) clk[1] = clock64();
  if (!flags.exact && bounds_decide(bt, lb, ub, vol, st, lane == 0)) return true;
  if (pairsX) { if (lane == 0) pairsX[atomicAdd(nX, 1u)] = ij; return false; }
  const double zero3[3] = {0, 0, 0};
  double balls[8];
  const double L = pair_box(c1, c2, c, fr, balls);
  vol = hiv_volume_wave(hs, Mc, zero3, L, W, lane, st, balls);
  return true;
}
// NW waves, the feasible pair's M half-spaces in hs: wave 0 culls; then (b3R != 0 and not the pair-level probe) one more pair of bounds
// over the direction mesh refined twice, evaluated by the whole workgroup in the idle workspaces of waves 1 .. NW - 1; then the exact
// volume with the faces spread over 64 NW lanes and the terms added in the one-wave order (hiv_volume_block: bit-identical volume).
// Returned in wave 0.
template <int NW, class Second>
__device__ __forceinline__ double pair_volume_block(char* smem, const sdl::PairLds& lds, const HivLds& W, int M, const float* __restrict__ dist, int2 ij,
                                                    int R, const float* c1, const float* c2, const double c[3], Second second,
                                                    const float* __restrict__ b3verts, const int* __restrict__ b3faces, int b3R, int b3F,
                                                    const float* __restrict__ volume, float thr, bool probe, Stats* st, int tid) {
  double* hs = (double*)(smem + lds.hs());
  double* terms = (double*)(smem + lds.terms());
  int* shared = (int*)(smem + lds.shared());              // [0] = half-spaces kept by the cull
  const int lane = tid & 63, wave = tid >> 6;
  const PairExt fr = pair_extents(dist, ij, R, lane);
  if (wave == 0) {
    const int kept = pair_cull<Second, false>(hs, M, c1, c2, fr, c, W, lane, second);
    if (lane == 0) shared[0] = kept;
  }
  __syncthreads();
  const int Mc = shared[0];
  const double zero3[3] = {0, 0, 0};
  double balls[8];
  const double L = pair_box(c1, c2, c, fr, balls);
  if (b3R > 0 && !probe) {
    const BoundsTest bt(volume, ij, thr);
    double* wv = (double*)(smem + lds.extra(1));
    double lb, ub, vol;
    hiv_bounds_block<NW, 6>(hs, Mc, b3verts, b3faces, b3R, b3F, wv, (unsigned short*)(wv + 3 * b3R), terms, tid, lb, ub);
    if (bounds_decide(bt, lb, ub, vol, st, tid == 0)) return vol;
  }
  return hiv_volume_block<NW>(hs, Mc, zero3, L, W, lane, wave, terms, st, balls);
}

struct OddIsSecond { __device__ bool operator()(int k) const { return (k & 1) != 0; } };          // half-space 2f + w: polyhedron w
struct FromIndex { int n1; __device__ bool operator()(int k) const { return k >= n1; } };        // the hulls' planes: n1 of polyhedron 1 first

// what becomes of a pair's kernel volume (:1261-1277): suppress, or on to the hull stage
__device__ __forceinline__ void stage3_result(double vol, int2 ij, const float* __restrict__ volume, float thr, const SuppSink& sink,
                                              int2* __restrict__ pairs5, unsigned int* pair5Count, Stats* st) {
  atomicAdd(&st->kernel, 1ull);
  if (vol != vol) atomicAdd(&st->overflow, 1ull);   // polygon capacity overflow (reported as an error by the host)
  const float A_inter_kernel = (float)vol;                                  // function returns float :679
  const float A_min = fminf(volume[ij.x], volume[ij.y]);
  const float iou = (float)((double)A_inter_kernel / ((double)A_min + 1e-10));   // :1269
  if (fabsf(iou - thr) < 1e-6f) atomicAdd(&st->near_thr, 1ull);      // (a flip by the <= 1e-9 volume deviation from Qhull would need |iou - thr| ~ 1e-9)
  if (iou > thr) { sink.suppress(ij.x, ij.y); atomicAdd(&st->sup_kernel, 1ull); }
  else pairs5[atomicAdd(pair5Count, 1u)] = ij;
}
// what becomes of a pair's hull volume (:1282-1295): keep, or on to the render stage
__device__ __forceinline__ void stage4_result(double vol, int2 ij, const float* __restrict__ volume, float thr, int2* __restrict__ pairs5,
                                              unsigned int* pair5Count, Stats* st) {
  atomicAdd(&st->convex, 1ull);
  if (vol != vol) atomicAdd(&st->overflow, 1ull);
  const float A_inter_convex = (float)vol;
  const float A_min = fminf(volume[ij.x], volume[ij.y]);
  const float iou = (float)((double)A_inter_convex / ((double)A_min + 1e-10));     // :1289
  if (fabsf(iou - thr) < 1e-6f) atomicAdd(&st->near_thr, 1ull);
  if (iou <= thr) atomicAdd(&st->kept_convex, 1ull);                                // :1291-1295
  else pairs5[atomicAdd(pair5Count, 1u)] = ij;
}

// ------------------------------------------------------------------ stage 3: kernel ∩ kernel volume (:830-869)
// pairsX != nullptr: a pair the bounds leave undecided is queued for k_stage3x instead of being integrated here.  A bounds-only launch
// can do with the small workspace (ray-cast vectors instead of polygons) and, lean, without the seed table: the adjacency seeds are only
// read by the exact routine, and the cull's pos / orig tables by nobody -- 21.9 instead of 25.6 KB per wave, seven waves per CU instead
// of six.  volOut != nullptr: pair-level probe (sd_hiv_pairs_device): the volume itself.
__global__ void __launch_bounds__(64) k_stage3(const int2* __restrict__ pairs, unsigned int nPairs, const float* __restrict__ dist,
                                               const float* __restrict__ pts, const float* __restrict__ verts,
                                               const int* __restrict__ faces, const int* __restrict__ faceAdj, int R,
                                               const float* __restrict__ volume, float thr, SuppSink sink,
                                               int2* __restrict__ pairs5, unsigned int* pair5Count, Stats* st, sdl::PairLds lds, sdl::PairFlags flags,
                                               const float* __restrict__ bverts, const int* __restrict__ bfaces, int bR, int bF,
                                               double* __restrict__ volOut = nullptr, int2* __restrict__ pairsX = nullptr,
                                               unsigned int* __restrict__ nX = nullptr) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* hs = (double*)(smem + lds.hs());
  const HivLds W = hiv_lds(smem, lds, 0);
  const int lane = threadIdx.x, F = (int)lds.n;
  if (!lds.lean) kernel_seeds<64>(W.seed, faceAdj, F, lane);
  for (unsigned int p = blockIdx.x; p < nPairs; p += gridDim.x) {
    const long long t0 = flags.prof ? clock64() : 0;
    long long t1 = 0, clk[2] = {0, 0};
    const int2 ij = pairs[p];
    const float* c1 = pts + 3 * (size_t)ij.x;
    const float* c2 = pts + 3 * (size_t)ij.y;
    kernel_halfspaces<64>(hs, (float*)(smem + lds.work()), ij, c1, c2, dist, verts, faces, R, F, lane);
    if (flags.prof) t1 = clock64();
    const int M = 2 * F;
    double c[3];
    c[0] = .5 * (c1[0] + c2[0]); c[1] = .5 * (c1[1] + c2[1]); c[2] = .5 * (c1[2] + c2[2]);   // :857-859 (float add, then *.5 in double)
    double vol = 0;                                                 // err_value :865
    bool done = true;
    if (!interior_infeasible<64>(hs, M, c, lane)) {
      const PairExt fr = pair_extents(dist, ij, R, lane);
      __syncthreads();
      done = pair_volume_wave(hs, M, W, fr, c1, c2, c, OddIsSecond(), verts, faces, R, F, bverts, bfaces, bR, bF, volume, ij, thr, flags, pairsX, nX, st,
                              lane, vol, clk);
    }
    if (flags.prof && lane == 0 && clk[1]) {
      const long long t4 = clock64();
      atomicAdd(&st->cyc[0], (unsigned long long)(t1 - t0)); atomicAdd(&st->cyc[1], (unsigned long long)(clk[0] - t1));
      atomicAdd(&st->cyc[2], (unsigned long long)(clk[1] - clk[0])); atomicAdd(&st->cyc[3], (unsigned long long)(t4 - clk[1]));
      atomicAdd(&st->cyc[4], (unsigned long long)(t4 - t0)); atomicAdd(&st->cyc[5], 1ull);
    }
    if (!done) continue;
    if (lane == 0) {
      if (volOut) volOut[p] = vol;
      else stage3_result(vol, ij, volume, thr, sink, pairs5, pair5Count, st);
    }
  }
}

// Exact kernel ∩ kernel volume of the pairs the bounds left undecided (queued by k_stage3), NW waves per pair.  An exact volume is
// ~2 M wave cycles (one lane per face: six passes over the 2F half-spaces), ~1 ms: with one wave per pair every launch of a round
// lasted at least that long, however few pairs it held.  Here the faces of a pair are spread over 64 NW lanes (the culled
// half-spaces usually fit one pass).  b3R != 0: direction mesh (refined twice) of one more pair of volume bounds.
template <int NW>
__global__ void __launch_bounds__(64 * NW) k_stage3x(const int2* __restrict__ pairs, const unsigned int* __restrict__ nPairsPtr, unsigned int nPairsImm,
                                                     const float* __restrict__ dist, const float* __restrict__ pts, const float* __restrict__ verts,
                                                     const int* __restrict__ faces, const int* __restrict__ faceAdj, int R,
                                                     const float* __restrict__ volume, float thr, SuppSink sink, int2* __restrict__ pairs5,
                                                     unsigned int* pair5Count, Stats* st, sdl::PairLds lds, double* __restrict__ volOut,
                                                     const float* __restrict__ b3verts = nullptr, const int* __restrict__ b3faces = nullptr,
                                                     int b3R = 0, int b3F = 0) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* hs = (double*)(smem + lds.hs());
  const int tid = threadIdx.x, F = (int)lds.n;
  const HivLds W = hiv_lds(smem, lds, tid >> 6);
  kernel_seeds<64 * NW>(W.seed, faceAdj, F, tid);
  const unsigned int nPairs = nPairsPtr ? *nPairsPtr : nPairsImm;
  for (unsigned int p = blockIdx.x; p < nPairs; p += gridDim.x) {
    const int2 ij = pairs[p];
    const float* c1 = pts + 3 * (size_t)ij.x;
    const float* c2 = pts + 3 * (size_t)ij.y;
    kernel_halfspaces<64 * NW>(hs, (float*)(smem + lds.work()), ij, c1, c2, dist, verts, faces, R, F, tid);
    const int M = 2 * F;
    double c[3];
    c[0] = .5 * (c1[0] + c2[0]); c[1] = .5 * (c1[1] + c2[1]); c[2] = .5 * (c1[2] + c2[2]);   // :857-859 (float add, then *.5 in double)
    double vol = 0;
    if (!interior_infeasible<64 * NW>(hs, M, c, tid))
      vol = pair_volume_block<NW>(smem, lds, W, M, dist, ij, R, c1, c2, c, OddIsSecond(), b3verts, b3faces, b3R, b3F, volume, thr, volOut != nullptr, st, tid);
    if (tid == 0) {
      if (volOut) volOut[p] = vol;
      else stage3_result(vol, ij, volume, thr, sink, pairs5, pair5Count, st);
    }
  }
}

// ------------------------------------------------------------------ stage 4: hull ∩ hull volume (:872-939)
// The hulls (nms3d_hull.h) are computed ONCE per candidate that reaches this stage and cached in HBM.
// hullState: 0 = not requested, 1 = requested/computed
__global__ void k_hull_mark(const int2* __restrict__ pairs, unsigned int nPairs, int* __restrict__ hullState, int* __restrict__ hullList,
                            unsigned int* hullListCount) {
  const unsigned int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nPairs) return;
  const int2 ij = pairs[p];
  if (atomicExch(&hullState[ij.x], 1) == 0) hullList[atomicAdd(hullListCount, 1u)] = ij.x;
  if (atomicExch(&hullState[ij.y], 1) == 0) hullList[atomicAdd(hullListCount, 1u)] = ij.y;
}

// pairsX, the bounds-only forms of the LDS and volOut as in k_stage3 (the smaller footprint lets six waves share a CU instead of four)
__global__ void __launch_bounds__(64) k_stage4(const int2* __restrict__ pairs, unsigned int nPairs, const float* __restrict__ dist,
                                               const float* __restrict__ pts, const float* __restrict__ verts,
                                               const int* __restrict__ faces, int R, int F, const double* __restrict__ hullPlanes,
                                               const unsigned short* __restrict__ hullAdj, const int* __restrict__ hullCount,
                                               const float* __restrict__ volume, float thr,
                                               int2* __restrict__ pairs5, unsigned int* pair5Count, Stats* st, sdl::PairLds lds, sdl::PairFlags flags,
                                               const float* __restrict__ bverts, const int* __restrict__ bfaces, int bR, int bF,
                                               double* __restrict__ volOut = nullptr, int2* __restrict__ pairsX = nullptr,
                                               unsigned int* __restrict__ nX = nullptr) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* hs = (double*)(smem + lds.hs());
  const HivLds W = hiv_lds(smem, lds, 0);
  const int lane = threadIdx.x, cap = (int)lds.n;
  for (unsigned int p = blockIdx.x; p < nPairs; p += gridDim.x) {
    const int2 ij = pairs[p];
    const float* c1 = pts + 3 * (size_t)ij.x;
    const float* c2 = pts + 3 * (size_t)ij.y;
    const int n1 = hullCount[ij.x], n2 = hullCount[ij.y];
    const bool failed = (n1 < 4 || n2 < 4);
    const int M = failed ? 0 : n1 + n2;
    hull_halfspaces<64>(hs, lds.lean ? nullptr : W.seed, ij, cap, hullPlanes, hullAdj, n1, n2, failed, lane);
    double c[3];
    c[0] = .5 * ((double)c1[0] + (double)c2[0]); c[1] = .5 * ((double)c1[1] + (double)c2[1]); c[2] = .5 * ((double)c1[2] + (double)c2[2]);   // :919-921
    double vol = 1.e10;                                             // err_value :927
    bool done = true;
    if (!(interior_infeasible<64>(hs, M, c, lane) || failed)) {
      // (the cull drops the half-spaces of one hull that contain the other polyhedron's outer ball, which contains its hull)
      const PairExt fr = pair_extents(dist, ij, R, lane);
      done = pair_volume_wave(hs, M, W, fr, c1, c2, c, FromIndex{n1}, verts, faces, R, F, bverts, bfaces, bR, bF, volume, ij, thr, flags, pairsX, nX, st,
                              lane, vol, (long long*)nullptr);
    }
    if (!done) continue;
    if (lane == 0) {
      if (volOut) volOut[p] = vol;
      else stage4_result(vol, ij, volume, thr, pairs5, pair5Count, st);
    }
  }
}

// Exact hull ∩ hull volume of the pairs k_stage4 queued, NW waves per pair (see k_stage3x).
template <int NW>
__global__ void __launch_bounds__(64 * NW) k_stage4x(const int2* __restrict__ pairs, const unsigned int* __restrict__ nPairsPtr, unsigned int nPairsImm,
                                                     const float* __restrict__ dist, const float* __restrict__ pts, int R,
                                                     const double* __restrict__ hullPlanes, const unsigned short* __restrict__ hullAdj,
                                                     const int* __restrict__ hullCount, const float* __restrict__ volume, float thr,
                                                     int2* __restrict__ pairs5, unsigned int* pair5Count, Stats* st, sdl::PairLds lds, double* __restrict__ volOut,
                                                     const float* __restrict__ b3verts = nullptr, const int* __restrict__ b3faces = nullptr,
                                                     int b3R = 0, int b3F = 0) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* hs = (double*)(smem + lds.hs());
  const int tid = threadIdx.x, cap = (int)lds.n;
  const HivLds W = hiv_lds(smem, lds, tid >> 6);
  const unsigned int nPairs = nPairsPtr ? *nPairsPtr : nPairsImm;
  for (unsigned int p = blockIdx.x; p < nPairs; p += gridDim.x) {
    const int2 ij = pairs[p];
    const float* c1 = pts + 3 * (size_t)ij.x;
    const float* c2 = pts + 3 * (size_t)ij.y;
    const int n1 = hullCount[ij.x], n2 = hullCount[ij.y];
    const bool failed = (n1 < 4 || n2 < 4);
    const int M = failed ? 0 : n1 + n2;
    hull_halfspaces<64 * NW>(hs, W.seed, ij, cap, hullPlanes, hullAdj, n1, n2, failed, tid);
    double c[3];
    c[0] = .5 * ((double)c1[0] + (double)c2[0]); c[1] = .5 * ((double)c1[1] + (double)c2[1]); c[2] = .5 * ((double)c1[2] + (double)c2[2]);   // :919-921
    double vol = 1.e10;                                             // err_value :927
    if (!(interior_infeasible<64 * NW>(hs, M, c, tid) || failed))
      vol = pair_volume_block<NW>(smem, lds, W, M, dist, ij, R, c1, c2, c, FromIndex{n1}, b3verts, b3faces, b3R, b3F, volume, thr, volOut != nullptr, st, tid);
    if (tid == 0) {
      if (volOut) volOut[p] = vol;
      else stage4_result(vol, ij, volume, thr, pairs5, pair5Count, st);
    }
  }
}

// ------------------------------------------------------------------ stage 5: voxel rendering (:587-636, 1305-1330)
__global__ void __launch_bounds__(256) k_stage5(const int2* __restrict__ pairs, unsigned int nPairs, const float* __restrict__ dist,
                                                const float* __restrict__ pts, const float* __restrict__ verts,
                                                const int* __restrict__ faces, int R, int F, const int* __restrict__ bbox,
                                                const float* __restrict__ volume, float thr, SuppSink sink, Stats* st,
                                                sd3::ConeMap cm, int whole_box) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const sdl::RenderLds lds{R, F};
  float* pv1 = (float*)(smem + lds.pv1());     // 3R
  float* pv2 = (float*)(smem + lds.pv2());     // 3R
  int* fc = (int*)(smem + lds.faces());        // 3F
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

// more than 64 KiB of dynamic LDS needs an explicit opt-in (only reached with several hundred rays)
template <class Kernel>
int lds_optin(Kernel kernel, size_t bytes) {
  if (sdl::needs_optin(bytes)) SD_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return 0;
}
// the LDS layouts of a call with R rays and F faces; fails when a stage does not fit.  The four-wave kernels are optional
// (Nms3dLds::split3 / split4): option nms3d_split_exact and room for the four workspaces
int plan_lds(const char* who, int R, int F, sdl::Nms3dLds* out) {
  const sdl::Nms3dLds P = sdl::nms3d_lds(R, F);
  if (!P.ok()) { sd::set_error("%s: n_rays/n_faces too large for LDS staging", who); return -1; }
  if (lds_optin(k_stage3, P.s3.bytes()) || lds_optin(k_stage4, P.s4.bytes()) || lds_optin(k_stage5, P.render.bytes())) return -1;
  if (sd::option(sd::OPT_NMS3D_SPLIT_EXACT)) {
    if (P.split3() && lds_optin(k_stage3x<4>, P.s3x.bytes())) return -1;
    if (P.split4() && lds_optin(k_stage4x<4>, P.s4x.bytes())) return -1;
  }
  if (lds_optin(k_hull, P.hull.bytes())) return -1;
  *out = P;
  return 0;
}

int cone_map_build(const float* d_verts, const int* d_faces, int F, sd3::ConeMap* out, hipStream_t s) {
  sd::Arena& A = sd::arena();
  unsigned short* cmList = A.take_n<unsigned short>((size_t)SD_CM_CELLS * SD_CM_CAP);
  signed char* cmCount = A.take_n<signed char>(SD_CM_CELLS);
  if (!cmList || !cmCount) return -1;
  hipLaunchKernelGGL(k_cone_map, dim3(sd::div_up(SD_CM_CELLS, 64)), dim3(64), 0, s, d_verts, d_faces, F, cmList, cmCount);
  SD_LAUNCH_CHECK();
  out->list = cmList; out->count = cmCount;
  return 0;
}

}  // namespace

namespace sd {
int hull_planes(const float* d_dist, const float* d_points, const float* d_verts, int n, int R, HullPlanes* out, hipStream_t s) {
  if (R < 4 || R > 800) { sd::set_error("hull_planes: n_rays=%d unsupported (4..800)", R); return -1; }
  const sdl::HullLds lds{R, 2 * R};
  if (!sdl::fits(lds.bytes())) { sd::set_error("hull_planes: n_rays too large for LDS staging"); return -1; }
  if (lds_optin(k_hull, lds.bytes())) return -1;
  sd::Arena& A = sd::arena();
  HullPlanes H;
  H.cap = lds.cap;
  H.planes = A.take_n<double>((size_t)n * H.cap * 4);
  H.adj = A.take_n<unsigned short>((size_t)n * H.cap * 3);
  H.count = A.take_n<int>(n);
  int* list = A.take_n<int>(n);
  if (!H.planes || !H.adj || !H.count || !list) return -1;
  hipLaunchKernelGGL(k_iota, dim3(sd::div_up(n, 256)), dim3(256), 0, s, list, n);
  const unsigned int bh = n < 32768 ? (unsigned int)n : 32768u;
  hipLaunchKernelGGL(k_hull, dim3(bh), dim3(64), lds.bytes(), s, list, (unsigned int)n, d_dist, d_points, d_verts, R, H.cap, H.planes, H.adj, H.count);
  SD_LAUNCH_CHECK();
  *out = H;
  return 0;
}

int cone_map(const float* d_verts, const int* d_faces, int F, sd3::ConeMap* out, hipStream_t s, SideJoin* fork) {
  out->list = nullptr; out->count = nullptr;
  if (F > 65535 || sd::option(sd::OPT_NMS3D_CONE_MAP) == 0) return 0;
  hipStream_t side = fork ? sd::side_stream() : nullptr;          // (nullptr: everything stays on the caller's stream)
  if (side && fork->begin(s, side)) return -1;
  if (cone_map_build(d_verts, d_faces, F, out, side ? side : s)) return -1;
  return side ? fork->end(side) : 0;
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
  sdl::Nms3dLds lds;
  if (plan_lds("sd_hiv_pairs", R, F, &lds)) return -1;
  const bool split = sd::option(sd::OPT_NMS3D_SPLIT_EXACT) != 0;      // the routine the cascade uses: four waves per pair
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
  const unsigned int nb = (unsigned int)n_pairs < 16384u ? (unsigned int)n_pairs : 16384u, nbx = (unsigned int)n_pairs < 1024u ? (unsigned int)n_pairs : 1024u;
  const sdl::PairFlags exact{0, 0, 1};
  if (d_vol_kernel && split && lds.split3()) {
    hipLaunchKernelGGL(k_stage3x<4>, dim3(nbx), dim3(256), lds.s3x.bytes(), s, pairs, (const unsigned int*)nullptr,
                       (unsigned int)n_pairs, d_dist, d_points, d_verts, d_faces, faceAdj, R, volume, 0.f, SuppSink{state, nullptr, nullptr, 0u}, (int2*)nullptr,
                       dummyCount, d_st, lds.s3x, d_vol_kernel);
    SD_LAUNCH_CHECK();
  } else if (d_vol_kernel) {
    hipLaunchKernelGGL(k_stage3, dim3(nb), dim3(64), lds.s3.bytes(), s, pairs, (unsigned int)n_pairs, d_dist, d_points, d_verts, d_faces, faceAdj, R, volume,
                       0.f, SuppSink{state, nullptr, nullptr, 0u}, (int2*)nullptr, dummyCount, d_st, lds.s3, exact, d_verts, d_faces, R, F, d_vol_kernel);
    SD_LAUNCH_CHECK();
  }
  if (d_vol_hull) {
    sd::HullPlanes H;
    if (sd::hull_planes(d_dist, d_points, d_verts, N, R, &H, s)) return -1;
    if (split && lds.split4())
      hipLaunchKernelGGL(k_stage4x<4>, dim3(nbx), dim3(256), lds.s4x.bytes(), s, pairs, (const unsigned int*)nullptr,
                         (unsigned int)n_pairs, d_dist, d_points, R, H.planes, H.adj, H.count, volume, 0.f, (int2*)nullptr, dummyCount, d_st, lds.s4x, d_vol_hull);
    else
      hipLaunchKernelGGL(k_stage4, dim3(nb), dim3(64), lds.s4.bytes(), s, pairs, (unsigned int)n_pairs, d_dist, d_points, d_verts, d_faces, R, F, H.planes,
                         H.adj, H.count, volume, 0.f, (int2*)nullptr, dummyCount, d_st, lds.s4, exact, d_verts, d_faces, R, F, d_vol_hull);
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
  if (use_cone_map && cone_map_build(d_verts, d_faces, n_faces, &cm, s)) return -1;
  long long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_inside_probe, dim3((unsigned int)blocks), dim3(256), (size_t)3 * n_rays * sizeof(float), s, d_dist, d_centre, n_rays, n_faces, d_verts,
                     d_faces, d_points, n, cm, d_out);
  SD_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ the driver
namespace {

struct Mesh { const float* verts; const int* faces; int R, F; };
struct Counters { int nU, nK, nS; unsigned int nP3, nP4, nP5, nHull, nX3, nX4; };     // (the first three: k_round_triage / k_round_scan)

// One call of sd_nms3d_device: what its phases hand to each other.  Every phase returns 0 or -1 (error set).
struct Nms3d {
  // the call
  hipStream_t s;
  const float *dist, *pts;
  Mesh rays;
  int N, R, F;
  float thr;
  int use_bbox, use_kdtree, verbose;
  bool wantStats;
  sd::Arena& A;
  // plan
  sdl::Nms3dLds lds;
  int splitOpt = 0;
  bool split3 = false, split4 = false, trace = false;
  unsigned int split3Max = 0, split4Max = 0;
  Timer stageTimer, broadTimer;
  double ns3 = 0, ns4 = 0, ns5 = 0;
  // precompute
  float *volume = nullptr, *r_outer = nullptr, *r_outer_iso = nullptr, *r_inner_iso = nullptr, max_dist = 0;
  int *bbox = nullptr, *gi = nullptr, *candCell = nullptr, g[8];      // g: max outer radius bits, min / max of the centres (z, y, x)
  unsigned char* state = nullptr;
  Aniso an;
  sd3::ConeMap cmap{nullptr, nullptr};
  sd::SideJoin coneJoin;
  // grid
  Grid3 gr;
  static constexpr int W = 2;
  int *cellStart = nullptr, *nbrCount = nullptr, *nbrLow = nullptr;
  CellRec3* cellRec = nullptr;
  i64* nbrStart = nullptr;
  void* scanTmp = nullptr;
  size_t scanBytes = 0;
  bool singlePass = false;
  NmsFlags f;
  // mesh: the rays' edge adjacency; direction meshes of the volume bounds: refined once (or the rays), refined twice (or none)
  int* faceAdj = nullptr;
  bool mesh_ok = false, use_bounds = false;
  Mesh b, b3{nullptr, nullptr, 0, 0};
  // lists and rounds
  NbrLists L{};
  unsigned int pairCap = 0, hDef = 0;              // hDef: pairs deferred so far (host mirror: the counters of every round are read anyway)
  int *Ucur = nullptr, *Unext = nullptr, *Kl = nullptr, *Sl = nullptr, *hullState = nullptr, *hullCount = nullptr, *hullList = nullptr, *d_left = nullptr;
  int2 *pairs3 = nullptr, *pairs4 = nullptr, *pairs5 = nullptr, *pairsX = nullptr, *supEdges = nullptr, *dfr = nullptr;
  unsigned int *supCount = nullptr, *dfrCount = nullptr;
  unsigned char *blocked = nullptr, *pend = nullptr;
  Counters *d_cnt = nullptr, h;
  Stats* d_st = nullptr;
  double* hullPlanes = nullptr;                    // N * hullCap * 4 doubles, allocated on first use
  unsigned short* hullAdj = nullptr;               // N * hullCap * 3
  int hullCap = 0, nU = 0, rounds = 0, tailT = -1, deferFrom = 0;
  bool forceTail = false, leanOpt = false;
  static constexpr unsigned int dfrCap = 262144u;
  sdl::PairFlags flags3{0, 0, 0}, flags4{0, 0, 0};

  Nms3d(hipStream_t s_, const float* dist_, const float* pts_, int N_, int R_, int F_, const float* verts_, const int* faces_, float thr_, int use_bbox_,
        int use_kdtree_, int verbose_, bool wantStats_)
      : s(s_), dist(dist_), pts(pts_), rays{verts_, faces_, R_, F_}, N(N_), R(R_), F(F_), thr(thr_), use_bbox(use_bbox_), use_kdtree(use_kdtree_),
        verbose(verbose_), wantStats(wantStats_), A(sd::arena()), b(rays) {}

  // validation, options, LDS layouts and function attributes; begins the arena pass and the broad-phase time
  int plan() {
    if (R < 4 || F < 4) { sd::set_error("sd_nms3d: need n_rays >= 4 and n_faces >= 4"); return -1; }
    if (R > 800) { sd::set_error("sd_nms3d: n_rays must be <= 800"); return -1; }
    if (plan_lds("sd_nms3d", R, F, &lds)) return -1;
    // exact volumes of the undecided pairs by four waves per pair (k_stage3x): when the four workspaces fit
    // (the launches of the later rounds hold few pairs and lasted as long as their slowest pair, an exact volume of ~1 ms by one wave;
    // in the first round the one-wave form is faster: thousands of exact volumes keep every SIMD busy either way)
    // option nms3d_split_exact: 0 exact volumes in place; 1 second pass (k_stage3x / k_stage4x: four waves per pair) for the smaller launches
    // (round 3); 2 (default): stage 3 ALWAYS splits, and a bounds-only first pass is launched with the small LDS footprint (no polygon
    // workspace: 25.6 instead of 39.3 KB per wave = six waves per CU instead of four) -- measured on the 256^3 bench set: stage 3
    // 12.9 -> 10.7 ms; stage 4 keeps its threshold (always splitting it: 12.6 -> 13.1 ms, the hull construction dominates there);
    // 3: both stages always split
    splitOpt = sd::option(sd::OPT_NMS3D_SPLIT_EXACT);
    split3 = splitOpt && lds.split3();
    split4 = splitOpt && lds.split4();
    split3Max = splitOpt >= 2 ? 0x7fffffffu : 32768u; split4Max = splitOpt >= 3 ? 0x7fffffffu : 16384u;   // pairs per launch up to which the second pass pays
    if (A.begin(s)) return -1;
    if (wantStats && (stageTimer.init() || broadTimer.init() || broadTimer.start(s))) return -1;      // broad phase: precompute, grid, neighbour lists (the HBM-bound scan)
    trace = sd::option(sd::OPT_TRACE) != 0;
    return 0;
  }

  // per candidate: volume, bounding box, radii; the extent of the centres; the anisotropy; the cone map of stage 5 next to it
  int precompute() {
    volume = A.take_n<float>(N);
    bbox = A.take_n<int>((size_t)6 * N);
    r_outer = A.take_n<float>(N);
    r_outer_iso = A.take_n<float>(N);
    r_inner_iso = A.take_n<float>(N);
    gi = A.take_n<int>(8);
    state = A.take_n<unsigned char>(N);
    candCell = A.take_n<int>(N);
    if (!volume || !bbox || !r_outer || !r_outer_iso || !r_inner_iso || !gi || !state || !candCell) return -1;
    static const int gi_init[8] = {0, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, 0};
    SD_CHECK(hipMemcpyAsync(gi, gi_init, sizeof(gi_init), hipMemcpyHostToDevice, s));
    SD_CHECK(hipMemsetAsync(state, 0, N, s));
    const int staged = lds.rows.staged() ? 1 : 0;
    if (lds_optin(k_pre1, lds.rows.bytes()) || lds_optin(k_pre2, lds.rows.bytes())) return -1;
    hipLaunchKernelGGL(k_pre1, dim3(sd::div_up(N, sdl::RowsLds::ROWS)), dim3(sdl::RowsLds::ROWS), lds.rows.bytes(), s, dist, pts, rays.verts, rays.faces, N, R, F, volume,
                       bbox, staged);
    SD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_minmax3, dim3(sd::div_up(N, 256)), dim3(256), 0, s, pts, N, gi + 1);
    // cone map for the voxel tests of stage 5 (geom3d.h); option "nms3d_cone_map" = 0 tests every face as the reference does.  It depends on
    // the ray mesh only and is a latency-bound launch of a few workgroups (0.23 ms at 96 rays): it runs on a helper stream NEXT TO the
    // read-back of the bounding boxes and the host's sequential anisotropy sum below (0.3 ms of otherwise idle device), joined before the rounds
    if (sd::cone_map(rays.verts, rays.faces, F, &cmap, s, &coneJoin)) return -1;
    // anisotropy: sequential fp32 accumulation over candidates (:1008-1010) on the host
    std::vector<int> hb((size_t)6 * N);
    SD_CHECK(hipMemcpyAsync(hb.data(), bbox, (size_t)6 * N * sizeof(int), hipMemcpyDeviceToHost, s));
    SD_CHECK(hipStreamSynchronize(s));
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
    hipLaunchKernelGGL(k_pre2, dim3(sd::div_up(N, sdl::RowsLds::ROWS)), dim3(sdl::RowsLds::ROWS), lds.rows.bytes(), s, dist, rays.verts, rays.faces, N, R, F, an, r_outer,
                       r_outer_iso, r_inner_iso, gi, staged);
    SD_LAUNCH_CHECK();
    SD_CHECK(hipMemcpyAsync(g, gi, sizeof(g), hipMemcpyDeviceToHost, s));
    SD_CHECK(hipStreamSynchronize(s));
    memcpy(&max_dist, &g[0], 4);
    return 0;
  }

  // uniform grid over the centres, the candidates' records in cell order
  int build_grid() {
    float cs = (2.f * max_dist + 1.f) * 0.5f * 1.0001f + 1e-3f;
    if (!(cs >= 1.f)) cs = 1.f;
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
    cellStart = A.take_n<int>(nCells + 1);
    int* cellFill = A.take_n<int>(nCells + 1);
    cellRec = A.take_n<CellRec3>(N);
    nbrCount = A.take_n<int>(N + 1);
    nbrLow = A.take_n<int>(N + 1);
    nbrStart = A.take_n<i64>(N + 1);
    if (!cellCount || !cellStart || !cellFill || !cellRec || !nbrCount || !nbrLow || !nbrStart) return -1;
    SD_CHECK(hipMemsetAsync(cellCount, 0, (nCells + 1) * sizeof(int), s));
    SD_CHECK(hipMemsetAsync(cellFill, 0, (nCells + 1) * sizeof(int), s));
    hipLaunchKernelGGL(k_cell_count3, dim3(sd::div_up(N, 256)), dim3(256), 0, s, pts, N, gr, cellCount, candCell);
    size_t tb2 = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scanBytes, cellCount, cellStart, nCells + 1, s);
    (void)exclusive_sum_i64(nullptr, tb2, nbrCount, nbrStart, N + 1, s);
    if (tb2 > scanBytes) scanBytes = tb2;
    scanTmp = A.take(scanBytes + 256);
    if (!scanTmp) return -1;
    SD_CHECK(hipcub::DeviceScan::ExclusiveSum(scanTmp, scanBytes, cellCount, cellStart, nCells + 1, s));
    // neighbour lists in ONE pass (option "nms3d_neighbours_single_pass", default 1; nms2d.hip has the 2D twin): slots sized from the cell
    // table, better-scored neighbours from the slot's front, the others from its back, the exact total summed afterwards; the two-pass form
    // (count, scan, fill: every candidate test done twice) remains for inputs whose slots would exceed 32-bit indices or the workspace
    singlePass = sd::option(sd::OPT_NMS3D_NBR_SINGLE) != 0;
    SD_CHECK(hipMemsetAsync(nbrCount, 0, (N + 1) * sizeof(int), s));
    hipLaunchKernelGGL(k_cell_fill3, dim3(sd::div_up(N, 256)), dim3(256), 0, s, N, candCell, cellStart, cellFill, pts, bbox, cellRec, gr, W,
                       singlePass ? nbrCount : (int*)nullptr);
    SD_LAUNCH_CHECK();
    f.use_kdtree = use_kdtree; f.use_bbox = use_bbox; f.thr_nonneg = (thr >= 0.f); f.thr = thr; f.max_dist = max_dist;
    return 0;
  }

  // *out = `in` with every triangle split in four (k_refine_mesh); adj: the edge adjacency of `in`, nullptr: computed here
  int refine_mesh(const Mesh& in, const int* adj, Mesh* out) {
    const int R2 = in.R + 3 * in.F / 2, F2 = 4 * in.F;
    int* adjOwn = adj ? nullptr : A.take_n<int>((size_t)3 * in.F);
    float* v2 = A.take_n<float>((size_t)3 * R2);
    int* f2 = A.take_n<int>((size_t)3 * F2);
    int* edgeId = A.take_n<int>((size_t)3 * in.F);
    int* ecount = A.take_n<int>(1);
    if ((!adj && !adjOwn) || !v2 || !f2 || !edgeId || !ecount) return -1;
    SD_CHECK(hipMemsetAsync(ecount, 0, sizeof(int), s));
    if (!adj) { hipLaunchKernelGGL(k_face_adj, dim3(in.F), dim3(64), 0, s, in.faces, in.F, adjOwn); adj = adjOwn; }
    hipLaunchKernelGGL(k_refine_edges, dim3(sd::div_up(3 * in.F, 64)), dim3(64), 0, s, in.faces, adj, in.F, edgeId, ecount);
    hipLaunchKernelGGL(k_refine_mesh, dim3(sd::div_up(in.F > in.R ? in.F : in.R, 64)), dim3(64), 0, s, in.verts, in.faces, adj, in.R, in.F, edgeId, v2, f2);
    SD_LAUNCH_CHECK();
    *out = Mesh{v2, f2, R2, F2};
    return 0;
  }

  // ray mesh: edge adjacency (seeds of the exact volume routine), validity (precondition of the volume bounds), the bounds' finer meshes
  int prepare_mesh() {
    faceAdj = A.take_n<int>((size_t)3 * F);
    int* d_mesh = A.take_n<int>(4);
    double* d_mesh_sa = A.take_n<double>(1);
    if (!faceAdj || !d_mesh || !d_mesh_sa) return -1;
    SD_CHECK(hipMemsetAsync(d_mesh, 0, 4 * sizeof(int), s));
    SD_CHECK(hipMemsetAsync(d_mesh_sa, 0, sizeof(double), s));
    hipLaunchKernelGGL(k_face_adj, dim3(F), dim3(64), 0, s, rays.faces, F, faceAdj);
    hipLaunchKernelGGL(k_mesh_check, dim3(sd::div_up(F, 64)), dim3(64), 0, s, rays.verts, rays.faces, faceAdj, F, d_mesh, d_mesh_sa);
    SD_LAUNCH_CHECK();
    int h_mesh[4]; double h_mesh_sa = 0;
    SD_CHECK(hipMemcpyAsync(h_mesh, d_mesh, sizeof(h_mesh), hipMemcpyDeviceToHost, s));
    SD_CHECK(hipMemcpyAsync(&h_mesh_sa, d_mesh_sa, sizeof(double), hipMemcpyDeviceToHost, s));
    SD_CHECK(hipStreamSynchronize(s));
    mesh_ok = h_mesh[0] == 0 && fabs(h_mesh_sa - 4.0 * M_PI) < 1e-6;
    use_bounds = mesh_ok && sd::option(sd::OPT_NMS3D_VOLUME_BOUNDS) != 0;
    if (trace) printf("ray mesh: open/degenerate flags %d, orientation +%d/-%d, solid angle %.9f -> volume bounds %s\n", h_mesh[0], h_mesh[1], h_mesh[2],
                      h_mesh_sa, use_bounds ? "on" : "off");
    // direction mesh of the volume bounds: refined once when its ray-cast workspace fits the LDS the stages have anyway
    const int refineOpt = sd::option(sd::OPT_NMS3D_REFINE_MESH);
    if (use_bounds && sdl::refined_once_fits(R, F, lds.s3.ws) && refineOpt != 0 && refine_mesh(rays, faceAdj, &b)) return -1;
    // refined once more for the pairs that reach the exact-volume kernels (k_stage3x / k_stage4x evaluate it with the whole workgroup;
    // its ray-cast vectors live in the polygon workspaces of waves 1..3, which are idle until the integration starts)
    if (b.R != R && splitOpt && refineOpt >= 2 && sdl::refined_twice_fits(b.R, b.F) && refine_mesh(b, nullptr, &b3)) return -1;
    return 0;
  }

  // neighbour lists (build_neighbour_lists, nms_rounds.h); ends the broad-phase time
  int build_lists() {
    const int nbBlocks = (sd::div_up(N, 4) + 7) & ~7;
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
    const int rcLists = build_neighbour_lists(A, s, N, singlePass, scanTmp, scanBytes, launch_neighbours, []() { return 0; }, L);
    // capacity of one call (32-bit indices into the neighbour lists and pair queues, N * n_rays * 4 bytes of distances): beyond it the
    // input has to be sharded -- predict_instances_sharded / predict_instances_big do exactly that
    if (rcLists > 0 || (rcLists == 0 && (i64)N * R >= (i64)0x3fffffff)) {
      sd::set_error("sd_nms3d: %d candidates (%lld neighbour entries) exceed the capacity of one call (2^30 distance values, 2^31 - 1 "
                    "neighbour entries): shard the input (predict_instances_sharded / predict_instances_big)", N, (long long)L.total);
      return -1;
    }
    if (rcLists) return -1;
    return broadTimer.stop(s);
  }

  // queues, counters and switches of the greedy rounds
  int begin_rounds() {
    // (the cone map of stage 5 was started on the helper stream in front of the anisotropy sum; from here on the caller's stream waits for it)
    if (coneJoin.join(s)) return -1;
    pairCap = (unsigned int)((L.total / 2 + 64) < (1ll << 31) ? (L.total / 2 + 64) : ((1ll << 31) - 1));
    Ucur = A.take_n<int>(N);
    Unext = A.take_n<int>(N);
    Kl = A.take_n<int>(N);
    Sl = A.take_n<int>(N);
    pairs3 = A.take_n<int2>(pairCap);
    pairs4 = A.take_n<int2>(pairCap);
    pairs5 = A.take_n<int2>(pairCap);
    pairsX = (split3 || split4) ? A.take_n<int2>(pairCap) : nullptr;          // pairs whose exact volume is needed
    d_cnt = (Counters*)A.take(sizeof(Counters));
    d_st = (Stats*)A.take(sizeof(Stats));
    if (!Ucur || !Unext || !Kl || !Sl || !pairs3 || !pairs4 || !pairs5 || !d_cnt || !d_st || ((split3 || split4) && !pairsX)) return -1;
    hullCap = lds.hull.cap;                          // a hull of R points has at most 2R-4 facets
    hullState = A.take_n<int>(N);
    hullCount = A.take_n<int>(N);
    hullList = A.take_n<int>(N);
    if (!hullState || !hullCount || !hullList) return -1;
    SD_CHECK(hipMemsetAsync(hullState, 0, (size_t)N * sizeof(int), s));
    SD_CHECK(hipMemsetAsync(d_st, 0, sizeof(Stats), s));
    hipLaunchKernelGGL(k_iota, dim3(sd::div_up(N, 256)), dim3(256), 0, s, Ucur, N);
    nU = N;
    // Tail batch: the late rounds hold few pairs, but every stage launch costs the latency of its slowest pair (an exact volume: ~1.5 ms).
    // Once few candidates are undecided (N/128, at least 512), the cascade is run ONCE over every pair of undecided candidates the
    // sequential loop could still evaluate (speculatively: i need not end up kept), suppressions are recorded as edges, and the remaining
    // greedy order is replayed on the device over those edges (k_tail3_mark / k_tail3_promote).  Same fixed point: j is suppressed iff
    // some KEPT i < j suppresses it.  The threshold is late on purpose: undecided candidates sit in dense clusters, so the speculative
    // pair count grows quickly with them (measured on the 256^3 bench set: at N/8 = 16 404 undecided candidates 71 674 stage-3 pairs
    // instead of the 2 397 the plain rounds evaluate -- slower than the rounds it replaces; at N/128 the three last rounds, ~7 ms of
    // launch latency, become one pass).  sd_set_option("nms3d_tail_batch", 0) keeps the plain rounds (the parity suite runs both).
    const int tailOpt = sd::option(sd::OPT_NMS3D_TAIL_BATCH), tailDiv = tailOpt >= 2 ? tailOpt : 32;       // option value >= 2: the divisor itself (tuning)
    tailT = tailOpt ? (N / tailDiv > 512 ? N / tailDiv : 512) : -1;
    // exact volumes of the late rounds carried into the tail batch (k_defer3): from round deferFrom on, while the queue has room for
    // the round's pairs.  Needs the tail batch and the split exact-volume passes (the bounds passes hand over the undecided pairs).
    deferFrom = (tailOpt && use_bounds && (split3 || split4)) ? sd::option(sd::OPT_NMS3D_DEFER_EXACT) : 0;
    if (deferFrom > 0) {
      dfr = A.take_n<int2>(dfrCap); dfrCount = A.take_n<unsigned int>(1); pend = A.take_n<unsigned char>(N);
      if (!dfr || !dfrCount || !pend) return -1;
      SD_CHECK(hipMemsetAsync(dfrCount, 0, sizeof(unsigned int), s));
      SD_CHECK(hipMemsetAsync(pend, 0, N, s));
    }
    flags3 = sdl::PairFlags{trace ? 1u : 0u, sd::option(sd::OPT_NMS3D_BOUNDS_REUSE) ? 0u : 1u, use_bounds ? 0u : 1u};
    flags4 = sdl::PairFlags{0, flags3.recast, flags3.exact};
    leanOpt = use_bounds && sd::option(sd::OPT_NMS3D_BOUNDS_LEAN) != 0;
    return 0;
  }

  // The second half of a volume stage, behind its bounds pass over nPairs pairs: the pairs that pass queued (sp) go to the tail batch
  // (k_defer3) or through the four-wave exact pass (launchExact); then ONE read-back of the round's counters and the stage's time.
  template <class Exact>
  int finish_volume_stage(bool sp, bool tail, unsigned int nPairs, unsigned int* d_nX, unsigned int Counters::*nX, Exact launchExact, double* ns, float* ms) {
    const bool defer = sp && !tail && deferFrom > 0 && rounds >= deferFrom && hDef + nPairs <= dfrCap;
    if (defer)
      hipLaunchKernelGGL(k_defer3, dim3(nPairs < 16384u ? sd::div_up(nPairs, 256) : 64), dim3(256), 0, s, pairsX, d_nX, dfr, dfrCount, dfrCap, pend, &d_st->overflow);
    else if (sp) launchExact();
    SD_LAUNCH_CHECK();
    if (stageTimer.stop(s)) return -1;
    SD_CHECK(hipMemcpyAsync(&h, d_cnt, sizeof(Counters), hipMemcpyDeviceToHost, s));
    SD_CHECK(hipStreamSynchronize(s));
    if (defer) hDef += h.*nX;
    if (stageTimer.ms(ms)) return -1;
    *ns += *ms * 1e6;
    return 0;
  }

  int run_stage3(bool tail, const SuppSink& sink) {
    const unsigned int nP3 = h.nP3, b3grid = nP3 < 16384u ? nP3 : 16384u;
    if (stageTimer.start(s)) return -1;
    const bool sp3 = split3 && nP3 <= split3Max;
    // bounds-only pass: the workspace only holds the ray-cast vectors (at least the vertex staging), lean: no seed / pos / orig tables behind it
    const sdl::PairLds small = sdl::stage3_lds(R, F, sdl::WS_SMALL, b.R, 1);
    const bool small3 = sp3 && splitOpt >= 2 && small.ws < lds.s3.ws;
    const sdl::PairLds l3 = !small3 ? lds.s3 : leanOpt ? sdl::stage3_lds(R, F, sdl::WS_LEAN, b.R, 1) : small;
    hipLaunchKernelGGL(k_stage3, dim3(b3grid), dim3(64), l3.bytes(), s, pairs3, nP3, dist, pts, rays.verts, rays.faces, faceAdj, R, volume,
                       thr, sink, pairs4, &d_cnt->nP4, d_st, l3, flags3, b.verts, b.faces, b.R, b.F, (double*)nullptr, sp3 ? pairsX : (int2*)nullptr, &d_cnt->nX3);
    float ms;
    if (finish_volume_stage(sp3, tail, nP3, &d_cnt->nX3, &Counters::nX3, [&]() {
          hipLaunchKernelGGL(k_stage3x<4>, dim3(nP3 < 256u ? nP3 : 256u), dim3(256), lds.s3x.bytes(), s, pairsX, &d_cnt->nX3, 0u, dist, pts, rays.verts, rays.faces, faceAdj,
                             R, volume, thr, sink, pairs4, &d_cnt->nP4, d_st, lds.s3x, (double*)nullptr, b3.verts, b3.faces, b3.R, b3.F);
        }, &ns3, &ms)) return -1;
    if (wantStats && trace) printf("round %d: nU=%d nK=%d stage3 pairs=%u %.3f ms -> stage4 pairs=%u\n", rounds, h.nU, h.nK, h.nP3, ms, h.nP4);
    return 0;
  }

  int run_stage4(bool tail) {
    const unsigned int nP4 = h.nP4, b4grid = nP4 < 16384u ? nP4 : 16384u;
    if (stageTimer.start(s)) return -1;
    if (!hullPlanes) {
      hullPlanes = A.take_n<double>((size_t)N * hullCap * 4);
      hullAdj = A.take_n<unsigned short>((size_t)N * hullCap * 3);
      if (!hullPlanes || !hullAdj) return -1;
    }
    SD_CHECK(hipMemsetAsync(&d_cnt->nHull, 0, sizeof(unsigned int), s));
    hipLaunchKernelGGL(k_hull_mark, dim3(sd::div_up(nP4, 256)), dim3(256), 0, s, pairs4, nP4, hullState, hullList, &d_cnt->nHull);
    {
      // no read-back of the hull count (~40 us of idle device per round): a pair asks for at most two hulls, the kernel reads the
      // length of its list on the device; the count reaches the host with the counters behind stage 4
      const unsigned long long ub = 2ull * nP4;
      const unsigned int bh = ub < 32768ull ? (unsigned int)ub : 32768u;
      hipLaunchKernelGGL(k_hull, dim3(bh), dim3(64), lds.hull.bytes(), s, hullList, 0u, dist, pts, rays.verts, R, hullCap, hullPlanes, hullAdj, hullCount,
                         (const unsigned int*)&d_cnt->nHull);
      SD_LAUNCH_CHECK();
    }
    const bool sp4 = split4 && nP4 <= split4Max;
    const sdl::PairLds small = sdl::stage4_lds(hullCap, sdl::WS_SMALL, b.R, 1);
    const bool small4 = sp4 && splitOpt >= 2 && small.ws < lds.s4.ws;
    const sdl::PairLds l4 = !small4 ? lds.s4 : leanOpt ? sdl::stage4_lds(hullCap, sdl::WS_LEAN, b.R, 1) : small;
    hipLaunchKernelGGL(k_stage4, dim3(b4grid), dim3(64), l4.bytes(), s, pairs4, nP4, dist, pts, rays.verts, rays.faces, R, F, hullPlanes, hullAdj, hullCount,
                       volume, thr, pairs5, &d_cnt->nP5, d_st, l4, flags4, b.verts, b.faces, b.R, b.F, (double*)nullptr, sp4 ? pairsX : (int2*)nullptr, &d_cnt->nX4);
    float ms;
    if (finish_volume_stage(sp4, tail, nP4, &d_cnt->nX4, &Counters::nX4, [&]() {
          hipLaunchKernelGGL(k_stage4x<4>, dim3(nP4 < 256u ? nP4 : 256u), dim3(256), lds.s4x.bytes(), s, pairsX, &d_cnt->nX4, 0u, dist, pts, R, hullPlanes, hullAdj,
                             hullCount, volume, thr, pairs5, &d_cnt->nP5, d_st, lds.s4x, (double*)nullptr, b3.verts, b3.faces, b3.R, b3.F);
        }, &ns4, &ms)) return -1;
    if (wantStats && trace) printf("         stage4 pairs=%u hulls=%u %.3f ms -> stage5 pairs=%u\n", h.nP4, h.nHull, ms, h.nP5);
    return 0;
  }

  int run_stage5(const SuppSink& sink) {
    const unsigned int b5grid = h.nP5 < 16384u ? h.nP5 : 16384u;
    if (stageTimer.start(s)) return -1;
    hipLaunchKernelGGL(k_stage5, dim3(b5grid), dim3(256), lds.render.bytes(), s, pairs5, h.nP5, dist, pts, rays.verts, rays.faces, R, F, bbox, volume,
                       thr, sink, d_st, cmap, mesh_ok ? 0 : 1);
    SD_LAUNCH_CHECK();
    float ms;
    if (stageTimer.stop(s) || stageTimer.wait() || stageTimer.ms(&ms)) return -1;
    ns5 += ms * 1e6;
    return 0;
  }

  // the remaining greedy order replayed over the suppressing edges of the tail batch
  int tail_replay() {
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
    return 0;
  }

  // one greedy round (or the tail batch): who survives, the pairs they form, the cascade over those pairs
  int run_round() {
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
      hipLaunchKernelGGL(k_round_triage, dim3(sd::div_up(nU, 256)), dim3(256), 0, s, Ucur, nU, state, L.waitOn, Unext, Kl, Sl, (int*)d_cnt, (const unsigned char*)pend);
      const int wgrid = sd::div_up(nU, 4) < 2048 ? sd::div_up(nU, 4) : 2048;
      hipLaunchKernelGGL(k_round_scan, dim3(wgrid), dim3(256), 0, s, Sl, state, nbrStart, nbrLow, L.nbr, L.waitOn, Unext, Kl, (int*)d_cnt, (const unsigned char*)pend);
      SD_LAUNCH_CHECK();
    }
    const SuppSink sink = tail ? SuppSink{state, supEdges, supCount, pairCap} : SuppSink{state, nullptr, nullptr, 0u};
    {
      // ONE read-back for the survivors, the undecided and the stage-3 pairs of the round: the emission takes the survivor count from
      // device memory (a persistent grid sized from the undecided candidates), as the 2D rounds do
      const int egrid = sd::div_up(nU, 4) < 2048 ? sd::div_up(nU, 4) : 2048;
      hipLaunchKernelGGL(k_round_emit3, dim3(egrid), dim3(256), 0, s, tail ? Ucur : Kl, tail ? nU : 0, tail ? (const int*)nullptr : (const int*)&d_cnt->nK, sink, tail ? 1 : 0,
                         nbrStart, nbrCount, (const int*)L.nbr, f, an, pts, bbox, volume, r_outer, r_outer_iso, r_inner_iso, pairs3, &d_cnt->nP3, pairCap, d_st);
      SD_LAUNCH_CHECK();
      SD_CHECK(hipMemcpyAsync(&h, d_cnt, sizeof(Counters), hipMemcpyDeviceToHost, s));
      SD_CHECK(hipStreamSynchronize(s));
    }
    if (!tail && h.nK == 0 && h.nU > 0) {
      if (!hDef) { sd::set_error("sd_nms3d: greedy scan made no progress (internal error)"); return -1; }
      // every remaining candidate is pending or waits for a pending one: the tail batch takes over from here
      forceTail = true;
      nU = h.nU;
      std::swap(Ucur, Unext);
      return 0;
    }
    const int nUndecided = tail ? 0 : h.nU;
    if (h.nP3 > pairCap) { sd::set_error("sd_nms3d: pair queue overflow (internal error)"); return -1; }
    if (h.nP3 > 0) {
      if (run_stage3(tail, sink)) return -1;
      if (h.nP4 > 0 && run_stage4(tail)) return -1;
      if (h.nP4 > 0 && h.nP5 > 0 && run_stage5(sink)) return -1;
    }
    if (tail) {
      if (tail_replay()) return -1;
      nU = 0;
      return 0;
    }
    nU = nUndecided;
    std::swap(Ucur, Unext);
    return 0;
  }

  // keep flags, statistics, the reference's printed summary
  int report(uint8_t* d_keep, int64_t* stats) {
    hipLaunchKernelGGL(k_keep, dim3(sd::div_up(N, 256)), dim3(256), 0, s, state, d_keep, N);
    SD_LAUNCH_CHECK();
    Stats hs_;
    SD_CHECK(hipMemcpyAsync(&hs_, d_st, sizeof(Stats), hipMemcpyDeviceToHost, s));
    SD_CHECK(hipStreamSynchronize(s));
    if (hs_.overflow) { sd::set_error("sd_nms3d: half-space intersection capacity exceeded (%llu pairs)", hs_.overflow); return -1; }
    if (stats) {
      stats[0] = (int64_t)hs_.upper; stats[1] = (int64_t)hs_.lower; stats[2] = (int64_t)hs_.kernel; stats[3] = (int64_t)hs_.render;
      stats[4] = rounds; stats[5] = L.total; stats[6] = (int64_t)hs_.sup_kernel; stats[7] = (int64_t)hs_.sup_render;
      stats[8] = (int64_t)ns3; stats[9] = (int64_t)ns4; stats[10] = (int64_t)ns5; stats[11] = (int64_t)hs_.convex; stats[12] = (int64_t)hs_.kept_convex;
      stats[13] = (int64_t)hs_.near_thr; stats[14] = (int64_t)hs_.hiv_fallback;
      { float msb = 0; if (broadTimer.ms(&msb)) return -1; stats[15] = (int64_t)(msb * 1e6); }
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
      printf("NMS: greedy rounds: %d, neighbour entries: %lld\n", rounds, (long long)L.total);
      fflush(stdout);
    }
    if (trace) fflush(stdout);
    return 0;
  }
};

}  // namespace

extern "C" int sd_nms3d_device(const float* d_scores, const float* d_dist, const float* d_points, int n_polys, int n_rays, int n_faces,
                               const float* d_verts, const int* d_faces, float threshold, int use_bbox, int use_kdtree, int verbose,
                               uint8_t* d_keep, int64_t* stats, void* stream_) {
  (void)d_scores;   // unused by the reference's arithmetic as well
  hipStream_t s = (hipStream_t)stream_;
  if (stats) memset(stats, 0, 16 * sizeof(int64_t));
  if (verbose) {
    printf("Non Maximum Suppression (3D) ++++ \n");
    printf("NMS: n_polys  = %d \nNMS: n_rays   = %d  \nNMS: n_faces  = %d \nNMS: thresh   = %.3f \nNMS: use_bbox = %d \nNMS: use_kdtree = %d \n",
           n_polys, n_rays, n_faces, threshold, use_bbox, use_kdtree);
    printf("NMS: using HIP (gfx950)\n");
    fflush(stdout);
  }
  if (n_polys <= 0) return 0;
  Nms3d c(s, d_dist, d_points, n_polys, n_rays, n_faces, d_verts, d_faces, threshold, use_bbox, use_kdtree, verbose, stats != nullptr);
  if (c.plan()) return -1;
  if (!use_kdtree && !use_bbox && threshold < 0) {   // every (0, j) passes and iou >= 0 > thr at stage 2
    SD_CHECK(hipMemsetAsync(d_keep, 0, n_polys, s));
    SD_CHECK(hipMemsetAsync(d_keep, 1, 1, s));
    SD_CHECK(hipStreamSynchronize(s));
    return 0;
  }
  if (c.precompute() || c.build_grid() || c.prepare_mesh() || c.build_lists() || c.begin_rounds()) return -1;
  while (c.nU > 0)
    if (c.run_round()) return -1;
  return c.report(d_keep, stats);
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
