// nms3d_hull.h -- convex hulls of the candidates that reach stage 4 of the 3D NMS (nms3d.hip; also the hull factor of the 3D
// rasteriser, raster3d.hip), in place of Qhull's (halfspaces_convex, stardist3d_impl.cpp:767-795): the facet planes and their edge
// adjacency, one wave per polyhedron.  Device code of ONE translation unit (anonymous namespace).
#pragma once
#include "nms3d_hiv.h"

namespace {

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
  const sdl::HullLds L{R, cap};
  double* pv = (double*)(smem + L.pv());                        // 3R doubles
  unsigned int* tri = (unsigned int*)(smem + L.tri());          // cap packed facets a | b << 10 | c << 20
  unsigned int* frA = (unsigned int*)(smem + L.frA());          // fast path only: 6R + 6R open edges, R*R edge use counts
  unsigned int* frB = (unsigned int*)(smem + L.frB());
  unsigned int* cnt = (unsigned int*)(smem + L.cnt());          // R*R edge use counts, two bits each
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

}  // namespace
