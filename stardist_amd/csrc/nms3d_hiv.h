// nms3d_hiv.h -- volume of a half-space intersection by one wave or one workgroup (stages 3 and 4 of the 3D NMS, nms3d.hip), in place
// of Qhull's half-space intersection (qhull_overlap_kernel / qhull_overlap_convex_hulls, stardist3d_impl.cpp:830-939): the exact
// volume (one half-space per lane, its face polygon clipped against the others in fp64, volume = 1/3 sum(area * height)), the cull
// of the half-spaces that cannot bound the intersection, and the rigorous lower / upper volume bounds from one ray cast per direction
// of a mesh.  Half-spaces h = (n, d): inside <=> n.p + d <= 0.  Device code of ONE translation unit (anonymous namespace).
#pragma once
#include "nms3d_lds.h"

namespace {

// counters of one NMS call (the volume routines add to hiv_*; the stage kernels to the rest)
struct Stats { unsigned long long upper, lower, kernel, render, kept_pre, sup_pre, sup_kernel, sup_render, convex, kept_convex, overflow, hiv_faces, hiv_fallback, hiv_list, hiv_clips, hiv_rest, lb_decided, ub_decided, near_thr;
               unsigned long long cyc[6]; };   // SD_TRACE: stage-3 wave cycles spent in load+half-spaces / cull / bounds / exact volume / total

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
#define HIV_NONE 0xFFFFu
struct HivLds {
  double* S; double* T;                 // polygon vertices [HIV_CAPL][64]
  unsigned short* list;                 // [HIV_LCAP][64] per-lane list of half-spaces that may cut the polygon
  unsigned short* seed;                 // [M_orig][3]: original indices of the edge-adjacent half-spaces (HIV_NONE: unknown)
  unsigned short* pos;                  // [M_orig]: original index -> index after culling (HIV_NONE: culled)
  unsigned short* orig;                 // [M]: index after culling -> original index
};
// the workspace of `wave` and the tables shared by the waves of a pair, in the LDS of a volume kernel laid out as L
__device__ __forceinline__ HivLds hiv_lds(char* smem, const sdl::PairLds& L, int wave) {
  HivLds W;
  W.S = (double*)(smem + (wave == 0 ? L.work() : L.extra(wave)));
  W.T = W.S + HIV_CAPL * 64; W.list = (unsigned short*)(W.T + HIV_CAPL * 64);
  W.seed = (unsigned short*)(smem + L.seed()); W.pos = (unsigned short*)(smem + L.pos()); W.orig = (unsigned short*)(smem + L.orig());
  return W;
}

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
// (hiv_bounds_wave: one wave; hiv_bounds_block: a workgroup; both from the two routines below.)

// The ray cast of the directions kbeg .. R - 1 by NT threads: the plane loop is the outer one and a thread keeps up to NB directions in
// registers -- one LDS read of a plane serves NB independent compare chains (a loop over planes per direction is bound by LDS latency +
// its loop-carried dependency: 358k cycles per pair measured with the refined mesh, 80 % of stage 3)
template <int NT, int NB>
__device__ __forceinline__ void hiv_raycast(const double* __restrict__ hs, int M, const float* __restrict__ verts, int R, int kbeg, double* wv,
                                            unsigned short* hit, int tid) {
#pragma clang fp contract(fast)
  for (int k0 = kbeg; k0 < R; k0 += NT * NB) {
    double dz[NB], dy[NB], dx[NB], ne_b[NB], q_b[NB];
    int m_b[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int k = k0 + j * NT + tid;
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
      const int k = k0 + j * NT + tid;
      if (k < R) {
        const double t = (q_b[j] > 0) ? ne_b[j] / q_b[j] : 0.0;
        wv[3 * k] = t * dz[j]; wv[3 * k + 1] = t * dy[j]; wv[3 * k + 2] = t * dx[j];
        hit[k] = (unsigned short)((q_b[j] > 0) ? m_b[j] : HIV_NONE);
      }
    }
  }
}
// this thread's share (triangles tid, tid + NT, ...) of 6 x the two bounds; true when a triangle has no upper bound
template <int NT>
__device__ __forceinline__ bool hiv_bound_sums(const double* __restrict__ hs, const int* __restrict__ faces, int F, const double* wv,
                                               const unsigned short* hit, int tid, double& accl, double& accu) {
#pragma clang fp contract(fast)
  accl = 0; accu = 0;
  bool bad = false;
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
      if (ok) best = fmin(best, (ne * ne * ne) / qp);            // prod_y s_y = prod_y ne / q_y
    }
    if (best >= 1e300) bad = true;
    accu += det * fmax(best, 1.0);
  }
  return bad;
}
template <int NB>
__device__ __forceinline__ void hiv_bounds_wave(const double* __restrict__ hs, int M, const float* __restrict__ verts,
                                                const int* __restrict__ faces, int R, int F, double* wv, unsigned short* hit, int lane,
                                                double& lb, double& ub, int kdone = 0, const unsigned short* hitDone = nullptr) {
  // kdone != 0: the caller has just evaluated a coarser mesh whose kdone directions are the first kdone of this one (k_refine_mesh
  // keeps the parent's vertices in front), over the same planes: wv[0 .. 3 kdone) holds their boundary points already (the same
  // arithmetic on the same operands: bit for bit what this loop would store) and hitDone their planes, which only move to this mesh's
  // table -- a quarter of the once-refined mesh's directions is not cast twice
  if (kdone) {
    for (int k = lane; k < kdone; k += 64) hit[k] = hitDone[k];
    __syncthreads();                                            // hitDone lies where wv[3 kdone ..) is about to be written
  }
  hiv_raycast<64, NB>(hs, M, verts, R, kdone, wv, hit, lane);
  __syncthreads();
  double accl, accu;
  bool bad = hiv_bound_sums<64>(hs, faces, F, wv, hit, lane, accl, accu);
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
  hiv_raycast<64 * NW, NB>(hs, M, verts, R, 0, wv, hit, tid);
  __syncthreads();
  double accl, accu;
  const bool bad = hiv_bound_sums<64 * NW>(hs, faces, F, wv, hit, tid, accl, accu);
  for (int o = 32; o; o >>= 1) { accl += __shfl_xor(accl, o); accu += __shfl_xor(accu, o); }
  if ((tid & 63) == 0) { red[2 * (tid >> 6)] = accl; red[2 * (tid >> 6) + 1] = accu; }
  const bool anybad = __syncthreads_or(bad ? 1 : 0) != 0;
  accl = 0; accu = 0;
#pragma unroll
  for (int w_ = 0; w_ < NW; ++w_) { accl += red[2 * w_]; accu += red[2 * w_ + 1]; }
  __syncthreads();
  lb = accl / 6.0;
  ub = anybad ? 1e300 : accu / 6.0;
}

}  // namespace
