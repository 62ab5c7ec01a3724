// Decision shortcut of the 2D NMS: the exact area of P n Q plus / minus a BAND for what the reference's Clipper call can return instead
// ("area enclosure" in the names below; the band is validated empirically and adversarially, it is NOT a theorem about Clipper -- see the
// end of this comment and DESIGN.md 3.4; sd_set_option("nms2d_strict", 1) sends every pair to the Clipper-exact sweep instead).
//
// The reference decides  area_inter / min(area_i, area_j) > thr  (stardist2d.cpp:580-581) with area_inter from ClipperLib
// (poly_intersection_area :152-165).  Clipper's result is the intersection of the two integer polygons with every CROSSING
// POINT of their boundaries rounded to the lattice (clipper.cpp IntersectPoint: Round()), all other output vertices are input
// vertices.  The scan-beam sweep that reproduces it bit for bit (clip_beam.h) is a divergent per-lane state machine; most
// pairs of an NMS, however, are far from the threshold (candidates of one object overlap almost completely, those of
// neighbouring objects hardly at all).  For those this header computes
//   A  = the exact area of P n Q (up to float rounding), by integrating x dy - y dx along the boundary of the intersection:
//        dP inside Q plus dQ inside P.  An edge e = (a -> b) of P contributes cross(a, b) * lambda_e, lambda_e = the part of e
//        inside Q = [a inside Q] + sum over the crossings of e with dQ of  +-(1 - t)  (t: parameter of the crossing on e, + when
//        e enters Q).  All predicates (which edges cross, which vertex is inside) are evaluated EXACTLY on small integers
//        (coordinates relative to the pair, products below 2^24 held in floats), with a symbolic perturbation of Q by
//        (eps, eps^2) so that touching vertices, collinear edges and shared boundaries need no special cases: the perturbed
//        configuration is generic, and its area differs from the given one by O(eps).  n^2 edge pairs, no data-dependent control
//        flow: 32 lanes per pair, lane = edge of P, loop over the edges of Q.  What belongs to Q's edge alone is computed once per
//        pair, by the lane of that index, and kept as a per-edge RECORD in LDS (3 x 32 float4 per half-wave, 12 KB per block of four
//        waves; only the half-wave that wrote a record reads it, and a wave's LDS accesses are processed in order, so a wave barrier
//        orders them); the loop reads it with broadcast reads one edge ahead (pair_enclosure below).
//   K  = the number of boundary crossings, T = the number of edge pairs (e of P, f of Q) whose bounding boxes come within one lattice
//        step of each other, and the band
//        B = (0.5 K + max(NEAR_W T, STRIP_W S)) (lmax_P + lmax_Q) + 0.75 + (float error term),   NEAR_W = 0.15, STRIP_W = 0.45 (round 5:
//        0.125 T alone), S = the number of STRIPS = edges with at least one near partner (the larger of the two polygons' counts).
//        Three mechanisms separate Clipper's area from A.  (1) It rounds each of the K crossing points to the lattice: moving one vertex
//        of a polygon by delta changes its area by |delta x (v_next - v_prev)| / 2 <= 0.71 (|e| + |f|) / 2 -- at most 0.36 (lmax_P +
//        lmax_Q) per crossing (PROVEN for a crossing that is not clamped to its scan beam; the band carries 0.5).  (2) It orders the
//        active edges by their lattice-ROUNDED abscissae at the scan lines: two edges that run closer than one step without crossing can
//        tie, be inserted in the wrong order and later be "uncrossed", which moves the strip between them -- at most one step wide and
//        as long as the shorter edge -- to the wrong side (K = 0 pairs with a deviation of 0.5 exist: tests/test_cpu_area_enclosure.py);
//        along nearly coincident boundaries every edge is near about three edges of the other polygon, so T counts each such strip
//        about three times (measured on bench-like pairs: T / S = 2.7 .. 3.7): NEAR_W T charges a strip about 0.45 there, but charged the
//        ISOLATED near pairs of polygons with few long edges a third of that -- exactly the regime in which the round-5 adversary found its
//        smallest margins (0.53 of the band on K = 0, T = 3 pairs).  Round 6 charges every strip STRIP_W = 0.45 whatever the count splits
//        into, and raised NEAR_W from 0.125 to 0.15: both changes are monotone (the band only grows: pairs only LEAVE the shortcut for
//        the exact sweep, earlier evidence stays valid); the weights are EMPIRICAL.  (3) A polygon whose OWN vertex lies within half a step of one of its own edges
//        is re-ordered by Clipper on its own (found by the adversarial search of round 5): such polygons are not "robustly simple"
//        (poly_pass.h props_pair) and are never decided here.
//        Evidence for the band: 2.0 x 10^9 GPU pairs of eleven families against the exact sweep (round 6; worst 0.25 B), 18 M CPU pairs against the
//        vendored Clipper (0.27 B), and an annealing ADVERSARY linked to the vendored Clipper (test infrastructure, DESIGN.md 3.4:
//        4.8 x 10^9 evaluations over NMS-realisable (worst 0.42 B) and free integer polygons (worst 0.53 B); profiles/r05_area_band_adversary.txt).
// A pair is decided when (A -+ B) / min(area) clears the threshold by the margins below; everything else -- and every pair with
// a polygon that is not ROBUSTLY SIMPLE (the boundary integral weights regions by winding number, Clipper's NonZero rule does not), with
// polygons of opposite orientation, too large for exact float predicates, or whose reference result could be rounded by the
// float accumulation of area_from_path (:128-138) -- goes to the exact sweep as before.  Decisions, not areas, leave this header.
#pragma once
#include <hip/hip_runtime.h>

namespace sdarea {

enum { PP_PLAIN = 1, PP_POS = 2, PP_NEG = 4 };
struct PolyProps { float lmax, perim; int flags; int xmin, xmax, ymin, ymax; int pad; };   // integer bounding box of the vertices

__device__ __forceinline__ float sgnf(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }
__device__ __forceinline__ float half_sum(float v) { for (int o = 16; o; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ __forceinline__ float half_max(float v) { for (int o = 16; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o)); return v; }
__device__ __forceinline__ int half_sum_i(int v) { for (int o = 16; o; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ __forceinline__ int half_min_i(int v) { for (int o = 16; o; o >>= 1) { const int t = __shfl_xor(v, o); v = t < v ? t : v; } return v; }
__device__ __forceinline__ int half_max_i(int v) { for (int o = 16; o; o >>= 1) { const int t = __shfl_xor(v, o); v = t > v ? t : v; } return v; }

constexpr float NEAR_W = 0.15f, STRIP_W = 0.45f;   // band weights of an edge pair within one lattice step / of a strip (mechanism 2); the numpy statement under tests/ and the adversarial search tool of the test infrastructure carry the same values
constexpr int WINDOW = 2047;        // largest |relative coordinate| for which every predicate's products stay below 2^24

// The per-polygon record PolyProps -- longest edge, L1 perimeter, orientation, integer bounding box and whether the polygon is ROBUSTLY
// SIMPLE once zero-length edges are dropped (no two edges share a point except cyclic neighbours at their common vertex, no fold-back
// between neighbours, at least three edges, and no vertex within half a lattice step (along its scan line) of an edge it does not end) --
// is written by the build phase's per-polygon pass (poly_pass.h props_pair).

struct Enclosure { float area, band; int crossings, near; bool usable; };

// What one lane brings to a pair: lane l's vertex of each polygon (zero where l >= R or the half-wave is idle) and ONE word of the two
// polygons' records -- lanes 0..7 hold the eight words of P's PolyProps, lanes 8..15 those of Q's.  pair_enclosure hands the words round
// the half-wave where it needs them, before and after its edge loop, so that nothing of the two records occupies registers across
// the loop (sixteen registers per lane otherwise: one wave per SIMD less).
struct PairOperands { int word, px, py, qx, qy; };
__device__ __forceinline__ PairOperands load_operands(const int* __restrict__ px, const int* __restrict__ py, const int* __restrict__ qx,
                                                      const int* __restrict__ qy, const PolyProps* __restrict__ pp, const PolyProps* __restrict__ pq,
                                                      bool live, int l) {
  static_assert(sizeof(PolyProps) == 32, "eight words per record");
  PairOperands o;
  o.word = 0;
  if (l < 16) o.word = (l < 8 ? (const int*)pp : (const int*)pq)[l & 7];
  o.px = o.py = o.qx = o.qy = 0;
  if (live) { o.px = px[l]; o.py = py[l]; o.qx = qx[l]; o.qy = qy[l]; }
  return o;
}
__device__ __forceinline__ PolyProps props_from_lanes(int word, int first) {     // the record whose words lanes first .. first + 7 hold
  PolyProps p;
  p.lmax = __int_as_float(__shfl(word, first)); p.perim = __int_as_float(__shfl(word, first + 1)); p.flags = __shfl(word, first + 2);
  p.xmin = __shfl(word, first + 3); p.xmax = __shfl(word, first + 4); p.ymin = __shfl(word, first + 5); p.ymax = __shfl(word, first + 6);
  p.pad = 0;
  return p;
}

// Lane masks: a predicate of all 64 lanes as one wave-uniform 64-bit value (bit = lane; the lower word is the lower half-wave's pair).
// Boolean algebra on them and the parities of their halves run on the scalar unit, next to the vector arithmetic of another wave.
typedef unsigned long long lanemask;
__device__ __forceinline__ lanemask lanes_where(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ bool my_lane(lanemask m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
__device__ __forceinline__ unsigned int lower(lanemask m) { return (unsigned int)m; }
__device__ __forceinline__ unsigned int upper(lanemask m) { return (unsigned int)(m >> 32); }
// a b - c d + h for integer-valued a .. d with products below 2^22 and h = +-0.5: every intermediate is a multiple of 0.5 below 2^23, exact
__device__ __forceinline__ float cross_plus(float a, float b, float c, float d, float h) { return __fmaf_rn(a, b, __fmaf_rn(-c, d, h)); }
__device__ __forceinline__ int half_or_i(int v) { for (int o = 16; o; o >>= 1) v |= __shfl_xor(v, o); return v; }

enum { REC_ROWS = 3, REC_FLOAT4 = REC_ROWS * 32 };   // LDS of one half-wave: three rows of 32 float4, one column per edge of Q

// The 32 lanes of one half-wave evaluate one pair: P (props o.pp, lane l holds vertex l in o.px, o.py) against Q (o.pq, o.qx, o.qy; Q is
// the perturbed one).  rec: REC_FLOAT4 float4 of LDS private to this half-wave.  `active`: uniform within the half (an idle half still
// takes part in the wave-wide operations).  Every lane of the half returns the same values.
//
// Lane l first writes the RECORD of Q's edge f_l = (c -> d) -- everything the loop needs that belongs to f alone -- into column l:
//   row 0  c.x, c.y, d.x, d.y
//   row 1  f.x, f.y, cross(c, d), h_f      h_f = +0.5 where tie_f_pos, else -0.5
//   row 2  min / max of the edge's x, min / max of its y (its box); an EMPTY box (+inf, -inf) for a zero-length edge, which is near nothing
// The loop over the edges of Q reads column k with three broadcast reads (one address per half); the reads of column k + 1 are issued
// before column k is used.
//
// Sides.  An orientation o is an exact integer below 2^23 and "positive side" means  o > 0 || (o == 0 && tie):  that is  o + h > 0  with
// h = +-0.5 by the tie, and o + h is exact too.  The loop computes o + h directly (cross_plus) and recovers o = (o + h) - h only for a crossing,
// so a side costs one compare and no mask algebra.  Zero-length edges need no flag either: f = 0 puts a and b on the same side of f
// (both o_f + h_f = h_f) and makes c.y == d.y; e = 0 (also forced in lanes without a vertex) does the same for c, d and for a.y, b.y:
// no crossing, no hit of either ray.
//
// What is one bit per lane and carried between iterations -- sides, parities -- lives in lane masks.  The edge pairs within one lattice
// step are kept as one word per lane (bit k: my edge is near f_k); K, T and the two strip counts come from it after the loop.
__device__ __forceinline__ Enclosure pair_enclosure(const PairOperands& o, int R, bool active, float4* rec, int l, int half) {
  const int hb = half << 5;
  Enclosure E; E.area = 0.f; E.band = 0.f; E.crossings = 0; E.near = 0; E.usable = false;
  const PolyProps pp0 = props_from_lanes(o.word, hb), pq0 = props_from_lanes(o.word, hb + 8);
  bool use = active && (pp0.flags & PP_PLAIN) && (pq0.flags & PP_PLAIN) && ((pp0.flags & (PP_POS | PP_NEG)) == (pq0.flags & (PP_POS | PP_NEG)));
  // origin: the centre of P's box; both polygons within the window
  const int ox = use ? (int)(((long long)pp0.xmin + pp0.xmax) >> 1) : 0, oy = use ? (int)(((long long)pp0.ymin + pp0.ymax) >> 1) : 0;
  long long ext = 0;
  if (use) {
    const long long e0 = (long long)pp0.xmax - ox, e1 = (long long)ox - pp0.xmin, e2 = (long long)pp0.ymax - oy, e3 = (long long)oy - pp0.ymin;
    const long long e4 = (long long)pq0.xmax - ox, e5 = (long long)ox - pq0.xmin, e6 = (long long)pq0.ymax - oy, e7 = (long long)oy - pq0.ymin;
    ext = e0; ext = e1 > ext ? e1 : ext; ext = e2 > ext ? e2 : ext; ext = e3 > ext ? e3 : ext;
    ext = e4 > ext ? e4 : ext; ext = e5 > ext ? e5 : ext; ext = e6 > ext ? e6 : ext; ext = e7 > ext ? e7 : ext;
    if (ext > WINDOW / 2) use = false;              // differences of relative coordinates <= WINDOW: products < 2^22, sums of two < 2^24
  }
  const float extf = (float)ext;
  const bool sPpos = (pp0.flags & PP_POS) != 0, sQpos = (pq0.flags & PP_POS) != 0;
  const bool lv = use && l < R;
  float ax = 0.f, ay = 0.f, cqx = 0.f, cqy = 0.f;
  if (lv) { ax = (float)(o.px - ox); ay = (float)(o.py - oy); cqx = (float)(o.qx - ox); cqy = (float)(o.qy - oy); }
  const int ln = (l + 1 >= R) ? 0 : l + 1;
  const float bxs = __shfl(ax, hb + ln), bys = __shfl(ay, hb + ln);
  const float bx = lv ? bxs : ax, by = lv ? bys : ay;                          // (a lane without a vertex holds a zero-length edge)
  const float INF = __builtin_huge_valf();
  {                                                 // the record of Q's edge l
    const float dqx = __shfl(cqx, hb + ln), dqy = __shfl(cqy, hb + ln);
    const float fx = dqx - cqx, fy = dqy - cqy;
    const bool okf = use & ((fx != 0.f) | (fy != 0.f));
    const bool tie_f_pos = fy != 0.f ? fy > 0.f : fx < 0.f;
    rec[l] = make_float4(cqx, cqy, dqx, dqy);
    rec[32 + l] = make_float4(fx, fy, cqx * dqy - cqy * dqx, tie_f_pos ? 0.5f : -0.5f);
    rec[64 + l] = okf ? make_float4(fminf(cqx, dqx), fmaxf(cqx, dqx), fminf(cqy, dqy), fmaxf(cqy, dqy)) : make_float4(INF, -INF, INF, -INF);
  }
  __builtin_amdgcn_wave_barrier();                  // (a wave's LDS accesses are processed in order)
  const float ex = bx - ax, ey = by - ay;
  const bool oke = lv && (ex != 0.f || ey != 0.f);
  // a zero orientation takes the sign of the perturbation term:
  //   Q's vertex against my edge e:      cross(e, (eps, eps^2)) > 0  <=>  ey != 0 ? ey < 0 : ex > 0     (tie_e_pos)
  //   my vertex against Q's edge f:     -cross(f, (eps, eps^2)) > 0  <=>  fy != 0 ? fy > 0 : fx < 0     (tie_f_pos)
  const float h_e = (ey != 0.f ? ey < 0.f : ex > 0.f) ? 0.5f : -0.5f;
  const lanemask m_e_up = lanes_where(by > ay), m_sP = lanes_where(sPpos), m_sQ = lanes_where(sQpos);
  // my edge's box, one lattice step wider; empty for a zero-length edge
  const float exlo = oke ? fminf(ax, bx) - 1.f : INF, exhi = oke ? fmaxf(ax, bx) + 1.f : -INF;
  const float eylo = oke ? fminf(ay, by) - 1.f : INF, eyhi = oke ? fmaxf(ay, by) + 1.f : -INF;
  const float cab = ax * by - ay * bx;
  float accP = 0.f, accQ = 0.f;
  int K = 0;
  unsigned int nearbits = 0;                        // bit k: my edge and f_k are closer than one lattice step (bounding boxes)
  lanemask m_parA = 0;                              // a inside Q: parity of the hits of the ray towards +x
  float4 q0 = rec[0], q1 = rec[32], q2 = rec[64];
  // carried from one edge of Q to the next, whose c is this one's d: c - a, c's orientation against e (+ h_e) and side, c.y below a.y / b.y
  float dcx = q0.x - ax, dcy = q0.y - ay;
  float o_ec = cross_plus(ex, dcy, ey, dcx, h_e);
  lanemask m_pos_c = lanes_where(o_ec > 0.f), m_c_lt_a = lanes_where(q0.y < ay), m_c_lt_b = lanes_where(q0.y < by);
  const int Rw = __any(use) ? R : 0;                // (`use` is uniform within a half; the masks in the loop are wave-wide)
  // one edge f_k of Q, its record in (q0, q1, q2); requests the record of the next edge into (n0, n1, n2)
  auto edge = [&](int k, const float4& q0, const float4& q1, const float4& q2, float4& n0, float4& n1, float4& n2) {
    const int kn = (k + 1 >= R) ? 0 : k + 1;
    n0 = rec[kn]; n1 = rec[32 + kn]; n2 = rec[64 + kn];                     // in flight while this edge is worked on
    const float fx = q1.x, fy = q1.y, ccd = q1.z, h_f = q1.w;
    const float ddx = q0.z - ax, ddy = q0.w - ay;
    const float o_ed = cross_plus(ex, ddy, ey, ddx, h_e);                   // ex (d.y - ay) - ey (d.x - ax)
    const float o_fa = cross_plus(fy, dcx, fx, dcy, h_f);                   // fx (ay - c.y) - fy (ax - c.x)
    const float o_fb = o_fa + __fmaf_rn(fx, ey, -(fy * ex));                // fx (by - c.y) - fy (bx - c.x) = the above + cross(f, e)
    const lanemask m_pos_d = lanes_where(o_ed > 0.f), m_pos_a = lanes_where(o_fa > 0.f), m_pos_b = lanes_where(o_fb > 0.f);
    const bool nearb = (q2.x <= exhi) & (q2.y >= exlo) & (q2.z <= eyhi) & (q2.w >= eylo);
    nearbits |= nearb ? 1u << k : 0u;
    if (my_lane((m_pos_c ^ m_pos_d) & (m_pos_a ^ m_pos_b))) {                                 // e and f cross
      const float r_f = o_fa - h_f, r_c = o_ec - h_e;                                         // the orientations themselves; differences as before
      const float t = r_f * __builtin_amdgcn_rcpf(o_fa - o_fb), u = r_c * __builtin_amdgcn_rcpf(o_ec - o_ed);   // (1 ulp: far inside the band)
      const float wt = 1.f - t, wu = 1.f - u;
      accP += my_lane(~(m_pos_b ^ m_sQ)) ? wt : -wt;                                          // e enters Q: + (1 - t)
      accQ += ccd * (my_lane(~(m_pos_d ^ m_sP)) ? wu : -wu);
      ++K;
    }
    const lanemask m_d_lt_a = lanes_where(q0.w < ay), m_d_lt_b = lanes_where(q0.w < by);
    m_parA ^= (m_c_lt_a ^ m_d_lt_a) & ~(m_pos_a ^ lanes_where(fy > 0.f));                     // f straddles a.y and a is on its inner side
    const lanemask m_hit = (m_c_lt_a ^ m_c_lt_b) & ~(m_pos_c ^ m_e_up);                       // c inside P: (ay <= c.y) != (by <= c.y), pos_c == e_up
    const lanemask m_odd = (lanemask)(__popc(lower(m_hit)) & 1) | ((lanemask)(__popc(upper(m_hit)) & 1) << 32);   // lane 0 of a half with an odd count
    if (my_lane(m_odd)) accQ += ccd;
    dcx = ddx; dcy = ddy; o_ec = o_ed; m_pos_c = m_pos_d; m_c_lt_a = m_d_lt_a; m_c_lt_b = m_d_lt_b;
  };
  float4 p0, p1, p2;
  int k = 0;
  for (; k + 1 < Rw; k += 2) {                      // two edges per trip: the records alternate between two register sets
    edge(k, q0, q1, q2, p0, p1, p2);
    edge(k + 1, p0, p1, p2, q0, q1, q2);
  }
  if (k < Rw) edge(k, q0, q1, q2, p0, p1, p2);
  const float contrib = lv ? cab * ((my_lane(m_parA) ? 1.f : 0.f) + accP) + accQ : 0.f;
  const float tot = half_sum(contrib);
  // the band and the usability test take the two records from the lanes once more: nothing of them stays in registers across the loop
  const PolyProps pp = props_from_lanes(o.word, hb), pq = props_from_lanes(o.word, hb + 8);
  const float lsum = pp.lmax + pq.lmax, fterm = 2e-6f * extf * (pp.perim + pq.perim);
  const double psum = (double)pp.perim + (double)pq.perim;
  long long MM = 0;
  {
    const long long a0 = pp.xmin < 0 ? -(long long)pp.xmin : pp.xmin, a1 = pp.xmax < 0 ? -(long long)pp.xmax : pp.xmax;
    const long long a2 = pp.ymin < 0 ? -(long long)pp.ymin : pp.ymin, a3 = pp.ymax < 0 ? -(long long)pp.ymax : pp.ymax;
    const long long b0 = pq.xmin < 0 ? -(long long)pq.xmin : pq.xmin, b1 = pq.xmax < 0 ? -(long long)pq.xmax : pq.xmax;
    const long long b2 = pq.ymin < 0 ? -(long long)pq.ymin : pq.ymin, b3 = pq.ymax < 0 ? -(long long)pq.ymax : pq.ymax;
    long long M = (a0 > a1 ? a0 : a1); M = b0 > M ? b0 : M; M = b1 > M ? b1 : M;
    long long My = (a2 > a3 ? a2 : a3); My = b2 > My ? b2 : My; My = b3 > My ? b3 : My;
    MM = M + My + 2;
  }
  // (a lane without a vertex holds a zero-length edge: it crosses nothing and is near nothing)
  const int Kt = half_sum_i(K), Tt = half_sum_i(__popc(nearbits)), SPt = half_sum_i(nearbits != 0u ? 1 : 0), SQ = __popc((unsigned int)half_or_i((int)nearbits));
  const int St = SPt > SQ ? SPt : SQ;              // strips: edges with at least one near partner, the larger of the two polygons' counts
  E.area = 0.5f * fabsf(tot);
  E.crossings = Kt; E.near = Tt;
  // float error of the sum: <= 64 terms of magnitude <= ext * edge length, each with a few ulps
  E.band = (0.5f * (float)Kt + fmaxf(NEAR_W * (float)Tt, STRIP_W * (float)St)) * lsum + 0.75f + fterm;
  // area_from_path adds integer cross products in float: exact while the sum of their magnitudes stays below 2^24
  // (|p_i x p_{i+1}| <= |p_i| |p_{i+1} - p_i|; the output's edges are parts of the inputs' edges, crossing points moved by < 1.5)
  if (use) {
    const double bound = (double)MM * (psum + 3.0 * Kt + 4.0);
    if (!(bound < 16777216.0)) use = false;
  }
  E.usable = use;
  return E;
}

// thresholds of a decision: 1 = certainly not above thr (pair kept), 2 = certainly above (j suppressed), 0 = undecided
__device__ __forceinline__ int decide(const Enclosure& E, float area_i, float area_j, float thr) {
  if (!E.usable) return 0;
  const double amin = fmin((double)area_i + 1.e-10, (double)area_j + 1.e-10);                // :580
  if (!(amin > 0.25)) return 0;
  const double lo = ((double)E.area - (double)E.band) / amin, hi = ((double)E.area + (double)E.band) / amin;
  const double m = 4e-6 * fabs((double)thr) + 1e-6;                                            // float rounding of the quotient and of the comparison
  if (lo > (double)thr + m) return 2;
  if (hi < (double)thr - m) return 1;
  return 0;
}

}  // namespace sdarea
