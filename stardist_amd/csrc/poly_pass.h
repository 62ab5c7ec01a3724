// poly_pass.h -- the per-candidate work of the 2D NMS's build phase for n_rays <= 32 in ONE pass over the integer rings: the polygon
// properties of the decision shortcut (area_bounds.h PolyProps) and the prepared polygon of the bound-slot sweep (clip_beam.h
// PolyPrep<32>, Clipper::AddPath once per candidate).  Both records are byte for byte what the two separate kernels this pass replaces
// wrote (tests/test_gpu_beam_prep.py, tests/test_gpu_poly_pass.py).
//
// One wave per workgroup, 64 candidates per wave.
//   * STAGING + PROPERTIES: 32 steps of two candidates, half a wave per candidate (lane = input vertex, as the properties were always
//     computed: the same shuffles, the same xor-butterfly order of the float reductions).  Each step loads the two rings once (coalesced),
//     evaluates the properties and parks the ring in LDS for the preparation.  The robust-simplicity loop visits every unordered pair of
//     edges {l, l + dd}; a step dd is skipped wave-uniformly when no lane's two edges come within one lattice step of each other (bounding
//     boxes) and no lane meets its non-degenerate ring neighbour -- then every test of the step is false (see props_pair).
//   * PREPARATION: one thread per candidate, the order-dependent AddPath restated from PrepWork::prepare with a small working set: the
//     ring as 16-bit coordinates relative to vertex 0 packed into one LDS word per vertex (8 KB per wave, conflict-free lane-interleaved
//     layout), the doubly linked list of the cleanup as a 32-bit mask of the surviving input vertices (the list is always the surviving
//     vertices in cyclic index order, so next / previous are bit scans), the edge codes as three 32-bit masks and the local-minima list in
//     registers.  PrepWork<LdsStorage<64>, 32> took 30 KB of LDS per wave (1.25 waves per SIMD) and walked its list through LDS.  A ring
//     that does not fit 16-bit offsets runs PrepWork itself from private memory.
#pragma once
#include "clip_sweep.h"
#include "clip_beam.h"

namespace sdpass {

typedef long long i64;
constexpr int PASS_T = 64;                         // threads (= candidates) per workgroup
constexpr int PASS_V = 32;                         // vertex capacity

SD_HD int px_(int p) { return (int)(short)(p & 0xffff); }
SD_HD int py_(int p) { return p >> 16; }
SD_HD int pack_(int x, int y) { return (int)(((unsigned)y << 16) | ((unsigned)x & 0xffffu)); }

// Clipper::AddPath (clipper.cpp:1045-1221) for one ring of n_in <= 32 vertices, held in LDS at ring[i * PASS_T] as (x - x0, y - y0)
// packed by pack_; (x0, y0) = vertex 0.  Statement for statement PrepWork::prepare (clip_beam.h), same record.
struct FastPrep {
  const int* ring;
  int n;
  unsigned swm, l1m, l2m;                          // per compact edge: code bit 2 (Bot is vertex e+1), NextInLML = ring-next / ring-prev

  SD_HD int P(int i) const { return ring[i * PASS_T]; }
  SD_HD int cx(int i) const { return px_(P(i)); }
  SD_HD int cy(int i) const { return py_(P(i)); }
  SD_HD int nx(int e) const { return e + 1 == n ? 0 : e + 1; }
  SD_HD int pv(int e) const { return e == 0 ? n - 1 : e - 1; }
  SD_HD bool sw(int e) const { return (swm >> e) & 1u; }
  SD_HD int lmlc(int e) const { return ((l1m >> e) & 1u) ? 1 : (((l2m >> e) & 1u) ? 2 : 0); }
  SD_HD int botx(int e) const { return sw(e) ? cx(nx(e)) : cx(e); }
  SD_HD int boty(int e) const { return sw(e) ? cy(nx(e)) : cy(e); }
  SD_HD int topx(int e) const { return sw(e) ? cx(e) : cx(nx(e)); }
  SD_HD int topy(int e) const { return sw(e) ? cy(e) : cy(nx(e)); }
  SD_HD bool is_horz(int e) const { return cy(e) == cy(nx(e)); }
  SD_HD double dx(int e) const {                          // clipper.cpp:591-596 (differences: origin-free)
    const i64 dy = (i64)topy(e) - boty(e);
    if (dy == 0) return SD_HORIZONTAL;
    return (double)((i64)topx(e) - botx(e)) / (double)dy;
  }
  SD_HD void reverse_horizontal(int e) { swm ^= 1u << e; }
  SD_HD void set_lml(int e, int c) {
    const unsigned b = 1u << e;
    l1m = (l1m & ~b) | (c == 1 ? b : 0u); l2m = (l2m & ~b) | (c == 2 ? b : 0u);
  }

  SD_HD int find_next_loc_min(int E) const {                            // :911-925 (one exit flag, as PrepWork)
    bool done = false;
    int guard = 0;
    while (!done) {
      while (botx(E) != botx(pv(E)) || boty(E) != boty(pv(E)) || (cx(E) == topx(E) && cy(E) == topy(E))) E = nx(E);
      if (!is_horz(E) && !is_horz(pv(E))) done = true;
      else {
        while (is_horz(pv(E))) E = pv(E);
        const int E2 = E;
        while (is_horz(E)) E = nx(E);
        if (topy(E) != boty(pv(E))) {
          if (botx(pv(E2)) < botx(E)) E = E2;
          done = true;
        }
      }
      if (++guard > 4 * PASS_V) done = true;
    }
    return E;
  }
  SD_HD int process_bound(int E, bool fwd) {                            // :928-1042 (no skip edges)
    int Result = E, Horz;
    if (is_horz(E)) {
      int EStart = fwd ? pv(E) : nx(E);
      if (is_horz(EStart)) {
        if (botx(EStart) != botx(E) && topx(EStart) != botx(E)) reverse_horizontal(E);
      } else if (botx(EStart) != botx(E)) reverse_horizontal(E);
    }
    int EStart = E;
    if (fwd) {
      while (topy(Result) == boty(nx(Result))) Result = nx(Result);
      if (is_horz(Result)) {
        Horz = Result;
        while (is_horz(pv(Horz))) Horz = pv(Horz);
        if (topx(pv(Horz)) > topx(nx(Result))) Result = pv(Horz);
      }
      while (E != Result) {
        set_lml(E, 1);
        if (is_horz(E) && E != EStart && botx(E) != topx(pv(E))) reverse_horizontal(E);
        E = nx(E);
      }
      if (is_horz(E) && E != EStart && botx(E) != topx(pv(E))) reverse_horizontal(E);
      Result = nx(Result);
    } else {
      while (topy(Result) == boty(pv(Result))) Result = pv(Result);
      if (is_horz(Result)) {
        Horz = Result;
        while (is_horz(nx(Horz))) Horz = nx(Horz);
        if (topx(nx(Horz)) == topx(pv(Result)) || topx(nx(Horz)) > topx(pv(Result))) Result = nx(Horz);
      }
      while (E != Result) {
        set_lml(E, 2);
        if (is_horz(E) && E != EStart && botx(E) != topx(nx(E))) reverse_horizontal(E);
        E = pv(E);
      }
      if (is_horz(E) && E != EStart && botx(E) != topx(nx(E))) reverse_horizontal(E);
      Result = pv(Result);
    }
    return Result;
  }

  // ring: this thread's column of the LDS ring (written by the staging loop, compacted here in place); (ox, oy): vertex 0
  SD_HD void prepare(int* wring, int n_in, int ox, int oy, sdclip::PolyPrep<PASS_V>* out) {
    typedef sdclip::PolyPrep<PASS_V> Prep;
    ring = wring; n = 0; swm = l1m = l2m = 0u;
    int m = 0, n_lm = 0, st = 0;
    int highI = n_in - 1;
    const int p0 = P(0);
    while (highI > 0 && P(highI) == p0) --highI;
    while (highI > 0 && P(highI) == P(highI - 1)) --highI;
    if (highI >= 2) {
      // remove duplicate vertices and collinear edges (:1098-1122); the list = the surviving vertices in cyclic index order
      unsigned am = (highI >= 31) ? 0xffffffffu : ((2u << highI) - 1u);
      auto nxt = [&](int e) { const unsigned above = am & ~((2u << e) - 1u); return above ? __builtin_ctz(above) : __builtin_ctz(am); };
      auto prv = [&](int e) { const unsigned below = am & ((1u << e) - 1u); return below ? 31 - __builtin_clz(below) : 31 - __builtin_clz(am); };
      int eStart = 0, E = 0, eLoopStop = 0;
      for (;;) {
        const int en = nxt(E);
        const int pe = P(E), pn = P(en);
        if (pe == pn) {
          if (E == en) break;
          if (E == eStart) eStart = en;
          am &= ~(1u << E); E = en;
          eLoopStop = E;
          continue;
        }
        const int ep0 = prv(E);
        if (ep0 == en) break;
        const int pp = P(ep0);
        if (((i64)py_(pp) - py_(pe)) * ((i64)px_(pe) - px_(pn)) == ((i64)px_(pp) - px_(pe)) * ((i64)py_(pe) - py_(pn))) {   // SlopesEqual :554-563
          if (E == eStart) eStart = en;
          am &= ~(1u << E);
          E = ep0;
          eLoopStop = E;
          continue;
        }
        E = en;
        if (E == eLoopStop) break;
      }
      if (prv(E) != nxt(E)) {
        // compact the surviving ring in place (ring order = increasing input index; the traversal starts at the image of eStart)
        const int E0 = __builtin_popcount(am & ((1u << eStart) - 1u));
        for (int i = 0; i <= highI; ++i) {
          if (!((am >> i) & 1u)) continue;
          if (m != i) wring[m * PASS_T] = P(i);
          ++m;
        }
        n = m;
        bool isFlat = true;
        const int y0c = cy(0);
        for (int e = 0; e < m; ++e) {                                          // InitEdge2 :729-742
          const int en = nx(e);
          const int ye = cy(e), yn = cy(en);
          if (!(ye >= yn)) swm |= 1u << e;
          if (yn != y0c) isFlat = false;
        }
        if (isFlat) m = 0;
        else {
          E = E0;
          if (botx(pv(E)) == topx(pv(E)) && boty(pv(E)) == topy(pv(E))) E = nx(E);
          int EMin = -1, guard = 0;
          int lmy[sdclip::BEAM_MAXLM], lml[sdclip::BEAM_MAXLM], lmr[sdclip::BEAM_MAXLM];
#pragma unroll
          for (int i = 0; i < sdclip::BEAM_MAXLM; ++i) { lmy[i] = 0; lml[i] = 0; lmr[i] = 0; }
          for (;;) {
            E = find_next_loc_min(E);
            if (E == EMin) break;
            else if (EMin < 0) EMin = E;
            if (++guard > 2 * PASS_V + 2) { st |= sdclip::ST_ITER; break; }
            int left, right; bool leftFwd;
            if (dx(E) < dx(pv(E))) { left = pv(E); right = E; leftFwd = false; }
            else { left = E; right = pv(E); leftFwd = true; }
            const int y = boty(E);
            E = process_bound(left, leftFwd);
            const int E2 = process_bound(right, !leftFwd);
            if (n_lm < sdclip::BEAM_MAXLM) {
              // stable insertion by Y descending: the list is sorted, so the new entry goes behind every entry with Y >= y
              int k = 0;
#pragma unroll
              for (int i = 0; i < sdclip::BEAM_MAXLM; ++i) k += (i < n_lm && lmy[i] >= y) ? 1 : 0;
#pragma unroll
              for (int i = sdclip::BEAM_MAXLM - 1; i > 0; --i)
                if (i > k && i <= n_lm) { lmy[i] = lmy[i - 1]; lml[i] = lml[i - 1]; lmr[i] = lmr[i - 1]; }
#pragma unroll
              for (int i = 0; i < sdclip::BEAM_MAXLM; ++i)
                if (i == k) { lmy[i] = y; lml[i] = left; lmr[i] = right; }
              ++n_lm;
            } else st |= sdclip::ST_OVERFLOW_LM;
            if (!leftFwd) E = E2;
          }
          for (int i = 0; i < m; ++i) { const int p = P(i); out->v[i].x = px_(p) + ox; out->v[i].y = py_(p) + oy; }
          out->v[m].x = cx(0) + ox; out->v[m].y = cy(0) + oy;
          for (int i = 0; i < m; ++i) {
            const int c = lmlc(i);
            const int nl = (c == 1) ? nx(i) : (c == 2 ? pv(i) : -1);
            int cc = c | (sw(i) ? 4 : 0);
            if (nl >= 0 && is_horz(nl)) cc |= 8;
            out->ecode[i] = (unsigned char)cc;
            const int a = nx(i), b = pv(i);                                   // GetMaximaPair :2538-2545
            int mp = Prep::NONE;
            if (topx(a) == topx(i) && topy(a) == topy(i) && lmlc(a) == 0) mp = a;
            else if (topx(b) == topx(i) && topy(b) == topy(i) && lmlc(b) == 0) mp = b;
            out->mpair[i] = (typename Prep::pidx)mp;
            int last = i, g2 = 0;                                              // last horizontal of the run (:2519-2521)
            if (is_horz(i)) {
              for (;;) {
                const int c2 = lmlc(last);
                const int n2 = (c2 == 1) ? nx(last) : (c2 == 2 ? pv(last) : -1);
                if (n2 < 0 || !is_horz(n2)) break;
                last = n2;
                if (++g2 > PASS_V) { st |= sdclip::ST_ITER; break; }
              }
            }
            out->hlast[i] = (typename Prep::pidx)last;
          }
#pragma unroll
          for (int i = 0; i < sdclip::BEAM_MAXLM; ++i)
            if (i < n_lm) { out->lm_left[i] = (typename Prep::pidx)lml[i]; out->lm_right[i] = (typename Prep::pidx)lmr[i]; }
        }
      } else m = 0;
    }
    if (m == 0) { n_lm = 0; st = 0; }                                           // rejected path: the header only, all zero
    out->n = m; out->n_lm = n_lm; out->status = st; out->pad = 0;
  }
};

}  // namespace sdpass

// (the part above also compiles for the host: tests/host/poly_pass_lib.cpp checks FastPrep against PrepWork there)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "area_bounds.h"

namespace sdpass {

// The properties of the candidate of one half-wave (k_poly_props of earlier versions, unchanged arithmetic): X, Y = the lane's input
// vertex (valid: l < R of an existing candidate), sv = the half's 32-entry LDS ring.  Returns the record in every lane of the half.
__device__ __forceinline__ sdarea::PolyProps props_pair(int X, int Y, bool cv, bool valid, int R, int l, int half, float2* sv) {
  using namespace sdarea;
  const int hb = half << 5;
  const int x0 = __shfl(X, hb), y0 = __shfl(Y, hb);
  const int xmin = half_min_i(valid ? X : 0x7fffffff), xmax = half_max_i(valid ? X : (int)0x80000000);
  const int ymin = half_min_i(valid ? Y : 0x7fffffff), ymax = half_max_i(valid ? Y : (int)0x80000000);
  const bool small = cv && (long long)xmax - xmin <= WINDOW && (long long)ymax - ymin <= WINDOW;
  const int ln = (l + 1 >= R) ? 0 : l + 1;
  const int rx = valid && small ? X - x0 : 0, ry = valid && small ? Y - y0 : 0;           // |.| <= WINDOW
  const int rbx = __shfl(rx, hb + ln), rby = __shfl(ry, hb + ln);
  const float ax = (float)rx, ay = (float)ry, bx = (float)rbx, by = (float)rby;
  const float ex = bx - ax, ey = by - ay;
  const bool deg = !valid || (ex == 0.f && ey == 0.f);
  const unsigned long long bal = __ballot(!deg);
  const unsigned int m32 = (unsigned int)(half ? (bal >> 32) : bal);
  const int count = __popc(m32);
  auto next_of = [&](int e) {                       // the next edge of non-zero length after e
    int r = -1;
    if (m32) { const unsigned int above = (e >= 31) ? 0u : (m32 & ~((2u << e) - 1u)); r = above ? __ffs((int)above) - 1 : __ffs((int)m32) - 1; }
    return r;
  };
  const int nxt = next_of(l);
  const int area2 = half_sum_i(valid ? rx * rby - ry * rbx : 0);                            // exact: |terms| < 2^23, 32 of them
  bool bad = false;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // (the previous candidate's reads of sv come first)
  __builtin_amdgcn_wave_barrier();
  sv[l] = make_float2(ax, ay);
  __builtin_amdgcn_wave_barrier();                  // (a wave's LDS accesses are processed in order)
  // bounding box of my edge, one lattice step wider: every test below needs the two edges' boxes to meet
  const float exlo = fminf(ax, bx) - 1.f, exhi = fmaxf(ax, bx) + 1.f, eylo = fminf(ay, by) - 1.f, eyhi = fmaxf(ay, by) + 1.f;
  // every UNORDERED pair of edges {l, k} once: lane l meets k = l + dd (cyclically) for dd = 1 .. R / 2 and evaluates the symmetric
  // edge-against-edge test once and the vertex-against-edge rule in both directions
  for (int dd = 1; dd <= (R >> 1); ++dd) {
    int k = l + dd; if (k >= R) k -= R;
    if (!valid) k = 0;
    const int kn = (k + 1 >= R) ? 0 : k + 1;
    const float2 c2 = sv[k], d2 = sv[kn];
    const float cx = c2.x, cy = c2.y, dx = d2.x, dy = d2.y;
    const int nxt_k = next_of(k);
    const bool degk = ((m32 >> k) & 1u) == 0u;
    // a vertex-against-edge test can only fire when the vertex lies in the edge's box (its x within half a step of the edge's x range
    // means, for integers, within the range), the edge-against-edge test only when the boxes meet, the neighbour test only for
    // neighbours: when no lane of the wave has any of these, every test of this dd is false
    const bool boxes = (fminf(cx, dx) <= exhi) & (fmaxf(cx, dx) >= exlo) & (fminf(cy, dy) <= eyhi) & (fmaxf(cy, dy) >= eylo);
    if (!__any(valid && small && (boxes || k == nxt || nxt_k == l))) continue;
    const float fx = dx - cx, fy = dy - cy;
    //   my vertex a against edge k = (c -> d): within half a lattice step along its scan line (robust simplicity, area_bounds.h) ...
    if (valid && small && !degk && !((cx == ax && cy == ay) || (dx == ax && dy == ay)) && ay >= fminf(cy, dy) && ay <= fmaxf(cy, dy)) {
      if (fy == 0.f) { if (ax >= fminf(cx, dx) && ax <= fmaxf(cx, dx)) bad = true; }
      else if (2.f * fabsf((cx - ax) * fy + (ay - cy) * fx) <= fabsf(fy)) bad = true;            // |x_edge(ay) - ax| <= 1/2
    }
    //   ... and vertex c (the start of edge k) against my edge (a -> b)
    if (valid && small && !deg && !((ax == cx && ay == cy) || (bx == cx && by == cy)) && cy >= fminf(ay, by) && cy <= fmaxf(ay, by)) {
      if (ey == 0.f) { if (cx >= fminf(ax, bx) && cx <= fmaxf(ax, bx)) bad = true; }
      else if (2.f * fabsf((ax - cx) * ey + (cy - ay) * ex) <= fabsf(ey)) bad = true;
    }
    if (deg || degk || !valid) continue;
    if (k == nxt || nxt_k == l) {
      // cyclic neighbours: they share one vertex; anything more is a fold-back (when BOTH hold there are only two edges: count < 3)
      const float cr = ex * fy - ey * fx, dt = ex * fx + ey * fy;
      if (cr == 0.f && dt < 0.f) bad = true;
      continue;
    }
    const float o1 = ex * (cy - ay) - ey * (cx - ax), o2 = ex * (dy - ay) - ey * (dx - ax);
    const float o3 = fx * (ay - cy) - fy * (ax - cx), o4 = fx * (by - cy) - fy * (bx - cx);
    bool inter = (sgnf(o1) * sgnf(o2) <= 0.f) && (sgnf(o3) * sgnf(o4) <= 0.f);
    if (o1 == 0.f && o2 == 0.f)                     // collinear: overlap of the two intervals
      inter = fmaxf(fminf(ax, bx), fminf(cx, dx)) <= fminf(fmaxf(ax, bx), fmaxf(cx, dx)) &&
              fmaxf(fminf(ay, by), fminf(cy, dy)) <= fminf(fmaxf(ay, by), fmaxf(cy, dy));
    if (inter) bad = true;
  }
  const unsigned long long badm = __ballot(bad);
  const bool anybad = (unsigned int)(half ? (badm >> 32) : badm) != 0u;
  const float lmax = half_max(deg ? 0.f : sqrtf(ex * ex + ey * ey));
  const float perim = half_sum(deg ? 0.f : fabsf(ex) + fabsf(ey));
  PolyProps p;
  p.lmax = lmax * (1.f + 1e-6f); p.perim = perim;
  p.flags = ((small && !anybad && count >= 3 && area2 != 0) ? PP_PLAIN : 0) | (area2 > 0 ? PP_POS : 0) | (area2 < 0 ? PP_NEG : 0);
  p.xmin = xmin; p.xmax = xmax; p.ymin = ymin; p.ymax = ymax; p.pad = 0;
  return p;
}

// vx / vy: [n][R], R <= 32.  PROPS: write props[n]; PREP: write prep[n].
template <bool PROPS, bool PREP>
__global__ void __launch_bounds__(PASS_T) k_poly_pass(const int* __restrict__ vx, const int* __restrict__ vy, int n, int R,
                                                      sdarea::PolyProps* __restrict__ props, sdclip::PolyPrep<PASS_V>* __restrict__ prep) {
  __shared__ int ring[PREP ? PASS_V * PASS_T : 1];
  __shared__ float2 sv[2][32];
  const int lane = threadIdx.x, half = lane >> 5, l = lane & 31;
  const int base = blockIdx.x * PASS_T;
  int myx0 = 0, myy0 = 0;
  unsigned long long fitm = 0;                      // candidates whose ring fits 16-bit offsets from vertex 0 (staged in LDS)
  for (int p = 0; p < PASS_T / 2; ++p) {
    const int t = 2 * p + half;
    if (base + 2 * p >= n) break;                   // (uniform)
    const int cand = base + t;
    const bool cv = cand < n;                       // (uniform within a half)
    const bool valid = cv && l < R;
    int X = 0, Y = 0;
    if (valid) { X = vx[(size_t)cand * R + l]; Y = vy[(size_t)cand * R + l]; }
    if (PROPS) {
      const sdarea::PolyProps pr = props_pair(X, Y, cv, valid, R, l, half, sv[half]);
      if (cv && l == 0) props[cand] = pr;
    }
    if (PREP) {
      const int x0 = __shfl(X, half << 5), y0 = __shfl(Y, half << 5);
      const long long rx = (long long)X - x0, ry = (long long)Y - y0;
      const bool fits = rx >= -32768 && rx <= 32767 && ry >= -32768 && ry <= 32767;
      const unsigned long long nf = __ballot(valid && !fits);
      const bool hfit = cv && (unsigned int)(half ? (nf >> 32) : nf) == 0u;
      if (valid && hfit) ring[l * PASS_T + t] = pack_((int)rx, (int)ry);
      const unsigned long long fb = __ballot(hfit && l == 0);
      fitm |= ((fb & 1ull) << (2 * p)) | (((fb >> 32) & 1ull) << (2 * p + 1));
      const int x00 = __builtin_amdgcn_readlane(X, 0), y00 = __builtin_amdgcn_readlane(Y, 0);
      const int x01 = __builtin_amdgcn_readlane(X, 32), y01 = __builtin_amdgcn_readlane(Y, 32);
      if (lane == 2 * p) { myx0 = x00; myy0 = y00; }
      if (lane == 2 * p + 1) { myx0 = x01; myy0 = y01; }
    }
  }
  if (!PREP) return;
  __syncthreads();
  const int cand = base + lane;
  if (cand >= n) return;
  if ((fitm >> lane) & 1ull) {
    FastPrep w;
    w.prepare(ring + lane, R, myx0, myy0, prep + cand);
  } else {                                          // offsets beyond 16 bits: the 32-bit working set, in private memory
    sdclip::PrepWork<sdclip::PlainStorage, PASS_V> w;
    w.prepare(vx + (size_t)cand * R, vy + (size_t)cand * R, R, prep + cand);
  }
}

// props and / or prep may be nullptr (not written); 1 <= R <= 32 (props: 3 <= R)
inline int launch_poly_pass(const int* vx, const int* vy, int n, int R, sdarea::PolyProps* props, void* prep, hipStream_t s) {
  if (n <= 0 || (!props && !prep)) return 0;
  const dim3 grid((n + PASS_T - 1) / PASS_T), block(PASS_T);
  typedef sdclip::PolyPrep<PASS_V> Prep;
  if (props && prep) hipLaunchKernelGGL((k_poly_pass<true, true>), grid, block, 0, s, vx, vy, n, R, props, (Prep*)prep);
  else if (props) hipLaunchKernelGGL((k_poly_pass<true, false>), grid, block, 0, s, vx, vy, n, R, props, (Prep*)nullptr);
  else hipLaunchKernelGGL((k_poly_pass<false, true>), grid, block, 0, s, vx, vy, n, R, (sdarea::PolyProps*)nullptr, (Prep*)prep);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace sdpass
#endif
