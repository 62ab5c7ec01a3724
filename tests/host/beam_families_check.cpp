// tests/host/beam_families_check.cpp -- the bound-slot sweep (stardist_amd/csrc/clip_beam.h, compiled for the host) on pair families built to
// hit what its per-beam arithmetic depends on:
//   1 horizontals   edges that lie ON a scan line: runs of horizontals inside a bound, at a maximum, at a minimum, on a scan line of the other polygon
//   2 ties          edges with dy = 2m, dx = m * odd and vertices of the other polygon on their odd scan lines: dx * k / dy is an exact half-integer
//                   there (TopX rounds a tie), both signs, next to the bottom and next to the top of the edge
//   3 offsets       a vertex at +-32 766 ... +-32 769 (and far beyond) from the pair's origin: the 16-bit form holds it or flags the pair
//   4 random        3- to 32-gons, radii 1 - 150, noise 0.05 - 0.9 (as beam_check.cpp)
//   5 coincident    identical rings (same / rotated / reversed), rings touching in a vertex or along an edge, shifted by one
// Every pair is evaluated by the tier-1 form (K = 8, 16-bit coordinates through HostLds), the tier-2 form
// (K = 15), clip_sweep.h's Sweep and SweepFull, and -- unless built with -DNO_CLIPPER_REF -- the reference's Clipper (oracle/_ref).  No pair is
// left out: one that a tier flags for capacity must be held by the next one, with the same area.
// All coordinates come from std::mt19937's raw draws, a table of the 32 ray directions and single float operations: the same on every host.
//   main:  check FAMILY N SEED   |   golden N SEED OUT.f32   (Clipper's areas of the mixed set fam_generate(0, ...), for tests/golden)
//   C ABI (tests/test_gpu_beam_families.py): fam_generate, fam_host_probe
#include "../../stardist_amd/csrc/clip_sweep.h"
#include "../../stardist_amd/csrc/clip_sweep_full.h"
#include "../../stardist_amd/csrc/clip_beam.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#ifndef NO_CLIPPER_REF
extern "C" float clipper_ref_area(const int64_t*, const int64_t*, int, const int64_t*, const int64_t*, int);
#endif

namespace {
enum { R = 32 };
typedef sdclip::Sweep<128, 512, 128> SweepT;
typedef sdclip::SweepFull<32, 64, 32, 192, 64> SweepF;               // the general path of the device probe
typedef sdclip::PolyPrep<R> Prep;
typedef sdclip::LdsStorage<4> LdsP;
typedef sdclip::PrepWork<LdsP, R> PrepWL;
typedef sdclip::Beam<R, 8, 6, 4, sdclip::LdsStorage16<4>> BeamT1;             // tier 1: 16-bit coordinates, slopes recomputed
typedef sdclip::Beam<R, 15, 16, 8, LdsP> BeamT2;                             // tier 2
const int CAP = sdclip::ST_OVERFLOW_IL | sdclip::ST_OVERFLOW_REC | sdclip::ST_OVERFLOW_AEL | sdclip::ST_OVERFLOW_LM | sdclip::ST_OVERFLOW_GJ;

struct Rng {
  std::mt19937 g;
  explicit Rng(unsigned s) : g(s) {}
  unsigned raw() { return (unsigned)g(); }
  float u01() { return (float)(raw() >> 8) * (1.f / 16777216.f); }
  int below(int n) { return (int)(raw() % (unsigned)n); }
  int sign() { return (raw() & 1u) ? 1 : -1; }
};
const float kQuarter[9] = {1.f, 0.98078528f, 0.92387953f, 0.83146961f, 0.70710678f, 0.55557023f, 0.38268343f, 0.19509032f, 0.f};
float cos32(int k) { k &= 31; return k <= 8 ? kQuarter[k] : k <= 16 ? -kQuarter[16 - k] : k <= 24 ? -kQuarter[k - 16] : kQuarter[32 - k]; }
float sin32(int k) { return cos32(k - 8); }

struct Poly { int n; int x[R], y[R]; };
void star(Rng& r, int n, float radius, float noise, int cy, int cx, Poly& p) {
  p.n = n;
  for (int i = 0; i < n; ++i) {
    const int k = i * 32 / n;
    float d = radius * (1.f + noise * (2.f * r.u01() - 1.f));
    if (d < 1e-3f) d = 1e-3f;
    p.x[i] = (int)((float)cx + d * cos32(k)); p.y[i] = (int)((float)cy + d * sin32(k));
  }
}
void rect(int x0, int y0, int x1, int y1, Poly& p) { p.n = 4; p.x[0] = x0; p.y[0] = y0; p.x[1] = x1; p.y[1] = y0; p.x[2] = x1; p.y[2] = y1; p.x[3] = x0; p.y[3] = y1; }
void random_pair(Rng& r, float rmin, float rmax, Poly& a, Poly& b) {
  const float radius = rmin + (rmax - rmin) * r.u01() * r.u01();
  const float noise = 0.05f + 0.85f * r.u01();
  const int cy = 200 + r.below(20), cx = 200 + r.below(20);
  const float sep = r.u01() * 2.2f * radius;
  const int dir = r.below(32);
  const int cy2 = cy + (int)(sep * sin32(dir)), cx2 = cx + (int)(sep * cos32(dir));
  const float r2 = radius * (0.5f + r.u01());
  star(r, 3 + r.below(30), radius, noise, cy, cx, a);
  star(r, 3 + r.below(30), r2, noise, cy2, cx2, b);
}
void flatten(Rng& r, Poly& p, const Poly& other) {
  const int runs = 1 + r.below(3);
  for (int t = 0; t < runs; ++t) {
    const int k = r.below(p.n), len = 1 + r.below(3);
    int y = p.y[k];
    if (r.below(3) == 0) y = other.y[r.below(other.n)];                       // on a scan line of the other polygon
    for (int i = 0; i <= len; ++i) p.y[(k + i) % p.n] = y;
  }
  for (int ext = 0; ext < 2; ++ext) {
    if (r.below(2)) continue;
    int m = 0;
    for (int i = 1; i < p.n; ++i) if (ext ? p.y[i] > p.y[m] : p.y[i] < p.y[m]) m = i;
    p.y[(m + 1) % p.n] = p.y[m];                                               // a horizontal at the maximum / the minimum
    if (r.below(2)) p.y[(m + p.n - 1) % p.n] = p.y[m];
  }
}
void gen_pair(int family, Rng& r, Poly& a, Poly& b) {
  if (family == 0) family = 1 + r.below(5);
  if (family == 1) {
    random_pair(r, 3.f, 25.f, a, b);
    flatten(r, a, b); flatten(r, b, a);
  } else if (family == 2) {
    random_pair(r, 4.f, 30.f, a, b);
    Poly* p = r.below(2) ? &a : &b; Poly* q = (p == &a) ? &b : &a;
    const int k = r.below(p->n), k1 = (k + 1) % p->n;
    const int m = 1 + r.below(3), odd = 2 * r.below(4) + 1;
    const int dy = 2 * m * r.sign(), dx = m * odd * r.sign();
    p->x[k1] = p->x[k] + dx; p->y[k1] = p->y[k] + dy;
    const int s = dy > 0 ? 1 : -1;
    q->y[r.below(q->n)] = p->y[k] + s;                                         // the odd scan line next to one end ...
    q->y[r.below(q->n)] = p->y[k] + s * (2 * m - 1);                           // ... and next to the other
  } else if (family == 3) {
    random_pair(r, 5.f, 50.f, a, b);
    static const int D[12] = {32766, 32767, 32768, 32769, -32766, -32767, -32768, -32769, 40000, -40000, 70000, 20000};
    const int d = D[r.below(12)];
    Poly* p = r.below(2) ? &a : &b;
    const int k = (p == &a) ? 1 + r.below(p->n - 1) : r.below(p->n);          // (vertex 0 of A is the origin itself)
    if (r.below(2)) p->x[k] = a.x[0] + d; else p->y[k] = a.y[0] + d;
  } else if (family == 4) {
    static const float RMAX[6] = {2.f, 5.f, 12.f, 30.f, 80.f, 150.f};
    random_pair(r, 1.f, RMAX[r.below(6)], a, b);
  } else {
    const int v = r.below(9);
    if (v >= 6) {
      const int x0 = 50 + r.below(10), y0 = 50 + r.below(10), w = 1 + r.below(12), h = 1 + r.below(12), s = r.below(5) - 2;
      rect(x0, y0, x0 + w, y0 + h, a);
      if (v == 6) rect(x0 + w, y0 + s, x0 + w + 1 + r.below(8), y0 + h + s, b);       // along a vertical edge
      else if (v == 7) rect(x0 + s, y0 + h, x0 + w + s, y0 + h + 1 + r.below(8), b);  // along a horizontal edge
      else rect(x0 + w, y0 + h, x0 + w + 3, y0 + h + 3, b);                            // in one corner
    } else {
      Poly t; random_pair(r, 2.f, 30.f, a, t);
      b = a;
      int minx = a.x[0], maxx = a.x[0], miny = a.y[0], maxy = a.y[0];
      for (int i = 1; i < a.n; ++i) { if (a.x[i] < minx) minx = a.x[i]; if (a.x[i] > maxx) maxx = a.x[i]; if (a.y[i] < miny) miny = a.y[i]; if (a.y[i] > maxy) maxy = a.y[i]; }
      if (v == 1) { const int s = 1 + r.below(a.n - 1); for (int i = 0; i < a.n; ++i) { b.x[i] = a.x[(i + s) % a.n]; b.y[i] = a.y[(i + s) % a.n]; } }
      else if (v == 2) for (int i = 0; i < a.n; ++i) { b.x[i] = a.x[a.n - 1 - i]; b.y[i] = a.y[a.n - 1 - i]; }
      else if (v == 3) for (int i = 0; i < a.n; ++i) b.x[i] += maxx - minx;
      else if (v == 4) for (int i = 0; i < a.n; ++i) b.y[i] += maxy - miny;
      else if (v == 5) for (int i = 0; i < a.n; ++i) { b.x[i] += r.below(3) - 1; b.y[i] += r.below(3) - 1; }
    }
  }
}
void pad(const Poly& p, int32_t* x, int32_t* y) { for (int i = 0; i < R; ++i) { const int k = i < p.n ? i : p.n - 1; x[i] = p.x[k]; y[i] = p.y[k]; } }

// scan lines on which some edge's TopX is an exact tie: vertices' Ys strictly inside an edge's Y range with 2 * dx * k an odd multiple of dy
long count_ties(const int32_t* xa, const int32_t* ya, const int32_t* xb, const int32_t* yb) {
  long ties = 0;
  const int32_t* X[2] = {xa, xb}; const int32_t* Y[2] = {ya, yb};
  for (int p = 0; p < 2; ++p) for (int e = 0; e < R; ++e) {
    const long long x0 = X[p][e], y0 = Y[p][e], x1 = X[p][(e + 1) % R], y1 = Y[p][(e + 1) % R];
    const long long dy = y1 - y0, dx = x1 - x0;
    if (dy == 0) continue;
    for (int q = 0; q < 2; ++q) for (int v = 0; v < R; ++v) {
      const long long k = Y[q][v] - y0;
      if ((dy > 0) ? (k <= 0 || k >= dy) : (k >= 0 || k <= dy)) continue;
      const long long num = 2 * dx * k;
      if (num % dy == 0 && ((num / dy) & 1)) { ++ties; goto next_edge; }
    }
    next_edge:;
  }
  return ties;
}

struct Res { long long t; int st, nj; long long sabs; };      // sabs: sum of |cross terms| (the reference sums them in float: exact below 2^24)
alignas(64) char g_lds[1 << 16];
template <class BeamX> Res run_beam(const Prep* pa, const Prep* pb, long p) {
  static_assert(BeamX::lds_bytes() <= sizeof(g_lds), "host LDS buffer");
  sdclip::HostLds::base() = g_lds; sdclip::HostLds::tid() = (int)(p & 3);
  BeamX bm;
  bm.reset_state(pa, pb);
  Res r; r.t = bm.execute(); r.st = bm.status; r.nj = bm.n_joins; r.sabs = bm.sum_abs_terms;
  return r;
}
void prepare(const int32_t* xa, const int32_t* ya, const int32_t* xb, const int32_t* yb, long p, Prep* pa, Prep* pb) {
  static_assert(PrepWL::lds_bytes() <= sizeof(g_lds), "host LDS buffer");
  sdclip::HostLds::base() = g_lds; sdclip::HostLds::tid() = (int)(p & 3);
  PrepWL w;
  w.prepare(xa, ya, R, pa);
  w.prepare(xb, yb, R, pb);
}
Res run_full(const int32_t* xa, const int32_t* ya, const int32_t* xb, const int32_t* yb) {
  static SweepF sf;
  sf.reset_state();
  sf.add_path(xa, ya, R, sdclip::kClip, 0);
  sf.add_path(xb, yb, R, sdclip::kSubject, 32);
  Res r; r.t = sf.execute(); r.st = sf.status; r.nj = 0; r.sabs = 0;
  return r;
}
}  // namespace

// n pairs of `family` (0: every pair draws its own family, so neighbouring lanes differ) as R = 32 vertex arrays (short rings padded with
// their last vertex, which AddPath drops again)
extern "C" void fam_generate(int family, long n, unsigned seed, int32_t* xa, int32_t* ya, int32_t* xb, int32_t* yb) {
  Rng r(seed);
  Poly a, b;
  for (long p = 0; p < n; ++p) { gen_pair(family, r, a, b); pad(a, xa + p * R, ya + p * R); pad(b, xb + p * R, yb + p * R); }
}
// what the device probe sd_clip_pairs_device (tier 1) computes, on the host: prepare + tier-1 sweep; the general sweep when that flags a
// capacity or records joins.  flags as the probe's: status | 512 (bound-slot result) or | 256 (general path); joins: the tier-1 sweep recorded
// some; sabs: its sum of |cross terms| (the reference's float sum is exact below 2^24)
extern "C" void fam_host_probe(const int32_t* xa, const int32_t* ya, const int32_t* xb, const int32_t* yb, long n, int64_t* twice, int32_t* flags, int32_t* joins, int64_t* sabs) {
  static Prep pa, pb;
  for (long p = 0; p < n; ++p) {
    prepare(xa + p * R, ya + p * R, xb + p * R, yb + p * R, p, &pa, &pb);
    const Res b = run_beam<BeamT1>(&pa, &pb, p);
    long long t = b.t; int fl = b.st | 512;
    // (as k_probe; the NMS sends sum_abs_terms >= 2^24 on as well)
    if ((b.st & ~sdclip::ST_FAIL) != 0 || b.nj > 0) { const Res f = run_full(xa + p * R, ya + p * R, xb + p * R, yb + p * R); t = f.t; fl = f.st | 256; }
    twice[p] = t; flags[p] = fl; joins[p] = b.nj > 0; sabs[p] = b.sabs;
  }
}

#ifndef NO_CLIPPER_REF
static float ref_area(const int32_t* xa, const int32_t* ya, const int32_t* xb, const int32_t* yb) {
  int64_t v[4][R];
  for (int i = 0; i < R; ++i) { v[0][i] = xa[i]; v[1][i] = ya[i]; v[2][i] = xb[i]; v[3][i] = yb[i]; }
  return clipper_ref_area(v[0], v[1], R, v[2], v[3], R);
}
int main(int argc, char** argv) {
  if (argc < 5) { printf("usage: check FAMILY N SEED | golden N SEED OUT\n"); return 2; }
  if (!strcmp(argv[1], "golden")) {
    const long n = atol(argv[2]);
    std::vector<int32_t> xa(n * R), ya(n * R), xb(n * R), yb(n * R);
    fam_generate(0, n, (unsigned)atoi(argv[3]), xa.data(), ya.data(), xb.data(), yb.data());
    std::vector<float> ref(n);
    for (long p = 0; p < n; ++p) ref[p] = ref_area(&xa[p * R], &ya[p * R], &xb[p * R], &yb[p * R]);
    FILE* f = fopen(argv[4], "wb");
    if (!f || fwrite(ref.data(), sizeof(float), n, f) != (size_t)n) return 2;
    fclose(f);
    return 0;
  }
  const int family = atoi(argv[2]); const long n = atol(argv[3]); const unsigned seed = (unsigned)atoi(argv[4]);
  int verbose = argc > 5 ? atoi(argv[5]) : 0;
  Rng r(seed);
  static SweepT sw;
  static Prep pa, pb;
  long bad = 0, ties = 0, t1_cap = 0, t2_cap = 0, joins = 0, nonzero = 0, rel16 = 0, full = 0;
  for (long p = 0; p < n; ++p) {
    Poly A, B; gen_pair(family, r, A, B);
    int32_t xa[R], ya[R], xb[R], yb[R]; pad(A, xa, ya); pad(B, xb, yb);
    ties += count_ties(xa, ya, xb, yb);
    const float ref = ref_area(xa, ya, xb, yb);
    if (ref != 0) ++nonzero;
    sw.reset_state();
    sw.add_path(xa, ya, R, sdclip::kClip, 0);
    sw.add_path(xb, yb, R, sdclip::kSubject, 128);
    Res s; s.t = sw.execute(); s.st = sw.status; s.nj = sw.n_joins; s.sabs = sw.sum_abs_terms;
    prepare(xa, ya, xb, yb, p, &pa, &pb);
    const Res t1 = run_beam<BeamT1>(&pa, &pb, p), t2 = run_beam<BeamT2>(&pa, &pb, p);
    int why = 0;
    // a tier that holds the pair reproduces Sweep: area, join flag, failure; and Clipper wherever no join is recorded
    for (const Res* b : {&t1, &t2}) {
      if (b->st & CAP) continue;
      if (b->st & ~(CAP | sdclip::ST_FAIL)) why |= 2;
      if (b->t != s.t) why |= 4;
      if ((b->nj > 0) != (s.nj > 0)) why |= 8;
      if ((b->st & sdclip::ST_FAIL) != (s.st & sdclip::ST_FAIL)) why |= 16;
      if (b->sabs != s.sabs) why |= 128;
      if (b->nj == 0 && b->sabs < (1ll << 24) && 0.5f * (float)b->t != ref) why |= 32;
    }
    if (t1.st & CAP) { ++t1_cap; if (t1.st & sdclip::ST_REL16_OVERFLOW) ++rel16; }
    if (t2.st & CAP) ++t2_cap;
    if (s.nj > 0) ++joins;
    // what no tier holds, and every pair with joins, is the general path's: it must give Clipper's area
    if ((t2.st & CAP) || s.nj > 0 || (s.st & ~sdclip::ST_FAIL) || s.sabs >= (1ll << 24)) {
      ++full;
      const Res f = run_full(xa, ya, xb, yb);
      if ((f.st & ~sdclip::ST_FAIL) || 0.5f * (float)f.t != ref) why |= 64;
    }
    if (why) {
      ++bad;
      if (verbose > 0) {
        --verbose;
        printf("MISMATCH pair %ld (why %d): ref %.1f sweep %lld (st %d nj %d) t1 %lld (st %d nj %d) t2 %lld (st %d nj %d)\nA:", p, why, ref, s.t, s.st, s.nj,
               t1.t, t1.st, t1.nj, t2.t, t2.st, t2.nj);
        for (int k = 0; k < A.n; ++k) printf(" (%d,%d)", A.x[k], A.y[k]);
        printf("\nB:");
        for (int k = 0; k < B.n; ++k) printf(" (%d,%d)", B.x[k], B.y[k]);
        printf("\n");
      }
    }
  }
  printf("family=%d pairs=%ld nonzero=%ld mismatches=%ld tie_edges=%ld tier1_flagged=%ld (16-bit range or bound slots: %ld) tier2_flagged=%ld with_joins=%ld general_path=%ld\n",
         family, n, nonzero, bad, ties, t1_cap, rel16, t2_cap, joins, full);
#ifdef BEAM_VERIFY_CURX
  // counting build: Curr.X as build_intersect_list left it against TopX recomputed at the top of the scan-beam, in every sweep above
  printf("curx_checks=%ld curx_differences=%ld\n", sd_curx_checks()[0], sd_curx_checks()[1]);
  if (sd_curx_checks()[1]) return 1;
#endif
  return bad ? 1 : 0;
}
#endif
