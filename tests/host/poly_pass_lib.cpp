// tests/host/poly_pass_lib.cpp -- host statements of the 2D NMS's per-polygon pass (stardist_amd/csrc/poly_pass.h) as a tiny shared
// library for tests/test_cpu_poly_pass.py and tests/test_gpu_poly_pass.py:
//   * poly_pass_prep_host: the pass's own preparation (FastPrep, compiled for the host) on the same 16-bit relative ring the kernel
//     stages, PrepWork from private memory where the ring does not fit -- compared with PrepWork (beam_prep_lib.cpp) on the CPU;
//   * poly_props_host: the polygon properties of the decision shortcut (area_bounds.h PolyProps) restated lane by lane, with the
//     reductions in the device's xor-butterfly order -- the record the device pass must write byte for byte.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC (no FMA contraction, as the device build).
#include "../../stardist_amd/csrc/poly_pass.h"
#include <cmath>
#include <cstring>

namespace {
struct HostProps { float lmax, perim; int flags; int xmin, xmax, ymin, ymax; int pad; };   // = sdarea::PolyProps
enum { PP_PLAIN = 1, PP_POS = 2, PP_NEG = 4 };
constexpr int WINDOW = 2047;
constexpr float WIN_LMAX_SCALE = 1.f + 1e-6f;

float sgnf(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }
// lane 0's result of the device's butterfly over 32 lanes (offsets 16, 8, 4, 2, 1)
template <class F> float butterfly(const float* in, F op) {
  float v[32];
  for (int i = 0; i < 32; ++i) v[i] = in[i];
  for (int o = 16; o; o >>= 1) {
    float w[32];
    for (int i = 0; i < 32; ++i) w[i] = op(v[i], v[i ^ o]);
    memcpy(v, w, sizeof(v));
  }
  return v[0];
}

HostProps props_one(const int* X, const int* Y, int R) {
  HostProps p;
  int xmin = X[0], xmax = X[0], ymin = Y[0], ymax = Y[0];
  for (int l = 1; l < R; ++l) { xmin = X[l] < xmin ? X[l] : xmin; xmax = X[l] > xmax ? X[l] : xmax; ymin = Y[l] < ymin ? Y[l] : ymin; ymax = Y[l] > ymax ? Y[l] : ymax; }
  const bool small = (long long)xmax - xmin <= WINDOW && (long long)ymax - ymin <= WINDOW;
  float ax[32] = {}, ay[32] = {}, ex[32] = {}, ey[32] = {};
  bool deg[32];
  int rx[32] = {}, ry[32] = {};
  for (int l = 0; l < 32; ++l) {
    deg[l] = true;
    if (l < R && small) { rx[l] = X[l] - X[0]; ry[l] = Y[l] - Y[0]; }
  }
  unsigned m32 = 0;
  int area2 = 0;
  for (int l = 0; l < R; ++l) {
    const int ln = (l + 1 >= R) ? 0 : l + 1;
    ax[l] = (float)rx[l]; ay[l] = (float)ry[l];
    ex[l] = (float)rx[ln] - ax[l]; ey[l] = (float)ry[ln] - ay[l];
    deg[l] = ex[l] == 0.f && ey[l] == 0.f;
    if (!deg[l]) m32 |= 1u << l;
    area2 += rx[l] * ry[ln] - ry[l] * rx[ln];
  }
  auto next_of = [&](int e) {
    if (!m32) return -1;
    const unsigned above = (e >= 31) ? 0u : (m32 & ~((2u << e) - 1u));
    return above ? __builtin_ctz(above) : __builtin_ctz(m32);
  };
  bool anybad = false;
  for (int l = 0; l < R; ++l) {
    const float Ax = ax[l], Ay = ay[l], Ex = ex[l], Ey = ey[l];
    const int ln = (l + 1 >= R) ? 0 : l + 1;
    const float Bx = ax[ln], By = ay[ln];
    const int nxt = next_of(l);
    for (int dd = 1; dd <= (R >> 1); ++dd) {
      int k = l + dd; if (k >= R) k -= R;
      const int kn = (k + 1 >= R) ? 0 : k + 1;
      const float cx = ax[k], cy = ay[k], dx = ax[kn], dy = ay[kn];
      const int nxt_k = next_of(k);
      const bool degk = ((m32 >> k) & 1u) == 0u;
      const float fx = dx - cx, fy = dy - cy;
      if (small && !degk && !((cx == Ax && cy == Ay) || (dx == Ax && dy == Ay)) && Ay >= fminf(cy, dy) && Ay <= fmaxf(cy, dy)) {
        if (fy == 0.f) { if (Ax >= fminf(cx, dx) && Ax <= fmaxf(cx, dx)) anybad = true; }
        else if (2.f * fabsf((cx - Ax) * fy + (Ay - cy) * fx) <= fabsf(fy)) anybad = true;
      }
      if (small && !deg[l] && !((Ax == cx && Ay == cy) || (Bx == cx && By == cy)) && cy >= fminf(Ay, By) && cy <= fmaxf(Ay, By)) {
        if (Ey == 0.f) { if (cx >= fminf(Ax, Bx) && cx <= fmaxf(Ax, Bx)) anybad = true; }
        else if (2.f * fabsf((Ax - cx) * Ey + (cy - Ay) * Ex) <= fabsf(Ey)) anybad = true;
      }
      if (deg[l] || degk) continue;
      if (k == nxt || nxt_k == l) {
        const float cr = Ex * fy - Ey * fx, dt = Ex * fx + Ey * fy;
        if (cr == 0.f && dt < 0.f) anybad = true;
        continue;
      }
      const float o1 = Ex * (cy - Ay) - Ey * (cx - Ax), o2 = Ex * (dy - Ay) - Ey * (dx - Ax);
      const float o3 = fx * (Ay - cy) - fy * (Ax - cx), o4 = fx * (By - cy) - fy * (Bx - cx);
      bool inter = (sgnf(o1) * sgnf(o2) <= 0.f) && (sgnf(o3) * sgnf(o4) <= 0.f);
      if (o1 == 0.f && o2 == 0.f)
        inter = fmaxf(fminf(Ax, Bx), fminf(cx, dx)) <= fminf(fmaxf(Ax, Bx), fmaxf(cx, dx)) &&
                fmaxf(fminf(Ay, By), fminf(cy, dy)) <= fminf(fmaxf(Ay, By), fmaxf(cy, dy));
      if (inter) anybad = true;
    }
  }
  float len[32], l1[32];
  for (int l = 0; l < 32; ++l) {
    const bool d = l >= R || deg[l];
    len[l] = d ? 0.f : sqrtf(ex[l] * ex[l] + ey[l] * ey[l]);
    l1[l] = d ? 0.f : fabsf(ex[l]) + fabsf(ey[l]);
  }
  const int count = __builtin_popcount(m32);
  p.lmax = butterfly(len, [](float a, float b) { return fmaxf(a, b); }) * WIN_LMAX_SCALE;
  p.perim = butterfly(l1, [](float a, float b) { return a + b; });
  p.flags = ((small && !anybad && count >= 3 && area2 != 0) ? PP_PLAIN : 0) | (area2 > 0 ? PP_POS : 0) | (area2 < 0 ? PP_NEG : 0);
  p.xmin = xmin; p.xmax = xmax; p.ymin = ymin; p.ymax = ymax; p.pad = 0;
  return p;
}
}  // namespace

extern "C" long poly_props_record_bytes() { return sizeof(HostProps); }

extern "C" void poly_props_host(const int* x, const int* y, int n, int R, void* out) {
  HostProps* o = (HostProps*)out;
  for (int i = 0; i < n; ++i) o[i] = props_one(x + (size_t)i * R, y + (size_t)i * R, R);
}

// the pass's preparation for R <= 32: FastPrep on the staged ring (one column of the kernel's LDS array), PrepWork where it does not fit
extern "C" void poly_pass_prep_host(const int* x, const int* y, int n, int R, void* out) {
  typedef sdclip::PolyPrep<sdpass::PASS_V> Prep;
  Prep* o = (Prep*)out;
  static int ring[sdpass::PASS_V * sdpass::PASS_T];
  for (int i = 0; i < n; ++i) {
    const int* xs = x + (size_t)i * R;
    const int* ys = y + (size_t)i * R;
    bool fits = true;
    for (int l = 0; l < R; ++l) {
      const long long rx = (long long)xs[l] - xs[0], ry = (long long)ys[l] - ys[0];
      fits = fits && rx >= -32768 && rx <= 32767 && ry >= -32768 && ry <= 32767;
    }
    if (fits) {
      for (int l = 0; l < R; ++l) ring[l * sdpass::PASS_T] = sdpass::pack_(xs[l] - xs[0], ys[l] - ys[0]);
      sdpass::FastPrep w;
      w.prepare(ring, R, xs[0], ys[0], o + i);
    } else {
      sdclip::PrepWork<sdclip::PlainStorage, sdpass::PASS_V> w;
      w.prepare(xs, ys, R, o + i);
    }
  }
}
