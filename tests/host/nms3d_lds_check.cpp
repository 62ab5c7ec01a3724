// Host harness of tests/test_cpu_nms3d_lds.py: walks the LDS layouts of the 3D NMS (csrc/nms3d_lds.h) with a plain host compiler.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../stardist_amd/csrc/nms3d_lds.h"

namespace {
struct Region { const char* name; size_t beg, end, align; };
char* g_msg; int g_cap;
int fail(const char* what, int R, int n, int form, int nw, const char* a, const char* b) {
  snprintf(g_msg, g_cap, "%s: R=%d n=%d form=%d nw=%d (%s%s%s)", what, R, n, form, nw, a, b[0] ? " / " : "", b);
  return 1;
}
// regions pairwise disjoint, aligned, inside bytes(), and bytes() = the end of the last one
int walk(const std::vector<Region>& rs, size_t bytes, int R, int n, int form, int nw) {
  size_t last = 0;
  for (size_t i = 0; i < rs.size(); ++i) {
    if (rs[i].beg % rs[i].align) return fail("misaligned", R, n, form, nw, rs[i].name, "");
    if (rs[i].end > bytes) return fail("beyond bytes()", R, n, form, nw, rs[i].name, "");
    if (rs[i].end > last) last = rs[i].end;
    for (size_t j = 0; j < i; ++j)
      if (rs[i].beg < rs[j].end && rs[j].beg < rs[i].end && rs[i].end > rs[i].beg && rs[j].end > rs[j].beg) return fail("overlap", R, n, form, nw, rs[i].name, rs[j].name);
  }
  if (last != bytes) return fail("bytes() is not the end of the last region", R, n, form, nw, "", "");
  return 0;
}
// aliasB bytes at the start of the workspace are the documented alias (stage 3: the vertex staging; every stage: the ray-cast vectors)
int check_pair(const sdl::PairLds& L, int R, int form, size_t aliasB) {
  const size_t n = L.n;
  std::vector<Region> rs;
  rs.push_back({"hs", L.hs(), L.hs() + 64 * n, 16});
  if (aliasB > L.ws) return fail("alias exceeds the workspace", R, (int)n, form, L.nw, "work", "");
  if (L.lean) {
    // pos / orig lie in the workspace (closed meshes only: 8 n bytes of tables in at least 6 R floats)
    if (L.orig() + 4 * n > L.work() + L.ws) return fail("lean tables exceed the workspace", R, (int)n, form, L.nw, "orig", "");
    if (L.pos() != L.work() || L.orig() != L.pos() + 4 * n) return fail("lean tables", R, (int)n, form, L.nw, "pos", "orig");
    rs.push_back({"work", L.work(), L.work() + L.ws, 16});
  } else {
    rs.push_back({"work", L.work(), L.work() + L.ws, 16});
    rs.push_back({"seed", L.seed(), L.seed() + 12 * n, 2});
    rs.push_back({"pos", L.pos(), L.pos() + 4 * n, 2});
    rs.push_back({"orig", L.orig(), L.orig() + 4 * n, 2});
  }
  if (L.nw > 1) {
    rs.push_back({"terms", L.terms(), L.terms() + 16 * n, 16});
    rs.push_back({"shared", L.shared(), L.shared() + 16, 8});
    for (int w = 1; w < L.nw; ++w) rs.push_back({"extra", L.extra(w), L.extra(w) + sdl::poly_bytes(), 16});
  }
  return walk(rs, L.bytes(), R, (int)n, form, L.nw);
}
int check_all_for(int R, int F) {
  const sdl::Nms3dLds P = sdl::nms3d_lds(R, F);
  const bool once = sdl::refined_once_fits(R, F, P.s3.ws);
  const int bR = once ? R + 3 * F / 2 : R;
  const size_t staging = (size_t)24 * R, cast0 = sdl::raycast_bytes(R), cast = sdl::raycast_bytes(bR);
  // what lives in the workspace before / instead of the polygons: stage 3 stages the vertices there, both stages cast the rays of the
  // coarse and of the refined direction mesh there
  const size_t need4 = cast > cast0 ? cast : cast0, need3 = staging > need4 ? staging : need4;
  const bool closed = F == 2 * R - 4;
  for (int nw = 1; nw <= 4; nw += 3) {
    if (check_pair(sdl::stage3_lds(R, F, sdl::WS_FULL, bR, nw), R, 0, need3 > sdl::poly_bytes() ? need3 : sdl::poly_bytes())) return 1;
    if (check_pair(sdl::stage4_lds(2 * R, sdl::WS_FULL, bR, nw), R, 0, need4 > sdl::poly_bytes() ? need4 : sdl::poly_bytes())) return 1;
  }
  if (check_pair(sdl::stage3_lds(R, F, sdl::WS_SMALL, bR, 1), R, 1, need3)) return 1;
  if (check_pair(sdl::stage4_lds(2 * R, sdl::WS_SMALL, bR, 1), R, 1, need4)) return 1;
  if (closed) {                     // (the lean form is only launched with the volume bounds on, which need a closed ray mesh)
    if (check_pair(sdl::stage3_lds(R, F, sdl::WS_LEAN, bR, 1), R, 2, need3)) return 1;
    if (check_pair(sdl::stage4_lds(2 * R, sdl::WS_LEAN, bR, 1), R, 2, need4)) return 1;
  }
  {
    const sdl::HullLds H = P.hull;
    std::vector<Region> rs = {{"pv", H.pv(), H.pv() + (size_t)24 * R, 16}, {"tri", H.tri(), H.tri() + (size_t)4 * H.cap, 4}};
    if (H.fast()) {
      rs.push_back({"frA", H.frA(), H.frA() + (size_t)24 * R, 4});
      rs.push_back({"frB", H.frB(), H.frB() + (size_t)24 * R, 4});
      rs.push_back({"cnt", H.cnt(), H.cnt() + (size_t)((R * R + 15) / 16) * 4, 4});
      // the facet adjacency keeps a [R][12] table of shorts in frA and R ints in frB
      if ((size_t)24 * R > H.frB() - H.frA() || (size_t)4 * R > H.cnt() - H.frB()) return fail("vertex-facet table", R, H.cap, 0, 1, "frA", "frB");
    }
    if (walk(rs, H.bytes(), R, H.cap, 0, 1)) return 1;
  }
  {
    const sdl::RenderLds S = P.render;
    if (walk({{"pv1", S.pv1(), S.pv1() + (size_t)12 * R, 16}, {"pv2", S.pv2(), S.pv2() + (size_t)12 * R, 4}, {"faces", S.faces(), S.faces() + (size_t)12 * F, 4}},
             S.bytes(), R, F, 0, 4)) return 1;
  }
  {
    const sdl::RowsLds W = P.rows;
    if (W.pitch() != R + 1) return fail("row pitch", R, F, 0, 2, "", "");
    if (W.bytes() != (W.staged() ? (size_t)128 * (R + 1) * 4 : 0) || !sdl::fits(W.bytes())) return fail("row staging", R, F, 0, 2, "", "");
  }
  return 0;
}
}  // namespace

extern "C" int sdl_check(int R, int F, char* msg, int cap) {
  g_msg = msg; g_cap = cap; msg[0] = 0;
  return check_all_for(R, F);
}

// the totals the driver works with, in the order of the table in the test
extern "C" void sdl_totals(int R, int F, long long* out) {
  const sdl::Nms3dLds P = sdl::nms3d_lds(R, F);
  const bool once = sdl::refined_once_fits(R, F, P.s3.ws);
  const int bR = once ? R + 3 * F / 2 : R, bF = once ? 4 * F : F;
  const bool twice = once && sdl::refined_twice_fits(bR, bF);
  int k = 0;
  out[k++] = P.s3.ws; out[k++] = (long long)P.s3.bytes();
  out[k++] = (long long)sdl::stage3_lds(R, F, sdl::WS_SMALL, bR, 1).bytes(); out[k++] = (long long)sdl::stage3_lds(R, F, sdl::WS_LEAN, bR, 1).bytes();
  out[k++] = (long long)P.s3x.bytes(); out[k++] = (long long)P.s4.bytes();
  out[k++] = (long long)sdl::stage4_lds(2 * R, sdl::WS_SMALL, bR, 1).bytes(); out[k++] = (long long)sdl::stage4_lds(2 * R, sdl::WS_LEAN, bR, 1).bytes();
  out[k++] = (long long)P.s4x.bytes(); out[k++] = (long long)P.hull.bytes(); out[k++] = (long long)P.render.bytes(); out[k++] = (long long)P.rows.bytes();
  out[k++] = sdl::stage3_lds(R, F, sdl::WS_SMALL, bR, 1).ws;
  out[k++] = once; out[k++] = twice; out[k++] = sdl::needs_optin(P.s3.bytes()); out[k++] = P.split3(); out[k++] = P.split4(); out[k++] = !P.ok();
}
