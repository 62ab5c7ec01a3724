// nms3d_lds.h -- the dynamic-LDS layouts of the 3D NMS kernels (nms3d.hip), each written ONCE: the kernels take their pointers from
// these value types, the host takes its byte counts, budget tests and launch flags from them, and tests/host/nms3d_lds_check.cpp
// walks them on the CPU (regions disjoint and aligned, totals against a recorded table).  Plain C++, no HIP include.
//
//   PairLds    k_stage3 / k_stage3x (n = F faces, half-space 2f + w) and k_stage4 / k_stage4x (n = cap = 2 R hull facets):
//                hs | workspace | seed pos orig | terms shared | extra workspaces          (the last two only with nw > 1 waves)
//              the workspace is wave 0's polygon workspace; the vertex staging of stage 3 (dead once hs is built) and the ray-cast
//              vectors of the volume bounds alias it.  Three forms:
//                WS_FULL   room for the polygon workspace of the exact routine
//                WS_SMALL  a bounds-only launch: room for the ray-cast vectors only
//                WS_LEAN   WS_SMALL without the seed table; pos / orig (written by the cull, read by nobody) lie in the workspace
//   HullLds    k_hull        points | facets | two frontiers | edge use counts     (the last two only up to HULL_FAST_MAXR points)
//   RenderLds  k_stage5      vertices of both polyhedra | faces
//   RowsLds    k_pre1/k_pre2 128 candidate rows of pitch R + 1
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define SDL_HD __host__ __device__ inline
#else
#define SDL_HD inline
#endif

#define HIV_CAPL 16           // vertices of a face polygon in LDS (per lane)
#define HIV_LCAP 56           // entries of a lane's cutter list
#define HULL_FAST_MAXR 192    // gift wrapping (and its LDS tables) up to this many points

namespace sdl {

SDL_HD size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
// one wave's polygon workspace: S, T [HIV_CAPL][64] doubles, list [HIV_LCAP][64] shorts
SDL_HD size_t poly_bytes() { return (size_t)2 * HIV_CAPL * 64 * sizeof(double) + (size_t)HIV_LCAP * 64 * sizeof(unsigned short); }
// ray-cast vectors of the volume bounds over a direction mesh of R directions: 3 R doubles, R shorts
SDL_HD size_t raycast_bytes(int R) { return (size_t)3 * R * sizeof(double) + (size_t)2 * R; }

// what a workgroup may ask for, and from where on hipFuncSetAttribute(MaxDynamicSharedMemorySize) is needed
SDL_HD bool fits(size_t bytes) { return bytes <= (size_t)150 * 1024; }
SDL_HD bool needs_optin(size_t bytes) { return bytes > (size_t)64 * 1024; }

// the direction mesh refined once (R + 3F/2 directions) is cast in a stage's own workspace, the one refined twice in the three
// further workspaces of the four-wave kernels
// (the planes hit are kept as 16-bit ids, and k_refine_mesh splits a closed mesh: an even face count)
SDL_HD bool refined_once_fits(int R, int F, size_t wsFull) {
  const int R2 = R + 3 * F / 2;
  return F % 2 == 0 && raycast_bytes(R2) <= poly_bytes() && raycast_bytes(R2) <= wsFull && R2 < 65535;
}
SDL_HD bool refined_twice_fits(int bR, int bF) { const int R3 = bR + 3 * bF / 2; return raycast_bytes(R3) <= (size_t)3 * poly_bytes() && R3 < 65535; }

enum WsForm { WS_FULL = 0, WS_SMALL = 1, WS_LEAN = 2 };

struct PairLds {
  unsigned int n;        // half-spaces / 2: F (stage 3), cap (stage 4)
  unsigned int ws;       // bytes of the workspace behind the half-spaces
  int lean;              // WS_LEAN
  int nw;                // waves per pair
  SDL_HD size_t hs() const { return 0; }                                         // 2n half-spaces of 4 doubles
  SDL_HD size_t work() const { return (size_t)8 * n * sizeof(double); }          // = vertex staging pv1 (3 R floats), pv2 behind it
  SDL_HD size_t seed() const { return work() + ws; }                             // 2n * 3 shorts (absent when lean)
  SDL_HD size_t pos() const { return lean ? work() : seed() + (size_t)6 * n * sizeof(unsigned short); }     // 2n shorts
  SDL_HD size_t orig() const { return pos() + (size_t)2 * n * sizeof(unsigned short); }                      // 2n shorts
  SDL_HD size_t tables_end() const { return seed() + (lean ? (size_t)0 : (size_t)10 * n * sizeof(unsigned short)); }
  SDL_HD size_t terms() const { return align16(tables_end()); }                  // nw > 1: 2n doubles
  SDL_HD size_t shared() const { return terms() + (size_t)2 * n * sizeof(double); }          // 4 ints
  SDL_HD size_t extra(int wave) const { return shared() + 16 + (size_t)(wave - 1) * poly_bytes(); }     // workspace of wave 1 .. nw - 1
  SDL_HD size_t bytes() const { return nw > 1 ? extra(nw) : tables_end(); }
};
// bR: directions of the mesh the bounds pass casts (the small forms hold its vectors, and at least the vertex staging)
SDL_HD PairLds stage3_lds(int R, int F, WsForm form, int bR, int nw) {
  const size_t full = raycast_bytes(R) > poly_bytes() ? align16(raycast_bytes(R)) : poly_bytes();     // >= 6R floats
  const size_t stagingB = (size_t)6 * R * sizeof(float);
  const size_t small = align16(stagingB > raycast_bytes(bR) ? stagingB : raycast_bytes(bR));
  return PairLds{(unsigned int)F, (unsigned int)(form == WS_FULL ? full : small), form == WS_LEAN, nw};
}
SDL_HD PairLds stage4_lds(int cap, WsForm form, int bR, int nw) {
  return PairLds{(unsigned int)cap, (unsigned int)(form == WS_FULL ? poly_bytes() : align16(raycast_bytes(bR))), form == WS_LEAN, nw};
}

// how a volume kernel is to run (what used to travel in spare bits of the workspace size)
struct PairFlags {
  unsigned int prof : 1;        // stage 3: accumulate wave cycles per phase (option "trace")
  unsigned int recast : 1;      // refined bounds pass casts every direction again ("nms3d_bounds_reuse" = 0)
  unsigned int exact : 1;       // bound shortcuts off: every feasible pair is integrated
};

struct HullLds {
  int R, cap;
  SDL_HD bool fast() const { return R <= HULL_FAST_MAXR; }
  SDL_HD size_t pv() const { return 0; }                                         // 3 R doubles
  SDL_HD size_t tri() const { return (size_t)3 * R * sizeof(double); }           // cap packed facets
  SDL_HD size_t frA() const { return tri() + (size_t)cap * sizeof(unsigned int); }           // fast: 6 R open edges
  SDL_HD size_t frB() const { return frA() + (size_t)6 * R * sizeof(unsigned int); }         // fast: 6 R open edges
  SDL_HD size_t cnt() const { return frB() + (size_t)6 * R * sizeof(unsigned int); }         // fast: R * R edge use counts, two bits each
  SDL_HD size_t bytes() const { return fast() ? cnt() + (size_t)((R * R + 15) / 16) * 4 : frA(); }
};

struct RenderLds {
  int R, F;
  SDL_HD size_t pv1() const { return 0; }                                        // 3 R floats
  SDL_HD size_t pv2() const { return (size_t)3 * R * sizeof(float); }            // 3 R floats
  SDL_HD size_t faces() const { return (size_t)6 * R * sizeof(float); }          // 3 F ints
  SDL_HD size_t bytes() const { return faces() + (size_t)3 * F * sizeof(int); }
};

struct RowsLds {
  int R;
  static constexpr int ROWS = 128;           // = the workgroup size of k_pre1 / k_pre2
  SDL_HD int pitch() const { return R + 1; }
  SDL_HD bool staged() const { return fits((size_t)ROWS * pitch() * sizeof(float)); }        // several hundred rays: rows stay in memory
  SDL_HD size_t bytes() const { return staged() ? (size_t)ROWS * pitch() * sizeof(float) : 0; }
};

// every launch form of one call (n_rays = R, n_faces = F, hulls of up to 2 R facets); the bounds-only forms of the two volume stages
// depend on the direction mesh chosen later: stage3_lds / stage4_lds with WS_SMALL / WS_LEAN
struct Nms3dLds {
  PairLds s3, s3x, s4, s4x;        // one wave per pair; four waves per pair (exact volumes of the pairs the bounds leave undecided)
  HullLds hull;
  RenderLds render;
  RowsLds rows;
  SDL_HD bool ok() const { return fits(s3.bytes()) && fits(render.bytes()) && fits(s4.bytes()); }
  SDL_HD bool split3() const { return fits(s3x.bytes()); }
  SDL_HD bool split4() const { return fits(s4x.bytes()); }
};
SDL_HD Nms3dLds nms3d_lds(int R, int F) {
  return Nms3dLds{stage3_lds(R, F, WS_FULL, R, 1), stage3_lds(R, F, WS_FULL, R, 4), stage4_lds(2 * R, WS_FULL, R, 1), stage4_lds(2 * R, WS_FULL, R, 4),
                  HullLds{R, 2 * R}, RenderLds{R, F}, RowsLds{R}};
}

}  // namespace sdl
