// label_cc.h -- connected components of a 2D / 3D image (stardist_amd.utils.label_components): the backward neighbour offsets per
// connectivity, find, the union step, the tile geometry and what one pixel does in each of the four phases.
//
// Everything here is __host__ __device__ and free of HIP headers when compiled by a host compiler: csrc/label_cc.hip runs it with one
// thread per pixel and atomics behind `Mem`, tests/host/label_cc_check.cpp with plain loops (in two visiting orders), and
// tests/test_cpu_label_components.py compares the latter with the host function.
//
// Two pixels are joined when they are neighbours under the connectivity, their values are equal and that value is not the
// background.  par[] is a forest over linear pixel indices p = (z * Y + y) * X + x (int32: at most 2^31 - 1 pixels), -1 for background.
//   1 tile     one tile (LCC_TILE_Y x LCC_TILE_X pixels of an image, LCC_TILE_Z x LCC_VOL_TILE_Y x LCC_TILE_X of a volume) in local
//              memory: every edge with both ends in the tile is united there; then par[p] = global index of p's tile-local root.
//   2 border   every edge with its ends in two tiles is united in the global array.  Each edge of the pixel graph is the backward
//              offset of exactly one of its ends, so phases 1 and 2 together see every edge once; an edge that leaves the tile does so
//              through a face pixel (the low faces, and the high y / x faces for the offsets with a positive component).
//   3 flatten  every foreground pixel walks to its root and stores it.
//   4 number   roots are the pixels with par[p] == p; an exclusive prefix sum over these flags in raster order gives rank[]; the
//              result is rank[par[p]] + 1, the count is the number of flags.
//
// INVARIANT A: par[p] <= p holds at every instant, for every interleaving.  par[p] starts as p; the only later writes are min(par[a], b)
// with b < a (unite) and par[p] = an ancestor of p (tile_store, flatten), and an ancestor is reached by values that are <= by induction.
// Hence every find is a strictly descending walk (it moves only while par[p] != p, i.e. par[p] < p) and ends after at most p steps,
// and every retry of unite continues from a strictly smaller index: each loop terminates without an iteration cap, whatever the
// races and however stale a value a reader sees (every value a cell ever held is <= its index, and a cell's old value stays in its tree
// for ever, because trees are only ever merged).
// INVARIANT B: the root of a finished component is its smallest linear index.  Every non-root has par[p] < p, so the smallest index m
// of a component cannot be a non-root (par[m] would be a smaller member); and when all unions have returned there is one root per
// component: unite(a, b) returns only when both finds met in one root, or when its min found `a` still a root and hung it under b.
// (A min that finds `a` already hung under `old` may replace that link by b < old; the retry then unites old with b, which restores
// what the replaced link said.)  The output is therefore a function of the input alone: ids follow the raster order of each
// component's first pixel, as scipy.ndimage.label and skimage.measure.label number them.  No floating point anywhere; no atomic's
// result reaches the output except through min.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LCC_HD __host__ __device__ __forceinline__
#else
#define LCC_HD inline
#endif

namespace label_cc {

enum {
  LCC_TILE_X = 64,          // columns of a tile, images and volumes
  LCC_TILE_Y = 32,          // rows of an image's tile
  LCC_TILE_Z = 4,           // planes of a volume's tile
  LCC_VOL_TILE_Y = 8,       // rows of a volume's tile
  LCC_TILE_PIXELS = 2048,   // either tile; two int arrays of this size are the local memory of phase 1 (16 KiB)
  LCC_THREADS = 256,        // a workgroup; LCC_TILE_PIXELS / LCC_THREADS pixels per thread
  LCC_MAX_OFFSETS = 13,
  // the tile extents are powers of two: local coordinates are shifts and masks, not divisions
  LCC_TILE_X_SHIFT = 6, LCC_TILE_Y_SHIFT = 5, LCC_VOL_TILE_Y_SHIFT = 3
};
static_assert((1 << LCC_TILE_X_SHIFT) == LCC_TILE_X && (1 << LCC_TILE_Y_SHIFT) == LCC_TILE_Y && (1 << LCC_VOL_TILE_Y_SHIFT) == LCC_VOL_TILE_Y,
              "tile shifts");
static_assert(LCC_TILE_Y * LCC_TILE_X == LCC_TILE_PIXELS && LCC_TILE_Z * LCC_VOL_TILE_Y * LCC_TILE_X == LCC_TILE_PIXELS, "tile sizes");
static_assert(LCC_TILE_PIXELS % LCC_THREADS == 0, "whole pixels per thread");

// dtype codes of sd_label_components_device: those of csrc/measure.hip, and 3 for int32 (2, float32, is not taken here)
enum { LCC_U8 = 0, LCC_U16 = 1, LCC_I32 = 3 };

// backward offsets (dz, dy, dx): the lexicographically negative half of the 3^3 - 1 neighbours, ordered by their number of non-zero
// coordinates, so that connectivity c uses the first offset_count(c) of them
LCC_HD int offset_count(int connectivity) { return connectivity <= 1 ? 3 : (connectivity == 2 ? 9 : 13); }

LCC_HD void offset_at(int k, int& dz, int& dy, int& dx) {
  // two bits per coordinate (value + 1), dz in bits 4-5, dy in bits 2-3, dx in bits 0-1
  constexpr unsigned char T[LCC_MAX_OFFSETS] = {
      0x14, 0x11, 0x05,                          // (0,0,-1) (0,-1,0) (-1,0,0)
      0x10, 0x12, 0x04, 0x06, 0x01, 0x09,        // (0,-1,-1) (0,-1,1) (-1,0,-1) (-1,0,1) (-1,-1,0) (-1,1,0)
      0x00, 0x02, 0x08, 0x0a};                   // (-1,-1,-1) (-1,-1,1) (-1,1,-1) (-1,1,1)
  const int c = T[k];
  dz = (c >> 4) - 1; dy = ((c >> 2) & 3) - 1; dx = (c & 3) - 1;
}

struct Geometry {
  int Z, Y, X;       // the image (Z = 1: a 2D image)
  int tz, ty, tx;    // the tile
  int ty_shift;      // ty = 1 << ty_shift
  int nz, ny, nx;    // tiles per axis
};

LCC_HD Geometry geometry_of(int Z, int Y, int X) {
  Geometry g;
  g.Z = Z; g.Y = Y; g.X = X;
  g.tz = Z > 1 ? (int)LCC_TILE_Z : 1;
  g.ty = Z > 1 ? (int)LCC_VOL_TILE_Y : (int)LCC_TILE_Y;
  g.tx = LCC_TILE_X;
  g.ty_shift = Z > 1 ? (int)LCC_VOL_TILE_Y_SHIFT : (int)LCC_TILE_Y_SHIFT;
  g.nz = (Z - 1) / g.tz + 1; g.ny = (Y - 1) / g.ty + 1; g.nx = (X - 1) / g.tx + 1;
  return g;
}

LCC_HD long long tile_count(const Geometry& g) { return (long long)g.nz * g.ny * g.nx; }

struct Origin { int z, y, x; };   // first pixel of a tile

LCC_HD Origin tile_origin(const Geometry& g, long long t) {
  Origin o;
  o.x = (int)(t % g.nx) * g.tx;
  o.y = (int)((t / g.nx) % g.ny) * g.ty;
  o.z = (int)(t / ((long long)g.nx * g.ny)) * g.tz;
  return o;
}

// local index l = (lz * ty + ly) * tx + lx: the raster order of the tile is the raster order of the image, so the smallest local
// index of a set of tile pixels is also its smallest global one
LCC_HD void local_coords(const Geometry& g, int l, int& lz, int& ly, int& lx) {
  lx = l & (LCC_TILE_X - 1);
  ly = (l >> LCC_TILE_X_SHIFT) & (g.ty - 1);
  lz = l >> (LCC_TILE_X_SHIFT + g.ty_shift);
}

LCC_HD bool in_tile(const Geometry& g, int lz, int ly, int lx) {
  return lz >= 0 && lz < g.tz && ly >= 0 && ly < g.ty && lx >= 0 && lx < g.tx;
}

// tile pixel (lz, ly, lx), coordinates possibly outside the tile, inside the image?  (no sum that could pass INT_MAX)
LCC_HD bool in_image(const Geometry& g, const Origin& o, int lz, int ly, int lx) {
  return lz >= -o.z && lz < g.Z - o.z && ly >= -o.y && ly < g.Y - o.y && lx >= -o.x && lx < g.X - o.x;
}

LCC_HD int global_index(const Geometry& g, const Origin& o, int lz, int ly, int lx) {
  return (int)(((long long)(o.z + lz) * g.Y + (o.y + ly)) * g.X + (o.x + lx));
}

// Mem: load(const int*) and min(int*, int) -> the value before; plain memory on the host, atomics on the device
template <class M>
LCC_HD int find(const int* par, int p, M& mem) {
  for (;;) {
    const int q = mem.load(par + p);
    if (q == p) return p;
    p = q;                                  // q < p (invariant A)
  }
}

// lock-free union: find both roots, min the larger root's parent to the smaller, retry from the value the min returns
template <class M>
LCC_HD void unite(int* par, int a, int b, M& mem) {
  for (;;) {
    a = find(par, a, mem);
    b = find(par, b, mem);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = mem.min(par + a, b);    // b < a
    if (old == a) return;                   // a was a root and hangs under b now
    a = old;                                // a had been hung under old < a meanwhile: unite that with b
  }
}

// ---- phase 1, per tile pixel l; val[] and par[] are the tile's local arrays of LCC_TILE_PIXELS ints -------------------------------
template <typename T>
LCC_HD void tile_load(const Geometry& g, const Origin& o, int l, const T* __restrict__ img, long long background, int* val, int* par) {
  int lz, ly, lx;
  local_coords(g, l, lz, ly, lx);
  int v = 0;
  bool fg = false;
  if (in_image(g, o, lz, ly, lx)) {
    v = (int)img[global_index(g, o, lz, ly, lx)];
    fg = (long long)v != background;
  }
  val[l] = v;
  par[l] = fg ? l : -1;                     // a tile pixel outside the image counts as background
}

template <class M>
LCC_HD void tile_link(const Geometry& g, int l, int n_offsets, const int* val, int* par, M& mem) {
  if (mem.load(par + l) < 0) return;
  int lz, ly, lx;
  local_coords(g, l, lz, ly, lx);
  for (int k = 0; k < n_offsets; ++k) {
    int dz, dy, dx;
    offset_at(k, dz, dy, dx);
    if (!in_tile(g, lz + dz, ly + dy, lx + dx)) continue;
    const int m = ((lz + dz) * g.ty + (ly + dy)) * g.tx + (lx + dx);
    if (mem.load(par + m) >= 0 && val[m] == val[l]) unite(par, l, m, mem);
  }
}

template <class M>
LCC_HD void tile_store(const Geometry& g, const Origin& o, int l, const int* par, int* __restrict__ out, M& mem) {
  int lz, ly, lx;
  local_coords(g, l, lz, ly, lx);
  if (!in_image(g, o, lz, ly, lx)) return;
  int r = -1;
  if (mem.load(par + l) >= 0) {
    const int root = find(par, l, mem);
    int rz, ry, rx;
    local_coords(g, root, rz, ry, rx);
    r = global_index(g, o, rz, ry, rx);
  }
  out[global_index(g, o, lz, ly, lx)] = r;
}

// ---- phase 2, per tile pixel l: the backward neighbours outside the tile; par[] is the global array -------------------------------
LCC_HD bool on_face(const Geometry& g, int lz, int ly, int lx) {
  return lx == 0 || lx == g.tx - 1 || ly == 0 || ly == g.ty - 1 || (g.Z > 1 && (lz == 0 || lz == g.tz - 1));
}

template <typename T, class M>
LCC_HD void border_link(const Geometry& g, const Origin& o, int l, const T* __restrict__ img, long long background, int n_offsets, int* par,
                        M& mem) {
  int lz, ly, lx;
  local_coords(g, l, lz, ly, lx);
  if (!on_face(g, lz, ly, lx) || !in_image(g, o, lz, ly, lx)) return;
  const int p = global_index(g, o, lz, ly, lx);
  const int v = (int)img[p];
  if ((long long)v == background) return;
  for (int k = 0; k < n_offsets; ++k) {
    int dz, dy, dx;
    offset_at(k, dz, dy, dx);
    if (in_tile(g, lz + dz, ly + dy, lx + dx) || !in_image(g, o, lz + dz, ly + dy, lx + dx)) continue;
    const int q = global_index(g, o, lz + dz, ly + dy, lx + dx);
    if ((int)img[q] == v) unite(par, p, q, mem);
  }
}

// ---- phases 3 and 4, per pixel p -------------------------------------------------------------------------------------------------
template <class M>
LCC_HD void flatten_pixel(int* par, int p, M& mem) {
  if (mem.load(par + p) >= 0) par[p] = find(par, p, mem);
}

LCC_HD int is_root(const int* par, int p) { return par[p] == p ? 1 : 0; }

// par[p] is p's root (phase 3), rank[] the exclusive prefix sum of is_root; in place: a pixel reads no cell of par but its own
LCC_HD void number_pixel(int* par, const int* __restrict__ rank, int p) {
  const int r = par[p];
  par[p] = r < 0 ? 0 : rank[r] + 1;
}

}  // namespace label_cc
