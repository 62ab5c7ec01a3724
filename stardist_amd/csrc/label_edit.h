// label_edit.h -- the per-pixel rules of the label clean-up functions (stardist_amd.utils.find_boundaries, clear_border,
// remove_small_objects): the tile with its halo and what one pixel decides from its 3^nd window, the pixels of the border band, the
// flag a pixel sets and the value a flagged pixel gets.
//
// Everything here is __host__ __device__ and free of HIP headers when compiled by a host compiler: csrc/label_edit.hip runs it with one
// thread per pixel, tests/host/label_edit_check.cpp with plain loops in the kernel's tile order, and tests/test_cpu_label_edit.py
// compares the latter with the host routes.  Integer arithmetic only.
//
// find_boundaries (scikit-image 0.18's, modes thick / inner / outer).  N_c(p): the in-image neighbours of p whose offsets have at most
// c non-zero coordinates; a neighbour outside the image does not exist.
//   thick(p) = some q in N_c(p) has L(q) != L(p)
//   inner(p) = thick(p) and L(p) != background
//   outer(p) = thick(p) and (L(p) == background or max of L over W(p) != min of L' over W(p)), W(p) = N_nd(p) + {p} (the window of full
//              connectivity whatever c is), L' = L with every background pixel replaced by the sentinel, the largest value of the
//              image's dtype
// A tile cell outside the image holds the value of the image pixel with the clamped coordinates.  For a centre p and an offset o that
// leaves the image, clamping moves exactly the coordinates that left back onto p's own, so the cell holds L(p + o') with o' = o with
// those coordinates zeroed: a pixel of N_c(p) + {p} again (o' has no more non-zero coordinates than o).  It adds no value to a window
// that the window does not hold already, so every rule above reads the plain 3^nd window and needs no test against the image's edges.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LE_HD __host__ __device__ __forceinline__
#else
#define LE_HD inline
#endif

namespace label_edit {

enum {
  LE_TILE_X = 64,           // columns of a tile, images and volumes
  LE_TILE_Y = 32,           // rows of an image's tile
  LE_TILE_Z = 4,            // planes of a volume's tile
  LE_VOL_TILE_Y = 8,        // rows of a volume's tile
  LE_TILE_PIXELS = 2048,    // either tile
  LE_THREADS = 256,         // a workgroup; LE_TILE_PIXELS / LE_THREADS pixels per thread
  // the tile with a halo of 1: 34 x 66 cells of an image, 6 x 10 x 66 of a volume.  A wave reads 64 consecutive cells of one row, so
  // the 32 lanes of a group hit 32 different banks whatever the row stride is; the rows need no padding
  LE_LDS_CELLS = (LE_TILE_Z + 2) * (LE_VOL_TILE_Y + 2) * (LE_TILE_X + 2),
  LE_TILE_X_SHIFT = 6, LE_TILE_Y_SHIFT = 5, LE_VOL_TILE_Y_SHIFT = 3
};
static_assert((1 << LE_TILE_X_SHIFT) == LE_TILE_X && (1 << LE_TILE_Y_SHIFT) == LE_TILE_Y && (1 << LE_VOL_TILE_Y_SHIFT) == LE_VOL_TILE_Y,
              "tile shifts");
static_assert(LE_TILE_Y * LE_TILE_X == LE_TILE_PIXELS && LE_TILE_Z * LE_VOL_TILE_Y * LE_TILE_X == LE_TILE_PIXELS, "tile sizes");
static_assert((LE_TILE_Y + 2) * (LE_TILE_X + 2) <= LE_LDS_CELLS, "the image's tile fits the local array");
static_assert(LE_TILE_PIXELS % LE_THREADS == 0, "whole pixels per thread");

enum { LE_THICK = 0, LE_INNER = 1, LE_OUTER = 2 };      // mode of sd_find_boundaries_device

struct Tile {
  int Z, Y, X;       // the image (Z = 1: a 2D image, no halo along z)
  int tz, ty, tx;    // the tile
  int ty_shift;      // ty = 1 << ty_shift
  int hz;            // the halo along z: 1 for a volume, else 0
  int cy, cx;        // cells per row and column of the local array: ty + 2, tx + 2
  int nz, ny, nx;    // tiles per axis
};

LE_HD Tile tile_of(int Z, int Y, int X) {
  Tile g;
  g.Z = Z; g.Y = Y; g.X = X;
  g.tz = Z > 1 ? (int)LE_TILE_Z : 1;
  g.ty = Z > 1 ? (int)LE_VOL_TILE_Y : (int)LE_TILE_Y;
  g.tx = LE_TILE_X;
  g.ty_shift = Z > 1 ? (int)LE_VOL_TILE_Y_SHIFT : (int)LE_TILE_Y_SHIFT;
  g.hz = Z > 1 ? 1 : 0;
  g.cy = g.ty + 2; g.cx = g.tx + 2;
  g.nz = (Z - 1) / g.tz + 1; g.ny = (Y - 1) / g.ty + 1; g.nx = (X - 1) / g.tx + 1;
  return g;
}

LE_HD long long tile_count(const Tile& g) { return (long long)g.nz * g.ny * g.nx; }

LE_HD int cell_count(const Tile& g) { return (g.tz + 2 * g.hz) * g.cy * g.cx; }

struct Origin { int z, y, x; };   // first pixel of a tile

LE_HD Origin tile_origin(const Tile& g, long long t) {
  Origin o;
  o.x = (int)(t % g.nx) * g.tx;
  o.y = (int)((t / g.nx) % g.ny) * g.ty;
  o.z = (int)(t / ((long long)g.nx * g.ny)) * g.tz;
  return o;
}

LE_HD int clamp_to(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// the image pixel whose value cell c of the tile at o holds: the cell's own coordinates, clamped to the image (64-bit offset)
LE_HD long long cell_source(const Tile& g, const Origin& o, int c) {
  const int x = c % g.cx, y = (c / g.cx) % g.cy, z = c / (g.cx * g.cy);
  const int iz = clamp_to(o.z + z - g.hz, g.Z), iy = clamp_to(o.y + y - 1, g.Y), ix = clamp_to(o.x + x - 1, g.X);
  return ((long long)iz * g.Y + iy) * g.X + ix;
}

// tile pixel l = (lz * ty + ly) * tx + lx
LE_HD void local_coords(const Tile& g, int l, int& lz, int& ly, int& lx) {
  lx = l & (LE_TILE_X - 1);
  ly = (l >> LE_TILE_X_SHIFT) & (g.ty - 1);
  lz = l >> (LE_TILE_X_SHIFT + g.ty_shift);
}

LE_HD bool in_image(const Tile& g, const Origin& o, int lz, int ly, int lx) { return lz < g.Z - o.z && ly < g.Y - o.y && lx < g.X - o.x; }

LE_HD long long global_index(const Tile& g, const Origin& o, int lz, int ly, int lx) {
  return ((long long)(o.z + lz) * g.Y + (o.y + ly)) * g.X + (o.x + lx);
}

// 1 where tile pixel (lz, ly, lx) is a boundary pixel, else 0; cells[]: the tile's local array.  connectivity and mode are the same
// for every pixel of a launch, so the branches on them are uniform
LE_HD unsigned char boundary_at(const int* cells, const Tile& g, int lz, int ly, int lx, int connectivity, int mode, long long background,
                                long long sentinel) {
  const int centre_at = ((lz + g.hz) * g.cy + (ly + 1)) * g.cx + (lx + 1);
  const int centre = cells[centre_at];
  const bool whole_window = mode == LE_OUTER;
  bool thick = false;
  long long hi = centre, lo = (long long)centre == background ? sentinel : (long long)centre;
  for (int dz = -g.hz; dz <= g.hz; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int moved = (dz != 0) + (dy != 0) + (dx != 0);
        if (moved == 0 || (moved > connectivity && !whole_window)) continue;
        const int v = cells[centre_at + (dz * g.cy + dy) * g.cx + dx];
        if (moved <= connectivity && v != centre) thick = true;
        if (whole_window) {
          const long long w = (long long)v == background ? sentinel : (long long)v;
          hi = (long long)v > hi ? (long long)v : hi;
          lo = w < lo ? w : lo;
        }
      }
  if (!thick) return 0;
  if (mode == LE_THICK) return 1;
  const bool is_background = (long long)centre == background;
  if (mode == LE_INNER) return is_background ? 0 : 1;
  return (is_background || hi != lo) ? 1 : 0;
}

// ---- the border band of clear_border: the pixels within `ext` = buffer_size + 1 of an image edge along any axis (along z only for a
// volume given as such, has_z).  Its pixels are counted once each: whole planes of the z band, then whole rows of the y band in the
// other planes, then the x band of the other rows.
struct Band {
  int Z, Y, X;
  int ext;             // >= 1
  long long bz, by, bx;    // band coordinates per axis: min(2 ext, extent), along z 0 without a z axis
};

LE_HD Band band_of(int Z, int Y, int X, int has_z, int ext) {
  Band b;
  b.Z = Z; b.Y = Y; b.X = X; b.ext = ext;
  const long long two = 2ll * ext;
  b.bz = has_z ? (two < Z ? two : (long long)Z) : 0;
  b.by = two < Y ? two : (long long)Y;
  b.bx = two < X ? two : (long long)X;
  return b;
}

LE_HD long long band_count(const Band& b) { return b.bz * b.Y * b.X + (b.Z - b.bz) * b.by * b.X + (b.Z - b.bz) * (b.Y - b.by) * b.bx; }

// the k-th band coordinate of an axis of n pixels with nb band coordinates, ascending; the k-th coordinate that is not in the band
LE_HD long long band_coord(long long k, long long nb, long long n, int ext) { return (k < ext || nb == n) ? k : n - nb + k; }
LE_HD long long inner_coord(long long k, long long nb, int ext) { return (nb == 0 ? 0 : ext) + k; }

// the linear index of band pixel t, 0 <= t < band_count
LE_HD long long band_pixel(const Band& b, long long t) {
  long long z, y, x;
  const long long planes = b.bz * b.Y * b.X, rows = (b.Z - b.bz) * b.by * b.X;
  if (t < planes) {
    x = t % b.X; y = (t / b.X) % b.Y;
    z = band_coord(t / ((long long)b.X * b.Y), b.bz, b.Z, b.ext);
  } else if (t < planes + rows) {
    t -= planes;
    x = t % b.X;
    y = band_coord((t / b.X) % b.by, b.by, b.Y, b.ext);
    z = inner_coord(t / (b.X * b.by), b.bz, b.ext);
  } else {
    t -= planes + rows;
    x = band_coord(t % b.bx, b.bx, b.X, b.ext);
    y = inner_coord((t / b.bx) % (b.Y - b.by), b.by, b.ext);
    z = inner_coord(t / (b.bx * (b.Y - b.by)), b.bz, b.ext);
  }
  return (z * b.Y + y) * b.X + x;
}

// pixel p flags its key (a component id, 0 for the background); every writer stores the same 1, so the order does not matter.  A key
// outside the table is left alone: no key can make the store leave the table
LE_HD void flag_pixel(const int* __restrict__ key, long long p, unsigned char* flags, long long n_flags) {
  const int k = key[p];
  if (k >= 0 && k < n_flags) flags[k] = 1;
}

// the value of a pixel with value `val` and key `key` after the clear pass
LE_HD int cleared_value(int val, int key, const unsigned char* __restrict__ flags, long long n_flags, int bgval) {
  return (key >= 0 && key < n_flags && flags[key]) ? bgval : val;
}

}  // namespace label_edit
