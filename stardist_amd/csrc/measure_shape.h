// measure_shape.h -- what one pixel adds to the integer shape tables of its object (stardist_amd.utils.measure_labels(shape=True)):
// the second-order coordinate sums, the three contour-pixel classes of skimage.measure.perimeter and the histogram of 2 x 2 pixel
// configurations behind perimeter_crofton and euler_number.
//
// Everything here is __host__ __device__ and free of HIP headers when compiled by a host compiler: csrc/measure_shape.hip runs it with
// one thread per pixel, tests/host/measure_shape_check.cpp with plain loops over the tiles, and tests/test_cpu_measure_shape.py
// compares the latter with the host function.  All of it is integer arithmetic: the tables are sums of small integers, so neither
// the order in which pixels are visited nor the order in which atomics land shows in them.
//
// Moments.  With u_d = coordinate_d - (start of the object's box)_d, the local coordinates of scikit-image's regionprops:
//   m2[l] = { sum u_z u_z, sum u_z u_y, sum u_z u_x, sum u_y u_y, sum u_y u_x, sum u_x u_x } over the pixels of l (2D: u_z = 0).
//
// Contour counts (2D).  counts[l] = { n_1, n_r2, n_h, h_1 .. h_15 }:
//   border pixel of l   a pixel of l with a 4-neighbour that is not l (outside the image and other labels are not l).  For a border
//                       pixel, a = its 4-neighbours that are border pixels of l, d = the same among its diagonal neighbours; it
//                       counts into n_1 for (a, d) in {(2,0) (3,0) (2,1) (3,1) (2,2) (3,2)}, into n_r2 for {(0,2) (1,3)}, into n_h for
//                       {(1,1) (1,2)}: skimage.measure.perimeter(mask, 4)'s codes 1 + 2 a + 10 d with weights 1, sqrt 2, (1 + sqrt 2) / 2.
//   2 x 2 windows       for every window position i in [0, Y], j in [0, X] and every label l in the window, code = 1 [L(i,j) = l] +
//                       2 [L(i-1,j) = l] + 4 [L(i,j-1) = l] + 8 [L(i-1,j-1) = l] and h_code[l] += 1.  Here a window is counted by
//                       one of its pixels: the pixel of l whose bit is the lowest set bit of the code.  Every pixel looks at the four
//                       windows it lies in, so no thread is needed for the row i = Y and the column j = X.
// A pixel's counts need the labels within two pixels of it (a 5 x 5 footprint): border bits of its eight neighbours, each from that
// neighbour's own four neighbours.  A tile of MSH_TILE_Y x MSH_TILE_X pixels therefore reads labels with a halo of 2 (tile_label:
// 0 outside the image and for values outside 1 .. max_label) and computes border bits with a halo of 1.
//
// Packing.  What a pixel adds to the 18 counters of its label fits three 64-bit words of six 10-bit fields each: a pixel adds at
// most 1 to any field (the windows it counts have different lowest bits) and the 64 pixels of a wave at most 64 < 1024, so whole
// words can be added across the lanes of a run of equal labels without a carry between fields.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MSH_HD __host__ __device__ __forceinline__
#else
#define MSH_HD inline
#endif

namespace measure_shape {

enum {
  MSH_TILE_Y = 16, MSH_TILE_X = 64,                                    // pixels of a tile: one wave per row, four rows per wave
  MSH_HALO = 2,                                                        // labels are read this far around the tile
  MSH_LY = MSH_TILE_Y + 2 * MSH_HALO, MSH_LX = MSH_TILE_X + 2 * MSH_HALO,   // the label tile
  MSH_BY = MSH_TILE_Y + 2, MSH_BX = MSH_TILE_X + 2,                    // the border-bit tile (halo 1)
  MSH_COUNTS = 18, MSH_FIELD_BITS = 10, MSH_FIELDS_PER_WORD = 6, MSH_WORDS = 3,
  MSH_N1 = 0, MSH_NR2 = 1, MSH_NH = 2, MSH_H0 = 2                      // counter of configuration `code` (1 .. 15): MSH_H0 + code
};

MSH_HD int clamp_to(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the label of pixel (y, x) of plane z as the tables see it: 0 outside the image and for values outside 1 .. max_label; 64-bit offset
MSH_HD int tile_label(const int32_t* lbl, int Y, int X, int max_label, long long z, long long y, long long x) {
  if (y < 0 || y >= Y || x < 0 || x >= X) return 0;
  const int v = lbl[(z * Y + y) * (long long)X + x];
  return (v >= 1 && v <= max_label) ? v : 0;
}

// the six products of the local coordinates, in the table's order
MSH_HD void moment_terms(long long uz, long long uy, long long ux, long long* t) {
  t[0] = uz * uz; t[1] = uz * uy; t[2] = uz * ux; t[3] = uy * uy; t[4] = uy * ux; t[5] = ux * ux;
}

// the start of a box of sd_label_boxes_device's table, clamped to the image
MSH_HD void box_start(const int32_t* t, int Z, int Y, int X, int* z0, int* y0, int* x0) {
  *z0 = clamp_to(t[0], 0, Z); *y0 = clamp_to(t[1], 0, Y); *x0 = clamp_to(t[2], 0, X);
}

// the counter a border pixel with a / d border neighbours of its label along the axes / the diagonals counts into; -1: none
MSH_HD int contour_class(int a, int d) {
  if ((a == 2 || a == 3) && d <= 2) return MSH_N1;
  if ((a == 0 && d == 2) || (a == 1 && d == 3)) return MSH_NR2;
  if (a == 1 && (d == 1 || d == 2)) return MSH_NH;
  return -1;
}

MSH_HD void add_field(unsigned long long* w, int field) {
  w[field / MSH_FIELDS_PER_WORD] += 1ull << (MSH_FIELD_BITS * (field % MSH_FIELDS_PER_WORD));
}

MSH_HD int get_field(const unsigned long long* w, int field) {
  return (int)((w[field / MSH_FIELDS_PER_WORD] >> (MSH_FIELD_BITS * (field % MSH_FIELDS_PER_WORD))) & ((1u << MSH_FIELD_BITS) - 1u));
}

// border bit of the pixel at (ly, lx) of the label tile (row stride MSH_LX); 1 <= ly < MSH_LY - 1, 1 <= lx < MSH_LX - 1
MSH_HD int border_bit(const int32_t* tile, int ly, int lx) {
  const int32_t* p = tile + ly * MSH_LX + lx;
  const int l = p[0];
  return l != 0 && (p[-MSH_LX] != l || p[MSH_LX] != l || p[-1] != l || p[1] != l);
}

// what the pixel at (ty, tx) of the tile (0 <= ty < MSH_TILE_Y, 0 <= tx < MSH_TILE_X) adds to the counters of its label, packed;
// returns the label (0: background, w stays 0).  tile: labels, halo 2; border: border bits, halo 1 (row stride MSH_BX).
MSH_HD int pixel_counts(const int32_t* tile, const uint8_t* border, int ty, int tx, unsigned long long* w) {
  w[0] = w[1] = w[2] = 0;
  const int32_t* p = tile + (ty + MSH_HALO) * MSH_LX + tx + MSH_HALO;
  const int l = p[0];
  if (l == 0) return 0;
  const uint8_t* b = border + (ty + 1) * MSH_BX + tx + 1;
  if (b[0]) {
    const int a = (p[-MSH_LX] == l && b[-MSH_BX]) + (p[MSH_LX] == l && b[MSH_BX]) + (p[-1] == l && b[-1]) + (p[1] == l && b[1]);
    const int d = (p[-MSH_LX - 1] == l && b[-MSH_BX - 1]) + (p[-MSH_LX + 1] == l && b[-MSH_BX + 1]) + (p[MSH_LX - 1] == l && b[MSH_BX - 1]) +
                  (p[MSH_LX + 1] == l && b[MSH_BX + 1]);
    const int cls = contour_class(a, d);
    if (cls >= 0) add_field(w, cls);
  }
  // the four windows this pixel lies in: window (i, j) = (y + di, x + dj) holds the pixels (i, j) bit 1, (i-1, j) bit 2, (i, j-1)
  // bit 4, (i-1, j-1) bit 8; this pixel is its pixel (i - di, j - dj), bit 1 << (di + 2 dj)
  for (int dj = 0; dj < 2; ++dj)
    for (int di = 0; di < 2; ++di) {
      const int32_t* q = p + di * MSH_LX + dj;                         // pixel (i, j) of the window
      const int code = (q[0] == l) | ((q[-MSH_LX] == l) << 1) | ((q[-1] == l) << 2) | ((q[-MSH_LX - 1] == l) << 3);
      const int mine = 1 << (di + 2 * dj);
      if ((code & (mine - 1)) == 0) add_field(w, MSH_H0 + code);       // no pixel of l with a lower bit: this one counts the window
    }
  return l;
}

}  // namespace measure_shape
