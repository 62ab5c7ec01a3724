// fill_holes.h -- the bit-plane arithmetic of fill_label_holes (stardist/utils.py:137-153) for one object.
//
// Everything here is __host__ __device__ and free of HIP headers when compiled by a host compiler: csrc/fill_holes.hip runs the passes
// with one thread per row / column, tests/host/fill_holes_check.cpp with plain loops, and tests/test_cpu_fill_holes.py compares the
// latter with the host function.
//
// What is computed (equal to the reference's per-object binary_fill_holes on the grown bounding box, default cross structure):
//   out = max(lbl, 0); for every label L > 0 present, free = (lbl != L) on bbox(L); a 4- / 6-connected component of free that holds no
//   pixel of the outermost layer of the box (first and last index along every axis the image has) is a hole; out = max(out, L) there.
//
// Planes: one bit per pixel of the box, rows padded to 32-bit words: wx = ceil(bx / 32) words per row, rows = bz * by, words = rows * wx
// per plane; bit (x & 31) of word (z * by + y) * wx + (x >> 5), x counted from the box's first column.  The pad bits of a row's last
// word are 0 in both planes (not free: a wall).  Two planes per object: `free`, and `reach` = the free pixels connected to the outer
// layer.  reach starts as free & outer layer and grows to the fixpoint of
//   row pass     along x: every run of free bits that holds a reach bit becomes reach, across word boundaries (fill_row)
//   column pass  along y (and z): reach[k] |= reach[k -+ 1] & free[k], swept down and then up (sweep_column)
// Each pass only adds bits that belong to the least fixpoint, so the order of the passes, and which thread runs which row, cannot
// change the result; the loop ends when a whole round adds nothing.  holes = free & ~reach.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FH_HD __host__ __device__ __forceinline__
#else
#define FH_HD inline
#endif

namespace fillholes {

// LDS budget of one object, in 32-bit words, for its two planes together (64 KiB: two workgroups per CU); an object whose planes
// need more keeps them in global memory.  Objects whose planes fit FH_WAVE_WORDS (4 KiB: a 64 x 64 box needs 256 words) are worked
// off by single-wave workgroups, of which a CU holds many at once.
enum { FH_LDS_WORDS = 16384, FH_WAVE_WORDS = 1024 };

struct Geo {
  int z0, y0, x0;      // first pixel of the box in the image
  int bz, by, bx;      // box extents
  int wx;              // words per row
  int rows;            // bz * by
  long long words;     // per plane
};

// box = {z0, y0, x0, z1, y1, x1}, stops exclusive
FH_HD Geo geo_of(const int32_t* box) {
  Geo g;
  g.z0 = box[0]; g.y0 = box[1]; g.x0 = box[2];
  g.bz = box[3] - box[0]; g.by = box[4] - box[1]; g.bx = box[5] - box[2];
  g.wx = (g.bx + 31) >> 5;
  g.rows = g.bz * g.by;
  g.words = (long long)g.rows * g.wx;
  return g;
}

FH_HD bool fits_lds(const Geo& g) { return 2 * g.words <= (long long)FH_LDS_WORDS; }
FH_HD bool fits_wave(const Geo& g) { return 2 * g.words <= (long long)FH_WAVE_WORDS; }

// the bits of word w of a row that lie inside the box
FH_HD uint32_t valid_bits(const Geo& g, int w) {
  const int left = g.bx - 32 * w;
  return left >= 32 ? 0xffffffffu : ((1u << left) - 1u);
}

// word w of row (z, y) of the free plane: lbl is the whole image (Y, X its extents), L the object's label
FH_HD uint32_t free_word(const int32_t* __restrict__ lbl, int Y, int X, const Geo& g, int z, int y, int w, int L) {
  const int32_t* p = lbl + ((long long)(g.z0 + z) * Y + (g.y0 + y)) * X + g.x0 + 32 * w;
  const int n = g.bx - 32 * w < 32 ? g.bx - 32 * w : 32;
  uint32_t m = 0;
  for (int k = 0; k < n; ++k) m |= (uint32_t)(p[k] != L) << k;
  return m;
}

// word w of row (z, y) of the outer layer; the z axis takes part only where the image has one (volume != 0)
FH_HD uint32_t outer_word(const Geo& g, int volume, int z, int y, int w) {
  const uint32_t v = valid_bits(g, w);
  if (y == 0 || y == g.by - 1 || (volume && (z == 0 || z == g.bz - 1))) return v;
  uint32_t m = 0;
  if (w == 0) m |= 1u;
  if (w == g.wx - 1) m |= 1u << ((g.bx - 1) & 31);
  return m & v;
}

// reach spread towards higher bits along runs of free bits, inside one word (r is a subset of f)
FH_HD uint32_t spread_up(uint32_t r, uint32_t f) {
  r |= f & (r << 1);  f &= f << 1;
  r |= f & (r << 2);  f &= f << 2;
  r |= f & (r << 4);  f &= f << 4;
  r |= f & (r << 8);  f &= f << 8;
  r |= f & (r << 16);
  return r;
}

FH_HD uint32_t spread_down(uint32_t r, uint32_t f) {
  r |= f & (r >> 1);  f &= f >> 1;
  r |= f & (r >> 2);  f &= f >> 2;
  r |= f & (r >> 4);  f &= f >> 4;
  r |= f & (r >> 8);  f &= f >> 8;
  r |= f & (r >> 16);
  return r;
}

// Row pass: one row of wx words.  Left to right with the carry "the last pixel of the previous word is reached", then right to left
// with "the first pixel of the next word is reached"; after both, every run of the row that held a reach bit is reach.  Returns
// whether a bit was added.
template <typename P, typename Q>
FH_HD bool fill_row(P reach, Q free_, int wx) {
  bool changed = false;
  uint32_t carry = 0;
  for (int w = 0; w < wx; ++w) {
    const uint32_t f = free_[w], r0 = reach[w];
    const uint32_t r = spread_up((r0 | carry) & f, f);
    carry = r >> 31;
    if (r != r0) { reach[w] = r; changed = true; }
  }
  carry = 0;
  for (int w = wx - 1; w >= 0; --w) {
    const uint32_t f = free_[w], r0 = reach[w];
    const uint32_t r = spread_down((r0 | carry) & f, f);
    carry = (r & 1u) << 31;
    if (r != r0) { reach[w] = r; changed = true; }
  }
  return changed;
}

// Column pass: the n words reach[k * stride], k = 0 .. n - 1 (one word column along y or z): down, then up.
template <typename P, typename Q>
FH_HD bool sweep_column(P reach, Q free_, int n, long long stride) {
  bool changed = false;
  uint32_t above = 0;
  for (int k = 0; k < n; ++k) {
    const uint32_t r0 = reach[k * stride];
    const uint32_t r = r0 | (above & free_[k * stride]);
    if (r != r0) { reach[k * stride] = r; changed = true; }
    above = r;
  }
  above = 0;
  for (int k = n - 1; k >= 0; --k) {
    const uint32_t r0 = reach[k * stride];
    const uint32_t r = r0 | (above & free_[k * stride]);
    if (r != r0) { reach[k * stride] = r; changed = true; }
    above = r;
  }
  return changed;
}

// The three passes of a round, by item: rows = g.rows row items; y columns = bz * wx items (z, w); z columns = by * wx items (y, w).
template <typename P, typename Q>
FH_HD bool pass_rows(P reach, Q free_, const Geo& g, int item) {
  return fill_row(reach + (long long)item * g.wx, free_ + (long long)item * g.wx, g.wx);
}
template <typename P, typename Q>
FH_HD bool pass_y(P reach, Q free_, const Geo& g, int item) {
  const long long at = (long long)(item / g.wx) * g.by * g.wx + item % g.wx;
  return sweep_column(reach + at, free_ + at, g.by, g.wx);
}
template <typename P, typename Q>
FH_HD bool pass_z(P reach, Q free_, const Geo& g, int item) {
  return sweep_column(reach + item, free_ + item, g.bz, (long long)g.by * g.wx);
}

}  // namespace fillholes
