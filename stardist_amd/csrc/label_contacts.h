// label_contacts.h -- the per-pixel and per-wave rules of the contact table (stardist_amd.utils.label_contacts):
// which pixel pairs a pixel tests, the key of a contact, and how the 64 lanes of a wave combine equal keys into runs.
//
// Everything here is __host__ __device__ and free of HIP headers when compiled by a host compiler: csrc/label_contacts.hip runs it with
// one lane per pixel of a tile row, tests/host/label_contacts_check.cpp with plain loops over the same tiles, rows and lanes.  Integer
// arithmetic only.
//
// The definition.  The forward offsets of a connectivity c are the offsets (dz, dy, dx) in {-1, 0, 1}^3 with at most c non-zero
// coordinates that are lexicographically positive: every unordered pair of neighbouring pixels once.  A contact is a pixel pair
// (p, p + o), o a forward offset, both inside the image, with L(p) != L(p + o); its key is (min, max) of the two labels.  The image
// edge is no contact.
//
// The tile is csrc/label_edit.h's, with its halo of 1.  A cell outside the image holds the clamped pixel there.  For an offset along
// one axis that is the pixel itself (no contact), but for a diagonal offset it is a real, different pixel of the image, so the
// neighbour's coordinates are tested against the image here, always.
#pragma once
#include "label_edit.h"

namespace label_contacts {

using label_edit::Origin;
using label_edit::Tile;

enum {
  LC_WAVE = 64,             // lanes of a wave = pixels of a tile row (LE_TILE_X)
  LC_FIRST_CODE = 14,       // offset codes: code = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); 13 is the pixel itself, every later code is
  LC_CODES_2D = 18,         // lexicographically positive: 14 .. 17 stay in the plane, 18 .. 26 go one plane up
  LC_CODES_3D = 27
};
static_assert((int)LC_WAVE == (int)label_edit::LE_TILE_X, "a wave holds one row of a tile");

constexpr unsigned long long LC_NO_KEY = ~0ull;         // a lane without a contact; no key has more than 62 bits

struct Offset { int dz, dy, dx, moved; };   // moved: the number of non-zero coordinates

LE_HD Offset offset_of(int code) {
  Offset o;
  o.dz = code / 9 - 1; o.dy = (code / 3) % 3 - 1; o.dx = code % 3 - 1;
  o.moved = (o.dz != 0) + (o.dy != 0) + (o.dx != 0);
  return o;
}

// one past the last offset code of a tile: a tile without a halo along z (an image, a volume of one plane) has no plane above
LE_HD int code_count(const Tile& g) { return g.hz ? (int)LC_CODES_3D : (int)LC_CODES_2D; }

LE_HD int bits_of(int v) {
  int b = 0;
  for (unsigned u = v <= 0 ? 0u : (unsigned)v; u; u >>= 1) ++b;
  return b;
}

// the key of the pair of labels a != b, both >= 0: min << bits | max, bits = bits_of(largest label) <= 31
LE_HD unsigned long long pair_key(int a, int b, int bits) {
  const unsigned lo = (unsigned)(a < b ? a : b), hi = (unsigned)(a < b ? b : a);
  return ((unsigned long long)lo << bits) | (unsigned long long)hi;
}

// the key of the contact of tile pixel (lz, ly, lx) along offset o, or LC_NO_KEY: the pixel or its neighbour lies outside the image,
// the two labels are equal, or one of them is 0 and the background is not asked for.  cells[]: the tile's local array
LE_HD unsigned long long contact_key(const int* cells, const Tile& g, const Origin& org, int lz, int ly, int lx, const Offset& o,
                                     int with_background, int bits) {
  if (!label_edit::in_image(g, org, lz, ly, lx)) return LC_NO_KEY;
  const int nz = org.z + lz + o.dz, ny = org.y + ly + o.dy, nx = org.x + lx + o.dx;
  if (nz < 0 || nz >= g.Z || ny < 0 || ny >= g.Y || nx < 0 || nx >= g.X) return LC_NO_KEY;
  const int centre_at = ((lz + g.hz) * g.cy + (ly + 1)) * g.cx + (lx + 1);
  const int a = cells[centre_at], b = cells[centre_at + (o.dz * g.cy + o.dy) * g.cx + o.dx];
  if (a == b || (!with_background && (a == 0 || b == 0))) return LC_NO_KEY;
  return pair_key(a, b, bits);
}

// ---- runs of equal keys among the 64 lanes of a wave (one row of a tile, one offset).  Lane l starts a run where l = 0 or its key
// differs from lane l - 1's; a run of LC_NO_KEY separates two runs like any other and is not emitted.  Every lane's term is 1, so the
// sum of a run -- what csrc/wave_runs.h gets by its segmented shuffle reduction -- is the run's length, read off the ballot of heads.
LE_HD bool run_head(unsigned long long key, unsigned long long key_before, int lane) { return lane == 0 || key != key_before; }

LE_HD int first_bit(unsigned long long m) {          // m != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffsll((long long)m) - 1;
#else
  return __builtin_ctzll(m);
#endif
}

LE_HD int bit_count(unsigned long long m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(m);
#else
  return __builtin_popcountll(m);
#endif
}

// the length of the run that starts at `lane`; heads: bit l = lane l starts a run
LE_HD int run_length(unsigned long long heads, int lane) {
  const unsigned long long later = (heads >> lane) >> 1;
  return later ? first_bit(later) + 1 : (int)LC_WAVE - lane;
}

// the place of lane's run among the wave's emitted runs; emits: bit l = lane l starts a run with a key
LE_HD int run_slot(unsigned long long emits, int lane) { return bit_count(emits & ((1ull << lane) - 1ull)); }

// the (label_a << 32 | label_b) form of a key, as the table holds it
LE_HD long long unpacked_key(unsigned long long key, int bits) {
  const unsigned long long lo = key >> bits, hi = key & ((1ull << bits) - 1ull);
  return (long long)((lo << 32) | hi);
}

}  // namespace label_contacts
