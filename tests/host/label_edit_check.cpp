// label_edit_check.cpp -- the per-pixel rules of stardist_amd/csrc/label_edit.h on the host, in the order the kernels of
// csrc/label_edit.hip visit the pixels: tile after tile with the tile's cells in a local array, band pixel after band pixel, quad
// after quad.  A stand-alone program: it reads the records tests/test_cpu_label_edit.py wrote (inputs and the host routes' results),
// recomputes every result and compares.  It is built plain and under the address and undefined-behaviour sanitizers.
//
//   label_edit_check <records file>      prints "<n> records, <bad> bad"; exit status 0 only with 0 bad
//
// A record: int32 kind, Z, Y, X, a, b; int64 c, d; then the arrays of its kind (n = Z * Y * X):
//   kind 0  find_boundaries   a = connectivity, b = mode, c = background, d = sentinel; int32 lbl[n]; uint8 want[n]
//   kind 1  border flags + clear   a = ndim, b = buffer_size (-1: with a mask), c = bgval, d = n_flags; int32 val[n]; int32 key[n];
//           with a mask uint8 mask[n]; int32 want[n]
//   kind 2  clear by a table of flags   c = bgval, d = n_flags; int32 val[n]; int32 key[n]; uint8 flags[n_flags]; int32 want[n]
#include "../../stardist_amd/csrc/label_edit.h"

#include <limits.h>
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace label_edit;

// what sd_find_boundaries_device computes, with its argument checks
static int find_boundaries(const int* lbl, int Z, int Y, int X, int connectivity, int mode, long long background, long long sentinel,
                           unsigned char* out) {
  if (!lbl || !out || Z <= 0 || Y <= 0 || X <= 0) return -1;
  if (connectivity < 1 || connectivity > 3 || mode < LE_THICK || mode > LE_OUTER) return -1;
  if ((long long)Z * Y > INT_MAX || (long long)Z * Y * X > INT_MAX) return -1;
  const Tile g = tile_of(Z, Y, X);
  std::vector<int> cells(LE_LDS_CELLS);
  if (cell_count(g) > (int)LE_LDS_CELLS) return -2;
  for (long long t = 0; t < tile_count(g); ++t) {
    const Origin o = tile_origin(g, t);
    cells.assign(LE_LDS_CELLS, INT_MIN);                                   // a cell that is read without having been loaded shows
    for (int c = 0; c < cell_count(g); ++c) cells[c] = lbl[cell_source(g, o, c)];
    for (int l = 0; l < LE_TILE_PIXELS; ++l) {
      int lz, ly, lx;
      local_coords(g, l, lz, ly, lx);
      if (lz >= g.tz || !in_image(g, o, lz, ly, lx)) continue;
      out[global_index(g, o, lz, ly, lx)] = boundary_at(cells.data(), g, lz, ly, lx, connectivity, mode, background, sentinel);
    }
  }
  return 0;
}

// sd_label_border_flags_device
static int border_flags(const int* key, int Z, int Y, int X, int ndim, int buffer_size, const unsigned char* mask, long long n_flags,
                        unsigned char* flags) {
  if (!key || !flags || Z <= 0 || Y <= 0 || X <= 0 || n_flags <= 0) return -1;
  if ((ndim != 2 && ndim != 3) || (ndim == 2 && Z != 1) || (!mask && buffer_size < 0)) return -1;
  memset(flags, 0, (size_t)n_flags);
  const long long n = (long long)Z * Y * X;
  if (mask) {
    for (long long p = 0; p < n; ++p)
      if (!mask[p]) flag_pixel(key, p, flags, n_flags);
    return 0;
  }
  const Band b = band_of(Z, Y, X, ndim == 3, buffer_size + 1);
  const long long count = band_count(b);
  std::vector<unsigned char> seen((size_t)n, 0);
  for (long long t = 0; t < count; ++t) {
    const long long p = band_pixel(b, t);
    if (p < 0 || p >= n || seen[(size_t)p]) return -2;                      // every band pixel once, none outside the image
    seen[(size_t)p] = 1;
    flag_pixel(key, p, flags, n_flags);
  }
  return 0;
}

// sd_label_clear_flagged_device
static int clear_flagged(const int* val, const int* key, const unsigned char* flags, long long n_flags, long long n, int bgval, int* out) {
  if (!val || !key || !flags || !out || n <= 0 || n_flags <= 0) return -1;
  for (long long p = 0; p < n; ++p) out[p] = cleared_value(val[p], key[p], flags, n_flags, bgval);
  return 0;
}

template <typename T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n ? n : 1);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <records file>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int records = 0, bad = 0;
  for (;;) {
    int head[6];
    long long tail[2];
    if (fread(head, sizeof(int), 6, f) != 6) break;
    if (fread(tail, sizeof(long long), 2, f) != 2) { fprintf(stderr, "truncated record\n"); return 2; }
    const int kind = head[0], Z = head[1], Y = head[2], X = head[3];
    const size_t n = (size_t)Z * Y * X;
    std::vector<int> val, key, want, got(n ? n : 1, -5);
    std::vector<unsigned char> bytes, want8, got8(n ? n : 1, 7), flags;
    bool ok = true;
    int rc = 0;
    if (kind == 0) {
      ok = read_n(f, val, n) && read_n(f, want8, n);
      if (ok) rc = find_boundaries(val.data(), Z, Y, X, head[4], head[5], tail[0], tail[1], got8.data());
      if (ok && (rc != 0 || memcmp(got8.data(), want8.data(), n) != 0)) {
        ++bad;
        printf("record %d (find_boundaries %d x %d x %d, connectivity %d, mode %d): rc %d\n", records, Z, Y, X, head[4], head[5], rc);
      }
    } else if (kind == 1 || kind == 2) {
      const long long n_flags = tail[1];
      ok = read_n(f, val, n) && read_n(f, key, n);
      flags.assign((size_t)(n_flags > 0 ? n_flags : 1), 9);
      if (kind == 1) {
        const bool with_mask = head[5] < 0;
        if (ok && with_mask) ok = read_n(f, bytes, n);
        if (ok) rc = border_flags(key.data(), Z, Y, X, head[4], head[5], with_mask ? bytes.data() : nullptr, n_flags, flags.data());
      } else {
        ok = ok && read_n(f, flags, (size_t)n_flags);
      }
      ok = ok && read_n(f, want, n);
      if (ok && rc == 0) rc = clear_flagged(val.data(), key.data(), flags.data(), n_flags, (long long)n, (int)tail[0], got.data());
      if (ok && (rc != 0 || memcmp(got.data(), want.data(), n * sizeof(int)) != 0)) {
        ++bad;
        printf("record %d (kind %d, %d x %d x %d): rc %d\n", records, kind, Z, Y, X, rc);
      }
    } else {
      fprintf(stderr, "unknown record kind %d\n", kind);
      return 2;
    }
    if (!ok) { fprintf(stderr, "truncated record %d\n", records); return 2; }
    ++records;
  }
  fclose(f);
  // the argument checks of the entry points
  {
    int one = 1, out = 0;
    unsigned char o8 = 0, fl[2];
    const bool checks = find_boundaries(nullptr, 1, 1, 1, 1, 0, 0, 0, &o8) == -1 && find_boundaries(&one, 1, 0, 1, 1, 0, 0, 0, &o8) == -1 &&
                        find_boundaries(&one, 1, 1, 1, 0, 0, 0, 0, &o8) == -1 && find_boundaries(&one, 1, 1, 1, 4, 0, 0, 0, &o8) == -1 &&
                        find_boundaries(&one, 1, 1, 1, 1, 3, 0, 0, &o8) == -1 && find_boundaries(&one, 2, 1 << 15, 1 << 15, 1, 0, 0, 0, &o8) == -1 &&
                        find_boundaries(&one, 1, 1, 1, 1, 0, 0, 0, &o8) == 0 && o8 == 0 &&
                        border_flags(&one, 1, 1, 1, 4, 0, nullptr, 2, fl) == -1 && border_flags(&one, 2, 1, 1, 2, 0, nullptr, 2, fl) == -1 &&
                        border_flags(&one, 1, 1, 1, 2, -1, nullptr, 2, fl) == -1 && border_flags(&one, 1, 1, 1, 2, 0, nullptr, 0, fl) == -1 &&
                        border_flags(&one, 1, 1, 1, 2, 0, nullptr, 2, fl) == 0 && fl[0] == 0 && fl[1] == 1 &&
                        clear_flagged(&one, &one, fl, 2, 0, 0, &out) == -1 && clear_flagged(&one, &one, fl, 2, 1, 5, &out) == 0 && out == 5;
    if (!checks) { ++bad; printf("argument checks failed\n"); }
  }
  printf("%d records, %d bad\n", records, bad);
  return bad ? 1 : 0;
}
