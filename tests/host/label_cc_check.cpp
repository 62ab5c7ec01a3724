// Host harness of stardist_amd/csrc/label_cc.h: what csrc/label_cc.hip does -- the tile decomposition, the tile's two local arrays,
// the index arithmetic, the four phases -- with plain loops in place of threads, tile by tile; with `reversed` the tiles and the
// pixels of every phase are visited in descending order, so that the result's independence of the order is exercised.  Every write
// of a union is checked for par[p] <= p.  Built by tests/test_cpu_label_components.py (g++) as a shared library; with
// -DLABEL_CC_CHECK_MAIN it is a stand-alone program (for a sanitizer build) that reads cases from a file and compares the labels.
#include <limits.h>
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../stardist_amd/csrc/label_cc.h"

using namespace label_cc;

namespace {

// plain memory behind the Mem interface; counts the writes that break par[p] <= p
struct CheckedMem {
  const int* base;
  long long violations;
  int load(const int* p) { return *p; }
  int min(int* p, int v) {
    const int old = *p;
    if (v < old) *p = v;
    if (*p > (int)(p - base)) ++violations;
    return old;
  }
};

template <typename T>
long long label(const T* img, int Z, int Y, int X, int connectivity, long long background, bool reversed, int* out, int* count) {
  const Geometry g = geometry_of(Z, Y, X);
  const int n = (int)((long long)Z * Y * X), n_offsets = offset_count(connectivity);
  const long long tiles = tile_count(g);
  long long violations = 0;
  std::vector<int> val(LCC_TILE_PIXELS), par(LCC_TILE_PIXELS);
  // in `reversed` order index i of a loop over m items is m - 1 - i
  const auto at = [reversed](long long i, long long m) { return reversed ? m - 1 - i : i; };
  for (long long i = 0; i < tiles; ++i) {
    const Origin o = tile_origin(g, at(i, tiles));
    CheckedMem mem = {par.data(), 0};
    for (int k = 0; k < LCC_TILE_PIXELS; ++k) tile_load<T>(g, o, (int)at(k, LCC_TILE_PIXELS), img, background, val.data(), par.data());
    for (int k = 0; k < LCC_TILE_PIXELS; ++k) tile_link(g, (int)at(k, LCC_TILE_PIXELS), n_offsets, val.data(), par.data(), mem);
    for (int k = 0; k < LCC_TILE_PIXELS; ++k) tile_store(g, o, (int)at(k, LCC_TILE_PIXELS), par.data(), out, mem);
    violations += mem.violations;
  }
  CheckedMem mem = {out, 0};
  for (int p = 0; p < n; ++p)
    if (out[p] > p) ++mem.violations;
  for (long long i = 0; i < tiles; ++i) {
    const Origin o = tile_origin(g, at(i, tiles));
    for (int k = 0; k < LCC_TILE_PIXELS; ++k) border_link<T>(g, o, (int)at(k, LCC_TILE_PIXELS), img, background, n_offsets, out, mem);
  }
  for (int p = 0; p < n; ++p) {
    flatten_pixel(out, (int)at(p, n), mem);
    if (out[at(p, n)] > at(p, n)) ++mem.violations;
  }
  std::vector<int> rank((size_t)n);
  int roots = 0;
  for (int p = 0; p < n; ++p) { rank[p] = roots; roots += is_root(out, p); }
  for (int p = 0; p < n; ++p) number_pixel(out, rank.data(), (int)at(p, n));
  *count = roots;
  return violations + mem.violations;
}

}  // namespace

extern "C" {

int lcc_tile_x() { return LCC_TILE_X; }
int lcc_tile_y() { return LCC_TILE_Y; }
int lcc_tile_z() { return LCC_TILE_Z; }
int lcc_vol_tile_y() { return LCC_VOL_TILE_Y; }
int lcc_tile_pixels() { return LCC_TILE_PIXELS; }

// what sd_label_components_device computes, with its argument checks: 0, -1 for bad arguments, -2 if a write broke par[p] <= p
int lcc_label(const void* img, int dtype, int Z, int Y, int X, int connectivity, long long background, int reversed, int* out, int* count) {
  if (!img || !out || !count || Z <= 0 || Y <= 0 || X <= 0 || connectivity < 1 || connectivity > 3) return -1;
  if ((long long)Z * Y > INT_MAX || (long long)Z * Y * X > INT_MAX) return -1;
  long long bad;
  if (dtype == LCC_U8) bad = label<uint8_t>((const uint8_t*)img, Z, Y, X, connectivity, background, reversed != 0, out, count);
  else if (dtype == LCC_U16) bad = label<uint16_t>((const uint16_t*)img, Z, Y, X, connectivity, background, reversed != 0, out, count);
  else if (dtype == LCC_I32) bad = label<int32_t>((const int32_t*)img, Z, Y, X, connectivity, background, reversed != 0, out, count);
  else return -1;
  return bad ? -2 : 0;
}

}  // extern "C"

#ifdef LABEL_CC_CHECK_MAIN
#include <stdio.h>
#include <string.h>
// argv[1]: a file of records {int32 dtype, Z, Y, X, connectivity, count; int64 background; the image; the expected labels (int32)};
// every record is labelled in both visiting orders and compared
int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int bad = 0, records = 0;
  for (;;) {
    int32_t head[6];
    int64_t background;
    if (fread(head, sizeof head, 1, f) != 1) break;
    if (fread(&background, sizeof background, 1, f) != 1) { ++bad; break; }
    const int dtype = head[0], Z = head[1], Y = head[2], X = head[3];
    const size_t n = (size_t)Z * Y * X, item = dtype == LCC_U8 ? 1 : dtype == LCC_U16 ? 2 : 4;
    // exact-size heap blocks: a read or write one element outside them is an error to the sanitizer
    std::vector<unsigned char> raw(n * item);
    std::vector<int32_t> want(n), got(n);
    if (fread(raw.data(), item, n, f) != n || fread(want.data(), 4, n, f) != n) { ++bad; break; }
    for (int reversed = 0; reversed < 2; ++reversed) {
      int count = -1;
      const int rc = lcc_label(raw.data(), dtype, Z, Y, X, head[4], background, reversed, got.data(), &count);
      if (rc != 0 || count != head[5] || memcmp(got.data(), want.data(), n * 4) != 0) {
        printf("record %d (%d x %d x %d, connectivity %d, reversed %d): rc %d, count %d, want %d\n", records, Z, Y, X, head[4], reversed, rc,
               count, head[5]);
        ++bad;
      }
    }
    ++records;
  }
  fclose(f);
  printf("%d records, %d bad\n", records, bad);
  return bad || !records ? 1 : 0;
}
#endif
