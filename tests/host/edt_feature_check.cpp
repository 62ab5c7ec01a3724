// Host harness of stardist_amd/csrc/edt_feature.h: what csrc/edt_feature.hip does -- the passes in scipy's axis order, the carried
// (value, index) arrays, the epilogue -- with plain loops in place of threads, on exact-size heap blocks.  Built by
// tests/test_cpu_expand_labels.py (g++ -ffp-contract=off) as a shared library; with -DEDT_FEATURE_CHECK_MAIN it is a stand-alone
// program (for a sanitizer build) that reads cases from a file and compares the results bit for bit.
#include <limits.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../stardist_amd/csrc/edt_feature.h"

using namespace edt_feature;

namespace {

template <typename T>
void run(const T* img, int Z, int Y, int X, int feature_is_zero, double sz, double sy, double sx, double bound, const int* lbl, int* out_lbl,
         int* out_idx, double* out_dist) {
  const long long n = (long long)Z * Y * X;
  std::vector<double> val((size_t)n), val2(Z > 1 ? (size_t)n : 0);
  std::vector<int> idx((size_t)n), idx2(Z > 1 ? (size_t)n : 0);
  const ImageSource<T> src = {img, feature_is_zero};
  if (Z > 1) {
    for (long long p = 0; p < n; ++p) first_pass_pixel(src, p, (long long)Y * X, Z, sz, bound, val.data(), idx.data());
    for (long long p = 0; p < n; ++p) middle_pass_pixel(val.data(), idx.data(), p, (long long)X, Y, sy, bound, val2.data(), idx2.data());
    for (long long p = 0; p < n; ++p) last_pass_pixel(val2.data(), idx2.data(), p, X, sx, bound, lbl, out_lbl, out_idx, out_dist);
  } else {
    for (long long p = 0; p < n; ++p) first_pass_pixel(src, p, (long long)X, Y, sy, bound, val.data(), idx.data());
    for (long long p = 0; p < n; ++p) last_pass_pixel(val.data(), idx.data(), p, X, sx, bound, lbl, out_lbl, out_idx, out_dist);
  }
}

bool bad_geometry(int Z, int Y, int X, double sz, double sy, double sx) {
  if (Z <= 0 || Y <= 0 || X <= 0 || (long long)Z * Y > INT_MAX || (long long)Z * Y * X > INT_MAX) return true;
  return !(sz > 0) || !(sy > 0) || !(sx > 0) || sz == inf() || sy == inf() || sx == inf();
}

}  // namespace

extern "C" {

int edtf_threads() { return EDTF_THREADS; }

// what sd_nearest_feature_device computes, with its argument checks: 0, or -1 for bad arguments
int edtf_nearest(const void* img, int dtype, int Z, int Y, int X, int feature_is_zero, double sz, double sy, double sx, double max_distance,
                 int32_t* index, double* dist) {
  if (!img || bad_geometry(Z, Y, X, sz, sy, sx) || max_distance != max_distance || (feature_is_zero != 0 && feature_is_zero != 1)) return -1;
  const double bound = bound_of(max_distance);
  if (dtype == EDTF_U8) run<uint8_t>((const uint8_t*)img, Z, Y, X, feature_is_zero, sz, sy, sx, bound, nullptr, nullptr, index, dist);
  else if (dtype == EDTF_U16) run<uint16_t>((const uint16_t*)img, Z, Y, X, feature_is_zero, sz, sy, sx, bound, nullptr, nullptr, index, dist);
  else if (dtype == EDTF_I32) run<int32_t>((const int32_t*)img, Z, Y, X, feature_is_zero, sz, sy, sx, bound, nullptr, nullptr, index, dist);
  else return -1;
  return 0;
}

// what sd_expand_labels_device computes, with its argument checks
int edtf_expand(const int32_t* lbl, int Z, int Y, int X, double sz, double sy, double sx, double distance, int32_t* out) {
  if (!lbl || !out || lbl == out || bad_geometry(Z, Y, X, sz, sy, sx) || !(distance >= 0)) return -1;
  run<int32_t>(lbl, Z, Y, X, 0, sz, sy, sx, distance, lbl, out, nullptr, nullptr);
  return 0;
}

}  // extern "C"

#ifdef EDT_FEATURE_CHECK_MAIN
#include <stdio.h>
// argv[1]: a file of records {int32 kind, dtype, Z, Y, X, feature_is_zero; float64 sz, sy, sx, distance; the image; then for kind 0
// (nearest feature; distance = max_distance) the expected indices (int32) and distances (float64), for kind 1 (expand; int32 image) the
// expected labels (int32)}; compared as bytes
int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int bad = 0, records = 0;
  for (;;) {
    int32_t head[6];
    double par[4];
    if (fread(head, sizeof head, 1, f) != 1) break;
    if (fread(par, sizeof par, 1, f) != 1) { ++bad; break; }
    const int kind = head[0], dtype = head[1], Z = head[2], Y = head[3], X = head[4];
    const size_t n = (size_t)Z * Y * X, item = dtype == EDTF_U8 ? 1 : dtype == EDTF_U16 ? 2 : 4;
    // exact-size heap blocks: a read or write one element outside them is an error to the sanitizer
    std::vector<unsigned char> raw(n * item);
    std::vector<int32_t> want(n), got(n, -7);
    if (fread(raw.data(), item, n, f) != n || fread(want.data(), 4, n, f) != n) { ++bad; break; }
    int rc;
    bool same;
    if (kind == 0) {
      std::vector<double> want_dist(n), got_dist(n, -7.0);
      if (fread(want_dist.data(), 8, n, f) != n) { ++bad; break; }
      rc = edtf_nearest(raw.data(), dtype, Z, Y, X, head[5], par[0], par[1], par[2], par[3], got.data(), got_dist.data());
      same = memcmp(got.data(), want.data(), n * 4) == 0 && memcmp(got_dist.data(), want_dist.data(), n * 8) == 0;
    } else {
      rc = edtf_expand((const int32_t*)raw.data(), Z, Y, X, par[0], par[1], par[2], par[3], got.data());
      same = memcmp(got.data(), want.data(), n * 4) == 0;
    }
    if (rc != 0 || !same) {
      printf("record %d (kind %d, %d x %d x %d, spacing %g %g %g, distance %g): rc %d, %s\n", records, kind, Z, Y, X, par[0], par[1], par[2],
             par[3], rc, same ? "equal" : "different");
      ++bad;
    }
    ++records;
  }
  fclose(f);
  printf("%d records, %d bad\n", records, bad);
  return bad || !records ? 1 : 0;
}
#endif
