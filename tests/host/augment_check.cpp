// Host harness of stardist_amd/csrc/augment.h: what csrc/augment.hip does -- one augment_pixel per output pixel of every sample, after
// the entry point's check of the index maps -- with plain loops in place of threads.  Built by tests/test_cpu_augment.py (g++
// -ffp-contract=off) as a shared library; with -DAUGMENT_CHECK_MAIN it is a stand-alone program (for a sanitizer build) that reads cases
// from a file, runs them on exact-size heap blocks and compares the results, NaN matching NaN by position.
#include <limits.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../stardist_amd/csrc/augment.h"

using namespace augment;

extern "C" {

int aug_sample_bytes() { return (int)sizeof(Sample); }

// one Philox4x32-10 block, for the known answers
void aug_philox(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
  uint32_t c[4] = {counter[0], counter[1], counter[2], counter[3]};
  philox4x32_10(c, key[0], key[1]);
  memcpy(out, c, sizeof c);
}

// what sd_augment_batch_device computes, with its argument checks: 0, or -1 for bad arguments
int aug_batch(const float* x, const int32_t* y, int B, int nd, const int* shape, int flags, const void* table, const float* disp, int n_disp,
              float* ox, int32_t* oy) {
  if (!x || !y || !ox || !oy || !shape || !table || x == ox || y == oy) return -1;
  if ((nd != 2 && nd != 3) || B < 1 || B > 65535 || flags < 0 || flags > (AUG_WARP | AUG_REFLECT | AUG_INTENSITY | AUG_NOISE)) return -1;
  if (n_disp < 0 || n_disp > nd || (n_disp > 0) != (disp != nullptr) || (n_disp > 0 && !(flags & AUG_WARP))) return -1;
  Plan P;
  memset(&P, 0, sizeof(P));
  P.nd = nd; P.B = B; P.flags = flags; P.na = n_disp; P.npix = 1;
  for (int d = 0; d < nd; ++d) {
    if (shape[d] < 1) return -1;
    P.n[d] = shape[d];
    P.npix *= shape[d];
    if (P.npix > INT_MAX) return -1;
  }
  const Sample* tab = (const Sample*)table;
  if (check_table(P, tab)) return -1;
  for (int b = 0; b < B; ++b) {
    const long long at = (long long)b * P.npix;
    for (long long pix = 0; pix < P.npix; ++pix) {
      if (nd == 2) augment_pixel<2>(P, tab[b], x + at, y + at, disp ? disp + at * P.na : nullptr, pix, ox + at, oy + at);
      else augment_pixel<3>(P, tab[b], x + at, y + at, disp ? disp + at * P.na : nullptr, pix, ox + at, oy + at);
    }
  }
  return 0;
}

}  // extern "C"

#ifdef AUGMENT_CHECK_MAIN
#include <stdio.h>
// argv[1]: a file of records {int32 B, nd, n0, n1, n2, flags, n_disp; B table rows; x (float32); y (int32); the displacement field
// (B * n_disp * npix float32); the expected x and y}
int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int bad = 0, records = 0;
  for (;;) {
    int32_t head[7];
    if (fread(head, sizeof head, 1, f) != 1) break;
    const int B = head[0], nd = head[1], flags = head[5], n_disp = head[6];
    const int shape[3] = {head[2], head[3], head[4]};
    size_t npix = 1;
    for (int d = 0; d < nd; ++d) npix *= (size_t)shape[d];
    const size_t n = (size_t)B * npix;
    // exact-size heap blocks: a read or write one element outside them is an error to the sanitizer
    std::vector<Sample> tab((size_t)B);
    std::vector<float> x(n), disp(n * (size_t)n_disp), want_x(n), got_x(n, -7.0f);
    std::vector<int32_t> y(n), want_y(n), got_y(n, -7);
    if (fread(tab.data(), sizeof(Sample), (size_t)B, f) != (size_t)B || fread(x.data(), 4, n, f) != n || fread(y.data(), 4, n, f) != n ||
        fread(disp.data(), 4, disp.size(), f) != disp.size() || fread(want_x.data(), 4, n, f) != n || fread(want_y.data(), 4, n, f) != n) {
      ++bad;
      break;
    }
    const int rc = aug_batch(x.data(), y.data(), B, nd, shape, flags, tab.data(), n_disp ? disp.data() : nullptr, n_disp, got_x.data(), got_y.data());
    size_t differ = 0;
    for (size_t k = 0; k < n; ++k) {
      const bool nan_w = want_x[k] != want_x[k], nan_g = got_x[k] != got_x[k];
      if (nan_w != nan_g || (!nan_w && memcmp(&want_x[k], &got_x[k], 4) != 0) || want_y[k] != got_y[k]) ++differ;
    }
    if (rc != 0 || differ) {
      printf("record %d (%d x %d x %d x %d, flags %d): rc %d, %zu pixels differ\n", records, B, shape[0], shape[1], nd == 3 ? shape[2] : 1, flags, rc,
             differ);
      ++bad;
    }
    ++records;
  }
  fclose(f);
  printf("%d records, %d bad\n", records, bad);
  return bad || !records ? 1 : 0;
}
#endif
