// Host harness of stardist_amd/csrc/fill_holes.h: what csrc/fill_holes.hip does -- boxes, planes, the passes to the fixpoint, the max
// rule -- with plain loops in place of threads.  Built by tests/test_cpu_fill_holes.py (g++).
#include <limits.h>
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../stardist_amd/csrc/fill_holes.h"

using namespace fillholes;

extern "C" {

int fh_lds_words() { return FH_LDS_WORDS; }

// boxes[max_label + 1][6] with the sentinel of sd_label_boxes_device
int fh_boxes(const int32_t* lbl, int Z, int Y, int X, int max_label, int32_t* boxes) {
  if (!lbl || !boxes || Z <= 0 || Y <= 0 || X <= 0 || max_label < 0) return -1;
  for (long long i = 0; i < 6ll * (max_label + 1ll); ++i) boxes[i] = (i % 6) < 3 ? INT_MAX : 0;
  for (int z = 0; z < Z; ++z)
    for (int y = 0; y < Y; ++y)
      for (int x = 0; x < X; ++x) {
        const int l = lbl[((long long)z * Y + y) * X + x];
        if (l <= 0 || l > max_label) continue;
        int32_t* t = boxes + 6ll * l;
        if (z < t[0]) t[0] = z;
        if (y < t[1]) t[1] = y;
        if (x < t[2]) t[2] = x;
        if (z + 1 > t[3]) t[3] = z + 1;
        if (y + 1 > t[4]) t[4] = y + 1;
        if (x + 1 > t[5]) t[5] = x + 1;
      }
  return 0;
}

// out = the filled image; rounds_max (optional) = the largest number of rounds an object took, lds_objects / big_objects (optional)
// = how many objects fit the LDS budget and how many do not
int fh_fill(const int32_t* lbl, int Z, int Y, int X, int max_label, int32_t* out, int* rounds_max, int* lds_objects, int* big_objects) {
  if (!lbl || !out || Z <= 0 || Y <= 0 || X <= 0 || max_label < 0) return -1;
  std::vector<int32_t> boxes(6 * ((size_t)max_label + 1));
  fh_boxes(lbl, Z, Y, X, max_label, boxes.data());
  const long long n = (long long)Z * Y * X;
  for (long long p = 0; p < n; ++p) out[p] = (lbl[p] > 0 && lbl[p] <= max_label) ? lbl[p] : 0;
  const int volume = Z > 1 ? 1 : 0;
  int most = 0, n_lds = 0, n_big = 0;
  std::vector<uint32_t> fr, rc;
  for (int L = 1; L <= max_label; ++L) {
    const int32_t* t = boxes.data() + 6ll * L;
    if (t[2] >= t[5]) continue;
    const Geo g = geo_of(t);
    if (fits_lds(g)) ++n_lds; else ++n_big;
    fr.assign((size_t)g.words, 0);
    rc.assign((size_t)g.words, 0);
    for (long long i = 0; i < g.words; ++i) {
      const int w = (int)(i % g.wx), row = (int)(i / g.wx);
      const int y = row % g.by, z = row / g.by;
      fr[i] = free_word(lbl, Y, X, g, z, y, w, L);
      rc[i] = fr[i] & outer_word(g, volume, z, y, w);
    }
    int rounds = 0;
    for (;;) {
      bool ch = false;
      for (int r = 0; r < g.rows; ++r) ch |= pass_rows(rc.data(), fr.data(), g, r);
      for (int c = 0; c < g.bz * g.wx; ++c) ch |= pass_y(rc.data(), fr.data(), g, c);
      if (g.bz > 1)
        for (int c = 0; c < g.by * g.wx; ++c) ch |= pass_z(rc.data(), fr.data(), g, c);
      ++rounds;
      if (!ch) break;
    }
    if (rounds > most) most = rounds;
    for (long long i = 0; i < g.words; ++i) {
      const uint32_t h = fr[i] & ~rc[i];
      if (!h) continue;
      const int w = (int)(i % g.wx), row = (int)(i / g.wx);
      const int y = row % g.by, z = row / g.by;
      int32_t* o = out + ((long long)(g.z0 + z) * Y + (g.y0 + y)) * X + g.x0 + 32 * w;
      for (int k = 0; k < 32; ++k)
        if ((h >> k) & 1u) { if (o[k] < L) o[k] = L; }
    }
  }
  if (rounds_max) *rounds_max = most;
  if (lds_objects) *lds_objects = n_lds;
  if (big_objects) *big_objects = n_big;
  return 0;
}

// one row pass on caller-supplied words (the word-boundary and carry logic on its own)
int fh_fill_row(uint32_t* reach, const uint32_t* free_, int wx) { return fill_row(reach, free_, wx) ? 1 : 0; }

}  // extern "C"
