// rank_filter_check.cpp -- the per-element rules of csrc/rank_filter.h on the host: scipy's index maps, the keys, the minimum / maximum
// of a line, the selection by bisection, the top-hat's last operation and the tier predicates, with plain loops over the pixels where
// the device passes have one lane per pixel.  Reads records written by tests/test_cpu_rank_filters.py and compares with the host
// route's results (== on numbers, a NaN against any NaN).
//
// A record starts with int32 kind.
//   kind 0, a call: int32 dtype (0 uint8, 1 uint16, 2 float32), mode, fuse, stages; int64 n[3] (z y x; a 2D image has n[0] = 1);
//           float64 cval; per stage int32 op (0 minimum, 1 maximum, 2 rank), rank, count, is_box, extent[3], origin[3] and count x 3
//           int32 offsets (dz, dy, dx); the image; the expected result (the image's dtype).  A box minimum / maximum runs as separable
//           passes in the order 0, 1, 2 as the device's does, any other stage as one walk per pixel.
//   kind 1, a predicate: int32 which, bytes, p[4], expected.  which 0: box_tile_fits for a pass of size p[0] (p[1]: along the last
//           axis); which 1: footprint_tile_fits for extents p[1 .. 3] (p[0]: 3D); which 2: p[0] == MAX_WINDOW and p[1] == MAX_FOOTPRINT.
//
// Prints "<records> records, <bad> bad, <elements> elements" and exits 1 if a record differs.  Build: g++ -O2 -std=c++17.
#include "../../stardist_amd/csrc/rank_filter.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace rankf;

namespace {

template <typename T>
bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

long long elements = 0;

struct Stage {
  int32_t op, rank, count, is_box, extent[3], origin[3];
  std::vector<int32_t> offsets;
};

template <typename K>
struct Line {
  const K* keys;            // the line's element 0
  long long first, n, inner;
  int mode;
  K cval;
  K operator()(int j) const {
    const long long m = map_index(first + j, n, mode);
    return m < 0 ? cval : keys[m * inner];
  }
};

template <typename K>
struct Window {
  const K* keys;
  const int32_t* tab;
  long long z, y, x, n0, n1, n2;
  int mode;
  K cval;
  K operator()(int k) const {
    const long long mz = map_index(z + tab[3 * k], n0, mode), my = map_index(y + tab[3 * k + 1], n1, mode), mx = map_index(x + tab[3 * k + 2], n2, mode);
    return (mz | my | mx) < 0 ? cval : keys[(mz * n1 + my) * n2 + mx];
  }
};

template <typename K>
void box_stage(std::vector<K>& cur, const long long n[3], const Stage& S, int mode, K cval) {
  std::vector<K> next(cur.size());
  for (int a = 0; a < 3; ++a) {
    if (S.extent[a] <= 1) continue;
    const long long inner = a == 0 ? n[1] * n[2] : a == 1 ? n[2] : 1, outer = a == 0 ? 1 : a == 1 ? n[0] : n[0] * n[1];
    const int left = window_left(S.extent[a], S.origin[a]);
    for (long long o = 0; o < outer; ++o)
      for (long long p = 0; p < n[a]; ++p)
        for (long long i = 0; i < inner; ++i) {
          const Line<K> at = {cur.data() + o * n[a] * inner + i, p - left, n[a], inner, mode, cval};
          next[(o * n[a] + p) * inner + i] = minmax_line<K>(at, S.extent[a], S.op == 1);
          ++elements;
        }
    cur.swap(next);
  }
}

template <typename K>
void window_stage(std::vector<K>& cur, const long long n[3], const Stage& S, int mode, K cval, int bits) {
  std::vector<K> next(cur.size());
  const int rank = S.op == 0 ? 0 : S.op == 1 ? S.count - 1 : S.rank;
  for (long long z = 0; z < n[0]; ++z)
    for (long long y = 0; y < n[1]; ++y)
      for (long long x = 0; x < n[2]; ++x) {
        const Window<K> at = {cur.data(), S.offsets.data(), z - window_left(S.extent[0], S.origin[0]), y - window_left(S.extent[1], S.origin[1]),
                              x - window_left(S.extent[2], S.origin[2]), n[0], n[1], n[2], mode, cval};
        next[(z * n[1] + y) * n[2] + x] = select_rank<K>(at, S.count, rank, bits);
        ++elements;
      }
  cur.swap(next);
}

bool same_value(float a, float b) { return a == b || (a != a && b != b); }
bool same_value(uint8_t a, uint8_t b) { return a == b; }
bool same_value(uint16_t a, uint16_t b) { return a == b; }

uint8_t fuse_value(uint8_t x, uint8_t r, int op) { return fuse_u8(x, r, op); }
uint16_t fuse_value(uint16_t x, uint16_t r, int op) { return fuse<uint16_t>(x, r, op); }
float fuse_value(float x, float r, int op) { return fuse<float>(x, r, op); }

template <typename T>
bool call_record(FILE* f, int mode, int fuse_op, int stages, const long long n[3], double cval_in, bool* ok) {
  typedef typename KeyOf<T>::type K;
  std::vector<Stage> plan((size_t)stages);
  for (Stage& S : plan) {
    int32_t head[10];
    if (fread(head, sizeof(head), 1, f) != 1) return false;
    S.op = head[0]; S.rank = head[1]; S.count = head[2]; S.is_box = head[3];
    for (int a = 0; a < 3; ++a) { S.extent[a] = head[4 + a]; S.origin[a] = head[7 + a]; }
    if (S.count < 1 || S.count > (1 << 24) || !read_n(f, S.offsets, (size_t)S.count * 3)) return false;
  }
  const size_t count = (size_t)(n[0] * n[1] * n[2]);
  std::vector<T> img, want;
  if (!read_n(f, img, count) || !read_n(f, want, count)) return false;
  const K cval = to_key((T)cval_in);
  std::vector<K> cur(count);
  for (size_t i = 0; i < count; ++i) cur[i] = to_key(img[i]);
  for (const Stage& S : plan) {
    if (S.is_box && S.op != 2) box_stage<K>(cur, n, S, mode, cval);
    else window_stage<K>(cur, n, S, mode, cval, (int)KeyOf<T>::BITS);
  }
  *ok = true;
  for (size_t i = 0; i < count && *ok; ++i) {
    T v = from_key(cur[i], T());
    if (fuse_op != FUSE_NONE) v = fuse_value(v, img[i], fuse_op);
    *ok = same_value(v, want[i]);
  }
  return true;
}

bool predicate_record(FILE* f, bool* ok) {
  int32_t v[7];
  if (fread(v, sizeof(v), 1, f) != 1) return false;
  const int which = v[0], bytes = v[1];
  bool got;
  if (which == 0) got = box_tile_fits(v[3] ? B_LAST_A : B_INNER_A, v[3] ? 1 : B_INNER_I, v[2], bytes);
  else if (which == 1) { const int fs[3] = {v[3], v[4], v[5]}; got = footprint_tile_fits(v[2] != 0, fs, bytes); }
  else got = v[2] == MAX_WINDOW && v[3] == MAX_FOOTPRINT && bytes == LDS_BYTES;
  *ok = got == (v[6] != 0);
  ++elements;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s records.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  long long records = 0, bad = 0;
  for (;;) {
    int32_t kind;
    if (fread(&kind, sizeof(kind), 1, f) != 1) break;
    bool ok = false, read = false;
    if (kind == 0) {
      int32_t head[4];
      int64_t ext[3];
      double cval;
      if (fread(head, sizeof(head), 1, f) != 1 || fread(ext, sizeof(ext), 1, f) != 1 || fread(&cval, sizeof(cval), 1, f) != 1) { fprintf(stderr, "truncated record\n"); return 2; }
      const long long n[3] = {ext[0], ext[1], ext[2]};
      const int dtype = head[0];
      if (head[3] < 1 || head[3] > 8 || n[0] < 1 || n[1] < 1 || n[2] < 1 || n[0] * n[1] * n[2] > (1ll << 28)) { fprintf(stderr, "bad record\n"); return 2; }
      read = dtype == DT_U8 ? call_record<uint8_t>(f, head[1], head[2], head[3], n, cval, &ok)
           : dtype == DT_U16 ? call_record<uint16_t>(f, head[1], head[2], head[3], n, cval, &ok)
                             : call_record<float>(f, head[1], head[2], head[3], n, cval, &ok);
    } else {
      read = predicate_record(f, &ok);
    }
    if (!read) { fprintf(stderr, "truncated record\n"); return 2; }
    ++records;
    if (!ok) { ++bad; printf("record %lld (kind %d) differs\n", records - 1, kind); }
  }
  fclose(f);
  printf("%lld records, %lld bad, %lld elements\n", records, bad, elements);
  return bad ? 1 : 0;
}
