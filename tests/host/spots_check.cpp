// spots_check.cpp -- the per-element rules of csrc/spots.h on the host: the reflected index and the line rule of the Gaussian, the
// window test, the threshold and the sort key of peak_local_max, with plain loops over the pixels where the device pass has one lane
// per pixel.  Reads records written by tests/test_cpu_spots.py and compares with the host route's results.
//
// A record starts with int32 kind, dtype (0 uint8, 1 uint16, 2 float32) and int64 n[3] (z y x; a 2D image has n[0] = 1).
//   kind 0, Gaussian: int32 r[3] (< 0: the axis is skipped); the float64 weight tables of the axes that are not skipped, 2 r + 1 each;
//           the image; the expected float32 result (compared bit for bit, a NaN against any NaN).
//   kind 1, peaks: int32 d[3], has_labels, has_abs, has_rel; int64 b[3], per_label (< 0: none), num_peaks (< 0: none), count;
//           float64 threshold_abs, threshold_rel; the image; the labels (int32, if any); the expected raster indices (count int64).
//
// Prints "<records> records, <bad> bad, <elements> elements" and exits 1 if a record differs.  Build: g++ -O2 -std=c++17 -ffp-contract=off.
#include "../../stardist_amd/csrc/spots.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace spots;

namespace {

template <typename T>
bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

long long elements = 0;

struct Line {
  const float* base;
  long long a, n, inner;
  double operator()(int j) const { return (double)base[reflect_index(a + j, n) * inner]; }
};

// one pass along `axis` of a float image of extents n
void gauss_pass(const std::vector<float>& in, std::vector<float>& out, const long long n[3], int axis, int r, const double* w) {
  const long long inner = axis == 0 ? n[1] * n[2] : axis == 1 ? n[2] : 1;
  const long long outer = axis == 0 ? 1 : axis == 1 ? n[0] : n[0] * n[1];
  out.resize(in.size());
  for (long long o = 0; o < outer; ++o)
    for (long long a = 0; a < n[axis]; ++a)
      for (long long i = 0; i < inner; ++i) {
        const Line at = {in.data() + o * n[axis] * inner + i, a, n[axis], inner};
        out[(o * n[axis] + a) * inner + i] = gauss_point(at, r, w);
        ++elements;
      }
}

bool same_floats(const std::vector<float>& a, const std::vector<float>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i) {
    if (a[i] != a[i] && b[i] != b[i]) continue;
    if (memcmp(&a[i], &b[i], 4) != 0) return false;
  }
  return true;
}

template <typename T>
bool gauss_record(FILE* f, const long long n[3], bool* ok) {
  int32_t r[3];
  if (fread(r, sizeof(r), 1, f) != 1) return false;
  size_t taps = 0;
  for (int a = 0; a < 3; ++a) taps += r[a] >= 0 ? 2 * r[a] + 1 : 0;
  const size_t count = (size_t)(n[0] * n[1] * n[2]);
  std::vector<double> w;
  std::vector<T> img;
  std::vector<float> want;
  if (!read_n(f, w, taps) || !read_n(f, img, count) || !read_n(f, want, count)) return false;
  std::vector<float> cur(img.begin(), img.end()), next;                  // uint8 / uint16 -> float is exact
  const double* table = w.data();
  for (int a = 0; a < 3; ++a) {
    if (r[a] < 0) continue;
    gauss_pass(cur, next, n, a, r[a], table);
    cur.swap(next);
    table += 2 * r[a] + 1;
  }
  *ok = same_floats(cur, want);
  return true;
}

template <typename T>
struct PlainImg {
  const T* in;
  const int32_t* labels;
  long long n1, n2;
  float value(long long z, long long y, long long x) const { return (float)in[(z * n1 + y) * n2 + x]; }
  int label(long long z, long long y, long long x) const { return labels[(z * n1 + y) * n2 + x]; }
};

double value_of_key(uint32_t k, int dtype) {
  if (dtype != DT_F32) return (double)k;
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float v;
  memcpy(&v, &u, 4);
  return (double)v;
}

template <typename T>
bool peak_record(FILE* f, int dtype, const long long n[3], bool* ok) {
  int32_t head[6];
  int64_t tail[6];
  double thr_in[2];
  if (fread(head, sizeof(head), 1, f) != 1 || fread(tail, sizeof(tail), 1, f) != 1 || fread(thr_in, sizeof(thr_in), 1, f) != 1) return false;
  const int d[3] = {head[0], head[1], head[2]};
  const bool has_labels = head[3] != 0, has_abs = head[4] != 0, has_rel = head[5] != 0;
  const long long b[3] = {tail[0], tail[1], tail[2]}, per_label = tail[3], num_peaks = tail[4], expected = tail[5];
  const size_t count = (size_t)(n[0] * n[1] * n[2]);
  std::vector<T> img;
  std::vector<int32_t> labels;
  std::vector<int64_t> want;
  if (!read_n(f, img, count) || !read_n(f, labels, has_labels ? count : 0) || !read_n(f, want, (size_t)expected)) return false;
  // the threshold, from the least and greatest key as the device reduction finds them
  uint32_t lo = 0xffffffffu, hi = 0;
  for (size_t i = 0; i < count; ++i) {
    if (is_nan(img[i])) continue;
    const uint32_t k = value_key(img[i]);
    lo = std::min(lo, k);
    hi = std::max(hi, k);
  }
  double thr = std::numeric_limits<double>::infinity();
  if (lo <= hi) {
    thr = has_abs ? thr_in[0] : value_of_key(lo, dtype);
    if (has_rel) thr = std::max(thr, thr_in[1] * value_of_key(hi, dtype));
  }
  const PlainImg<T> view = {img.data(), labels.data(), n[1], n[2]};
  std::vector<uint64_t> keys;
  for (long long z = 0; z < n[0]; ++z)
    for (long long y = 0; y < n[1]; ++y)
      for (long long x = 0; x < n[2]; ++x) {
        const long long idx = (z * n[1] + y) * n[2] + x;
        const T v = img[idx];
        const int lab = has_labels ? labels[idx] : 1;
        ++elements;
        if (is_nan(v) || !((double)v > thr) || lab == 0) continue;
        if (z < b[0] || z >= n[0] - b[0] || y < b[1] || y >= n[1] - b[1] || x < b[2] || x >= n[2] - b[2]) continue;
        if (is_beaten(view, n, d, z, y, x, (float)v, has_labels, lab)) continue;
        keys.push_back(peak_key(v, (uint32_t)idx));
      }
  std::sort(keys.begin(), keys.end());
  if (per_label >= 0 && has_labels) {
    std::vector<size_t> order(keys.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    auto label_of = [&](size_t i) { return (uint32_t)labels[keys[i] & 0xffffffffull]; };
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t c) { return label_of(a) < label_of(c); });
    std::vector<char> keep(keys.size(), 0);
    for (size_t j = 0, start = 0; j < order.size(); ++j) {
      if (label_of(order[j]) != label_of(order[start])) start = j;
      keep[order[j]] = (long long)(j - start) < per_label;
    }
    std::vector<uint64_t> kept;
    for (size_t i = 0; i < keys.size(); ++i)
      if (keep[i]) kept.push_back(keys[i]);
    keys.swap(kept);
  }
  if (num_peaks >= 0 && (size_t)num_peaks < keys.size()) keys.resize((size_t)num_peaks);
  *ok = keys.size() == want.size();
  for (size_t i = 0; *ok && i < keys.size(); ++i) *ok = (int64_t)(keys[i] & 0xffffffffull) == want[i];
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s records.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  long long records = 0, bad = 0;
  for (;;) {
    int32_t head[2];
    int64_t ext[3];
    if (fread(head, sizeof(head), 1, f) != 1) break;
    if (fread(ext, sizeof(ext), 1, f) != 1) { fprintf(stderr, "truncated record\n"); return 2; }
    const long long n[3] = {ext[0], ext[1], ext[2]};
    bool ok = false, read = false;
    const int kind = head[0], dtype = head[1];
    if (kind == 0) read = dtype == DT_U8 ? gauss_record<uint8_t>(f, n, &ok) : dtype == DT_U16 ? gauss_record<uint16_t>(f, n, &ok) : gauss_record<float>(f, n, &ok);
    else read = dtype == DT_U8 ? peak_record<uint8_t>(f, dtype, n, &ok) : dtype == DT_U16 ? peak_record<uint16_t>(f, dtype, n, &ok) : peak_record<float>(f, dtype, n, &ok);
    if (!read) { fprintf(stderr, "truncated record\n"); return 2; }
    ++records;
    if (!ok) { ++bad; printf("record %lld (kind %d) differs\n", records - 1, kind); }
  }
  fclose(f);
  printf("%lld records, %lld bad, %lld elements\n", records, bad, elements);
  return bad ? 1 : 0;
}
