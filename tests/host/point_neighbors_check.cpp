// point_neighbors_check.cpp -- the per-query rules of csrc/point_neighbors.h on the host: the grid, the ring walk, the bound that ends it,
// the list of the k best and the rows of the radius lists, with a plain loop over the queries where the device pass has one lane per
// query.  Reads records written by tests/test_cpu_point_neighbors.py and compares with the host route's results, bit for bit.
//
// A record: int32 nd, mode (0 nearest, 1 counts, 2 lists), k, use_radius, own (the points are their own queries); int64 n, m, total;
// float64 r2, cell_size (0: automatic); then the points (n x nd float64, scaled), the queries (m x nd, absent with own) and the
// expected result: mode 0 indices (m x k int64) and d2 (m x k float64); mode 1 counts (m int64); mode 2 offsets (m + 1 int64), indices
// and d2 (total each).
//
// Prints "<records> records, <bad> bad, <rings> rings" and exits 1 if a record differs.  Build: g++ -O2 -std=c++17 -ffp-contract=off.
#include "../../stardist_amd/csrc/point_neighbors.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

using namespace point_neighbors;

namespace {

struct PlainStore {
  double* dd;
  int* ii;
  double d(int j) const { return dd[j]; }
  int i(int j) const { return ii[j]; }
  void set(int j, double d_, int i_) { dd[j] = d_; ii[j] = i_; }
};

template <typename T>
bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

long long rings_walked = 0;

// the rings a query walks before its search ends: a Nearest list that counts what search() asks of it
template <typename A>
struct Counting {
  A& acc;
  void add(double d, int i) { acc.add(d, i); }
  bool settled(double lb) const { ++rings_walked; return acc.settled(lb); }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s records.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  long long records = 0, bad = 0;
  for (;;) {
    int32_t head[5];
    int64_t sizes[3];
    double reals[2];
    if (fread(head, sizeof(head), 1, f) != 1) break;
    if (fread(sizes, sizeof(sizes), 1, f) != 1 || fread(reals, sizeof(reals), 1, f) != 1) { fprintf(stderr, "truncated record\n"); return 2; }
    const int nd = head[0], mode = head[1], k = head[2], own = head[4];
    const bool use_radius = head[3] != 0;
    const long long n = sizes[0], m = sizes[1], total = sizes[2];
    const double r2 = reals[0], cell_size = reals[1];
    std::vector<double> points, queries, want_d2;
    std::vector<int64_t> want_idx, want_counts;
    bool ok = read_n(f, points, (size_t)n * nd) && (own || read_n(f, queries, (size_t)m * nd));
    if (mode == 0) ok = ok && read_n(f, want_idx, (size_t)m * k) && read_n(f, want_d2, (size_t)m * k);
    if (mode == 1) ok = ok && read_n(f, want_counts, (size_t)m);
    if (mode == 2) ok = ok && read_n(f, want_counts, (size_t)m + 1) && read_n(f, want_idx, (size_t)total) && read_n(f, want_d2, (size_t)total);
    if (!ok) { fprintf(stderr, "truncated record\n"); return 2; }
    ++records;

    std::vector<int64_t> got_idx, got_counts;
    std::vector<double> got_d2;
    if (mode == 0) { got_idx.assign((size_t)m * k, -1); got_d2.assign((size_t)m * k, std::numeric_limits<double>::infinity()); }
    if (mode == 1) got_counts.assign((size_t)m, 0);
    if (mode == 2) { got_counts.assign((size_t)m + 1, 0); got_idx.assign((size_t)total, -7); got_d2.assign((size_t)total, -7.0); }
    if (n > 0 && m > 0) {
      // the grid, as the driver of the device pass builds it
      Grid g;
      g.nd = nd;
      const int shift = 3 - nd;
      double extent[3] = {0, 0, 0};
      g.lo[0] = 0;
      for (int a = 0; a < nd; ++a) {
        double lo = points[a], hi = points[a];
        for (long long i = 1; i < n; ++i) { lo = std::min(lo, points[i * nd + a]); hi = std::max(hi, points[i * nd + a]); }
        g.lo[a + shift] = lo;
        extent[a + shift] = hi - lo;
      }
      g.h = cell_size > 0 ? cell_size : automatic_cell(extent, n);
      g.inv_h = 1.0 / g.h;
      bool fits = g.h >= PN_MIN_CELL && g.h <= PN_MAX_CELL;
      for (int a = 0; a < 3; ++a) { g.dim[a] = cells_along(extent[a], g.h); fits = fits && g.dim[a] <= PN_MAX_DIM; }
      if (!fits || cell_count(g) > (1ll << 27)) { printf("record %lld: the grid does not fit (cell %g)\n", records, g.h); ++bad; continue; }
      if (cell_size == 0 && cell_count(g) > 2 * n + 16) { printf("record %lld: %lld cells for %lld points\n", records, cell_count(g), n); ++bad; continue; }
      std::vector<long long> cell(n);
      for (long long i = 0; i < n; ++i) { int c[3]; cell_of(g, &points[i * nd], c); cell[i] = linear_cell(g, c); }
      std::vector<int> order(n);
      std::iota(order.begin(), order.end(), 0);
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cell[a] < cell[b]; });
      std::vector<double> sorted((size_t)n * nd);
      std::vector<int> starts(cell_count(g) + 1, 0);
      for (long long s = 0; s < n; ++s) {
        for (int a = 0; a < nd; ++a) sorted[s * nd + a] = points[(long long)order[s] * nd + a];
        ++starts[cell[order[s]] + 1];
      }
      for (size_t c = 1; c < starts.size(); ++c) starts[c] += starts[c - 1];

      double best_d[PN_MAX_K];
      int best_i[PN_MAX_K];
      long long at = 0;
      for (long long qi = 0; qi < m; ++qi) {
        const double* q = own ? &points[qi * nd] : &queries[qi * nd];
        const int self = own ? (int)qi : -1;
        if (mode == 0) {
          Nearest<PlainStore> acc(PlainStore{best_d, best_i}, k);
          Counting<Nearest<PlainStore>> counting{acc};
          search(g, starts.data(), sorted.data(), order.data(), q, self, use_radius, r2, counting);
          for (int j = 0; j < acc.count; ++j) { got_idx[qi * k + j] = best_i[j]; got_d2[qi * k + j] = best_d[j]; }
        } else if (mode == 1) {
          Counter acc;
          search(g, starts.data(), sorted.data(), order.data(), q, self, true, r2, acc);
          got_counts[qi] = acc.count;
        } else {
          Counter counter;
          search(g, starts.data(), sorted.data(), order.data(), q, self, true, r2, counter);
          got_counts[qi] = at;
          const long long room = std::max(0ll, std::min(counter.count, total - at));
          Appender acc(got_idx.data() + at, room);
          search(g, starts.data(), sorted.data(), order.data(), q, self, true, r2, acc);
          sort_ascending(got_idx.data() + at, room);
          for (long long j = 0; j < room; ++j) got_d2[at + j] = squared_distance(q, &points[got_idx[at + j] * nd], nd);
          at += counter.count;
        }
      }
      if (mode == 2) got_counts[m] = at;
    }
    const bool equal = got_idx == want_idx && same_bits(got_d2, want_d2) && got_counts == want_counts;
    if (!equal) {
      ++bad;
      printf("record %lld differs: nd %d mode %d k %d radius %d own %d n %lld m %lld cell %g\n", records, nd, mode, k, (int)use_radius, own, n, m,
             cell_size);
    }
  }
  fclose(f);
  printf("%lld records, %lld bad, %lld rings\n", records, bad, rings_walked);
  return bad ? 1 : 0;
}
