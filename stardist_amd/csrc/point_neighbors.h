// point_neighbors.h -- the per-query rules of the nearest-point / points-within-a-radius search (stardist_amd.utils.point_neighbors,
// measure_labels(nearest=, within=)): the cell of a coordinate, the squared distance, the order of candidates, the
// walk over the rings of cells around a query and the bound that ends it.
//
// Everything here is __host__ __device__ and free of HIP headers when compiled by a host compiler: csrc/point_neighbors.hip runs it with
// one lane per query, tests/host/point_neighbors_check.cpp with a plain loop over the queries.  Built with -ffp-contract=off: every
// floating-point operation is rounded on its own, in float64.
//
// The definition.  Points and queries arrive scaled (coordinate * spacing, rounded once).  With 2 or 3 coordinates per point,
//     d2(q, p) = ((q0 - p0)^2 + (q1 - p1)^2) + (q2 - p2)^2          left to right, the last term only with 3 coordinates
// candidates are ordered by (d2, index), "within the radius" is d2 <= r2 with r2 = fl(radius * radius) formed by the caller, and a
// query that is point `self` of the set skips that one index (other points at the same place count, at distance 0).
//
// The grid.  Axis a of the points' box [lo, hi] is cut into dim[a] cells of one edge h for all axes; a coordinate x has the cell
//     cell(x) = clamp(floor(fl(fl(x - lo) * inv_h)), 0, dim - 1),   inv_h = fl(1 / h)
// which is monotone in x (both roundings are), so that points whose cells differ by more than R along an axis are more than
// (R - 2^-20) h apart along it: ring_bound().  Points are stored with 3 axes; a 2D point has axis 0 fixed (dim 1, coordinate 0).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PN_HD __host__ __device__ __forceinline__
#else
#define PN_HD inline
#endif

namespace point_neighbors {

enum {
  PN_MAX_K = 64,              // the longest list of nearest points a query keeps
  PN_MAX_DIM = 1 << 21,       // cells along one axis: ring_bound()'s margin of 2^-20 cells holds up to here
  PN_LANES = 64               // queries of one workgroup of the device pass: 64 lanes x 64 entries x 12 bytes of local memory
};

constexpr double PN_MIN_CELL = 0x1p-500, PN_MAX_CELL = 0x1p+500;     // the cell edge: its square neither underflows nor overflows
constexpr double PN_MAX_COORD = 0x1p+500;                            // |coordinate| stays below: d2 does not overflow

struct Grid {
  int nd;                     // coordinates per point as the caller has them, 2 or 3
  int dim[3];                 // cells per axis; dim[0] = 1 for nd = 2
  double lo[3];               // the box's lower corner
  double h, inv_h;            // the cell edge and fl(1 / h)
};

PN_HD int cell_coord(double x, double lo, double inv_h, int dim) {
  const double d = x - lo;
  const double t = d * inv_h;
  if (!(t >= 0.0)) return 0;
  if (t >= (double)dim) return dim - 1;
  return (int)t;                                                       // t >= 0: the truncation is the floor
}

// the cell of the point / query with the nd coordinates x[]: c[0 .. 2], and its linear index
PN_HD void cell_of(const Grid& g, const double* x, int* c) {
  const int shift = 3 - g.nd;
  c[0] = 0;
  for (int a = 0; a < g.nd; ++a) c[a + shift] = cell_coord(x[a], g.lo[a + shift], g.inv_h, g.dim[a + shift]);
}

PN_HD long long linear_cell(const Grid& g, const int* c) { return ((long long)c[0] * g.dim[1] + c[1]) * g.dim[2] + c[2]; }

PN_HD long long cell_count(const Grid& g) { return (long long)g.dim[0] * g.dim[1] * g.dim[2]; }

PN_HD double squared_distance(const double* q, const double* p, int nd) {
  const double a = q[0] - p[0], b = q[1] - p[1];
  double s = a * a + b * b;
  if (nd == 3) {
    const double c = q[2] - p[2];
    s = s + c * c;
  }
  return s;
}

// (d, i) comes before (e, j) in the order of candidates
PN_HD bool before(double d, long long i, double e, long long j) { return d < e || (d == e && i < j); }

// A lower bound of the COMPUTED d2 between a query and any point whose cell differs from the query's by more than R along some axis:
// 0 for R = 0.  DESIGN.md section 3v has the proof; in short, with t(x) = fl(fl(x - lo) * inv_h) <= 2^21 and three roundings of 2^-53
// each, such a pair is at least (R - 2^-29) h apart along that axis, and (R - 2^-20)^2 (1 - 2^-50) with its own three roundings stays
// below (R - 2^-29)^2 (1 - 2^-52)^2, which bounds the computed d2 from below, for every R up to 2^21.
PN_HD double ring_bound(int R, double h) {
  if (R <= 0) return 0.0;
  const double e = ((double)R - 0x1p-20) * h;
  return (e * e) * (1.0 - 0x1p-50);
}

// the number of rings that cover the grid from cell c: every cell differs from c by at most this along every axis
PN_HD int last_ring(const Grid& g, const int* c) {
  int r = 0;
  for (int a = 0; a < 3; ++a) {
    const int m = c[a] > g.dim[a] - 1 - c[a] ? c[a] : g.dim[a] - 1 - c[a];
    r = m > r ? m : r;
  }
  return r;
}

// f(linear cell) for every cell of the grid at Chebyshev distance exactly R from c.  The loops run over the clipped square of (axis 0,
// axis 1) offsets, at most (2 R + 1)^2 of them (2 R + 1 for a 2D grid), with a full row of axis 2 where one of the two is at distance R
// and the row's two ends elsewhere.
template <typename F>
PN_HD void each_ring_cell(const Grid& g, const int* c, int R, F f) {
  const int z0 = c[0] - R < 0 ? 0 : c[0] - R, z1 = c[0] + R > g.dim[0] - 1 ? g.dim[0] - 1 : c[0] + R;
  const int y0 = c[1] - R < 0 ? 0 : c[1] - R, y1 = c[1] + R > g.dim[1] - 1 ? g.dim[1] - 1 : c[1] + R;
  const int x0 = c[2] - R < 0 ? 0 : c[2] - R, x1 = c[2] + R > g.dim[2] - 1 ? g.dim[2] - 1 : c[2] + R;
  for (int z = z0; z <= z1; ++z) {
    const bool z_far = z - c[0] == R || c[0] - z == R;
    for (int y = y0; y <= y1; ++y) {
      const long long row = ((long long)z * g.dim[1] + y) * g.dim[2];
      if (z_far || y - c[1] == R || c[1] - y == R) {
        for (int x = x0; x <= x1; ++x) f(row + x);
      } else {                                                         // R > 0 here: the two ends are different cells
        if (c[2] - R >= 0) f(row + (c[2] - R));
        if (c[2] + R <= g.dim[2] - 1) f(row + (c[2] + R));
      }
    }
  }
}

// The k best candidates of one query, ascending by (d2, index), in storage S: S.d(j), S.i(j) read entry j, S.set(j, d, i) writes it.
template <typename S>
struct Nearest {
  S store;
  int k, count;
  PN_HD Nearest(S s, int k_) : store(s), k(k_), count(0) {}
  PN_HD void add(double d, int i) {
    if (count == k && !before(d, i, store.d(k - 1), store.i(k - 1))) return;
    int j = count < k ? count++ : k - 1;
    for (; j > 0 && before(d, i, store.d(j - 1), store.i(j - 1)); --j) store.set(j, store.d(j - 1), store.i(j - 1));
    store.set(j, d, i);
  }
  // nothing at lb or beyond can enter the list any more: it is full and its last entry is strictly below lb
  PN_HD bool settled(double lb) const { return count == k && store.d(k - 1) < lb; }
};

// counts the candidates; never settled
struct Counter {
  long long count = 0;
  PN_HD void add(double, int) { ++count; }
  PN_HD bool settled(double) const { return false; }
};

// appends the candidates' indices at out[0 .. cap) and counts all of them; never settled
struct Appender {
  int64_t* out;
  long long cap, count = 0;
  PN_HD Appender(int64_t* o, long long c) : out(o), cap(c) {}
  PN_HD void add(double, int i) {
    if (count < cap) out[count] = i;
    ++count;
  }
  PN_HD bool settled(double) const { return false; }
};

// The search of one query q: the rings R = 0, 1, ... of cells around q's cell, every point of a ring's cells offered to `acc` unless
// it is point `self` or, with use_radius, beyond r2.  After ring R everything not yet seen has a computed d2 >= ring_bound(R): the walk
// ends when that exceeds r2, when acc is settled below it, or when the rings cover the grid -- at most max(dim) trips, whatever the
// data.  starts: the cells' first slots (cell_count + 1 entries); slot s holds the point sorted[s * nd ..] with the index order[s].
template <typename A>
PN_HD void search(const Grid& g, const int* starts, const double* sorted, const int* order, const double* q, int self, bool use_radius,
                  double r2, A& acc) {
  int c[3];
  cell_of(g, q, c);
  const int last = last_ring(g, c);
  for (int R = 0; R <= last; ++R) {
    each_ring_cell(g, c, R, [&](long long cell) {
      const int stop = starts[cell + 1];
      for (int s = starts[cell]; s < stop; ++s) {
        const int i = order[s];
        if (i == self) continue;
        const double d = squared_distance(q, sorted + (long long)s * g.nd, g.nd);
        if (use_radius && !(d <= r2)) continue;
        acc.add(d, i);
      }
    });
    const double lb = ring_bound(R, g.h);
    if ((use_radius && lb > r2) || acc.settled(lb)) break;
  }
}

// heap sort of a[0 .. n), ascending, in place: the indices of one row of the radius lists
PN_HD void sort_ascending(int64_t* a, long long n) {
  auto sift = [&](long long root, long long end) {
    for (long long child = 2 * root + 1; child < end; child = 2 * root + 1) {
      if (child + 1 < end && a[child] < a[child + 1]) ++child;
      if (!(a[root] < a[child])) return;
      const int64_t t = a[root]; a[root] = a[child]; a[child] = t;
      root = child;
    }
  };
  for (long long s = n / 2 - 1; s >= 0; --s) sift(s, n);
  for (long long end = n - 1; end > 0; --end) {
    const int64_t t = a[0]; a[0] = a[end]; a[end] = t;
    sift(0, end);
  }
}

// the cells an axis of extent fl(hi - lo) gets with the edge h: cell(hi) + 1 before any clamp, so every point's cell is below it;
// capped at 4 PN_MAX_DIM, which is refused anyway
inline int cells_along(double extent, double h) {
  const double t = extent * (1.0 / h);
  return t >= (double)PN_MAX_DIM * 4 ? PN_MAX_DIM * 4 : (int)t + 1;
}

// The cell edge for n points in the box of extents e[0 .. 2] (0 for an axis without extent): about two points per cell over the axes
// that have an extent, doubled until no axis has more than PN_MAX_DIM cells and there are at most 2 n + 16 cells; 1 for a box that
// is a single place.  Host code: the box comes to the host once per call.
inline double automatic_cell(const double* e, long long n) {
  int axes = 0;
  double log_volume = 0;
  for (int a = 0; a < 3; ++a)
    if (e[a] > 0) { ++axes; log_volume += log2(e[a]); }
  if (!axes) return 1.0;
  const double target = n > 2 ? (double)n / 2 : 1.0;
  double h = exp2((log_volume - log2(target)) / axes);
  if (!(h >= PN_MIN_CELL)) h = PN_MIN_CELL;
  if (!(h <= PN_MAX_CELL)) h = PN_MAX_CELL;
  for (int it = 0; it < 1100 && h < PN_MAX_CELL; ++it) {
    long long cells = 1;
    bool wide = false;
    for (int a = 0; a < 3; ++a) {
      const int d = cells_along(e[a], h);
      wide = wide || d > PN_MAX_DIM;
      cells = cells > (1ll << 40) ? cells : cells * d;
    }
    if (!wide && cells <= 2 * n + 16) break;
    h *= 2;
  }
  return h;
}

}  // namespace point_neighbors
