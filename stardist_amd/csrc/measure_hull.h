// measure_hull.h -- the per-object arithmetic behind the hull columns of stardist_amd.utils.measure_labels(hull=True): convex_area,
// solidity and feret_diameter_max of scikit-image 0.18's regionprops_table, stated in integers.
//
// Everything here is __host__ __device__ and free of HIP headers when compiled by a host compiler: csrc/measure_hull.hip runs it with
// one wave per object, tests/host/measure_hull_check.cpp with plain loops in place of the lanes, and tests/test_cpu_measure_hull.py
// compares the latter with the host function.  All of it is integer arithmetic: int32 coordinates, int64 products.
//
// Doubled coordinates: pixel (r, c) has its centre at (2 r, 2 c) and the four diamond points (2 r - 1, 2 c), (2 r + 1, 2 c),
// (2 r, 2 c - 1), (2 r, 2 c + 1).  Extents stay below 2^30 (MH_MAX_EXTENT), so a doubled coordinate fits int32, a difference of two
// stays below 2^31, a product of two differences below 2^62 and a cross product or a squared distance below 2^63.
//
// Row table.  An object of h rows starting at row y0 is given by (first, last) column of every row; a row without a pixel holds
// first > last.  Its diamond points lie on the 2 h + 1 levels y = 2 y0 - 1 + k, k = 0 .. 2 h: an odd level k = 2 j + 1 runs through
// the centres of row j and holds x = 2 first - 1 .. 2 last + 1, an even level k = 2 j lies between the rows j - 1 and j and holds the
// even x from 2 min(first) to 2 max(last) of those two rows.  Only the least and the largest x of a level can be hull vertices
// (level_point), and the levels come sorted by y, so a monotone chain needs no sort (build_chain: the left chain from the least x, the
// right chain from the largest).
//
// Convex image.  The hull is the region between the two chains; at the height y = 2 (y0 + j) of row j its x range is [xl, xr] with xl,
// xr rational (chain_at: numerator / denominator), and pixel c of the row belongs to the convex image iff xl <= 2 c <= xr, that is
// ceil(xl / 2) <= c <= floor(xr / 2) by exact integer division (row_interval).  The hull lies within the diamond points' extent, so
// the interval lies within the object's box.  convex_area is the sum of the intervals' lengths; a row's interval may be empty.
//
// Feret.  The intervals are a row table again; the largest squared distance between two diamond points of the convex image is taken
// between two vertices of THEIR hull (build_chain once more, then far_pairs over all pairs of chain vertices).
#pragma once
#include <limits.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MH_HD __host__ __device__ __forceinline__
#else
#define MH_HD inline
#endif

namespace measure_hull {

enum {
  MH_MAX_EXTENT = 1 << 30,                                             // image extents are below this
  MH_LDS_ROWS = 64,                                                    // objects of up to this many rows are worked on in LDS
  MH_LDS_CHAIN = 2 * MH_LDS_ROWS + 2                                   // a chain of such an object: at most one vertex per level
};

struct Pt { int y, x; };                                               // doubled coordinates

// a pixel with label v whose neighbour in the row (before: to the left, after: to the right) holds `other` starts / ends a run of v
MH_HD bool run_edge(int v, bool has_other, int other) { return !has_other || other != v; }

// (b - a) x (c - a) with y as the first axis: > 0 when c lies towards larger x of the line from a to b (for b.y > a.y)
MH_HD long long cross(Pt a, Pt b, Pt c) {
  return ((long long)b.y - a.y) * ((long long)c.x - a.x) - ((long long)b.x - a.x) * ((long long)c.y - a.y);
}

MH_HD long long floor_div(long long a, long long b) {                  // b > 0
  const long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

MH_HD long long ceil_div(long long a, long long b) {                   // b > 0
  const long long q = a / b;
  return (a % b != 0 && a > 0) ? q + 1 : q;
}

MH_HD bool row_has(const int* rows, int j) { return rows[2 * j] <= rows[2 * j + 1]; }

// the number of levels of an object of h rows
MH_HD int level_count(int h) { return 2 * h + 1; }

// the extreme diamond point of level k (side < 0: the least x, else the largest); false: the level holds no point
MH_HD bool level_point(const int* rows, int h, int y0, int k, int side, Pt* p) {
  const int j = k >> 1;
  p->y = 2 * y0 - 1 + k;
  p->x = 0;
  if (k & 1) {
    if (!row_has(rows, j)) return false;
    p->x = side < 0 ? 2 * rows[2 * j] - 1 : 2 * rows[2 * j + 1] + 1;
    return true;
  }
  bool any = false;
  for (int r = j - 1; r <= j; ++r) {
    if (r < 0 || r >= h || !row_has(rows, r)) continue;
    const int v = side < 0 ? 2 * rows[2 * r] : 2 * rows[2 * r + 1];
    if (!any || (side < 0 ? v < p->x : v > p->x)) p->x = v;
    any = true;
  }
  return any;
}

// one step of the monotone chain: the point p, below every point of the chain st[0 .. n), is added; the points it makes concave (or
// collinear) leave.  Returns the new length.
MH_HD int chain_step(Pt* st, int n, Pt p, int side) {
  while (n >= 2) {
    const long long c = cross(st[n - 2], st[n - 1], p);
    if (side < 0 ? c > 0 : c < 0) break;
    --n;
  }
  st[n] = p;
  return n + 1;
}

// the left (side < 0) or right chain of the hull of the diamond points of a row table, top to bottom; st holds level_count(h) points
MH_HD int build_chain(const int* rows, int h, int y0, int side, Pt* st) {
  int n = 0;
  const int levels = level_count(h);
  for (int k = 0; k < levels; ++k) {
    Pt p;
    if (level_point(rows, h, y0, k, side, &p)) n = chain_step(st, n, p, side);
  }
  return n;
}

// the chain's x at the height y, as num / den with den > 0; false: y is outside the chain's heights
MH_HD bool chain_at(const Pt* st, int n, int y, long long* num, long long* den) {
  if (n <= 0 || y < st[0].y || y > st[n - 1].y) return false;
  int lo = 0, hi = n - 1;                                              // the last vertex at or above y
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (st[mid].y <= y) lo = mid; else hi = mid - 1;
  }
  const Pt a = st[lo];
  if (a.y == y) { *num = a.x; *den = 1; return true; }
  const Pt b = st[lo + 1];                                             // lo < n - 1, as y <= st[n - 1].y
  *den = (long long)b.y - a.y;
  *num = (long long)a.x * *den + ((long long)b.x - a.x) * ((long long)y - a.y);
  return true;
}

// the convex image's pixels of image row `row`: (first, last) into out[0], out[1], first > last for none; returns their number
MH_HD long long row_interval(const Pt* left, int nl, const Pt* right, int nr, int row, int* out) {
  long long ln, ld, rn, rd;
  out[0] = INT_MAX;
  out[1] = INT_MIN;
  if (!chain_at(left, nl, 2 * row, &ln, &ld) || !chain_at(right, nr, 2 * row, &rn, &rd)) return 0;
  const long long first = ceil_div(ln, 2 * ld), last = floor_div(rn, 2 * rd);
  if (first > last) return 0;
  out[0] = (int)first;
  out[1] = (int)last;
  return last - first + 1;
}

// the row table iv of the convex image from the two chains, the rows lane, lane + lanes, ..; returns the pixels of these rows
MH_HD long long intervals_of(const Pt* left, int nl, const Pt* right, int nr, int h, int y0, int* iv, int lane, int lanes) {
  long long area = 0;
  for (int j = lane; j < h; j += lanes) area += row_interval(left, nl, right, nr, y0 + j, iv + 2 * j);
  return area;
}

MH_HD Pt chain_vertex(const Pt* left, int nl, const Pt* right, int i) { return i < nl ? left[i] : right[i - nl]; }

MH_HD long long dist2(Pt a, Pt b) {
  const long long dy = (long long)a.y - b.y, dx = (long long)a.x - b.x;
  return dy * dy + dx * dx;
}

// the largest squared distance between vertex i and a later vertex, over i = lane, lane + lanes, ..
MH_HD long long far_pairs(const Pt* left, int nl, const Pt* right, int nr, int lane, int lanes) {
  long long best = 0;
  const int n = nl + nr;
  for (int i = lane; i < n; i += lanes) {
    const Pt a = chain_vertex(left, nl, right, i);
    for (int j = i + 1; j < n; ++j) {
      const long long d = dist2(a, chain_vertex(left, nl, right, j));
      if (d > best) best = d;
    }
  }
  return best;
}

// ints of workspace an object of h rows needs outside LDS: its interval table and two chains of level_count(h) points (rounded up to even)
MH_HD long long workspace_ints(int h) { return 2ll * h + 2ll * 2ll * (2ll * h + 2ll); }

}  // namespace measure_hull
