"""numpy statements of what the 2D NMS computes per candidate and per candidate pair before any polygon is clipped, for the tests of
csrc/nms2d.hip -- float32 where the reference (stardist2d.cpp, compiled with -ffp-contract=off) computes in float, int64 where it computes
in cInt:

  build(dist, points):  integer vertices (:454-471: centre + d * (sin, cos), multiply and add rounded separately, truncated toward zero),
                        integer bounding box (:142-148), outer radius, polygon area (:128-138: float accumulation of the int64 cross
                        products in path order; equal to the exact integer sum while sum |term| < 2^24).
  neighbour_pairs(...): the number of unordered pairs that pass the symmetric `may_interact` predicate of the neighbour lists, brute force.

and the triples scene of tests/test_gpu_nms2d_lists.py (proven against the compiled reference in tests/test_cpu_nms2d_lists_scene.py)."""
import ctypes
import ctypes.util

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in (_libm.sinf, _libm.cosf):
    _f.restype = ctypes.c_float
    _f.argtypes = [ctypes.c_float]


def ray_table(R):
    """(sin, cos) of the R ray angles as the library's host code and the reference compute them: float32 angle, the C library's sinf / cosf"""
    step = np.float32(2 * np.pi / R)
    ang = [np.float32(step * np.float32(k)) for k in range(R)]
    return (np.array([_libm.sinf(float(a)) for a in ang], np.float32), np.array([_libm.cosf(float(a)) for a in ang], np.float32))


def path_area(X, Y):
    """area_from_path (:128-138) of the closed integer paths in the rows of X, Y (n, R) int64 -> (area (n,) f32, sum |term| (n,) int64):
    the cross products a.X * b.Y - a.Y * b.X are exact in int64, each is converted to float and added to a float accumulator in path order;
    while sum |term| < 2^24 every partial sum is an integer below 2^24 and the float sum equals the exact one"""
    X = np.asarray(X, np.int64); Y = np.asarray(Y, np.int64)
    n, R = X.shape
    term = X * np.roll(Y, -1, 1) - Y * np.roll(X, -1, 1)
    s = term.sum(1); sum_abs = np.abs(term).sum(1)
    serial = np.zeros(n, np.float32)
    for k in range(R):                                       # the reference's own order, one float addition per edge
        serial = (serial + term[:, k].astype(np.float32)).astype(np.float32)
    a = np.where(sum_abs < (1 << 24), s.astype(np.float32), serial)
    return (0.5 * np.abs(a).astype(np.float64)).astype(np.float32), sum_abs


def build(dist, points):
    """dict(X, Y (n, R) int64, bbox (n, 4) int64 [xmin, xmax, ymin, ymax], radius (n,) f32, area (n,) f32, sum_abs (n,) int64,
    gstats (5,) int64: bits of the largest distance, min / max floor(y), min / max floor(x) of the centres)"""
    dist = np.ascontiguousarray(dist, np.float32); points = np.ascontiguousarray(points, np.float32)
    n, R = dist.shape
    assert n >= 1
    sn, cs = ray_table(R)
    y = (points[:, :1] + (dist * sn[None, :]).astype(np.float32)).astype(np.float32)
    x = (points[:, 1:2] + (dist * cs[None, :]).astype(np.float32)).astype(np.float32)
    X = np.trunc(x).astype(np.int64); Y = np.trunc(y).astype(np.int64)      # cInt(x): toward zero, not floor
    area, sum_abs = path_area(X, Y)
    bbox = np.stack([X.min(1), X.max(1), Y.min(1), Y.max(1)], 1)
    radius = np.maximum(dist.max(1), np.float32(0)).astype(np.float32)
    fy, fx = np.floor(points[:, 0]).astype(np.int64), np.floor(points[:, 1]).astype(np.int64)
    gstats = np.array([int(radius.max().view(np.int32)), fy.min(), fy.max(), fx.min(), fx.max()], np.int64)
    return dict(X=X, Y=Y, bbox=bbox, radius=radius, area=area, sum_abs=sum_abs, gstats=gstats)


REGIMES = ("a", "b", "c", "d")


def build_case(regime, n, R, seed=0):
    """dist (n, R) f32, points (n, 2) f32 of one regime of the build tests:
      a  centres in [0, 300), distances 10 +- 10 %: sum |term| < 2^24, the exact integer area;
      b  centres in [-50, 50], distances up to 60: vertices on both sides of zero (truncation toward zero is not floor);
      c  centres near (30 000, 30 000), distances 200 .. 300: sum |term| >= 2^24, the serial float accumulation in path order;
      d  distances 1e-3 around centres at least 0.1 away from the pixel borders: every vertex truncates to the same point, area 0."""
    rng = np.random.RandomState(1000 * R + n + 17 * seed)
    if regime == "a":
        pts = rng.uniform(0, 300, (n, 2)); dist = 10 * (1 + 0.1 * rng.uniform(-1, 1, (n, R)))
    elif regime == "b":
        pts = rng.uniform(-50, 50, (n, 2)); dist = rng.uniform(0, 60, (n, R))
    elif regime == "c":
        pts = 30000 + rng.uniform(-100, 100, (n, 2)); dist = rng.uniform(200, 300, (n, R))
    else:
        pts = np.floor(rng.uniform(0, 300, (n, 2))) + rng.uniform(0.1, 0.9, (n, 2)); dist = np.full((n, R), 1e-3)      # (no vertex crosses a pixel border)
    return np.ascontiguousarray(dist, np.float32), np.ascontiguousarray(pts, np.float32)


def neighbour_pairs(dist, points, use_kdtree, use_bbox, thr, block=512):
    """unordered pairs (i < j) that pass may_interact (csrc/nms2d.hip), in its float32 form"""
    b = build(dist, points)
    bb, ar = b["bbox"], b["area"]
    pts = np.ascontiguousarray(points, np.float32)
    n = len(pts)
    thr = np.float32(thr)
    max_dist = b["radius"].max() if n else np.float32(0)
    rr = np.float32(np.float32(2) * max_dist + np.float32(1))
    rr2 = np.float32(rr * rr)
    total = 0
    for i0 in range(0, n, block):
        i = np.arange(i0, min(i0 + block, n))[:, None]
        j = np.arange(n)[None, :]
        inter = (bb[j, 0] <= bb[i, 1]) & (bb[i, 0] <= bb[j, 1]) & (bb[j, 2] <= bb[i, 3]) & (bb[i, 2] <= bb[j, 3])
        if thr >= 0:
            w = (np.minimum(bb[i, 1], bb[j, 1]) - np.maximum(bb[i, 0], bb[j, 0])).astype(np.float32)
            h = (np.minimum(bb[i, 3], bb[j, 3]) - np.maximum(bb[i, 2], bb[j, 2])).astype(np.float32)
            wh = (w * h).astype(np.float32)
            lhs = (wh * np.float32(1.00001)).astype(np.float32)
            rhs = ((thr * np.minimum(ar[i], ar[j])).astype(np.float32) * np.float32(0.99999)).astype(np.float32)
            ok = inter & (lhs >= rhs)
        else:
            ok = np.ones((len(i), n), bool)
            if use_bbox:
                ok &= inter
            if use_kdtree:
                dy = (pts[i, 0] - pts[j, 0]).astype(np.float32); dx = (pts[i, 1] - pts[j, 1]).astype(np.float32)
                d2 = ((dy * dy).astype(np.float32) + (dx * dx).astype(np.float32)).astype(np.float32)
                ok &= d2 < rr2
        total += int((ok & (i < j)).sum())
    return total


def slot_capacities(dist, points, thr, use_bbox=1):
    """The slot capacities of the single-pass neighbour lists (csrc/nms2d.hip: build_grid, cell_of, cell_window, k_cell_fill), exactly:
    reach, cell size and grid origin as the host derives them from the largest distance and the floors of the centres (float32, the cell
    counts by a float64 quotient), the cell of a centre and the window of a bounding box in float32 -- one subtraction, one product and
    one truncation resp. floor each --, and per candidate the population of its window's cells minus itself.
    -> dict(cap (n,) int64, total int: their sum, ny, nx, reach f32, cs f32)"""
    f = np.float32
    b = build(dist, points)
    pts = np.ascontiguousarray(points, np.float32)
    gs = b["gstats"]
    max_dist = b["radius"].max()
    reach = f(f(f(max_dist + f(1)) * f(1.0001)) + f(1e-3))
    cs = f(f(0.5) * reach)
    if not cs >= f(1):
        cs = f(1)
    while True:
        ny = int((float(gs[2]) - float(gs[1])) / float(cs)) + 1
        nx = int((float(gs[4]) - float(gs[3])) / float(cs)) + 1
        if ny * nx <= (1 << 26):
            break
        cs = f(cs * f(2))
    y0, x0, inv_cs = f(gs[1]), f(gs[3]), f(f(1) / cs)

    def cell(v, v0, hi):                                  # cell_of: (int) truncates toward zero
        return np.clip(np.trunc(((v - v0).astype(f) * inv_cs).astype(f)).astype(np.int64), 0, hi - 1)

    def edge(v, v0, hi):                                  # cell_window: floorf((v -+ 0.5f - v0) * inv_cs), clamped
        return np.clip(np.floor(((v - v0).astype(f) * inv_cs).astype(f)).astype(np.int64), 0, hi - 1)
    cy, cx = cell(pts[:, 0], y0, ny), cell(pts[:, 1], x0, nx)
    if thr >= 0 or use_bbox:
        bb = b["bbox"].astype(f)
        lo_x, hi_x, lo_y, hi_y = (bb[:, 0] - reach).astype(f), (bb[:, 1] + reach).astype(f), (bb[:, 2] - reach).astype(f), (bb[:, 3] + reach).astype(f)
    else:
        rr = f(f(2) * reach)
        lo_x, hi_x, lo_y, hi_y = (pts[:, 1] - rr).astype(f), (pts[:, 1] + rr).astype(f), (pts[:, 0] - rr).astype(f), (pts[:, 0] + rr).astype(f)
    ylo, yhi = edge((lo_y - f(0.5)).astype(f), y0, ny), edge((hi_y + f(0.5)).astype(f), y0, ny)
    xlo, xhi = edge((lo_x - f(0.5)).astype(f), x0, nx), edge((hi_x + f(0.5)).astype(f), x0, nx)
    pop = np.zeros((ny + 1, nx + 1), np.int64)             # pop[a, b] = candidates in the cells [0, a) x [0, b)
    np.add.at(pop, (cy + 1, cx + 1), 1)
    pop = pop.cumsum(0).cumsum(1)
    cap = pop[yhi + 1, xhi + 1] - pop[ylo, xhi + 1] - pop[yhi + 1, xlo] + pop[ylo, xlo] - 1
    return dict(cap=cap, total=int(cap.sum()), ny=ny, nx=nx, reach=reach, cs=cs)


# ---- the triples scene: pairs whose j is suppressed by a decided pair of the same round
TRIPLES = 200
TRIPLES_THR = np.float32(0.4)


def triples_scene(n_rays=32):
    """200 well-separated triples of exact discs in NMS order (all B, then all A, then all j):
      j  radius 12;
      B  radius 5, 6 px from j's centre (inside j: overlap / smaller area = 1), the best score of its triple;
      A  radius 12 on the opposite side of j, 11.0 .. 12.5 px from j's centre in equal steps over the triples: two discs of radius 12 that far
         apart overlap by 0.44 .. 0.37 of their area, so with the threshold 0.4 some (A, j) lie inside any band around the threshold.
    A and B meet at most along a bounding-box edge of zero width (A ends where B begins at 11.0 px, and before it otherwise), so neither
    lists the other: both are survivors of round 1, B suppresses j, and (A, j) is a pair of the same round whose j is already gone.
    Returns dist (600, R) f32, points (600, 2) f32, kinds (600,) of 'B' / 'A' / 'j'."""
    t = np.arange(TRIPLES)
    cy = 40.37 + 40.0 * (t // 20) + 0.011 * t
    cx = 60.61 + 60.0 * (t % 20) + 0.007 * t
    d = np.linspace(11.0, 12.5, TRIPLES)
    pts = np.concatenate([np.stack([cy, cx + 6.0], 1), np.stack([cy, cx - d], 1), np.stack([cy, cx], 1)])
    rad = np.concatenate([np.full(TRIPLES, 5.0), np.full(TRIPLES, 12.0), np.full(TRIPLES, 12.0)])
    dist = np.repeat(rad[:, None], n_rays, 1)
    kinds = np.array(["B"] * TRIPLES + ["A"] * TRIPLES + ["j"] * TRIPLES)
    return np.ascontiguousarray(dist, np.float32), np.ascontiguousarray(pts, np.float32), kinds
