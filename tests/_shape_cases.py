"""Cases for stardist_amd.utils.measure_labels(shape=True), shared by tests/test_cpu_measure_shape.py (host route, brute force,
scikit-image golden, host harness of csrc/measure_shape.h) and tests/test_gpu_measure_shape.py (the kernels): deterministic and small.
`case(name)` gives the label image, `host(name)` the host route's table and `raw(name)` its raw integer columns, computed once per case
and kept read-only.  `brute_force` restates the definitions of the raw columns in Python integers, `vector_oracle` with whole-image
numpy operations written differently from the host route's (skimage's convolution codes)."""
import numpy as np

import _measure_cases as M

MSH_TILE_Y, MSH_TILE_X, MSH_HALO = 16, 64, 2      # restated from csrc/measure_shape.h (test_cpu_measure_shape.py checks the header)

_cache, _host, _raw = {}, {}, {}


def _patterns(bits, cell):
    """every non-empty bits x bits binary pattern as an object of its own, label = the pattern's number, in cells of `cell` pixels with
    the pattern at offset 1; the cells fill a square grid row by row"""
    n = 2 ** (bits * bits) - 1
    side = int(np.ceil(np.sqrt(n)))
    ids = np.arange(1, n + 1, dtype=np.int64)
    a = np.zeros((side * cell, side * cell), np.int32)
    cy, cx = (ids - 1) // side * cell + 1, (ids - 1) % side * cell + 1
    for k in range(bits * bits):
        on = (ids >> k) & 1 == 1
        a[cy[on] + k // bits, cx[on] + k % bits] = ids[on]
    return a


def patterns3x3():
    """the 511 non-empty 3 x 3 patterns in 5 x 5 cells: 115 x 115"""
    return _patterns(3, 5)


def patterns4x4():
    """the 65535 non-empty 4 x 4 patterns in 6 x 6 cells, 1536 x 1536: disconnected objects, diagonal chains, holes"""
    return _patterns(4, 6)


def blobs2d():
    """200 x 260: 100 rotated ellipses of radii 1 .. 22 with 3 % of their pixels knocked out, painted over one another"""
    rng = np.random.default_rng(5101)
    shape = (200, 260)
    a = np.zeros(shape, np.int32)
    yy, xx = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    for k in range(100):
        cy, cx, ry, rx, th = rng.uniform(0, shape[0]), rng.uniform(0, shape[1]), rng.uniform(1, 22), rng.uniform(1, 22), rng.uniform(0, np.pi)
        u = (yy - cy) * np.cos(th) + (xx - cx) * np.sin(th)
        v = -(yy - cy) * np.sin(th) + (xx - cx) * np.cos(th)
        a[((u / ry) ** 2 + (v / rx) ** 2 <= 1.0) & (rng.random(shape) >= 0.03)] = k + 1
    return a


def blobs3d():
    """48 x 70 x 64: 100 rotated ellipsoids of radii 1 .. 12 with 3 % of their pixels knocked out, painted over one another"""
    rng = np.random.default_rng(5102)
    shape = (48, 70, 64)
    a = np.zeros(shape, np.int32)
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), axis=-1)
    for k in range(100):
        c = np.array([rng.uniform(0, n) for n in shape])
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        r = rng.uniform(1, 12, 3)
        w = (grid - c) @ q / r
        a[((w * w).sum(axis=-1) <= 1.0) & (rng.random(shape) >= 0.03)] = k + 1
    return a


def edges(dy, dx):
    """(3 tiles + dy) x (2 tiles + dx) pixels: one-pixel lines along the four image borders and an object in every image corner, then
    painted over them a small disc on every tile corner and a bar across every tile edge"""
    Y, X = 3 * MSH_TILE_Y + dy, 2 * MSH_TILE_X + dx
    a = np.zeros((Y, X), np.int32)
    nxt = iter(range(1, 1000))
    yy, xx = np.mgrid[:Y, :X]
    a[0, 4:X - 4] = next(nxt)
    a[Y - 1, 4:X - 4] = next(nxt)
    a[4:Y - 4, 0] = next(nxt)
    a[4:Y - 4, X - 1] = next(nxt)
    for ys, xs in ((slice(0, 2), slice(0, 3)), (slice(0, 3), slice(X - 2, X)), (slice(Y - 2, Y), slice(0, 2)), (slice(Y - 1, Y), slice(X - 1, X))):
        a[ys, xs] = next(nxt)
    for ty in range(0, Y + MSH_TILE_Y, MSH_TILE_Y):
        for tx in range(0, X + MSH_TILE_X, MSH_TILE_X):
            a[(yy - ty) ** 2 + (xx - tx) ** 2 <= 6] = next(nxt)                                # a disc on the tile corner
            a[(np.abs(yy - ty) <= 2) & (np.abs(xx - tx - MSH_TILE_X // 2) <= 5)] = next(nxt)   # across a horizontal tile edge
            a[(np.abs(xx - tx) <= 2) & (np.abs(yy - ty - MSH_TILE_Y // 2) <= 3)] = next(nxt)   # across a vertical one
    return a


EDGE_DELTAS = ((-2, 1), (-1, 2), (1, -2), (2, -1))          # every delta in both axes

_LABELS = {
    "small_2d": M.small_2d, "small_3d": M.small_3d, "chunked": M.chunked, "patterns3x3": patterns3x3, "patterns4x4": patterns4x4,
    "blobs2d": blobs2d, "blobs3d": blobs3d,
    "one_pixel": lambda: np.array([[3]], np.int32),
    "row": lambda: np.array([[1, 1, 0, 2, 0, 3, 3, 3, 0, 0, 1, 7, 7]], np.int32),
    "column": lambda: np.array([[1, 1, 0, 2, 0, 3, 3, 3, 0, 0, 1, 7, 7]], np.int32).T.copy(),
    "huge_ids": lambda: M.huge_ids()[0],
    "empty_2d": lambda: np.zeros((7, 9), np.int32),
    "empty_3d": lambda: np.zeros((3, 7, 9), np.int32) - 1,
}
for _dy, _dx in EDGE_DELTAS:
    _LABELS["edges%+d%+d" % (_dy, _dx)] = (lambda dy=_dy, dx=_dx: edges(dy, dx))
EDGES = tuple(n for n in _LABELS if n.startswith("edges"))
NAMES = tuple(_LABELS)
SMALL = tuple(n for n in NAMES if n != "patterns4x4")        # what a per-object loop can afford
GOLDEN = ("small_2d", "small_3d", "patterns3x3", "blobs2d", "blobs3d")


def case(name):
    got = _cache.get(name)
    if got is None:
        got = _cache[name] = _LABELS[name]()
        got.setflags(write=False)
    return got


def host(name):
    """the host route's table with shape=True (read-only, computed once)"""
    got = _host.get(name)
    if got is None:
        from stardist_amd.utils import measure_labels
        got = _host[name] = measure_labels(case(name), shape=True)
        for v in got.values():
            v.setflags(write=False)
    return got


def raw(name):
    """the host route's raw columns with shape=True (read-only, computed once)"""
    got = _raw.get(name)
    if got is None:
        from stardist_amd.label_ops import _measure_raw_host
        got = _raw[name] = _measure_raw_host(case(name), None, True)
        for v in got.values():
            v.setflags(write=False)
    return got


def shape_keys(nd):
    """the columns shape=True appends, in order"""
    out = ["equivalent_diameter", "extent"] + ["inertia_tensor-%d-%d" % (i, j) for i in range(nd) for j in range(nd)]
    out += ["inertia_tensor_eigvals-%d" % k for k in range(nd)] + ["major_axis_length", "minor_axis_length"]
    if nd == 2:
        out += ["eccentricity", "orientation", "perimeter", "perimeter_crofton", "euler_number"]
    return out


LIBM = ("orientation", "equivalent_diameter")               # columns that call atan2 / pow (the latter in 3D only)


def brute_force(lbl):
    """{label: (m2 list of 6, contour list of 18 or None)} by the definitions, in Python integers, pixel by pixel"""
    a = np.where(lbl > 0, lbl, 0)
    nd = a.ndim
    L = a.tolist()
    shape = a.shape

    def at(*p):
        if any(c < 0 or c >= n for c, n in zip(p, shape)):
            return 0
        v = L
        for c in p:
            v = v[c]
        return v
    pixels = {}
    for p in zip(*np.nonzero(a)):
        pixels.setdefault(at(*p), []).append(tuple(int(c) for c in p))
    out = {}
    for l, pts in pixels.items():
        start = [min(p[d] for p in pts) for d in range(nd)]
        u = [[0] * (3 - nd) + [p[d] - start[d] for d in range(nd)] for p in pts]
        m2 = [sum(q[i] * q[j] for q in u) for i in range(3) for j in range(i, 3)]
        counts = None
        if nd == 2:
            border = lambda y, x: at(y, x) == l and any(at(y + dy, x + dx) != l for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)))
            counts = [0] * 18
            for y, x in pts:
                if not border(y, x):
                    continue
                na = sum(border(y + dy, x + dx) for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)))
                nd_ = sum(border(y + dy, x + dx) for dy, dx in ((-1, -1), (-1, 1), (1, -1), (1, 1)))
                if (na, nd_) in ((2, 0), (3, 0), (2, 1), (3, 1), (2, 2), (3, 2)):
                    counts[0] += 1
                elif (na, nd_) in ((0, 2), (1, 3)):
                    counts[1] += 1
                elif (na, nd_) in ((1, 1), (1, 2)):
                    counts[2] += 1
            windows = {(y + di, x + dj) for y, x in pts for di in (0, 1) for dj in (0, 1)}
            for i, j in windows:
                code = 1 * (at(i, j) == l) + 4 * (at(i, j - 1) == l) + 2 * (at(i - 1, j) == l) + 8 * (at(i - 1, j - 1) == l)
                counts[2 + code] += 1
        out[int(l)] = (m2, counts)
    return out


def vector_oracle(lbl):
    """(labels present, m2 (n, 6), contour (n, 18)) of a 2D image by whole-image numpy, the way scikit-image computes them for one
    mask -- erosion by the cross, the 10 / 2 / 1 neighbour code, the 1 / 2 / 4 / 8 window code -- with the label carried along"""
    a = np.where(lbl > 0, lbl, 0).astype(np.int64)
    Y, X = a.shape
    labels = np.unique(a[a > 0])
    top = int(labels.max())
    ys, xs = np.nonzero(a)
    l = a[ys, xs]
    y0 = np.full(top + 1, Y); x0 = np.full(top + 1, X)
    np.minimum.at(y0, l, ys); np.minimum.at(x0, l, xs)
    uy, ux = ys - y0[l], xs - x0[l]
    m2 = np.zeros((top + 1, 6), np.int64)
    order = np.argsort(l, kind="stable")
    first = np.searchsorted(l[order], labels)
    for k, v in ((3, uy * uy), (4, uy * ux), (5, ux * ux)):
        m2[labels, k] = np.add.reduceat(v[order], first)
    P = np.pad(a, 1)
    c = P[1:-1, 1:-1]
    eroded = (P[:-2, 1:-1] == c) & (P[2:, 1:-1] == c) & (P[1:-1, :-2] == c) & (P[1:-1, 2:] == c)
    bl = np.pad(np.where((c > 0) & ~eroded, c, 0), 1)       # the border image, carrying the label
    code = np.zeros((Y, X), np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            wgt = 1 if (dy, dx) == (0, 0) else (2 if dy == 0 or dx == 0 else 10)
            code += wgt * ((bl[1 + dy:1 + dy + Y, 1 + dx:1 + dx + X] == c) & (c > 0))
    code[bl[1:-1, 1:-1] == 0] = 0
    counts = np.zeros((top + 1, 18), np.int64)
    for field, codes in ((0, (5, 7, 15, 17, 25, 27)), (1, (21, 33)), (2, (13, 23))):
        counts[:, field] = np.bincount(a[np.isin(code, codes)], minlength=top + 1)
    Q = np.pad(a, 1)
    w = {1: Q[1:, 1:], 4: Q[1:, :-1], 2: Q[:-1, 1:], 8: Q[:-1, :-1]}
    key = np.zeros(0, np.int64)
    for bit, mine in w.items():                              # every (window, label) pair, then made unique
        xf = sum(b * (other == mine) for b, other in w.items())
        pos = np.flatnonzero(mine.reshape(-1) > 0)
        key = np.concatenate([key, (pos * (top + 1) + mine.reshape(-1)[pos]) * 16 + xf.reshape(-1)[pos]])
    key = np.unique(key)
    lab_of, code_of = (key // 16) % (top + 1), key % 16
    np.add.at(counts, (lab_of, 2 + code_of), 1)
    return labels, m2[labels], counts[labels]
