"""Cases for stardist_amd.utils.measure_labels, shared by tests/test_cpu_measure.py (host route, scipy oracle, scikit-image golden,
host harness of csrc/measure.h) and tests/test_gpu_measure.py (the kernels): deterministic by seed and small.  `case(name)` gives
(lbl, img), `host(name)` the host route's table, computed once per case and kept read-only; `float_oracle(name)` the correctly
rounded sums (math.fsum) of a float32 case, and `check_float_columns` the derived bounds of the float comparisons."""
import math

import numpy as np

MS_CHUNK_PIXELS = 65536              # restated from csrc/measure.h (test_cpu_measure.py checks the header against it)
MS_WAVE_PIXELS = 4096                # likewise: boxes up to this size go to single-wave workgroups

_cache, _host, _oracle = {}, {}, {}


def _grids(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


def small_2d():
    """67 x 131: 38 discs and star shapes painted over one another (touching; centres up to the image border and beyond), a ring that
    encloses a disc (overlapping boxes), a one-pixel object; ids permuted with gaps; one label negated (background)"""
    rng = np.random.default_rng(4101)
    shape = (67, 131)
    a = np.zeros(shape, np.int32)
    yy, xx = _grids(shape)
    ids = rng.permutation(np.arange(1, 130))[:42]
    for k in range(38):
        cy, cx = rng.uniform(-2, shape[0] + 2), rng.uniform(-2, shape[1] + 2)
        r0 = rng.uniform(3.0, 9.0)
        ang = np.arctan2(yy - cy, xx - cx)
        r = r0 * (1.0 + (0.35 * np.cos(int(rng.integers(3, 7)) * ang + rng.uniform(0, 6.28)) if k % 2 else 0.0))
        a[np.hypot(yy - cy, xx - cx) <= r] = ids[k]
    d = np.hypot(yy - 33, xx - 100)
    a[d <= 13] = 0
    a[(d <= 12) & (d >= 10)] = ids[38]                                      # the ring ...
    a[d <= 4] = ids[39]                                                     # ... and the object inside its box
    a[a == ids[5]] *= -1                                                    # a negative label
    a[64:67, 0:3] = 0
    a[65, 1] = ids[40]                                                      # one pixel
    return a


def small_3d():
    """9 x 33 x 70: 14 ellipsoids painted over one another and one object that lies in a single plane; ids with gaps"""
    rng = np.random.default_rng(4102)
    shape = (9, 33, 70)
    a = np.zeros(shape, np.int32)
    zz, yy, xx = _grids(shape)
    ids = rng.permutation(np.arange(1, 60))[:15]
    for k in range(14):
        c = [rng.uniform(0, n) for n in shape]
        rz, ry, rx = rng.uniform(1.5, 4), rng.uniform(3, 8), rng.uniform(3, 10)
        a[((zz - c[0]) / rz) ** 2 + ((yy - c[1]) / ry) ** 2 + ((xx - c[2]) / rx) ** 2 <= 1.0] = ids[k]
    a[4, 12:19, 30:41] = ids[14]                                            # a single plane
    return a


def chunked():
    """about 600 x 700: one frame-shaped object whose box is the whole image -- sized from the chunk constant: six whole chunks of rows
    and a partial seventh -- with small objects inside its box"""
    X = 700
    rows = MS_CHUNK_PIXELS // X
    Y = 6 * rows + rows // 2
    a = np.zeros((Y, X), np.int32)
    a[:3] = a[-3:] = 7
    a[:, :3] = a[:, -3:] = 7
    rng = np.random.default_rng(4103)
    for k in range(30):
        y, x = int(rng.integers(5, Y - 30)), int(rng.integers(5, X - 30))
        a[y:y + int(rng.integers(1, 24)), x:x + int(rng.integers(1, 24))] = 10 + 2 * k
    y, x = _grids((Y, X))
    a[np.hypot(y - 300, x - 350) <= 45] = 3                                 # more than MS_WAVE_PIXELS pixels, one chunk
    return a


def _image(shape, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "u8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "u16":
        return rng.integers(0, 65536, shape, dtype=np.uint16)
    if kind == "exact":                                                     # every float64 partial sum of values and squares is exact
        return (rng.integers(-1000, 1001, shape).astype(np.float32) * np.float32(2.0 ** -6)).astype(np.float32)
    if kind == "random":
        return (1e3 * rng.standard_normal(shape) + 500).astype(np.float32)
    raise KeyError(kind)


def non_finite():
    """(lbl, img, {label: what}) on the small 2D labels: one object with a NaN pixel, one with +inf, one with +inf and -inf"""
    lbl = small_2d()
    img = _image(lbl.shape, "random", 4110)
    big = [int(l) for l in np.unique(lbl[lbl > 0]) if (lbl == l).sum() >= 20][:3]
    what = {}
    for l, vals in zip(big, ((np.nan,), (np.inf,), (np.inf, -np.inf))):
        ys, xs = np.nonzero(lbl == l)
        for k, v in enumerate(vals):
            img[ys[3 + 5 * k], xs[3 + 5 * k]] = v
        what[l] = vals
    return lbl, img, what


def huge_ids():
    """the small 2D labels as int64 with ids up to 2^40 (ascending order kept): the compaction route of _device_labels"""
    lbl = small_2d().astype(np.int64)
    present = np.unique(lbl[lbl > 0])
    new = 1000 + 977 * np.arange(len(present), dtype=np.int64)
    new[-3:] = [2 ** 31 - 1, 2 ** 31 + 5, 2 ** 40]
    rename = np.zeros(int(present.max()) + 1, np.int64)
    rename[present] = new
    out = np.where(lbl > 0, rename[np.maximum(lbl, 0)], lbl)
    return out, present, new


_LABELS = {"2d": small_2d, "3d": small_3d, "chunked": chunked}
# name -> (labels, image kind or None, channels or None for no channel axis, seed)
_TABLE = {
    "2d_none": ("2d", None, None, 0),
    "2d_u8_rgb": ("2d", "u8", 3, 4120),                                    # 131 * 3 = 393 bytes per row
    "2d_u16": ("2d", "u16", None, 4121),
    "2d_u16_c1": ("2d", "u16", 1, 4121),
    "2d_f32_exact": ("2d", "exact", None, 4122),
    "2d_f32_random": ("2d", "random", None, 4123),
    "2d_f32_random_c2": ("2d", "random", 2, 4124),
    "3d_none": ("3d", None, None, 0),
    "3d_u8": ("3d", "u8", None, 4130),
    "3d_u16": ("3d", "u16", None, 4131),
    "3d_f32_exact": ("3d", "exact", None, 4132),
    "3d_f32_random": ("3d", "random", None, 4133),
    "chunked_u8_rgb": ("chunked", "u8", 3, 4140),
    "chunked_u16": ("chunked", "u16", None, 4141),
    "chunked_f32_exact": ("chunked", "exact", None, 4142),
    "chunked_f32_random": ("chunked", "random", None, 4143),
}
SPECIAL = ("all_65535", "non_finite", "huge_ids_u16", "empty_none", "empty_f32")
NAMES = tuple(_TABLE) + SPECIAL
INTEGER = tuple(n for n in NAMES if "_u8" in n or "_u16" in n or n == "all_65535")
FLOAT_EXACT = tuple(n for n in _TABLE if n.endswith("_exact"))
FLOAT_RANDOM = tuple(n for n in _TABLE if "_random" in n)


def case(name):
    """(lbl, img or None), read-only"""
    got = _cache.get(name)
    if got is None:
        if name in _TABLE:
            which, kind, C, seed = _TABLE[name]
            lbl = _LABELS[which]()
            img = None if kind is None else _image(lbl.shape + (() if C is None else (C,)), kind, seed)
        elif name == "all_65535":                                           # sum of squares 2.25e6 * 65535^2 ~ 2^53.1
            lbl, img = np.ones((1500, 1500), np.int32), np.full((1500, 1500), 65535, np.uint16)
        elif name == "non_finite":
            lbl, img, _ = non_finite()
        elif name == "huge_ids_u16":
            lbl, img = huge_ids()[0], _image((67, 131), "u16", 4121)
        elif name == "empty_none":
            lbl, img = np.zeros((11, 13), np.int32), None
        elif name == "empty_f32":
            lbl, img = np.zeros((4, 11, 13), np.int32) - 1, _image((4, 11, 13, 2), "random", 4150)
        else:
            raise KeyError(name)
        for a in (lbl, img):
            if a is not None:
                a.setflags(write=False)
        got = _cache[name] = (lbl, img)
    return got


def host(name):
    """the host route's table for the case (read-only, computed once)"""
    got = _host.get(name)
    if got is None:
        from stardist_amd.utils import measure_labels
        got = measure_labels(*case(name))
        for v in got.values():
            v.setflags(write=False)
        _host[name] = got
    return got


def keys(nd, C=None, channel_axis=False):
    """the columns of the table, in order"""
    out = ["label", "area"] + ["bbox-%d" % k for k in range(2 * nd)] + ["centroid-%d" % k for k in range(nd)]
    if C is not None:
        for name in ("sum_intensity", "mean_intensity", "min_intensity", "max_intensity", "std_intensity"):
            out += [("%s-%d" % (name, c)) for c in range(C)] if channel_axis else [name]
    return out


def case_keys(name):
    lbl, img = case(name)
    if img is None:
        return keys(lbl.ndim)
    return keys(lbl.ndim, 1 if img.ndim == lbl.ndim else img.shape[-1], img.ndim > lbl.ndim)


def float_oracle(name):
    """per label present (ascending) and channel of a float32 case: count (n,), and (n, C) float64 arrays S = fsum(v), S2 = fsum(v^2)
    (the squares are exact in float64), A = fsum(|v|)"""
    got = _oracle.get(name)
    if got is None:
        lbl, img = case(name)
        v = img.reshape(lbl.shape + (-1,)).astype(np.float64)
        labels = np.unique(lbl[lbl > 0])
        C = v.shape[-1]
        S, S2, A = (np.zeros((len(labels), C)) for _ in range(3))
        count = np.zeros(len(labels), np.int64)
        for k, l in enumerate(labels):
            vals = v[lbl == l]
            count[k] = len(vals)
            for c in range(C):
                col = vals[:, c].tolist()
                S[k, c], S2[k, c], A[k, c] = math.fsum(col), math.fsum(x * x for x in col), math.fsum(abs(x) for x in col)
        got = _oracle[name] = {"label": labels.astype(np.int64), "count": count, "S": S, "S2": S2, "A": A}
    return got


def sum_bounds(oracle):
    """the derived bounds of the float sums, per object and channel: any order of n float64 additions errs by at most (n - 1) u sum|x|
    to first order (u = 2^-53); device and oracle each get that much: count * 2^-52 * sum|v| for S, count * 2^-52 * sum v^2 for S2"""
    n = oracle["count"][:, None].astype(np.float64)
    return n * 2.0 ** -52 * oracle["A"], n * 2.0 ** -52 * oracle["S2"]


def check_float_columns(name, table, exact=False, sums2=None):
    """the sum / mean / std columns of a float32 case's table against math.fsum: within the derived bounds, or bit for bit where every
    partial sum is exact (`exact`); sums2: the (n, C) sums of squares where the caller has them"""
    o = float_oracle(name)
    lbl, img = case(name)
    chan = img.ndim > lbl.ndim
    bS, bS2 = sum_bounds(o)
    n = o["count"].astype(np.float64)
    for c in range(o["S"].shape[1]):
        col = lambda key: np.asarray(table[("%s-%d" % (key, c)) if chan else key])
        S = col("sum_intensity")
        assert S.dtype == np.float64
        mean_o = o["S"][:, c] / n
        var_o = np.maximum(0.0, o["S2"][:, c] / n - mean_o * mean_o)
        if exact:
            assert np.array_equal(S, o["S"][:, c]), name
            assert np.array_equal(col("mean_intensity"), mean_o), name
            assert np.array_equal(col("std_intensity"), np.sqrt(var_o)), name
            if sums2 is not None:
                assert np.array_equal(sums2[:, c], o["S2"][:, c]), name
            continue
        assert (np.abs(S - o["S"][:, c]) <= bS[:, c]).all(), name
        if sums2 is not None:
            assert (np.abs(sums2[:, c] - o["S2"][:, c]) <= bS2[:, c]).all(), name
        assert np.array_equal(col("mean_intensity"), S / n), name                               # mean = float64(sum) / count
        bound = 8 * 2.0 ** -53 * (o["S2"][:, c] / n + mean_o * mean_o) + (bS[:, c] + bS2[:, c]) / n
        std = col("std_intensity")
        assert (np.abs(std * std - var_o) <= bound).all(), name
