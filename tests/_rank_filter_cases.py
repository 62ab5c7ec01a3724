"""Cases of the rank-filter tests (tests/test_cpu_rank_filters.py, tests/test_gpu_rank_filters.py): images, windows, modes, origins and
ranks for the nine public functions of stardist_amd.rank_filters, and their definition as a loop over the pixels (brute): an explicit
index map per axis, sorted() per window, the NaN rule, the compositions of grey morphology."""
import numpy as np

DTYPES = (np.bool_, np.uint8, np.uint16, np.float32)
MODES = ("reflect", "nearest", "mirror", "constant")
FILTERS = ("minimum_filter", "maximum_filter", "median_filter", "rank_filter", "percentile_filter")
MORPHOLOGY = ("grey_opening", "grey_closing", "white_tophat", "black_tophat")


def noise(shape, dtype, seed=0):
    rng = np.random.RandomState(seed)
    if dtype == np.float32:
        return (rng.standard_normal(shape) * 100).astype(np.float32)
    if dtype == np.bool_:
        return rng.rand(*shape) > 0.5
    return rng.randint(0, np.iinfo(dtype).max + 1, shape).astype(dtype)


def a_cval(dtype, k=0):
    """a value of the dtype that is not the default, for mode constant"""
    return {"bool": (True, False), "uint8": (7, 200), "uint16": (300, 65000), "float32": (-2.5, 40.0)}[np.dtype(dtype).name][k % 2]


# ----------------------------------------------------------------------------- footprints

def disc(r):
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return y * y + x * x <= r * r


def ball(r):
    z, y, x = np.mgrid[-r:r + 1, -r:r + 1, -r:r + 1]
    return z * z + y * y + x * x <= r * r


def footprints():
    cross = np.zeros((5, 5), bool)
    cross[2, :] = cross[:, 2] = True
    ell = np.zeros((4, 3), bool)                                            # an asymmetric L
    ell[:, 0] = ell[3, :] = True
    single = np.zeros((3, 4), bool)                                         # one true element, off centre
    single[0, 3] = True
    rnd = np.random.RandomState(40).rand(4, 5) > 0.5
    rnd[0, 0] = True
    return {"disc3": disc(3), "cross": cross, "ell": ell, "single": single, "random4x5": rnd}


# ----------------------------------------------------------------------------- the definition as a loop

def index_map(n, left, size, mode):
    """(n, size) indices: the element of a line of n that the j-th window element of output i reads, -1 where mode constant reads cval.
    The line is extended by writing out one period of scipy's rule: reflect d c b a | a b c d | d c b a, mirror d c b | a b c d | c b a,
    nearest a a | a b c d | d d."""
    if mode == "reflect":
        period = list(range(n)) + list(range(n - 1, -1, -1))
    elif mode == "mirror":
        period = list(range(n)) + list(range(n - 2, 0, -1))
    out = np.empty((n, size), np.int64)
    for i in range(n):
        for j in range(size):
            p = i - left + j
            if 0 <= p < n:
                out[i, j] = p
            elif mode == "constant":
                out[i, j] = -1
            elif mode == "nearest":
                out[i, j] = 0 if p < 0 else n - 1
            else:
                out[i, j] = period[p % len(period)]
    return out


def brute_rank(img, rank, extent, footprint, mode, cval, origin):
    """the rank-th smallest (0-based, not negative) of the footprint's elements around every pixel, NaN where a window covers a NaN"""
    fp = np.ones(extent, bool) if footprint is None else np.asarray(footprint, bool)
    maps = [index_map(n, e // 2 + o, e, mode) for n, e, o in zip(img.shape, fp.shape, origin)]
    offsets = np.argwhere(fp)
    stack = np.empty((len(offsets),) + img.shape, img.dtype)
    for k, off in enumerate(offsets):
        idx = [m[:, o] for m, o in zip(maps, off)]
        outside = np.zeros(img.shape, bool)
        for ax, i in enumerate(idx):
            outside |= (i < 0).reshape([-1 if a == ax else 1 for a in range(img.ndim)])
        stack[k] = np.where(outside, img.dtype.type(cval), img[np.ix_(*[np.maximum(i, 0) for i in idx])])
    flat = stack.reshape(len(offsets), -1)
    out = np.empty(flat.shape[1], img.dtype)
    for p in range(flat.shape[1]):
        window = flat[:, p].tolist()
        out[p] = np.nan if any(v != v for v in window) else sorted(window)[rank]
    return out.reshape(img.shape)


def rank_of(fn, n, kw):
    """scipy's rank rules, restated"""
    if fn == "minimum_filter":
        return 0
    if fn == "maximum_filter":
        return n - 1
    if fn == "median_filter":
        return n // 2
    if fn == "rank_filter":
        return kw["rank"] + (n if kw["rank"] < 0 else 0)
    p = kw["percentile"] + (100 if kw["percentile"] < 0 else 0)
    return n - 1 if p == 100 else int(float(n) * p / 100.0)


def brute(fn, img, size=None, footprint=None, mode="reflect", cval=0, origin=0, **kw):
    """the public function `fn` by the definition, one pixel at a time"""
    nd = img.ndim
    fp = None if footprint is None else np.asarray(footprint, bool)
    extent = fp.shape if fp is not None else ((size,) * nd if np.isscalar(size) else tuple(size))
    n = int(fp.sum()) if fp is not None else int(np.prod(extent))
    if fn in FILTERS:
        origin = (origin,) * nd if np.isscalar(origin) else tuple(origin)
        return brute_rank(img, rank_of(fn, n, kw), extent, fp, mode, cval, origin)
    flipped = None if fp is None else fp[(slice(None, None, -1),) * nd]
    shifted = tuple(-1 if e % 2 == 0 else 0 for e in extent)
    lo = lambda a: brute_rank(a, 0, extent, fp, mode, cval, (0,) * nd)
    hi = lambda a: brute_rank(a, n - 1, extent, flipped, mode, cval, shifted)
    body = hi(lo(img)) if fn in ("grey_opening", "white_tophat") else lo(hi(img))
    if fn in ("grey_opening", "grey_closing"):
        return body
    if img.dtype == np.bool_:
        return np.logical_xor(img, body)
    with np.errstate(invalid="ignore", over="ignore"):
        return img - body if fn == "white_tophat" else body - img


# ----------------------------------------------------------------------------- data

def special_float_images():
    """float32 images with the values a comparison can trip on: +-inf, denormals, the dtype's extremes, both zeros in one window"""
    a = noise((21, 70), np.float32, 5)
    a[3, 5], a[3, 6], a[20, 60], a[10, 10], a[0, 0] = np.inf, np.inf, -np.inf, -np.inf, np.inf
    b = np.random.RandomState(6).randint(0, 1 << 10, (20, 65)).astype(np.uint32).view(np.float32).copy()       # denormals, and zeros
    b[::2] *= -1
    c = noise((9, 66), np.float32, 7) * np.float32(1e36)
    c[2, 3], c[4, 60] = np.finfo(np.float32).max, np.finfo(np.float32).min
    z = np.zeros((12, 66), np.float32)
    z[::2, ::3] = -0.0
    z[5, 7], z[9, 64] = 1.0, -1.0
    return {"inf": a, "denormals": b, "huge": c, "zeros": z}


def nan_images():
    """float32 with scattered NaNs, one in a corner and one on an edge so that the reflected border holds a NaN, and a NaN next to inf"""
    a = noise((23, 70), np.float32, 8)
    a[0, 0] = a[22, 35] = a[11, 69] = a[7, 7] = a[7, 9] = a[15, 40] = np.nan
    a[15, 42] = np.inf
    b = noise((4, 9, 66), np.float32, 9)
    b[0, 0, 0] = b[3, 8, 65] = b[2, 4, 30] = np.nan
    return {"nan2d": a, "nan3d": b}


# ----------------------------------------------------------------------------- the cases: name -> (function, image, keywords)

def cases():
    C = {}

    def add(name, fn, img, **kw):
        assert name not in C, name
        C[name] = (fn, img, kw)

    k = 0
    # every dtype under every mode at shapes that cross the tiles unevenly: a box minimum with an even size, a box maximum, a median
    for dtype in DTYPES:
        d = np.dtype(dtype).name
        for mode in MODES:
            img = noise((67, 131), dtype, k)
            k += 1
            add("min-4x3-%s-%s" % (d, mode), "minimum_filter", img, size=(4, 3), mode=mode, cval=a_cval(dtype, k))
            add("max-5-%s-%s" % (d, mode), "maximum_filter", img, size=5, mode=mode, cval=a_cval(dtype, k))
            add("median-3-%s-%s" % (d, mode), "median_filter", img, size=3, mode=mode, cval=a_cval(dtype, k + 1))
        vol = noise((5, 70, 33), dtype, k)
        add("min-3x4x2-%s-3d" % d, "minimum_filter", vol, size=(3, 4, 2))
        add("max-1x1x5-%s-3d" % d, "maximum_filter", vol, size=(1, 1, 5), mode="mirror")
        add("median-1x3x3-%s-3d" % d, "median_filter", vol, size=(1, 3, 3), mode="mirror")
        add("median-ball-%s-3d" % d, "median_filter", vol, footprint=ball(1), mode="nearest")
        add("max-ball2-%s-3d" % d, "maximum_filter", vol[:, :20], footprint=ball(2), mode="constant", cval=a_cval(dtype))
        add("opening-2x3x2-%s-3d" % d, "grey_opening", vol, size=(2, 3, 2))
        add("black-ball-%s-3d" % d, "black_tophat", vol[:, :20], footprint=ball(1), mode="mirror")
    # the smallest images, and an image far smaller than its window: every index reflects more than once
    for shape in ((1, 1), (1, 40), (40, 1)):
        s = "x".join(map(str, shape))
        for j, mode in enumerate(MODES):
            dtype = DTYPES[1 + j % 3]
            img = noise(shape, dtype, k)
            k += 1
            add("tiny-%s-median-%s" % (s, mode), "median_filter", img, size=3, mode=mode, cval=a_cval(dtype))
            add("tiny-%s-min-%s" % (s, mode), "minimum_filter", img, size=(2, 5), mode=mode, cval=a_cval(dtype))
            add("tiny-%s-tophat-%s" % (s, mode), "white_tophat", img, size=(3, 4), mode=mode, cval=a_cval(dtype))
    small = noise((5, 6), np.uint16, k)
    smallf = noise((5, 6), np.float32, k + 1)
    for mode in MODES:
        add("wide-min-%s" % mode, "minimum_filter", small, size=(11, 13), mode=mode, cval=300)
        add("wide-max-%s" % mode, "maximum_filter", smallf, size=(11, 13), mode=mode, cval=-2.5)
        add("wide-median-%s" % mode, "median_filter", small, size=(11, 13), mode=mode, cval=300)
        add("wide-p30-%s" % mode, "percentile_filter", smallf, percentile=30, size=(11, 13), mode=mode, cval=40.0)
        add("wide-closing-%s" % mode, "grey_closing", small, size=(11, 13), mode=mode, cval=300)
        add("wide-disc-%s" % mode, "median_filter", small, footprint=disc(6), mode=mode, cval=300)
    # every legal origin of an even and an odd size, the extremes included
    img8, imgf = noise((20, 70), np.uint8, k + 2), noise((20, 70), np.float32, k + 3)
    origins = [(o, 0) for o in range(-2, 2)] + [(0, o) for o in (-2, -1, 1, 2)] + [(-2, -2), (1, 2), (-2, 2), (1, -2)]
    for j, o in enumerate(origins):
        mode = MODES[j % 4]
        add("origin-min-%d_%d" % o, "minimum_filter", img8, size=(4, 5), origin=o, mode=mode, cval=7)
        add("origin-median-%d_%d" % o, "median_filter", imgf, size=(4, 5), origin=o, mode=mode, cval=-2.5)
        add("origin-max-fp-%d_%d" % o, "maximum_filter", img8, footprint=footprints()["random4x5"], origin=o, mode=mode, cval=200)
    add("origin-scalar", "rank_filter", img8, rank=2, size=3, origin=-1)
    add("origin-3d", "minimum_filter", noise((4, 9, 66), np.uint16, k + 4), size=(2, 3, 4), origin=(-1, 1, -2), mode="mirror")
    # mode constant with cval at the dtype's ends
    ends = [(np.bool_, False), (np.bool_, True), (np.uint8, 0), (np.uint8, 255), (np.uint16, 0), (np.uint16, 65535), (np.float32, np.inf),
            (np.float32, -np.inf), (np.float32, float(np.finfo(np.float32).max)), (np.float32, float(np.finfo(np.float32).min))]
    for j, (dtype, cval) in enumerate(ends):
        img = noise((20, 70), dtype, k + 5 + j)
        name = "%s-%d" % (np.dtype(dtype).name, j)
        add("cval-min-" + name, "minimum_filter", img, size=(3, 4), mode="constant", cval=cval)
        add("cval-max-" + name, "maximum_filter", img, size=(3, 4), mode="constant", cval=cval)
        add("cval-median-" + name, "median_filter", img, footprint=footprints()["cross"], mode="constant", cval=cval)
        add("cval-white-" + name, "white_tophat", img, size=3, mode="constant", cval=cval)
        add("cval-black-" + name, "black_tophat", img, footprint=disc(1), mode="constant", cval=cval)
    # footprints
    k += 20
    for fname, fp in footprints().items():
        for dtype in (np.uint16, np.float32, np.bool_):
            img = noise((40, 70), dtype, k)
            k += 1
            d = np.dtype(dtype).name
            mode = MODES[k % 4]
            add("fp-%s-min-%s" % (fname, d), "minimum_filter", img, footprint=fp, mode=mode, cval=a_cval(dtype))
            add("fp-%s-max-%s" % (fname, d), "maximum_filter", img, footprint=fp, mode=mode, cval=a_cval(dtype))
            add("fp-%s-median-%s" % (fname, d), "median_filter", img, footprint=fp, mode=mode, cval=a_cval(dtype))
            add("fp-%s-rank-%s" % (fname, d), "rank_filter", img, rank=-1 if fp.sum() < 3 else 2, footprint=fp, mode=mode, cval=a_cval(dtype))
            add("fp-%s-opening-%s" % (fname, d), "grey_opening", img, footprint=fp, mode=mode, cval=a_cval(dtype))
            add("fp-%s-white-%s" % (fname, d), "white_tophat", img, footprint=fp, mode=mode, cval=a_cval(dtype))
    add("fp-all-true", "median_filter", img8, footprint=np.ones((3, 2), bool))
    add("fp-all-true-min", "minimum_filter", img8, footprint=np.ones((2, 3), np.uint8))
    # ranks and percentiles: n = 12
    img16 = noise((20, 70), np.uint16, k)
    for rank in (0, 11, 6, -1, -12, 3):
        add("rank-%d-uint16" % rank, "rank_filter", img16, rank=rank, size=(3, 4))
        add("rank-%d-float32" % rank, "rank_filter", imgf, rank=rank, size=(3, 4), mode="mirror")
    for p in (0, 30, 50, 100, -25, 99.9, -100):
        add("percentile-%g-uint16" % p, "percentile_filter", img16, percentile=p, size=(3, 4))
        add("percentile-%g-float32" % p, "percentile_filter", imgf, percentile=p, footprint=disc(2), mode="nearest")
    # data: integer images at their maxima, masks, special floats, NaNs
    for dtype in (np.uint8, np.uint16):
        img = np.full((20, 70), np.iinfo(dtype).max, dtype)
        img[::5, ::7] = 0
        img[3:6, 10:30] = np.iinfo(dtype).max - 1
        d = np.dtype(dtype).name
        add("maxima-median-" + d, "median_filter", img, size=3)
        add("maxima-max-" + d, "maximum_filter", img, size=(2, 3))
        add("maxima-white-" + d, "white_tophat", img, size=4)
        add("maxima-black-" + d, "black_tophat", img, size=(3, 5))
    mask = np.zeros((30, 70), bool)
    mask[5:20, 10:50] = True
    mask[8, 15] = mask[12:14, 30:33] = False
    mask[25, 60] = mask[0, 0] = True
    for fn in MORPHOLOGY + ("minimum_filter", "maximum_filter", "median_filter"):
        add("mask-%s" % fn, fn, mask, size=3)
        add("mask-%s-4x2" % fn, fn, mask, size=(4, 2), mode="constant", cval=True)
    for name, img in special_float_images().items():
        for fn in ("minimum_filter", "maximum_filter", "median_filter") + MORPHOLOGY:
            add("%s-%s" % (name, fn), fn, img, size=(3, 4))
        add("%s-disc-p30" % name, "percentile_filter", img, percentile=30, footprint=disc(2), mode="mirror")
    for name, img in nan_images().items():
        nd = img.ndim
        for j, fn in enumerate(("minimum_filter", "maximum_filter", "median_filter") + MORPHOLOGY):
            add("%s-%s" % (name, fn), fn, img, size=3 if nd == 2 else (2, 3, 3), mode=MODES[j % 4], cval=np.inf if j % 2 else 1.5)
        if nd == 2:
            add("%s-ell-median" % name, "median_filter", img, footprint=footprints()["ell"])
            add("%s-ell-white" % name, "white_tophat", img, footprint=footprints()["ell"], mode="mirror")
            add("%s-origin" % name, "rank_filter", img, rank=1, size=(2, 4), origin=(-1, 1), mode="nearest")
    return C


def has_nan(img):
    return img.dtype == np.float32 and bool(np.isnan(img).any())


def same(got, want):
    """== with equal NaN positions, same dtype and shape"""
    return isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=want.dtype.kind == "f")
