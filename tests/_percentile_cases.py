"""Cases for stardist_amd.utils.measure_labels(percentiles=), shared by tests/test_cpu_measure_percentiles.py (host route, a brute-force
statement of the definition, np.percentile, the host harness of csrc/measure_rank.h) and tests/test_gpu_measure_percentiles.py (the
kernels): deterministic by seed and as small as the tiers allow.  `case(name)` gives (lbl, img, qs), read-only; `host(name)` the host
route's table, computed once per case and kept read-only."""
import numpy as np

MR_SORT_KEYS = 1024                  # restated from csrc/measure_rank.h (test_cpu_measure_percentiles.py checks the header against it)
MR_RANK_KEYS = 64                    # likewise: up to this many members the sort tier counts instead of running its network
MR_CHUNK_SLOTS = 128                 # likewise: (object, channel) slots of the chunk workspace
MR_MAX_Q = 8                         # likewise
MS_CHUNK_PIXELS = 65536              # restated from csrc/measure.h: a box beyond it is cut into chunks

Q5 = (0, 100, 50, 25, 99.8)
Q8 = (0, 100.0, 50, 25, 99.8, 99.9999, np.float64(50), np.int64(12))      # a duplicate (50), numpy scalars, a q just below 100
Q1 = (50,)

_cache, _host = {}, {}


def sizes():
    """60 x 700, ids with gaps: objects of 1, 2, 3, 2, 2, 63, 64, 65 and 257 pixels, a solid box of exactly MR_SORT_KEYS pixels (the sort
    tier's capacity), a solid box of one pixel more (5 rows: the block tier), and a comb with its complement (interlocked, one box).
    (n - 1) q / 100 is whole for q = 25 and n = 65, 257 and for q = 50 and n = 3, 63, 65, 257."""
    assert MR_SORT_KEYS % 32 == 0 and (MR_SORT_KEYS + 1) % 5 == 0 and MR_RANK_KEYS == 64    # the objects of 63, 64 and 65 pixels
    a = np.zeros((60, 700), np.int32)
    a[0, 0] = 3
    a[0, 3:5] = 7
    a[0, 7:10] = 8
    a[0, 12:14] = 9
    a[0, 16:18] = 10
    a[2:11, 0:7] = 20
    a[2:10, 10:18] = 21
    a[2:7, 20:33] = 22
    a[12, 0:257] = 40
    a[14:46, 0:MR_SORT_KEYS // 32] = 41
    a[48:53, 0:(MR_SORT_KEYS + 1) // 5] = 45
    _interlock(a, slice(14, 30), slice(100, 140), 50, 51)
    return a


def _interlock(a, rows, cols, one, two):
    """two objects with the same box: `one` takes the even columns, `two` the odd ones, and each a corner pixel of the other's"""
    a[rows, cols.start:cols.stop:2] = one
    a[rows, cols.start + 1:cols.stop:2] = two
    assert (cols.stop - cols.start) % 2 == 0
    a[rows.start, cols.stop - 1] = one
    a[rows.stop - 1, cols.start] = two


def chunks_2d():
    """530 x 560, sized from the chunk constant: a box of exactly one chunk (a frame with a checkerboard inside), a box one row beyond it
    (a comb), a thin diagonal in a box of several chunks, a solid box of several chunks, and a comb with its complement in a box of the
    block tier; small objects inside the large boxes"""
    side = int(round(MS_CHUNK_PIXELS ** 0.5))
    assert side * side == MS_CHUNK_PIXELS and side == 256
    a = np.zeros((530, 560), np.int32)
    a[0:side:2, 0:side:2] = 2
    a[0, 0:side] = a[side - 1, 0:side] = 2
    a[0:side, 0] = a[0:side, side - 1] = 2                                  # box (0:256, 0:256): the one-chunk limit
    a[258:258 + side + 1, 0:side:3] = 3
    a[258, 0:side] = 3                                                      # box (258:515, 0:256): one row beyond
    d = np.arange(270)
    a[d, 280 + d] = 5                                                       # box 270 x 270, 270 pixels
    a[270:530, 290:560] = 6                                                 # solid, 260 x 270
    _interlock(a, slice(516, 530), slice(0, side), 8, 9)                    # two boxes (516:530, 0:256)
    a[100:110, 400:420] = 11                                                # inside the diagonal's box
    a[300:303, 300:304] = 12                                                # inside the solid box
    return a


def volume():
    """5 x 120 x 125: a thin diagonal through a box of several chunks (5 x 120 x 120), small boxes and one box of the block tier inside
    it, an object in a single plane"""
    assert 5 * 120 * 120 > MS_CHUNK_PIXELS
    a = np.zeros((5, 120, 125), np.int32)
    i = np.arange(120)
    a[i * 5 // 120, i, i] = 4
    a[0:3, 2:8, 60:70] = 6
    a[1:5, 10:30, 70:100] = 9                                               # 4 x 20 x 30 = 2400 > MR_SORT_KEYS
    a[2, 50:60, 100:125] = 14
    a[4, 119, 124] = 15
    a[0:5, 100:103, 3:6] = 21
    return a


def diagonals():
    """257 x (257 + n): n = MR_CHUNK_SLOTS + 2 diagonals, one pixel apart, each in a box of 257 x 257 pixels (several chunks): more
    multi-chunk objects than the chunk workspace has slots"""
    n = MR_CHUNK_SLOTS + 2
    assert 257 * 257 > MS_CHUNK_PIXELS
    a = np.zeros((257, 257 + n), np.int32)
    i = np.arange(257)
    for k in range(n):
        a[i, i + k] = k + 1
    return a


def _floats(rng, shape):
    """float32 of every magnitude, subnormals included, both signs"""
    m = np.ldexp(rng.uniform(0.5, 1.0, shape), rng.integers(-149, 128, shape))
    return (m * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def _image(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "u8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "u8_ramp":                                                   # many ties
        x = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
        return ((x // 3) % 7 * 30).astype(np.uint8)
    if kind == "u16":
        return rng.integers(0, 65536, shape, dtype=np.uint16)
    if kind == "f32":
        return _floats(rng, shape)
    raise KeyError(kind)


def _paint(img, lbl, label, values, channel=None):
    """the first len(values) pixels of the label (raster order) get the values"""
    where = np.nonzero(lbl == label)
    at = tuple(w[:len(values)] for w in where) + (() if channel is None else (channel,))
    img[at] = values


def huge_ids():
    """the labels of sizes() as int64 with ids up to 2^40, ascending order kept: (lbl, old ids, new ids)"""
    lbl = sizes().astype(np.int64)
    present = np.unique(lbl[lbl > 0])
    new = 1000 + 977 * np.arange(len(present), dtype=np.int64)
    new[-3:] = [2 ** 31 - 1, 2 ** 31 + 5, 2 ** 40]
    rename = np.zeros(int(present.max()) + 1, np.int64)
    rename[present] = new
    return rename[lbl], present, new


def _build(name):
    if name == "sizes_u16":
        lbl = sizes()
        img = _image("u16", lbl.shape, 5101)
        _paint(img, lbl, 41, [0, 65535])                                    # both ends of the type in one object
        _paint(img, lbl, 45, [65535, 0])
        return lbl, img, Q8
    if name == "sizes_u8_ramp_rgb":
        lbl = sizes()
        return lbl, _image("u8_ramp", lbl.shape + (3,), 0), Q5
    if name == "sizes_f32":
        lbl = sizes()
        img = _image("f32", lbl.shape, 5102)
        _paint(img, lbl, 7, [-1.0, 2.0])                                    # the two order statistics straddle 0
        _paint(img, lbl, 9, [1.0, np.inf])
        _paint(img, lbl, 10, [np.inf, np.inf])
        img[lbl == 21] = 3.5                                                # all equal
        _paint(img, lbl, 22, [np.inf, -np.inf])
        _paint(img, lbl, 40, [np.nan])
        _paint(img, lbl, 50, [0.0, -0.0, 0.0])
        return lbl, img, Q8
    if name == "sizes_f32_q1":
        lbl = sizes()
        return lbl, _image("f32", lbl.shape, 5103), Q1
    if name == "huge_ids_u16":
        return huge_ids()[0], _build("sizes_u16")[1], Q5
    if name in ("chunks_u16", "chunks_f32_c1", "chunks_u8_rgb"):
        lbl = chunks_2d()
        rng = np.random.default_rng(5110)
        if name == "chunks_u16":
            img = _image("u16", lbl.shape, 5111)
            img[lbl == 2] = 777                                             # all equal: every digit in one bin
            img[lbl == 3] = 0x1200 + rng.integers(0, 256, int((lbl == 3).sum()))          # differ only in the lowest digit
            img[lbl == 5] = 0x34 + 256 * rng.integers(0, 256, int((lbl == 5).sum()))      # differ only in the highest digit
            _paint(img, lbl, 6, [0, 65535, 65535, 0])
            return lbl, img, Q5
        if name == "chunks_f32_c1":
            img = _image("f32", lbl.shape + (1,), 5112)
            bits = img.view(np.uint32)
            n3, n5, n8 = (int((lbl == l).sum()) for l in (3, 5, 8))
            bits[lbl == 3, 0] = 0x42280000 + rng.integers(0, 256, n3).astype(np.uint32)                   # lowest digit only
            bits[lbl == 5, 0] = 0x00345678 + (rng.integers(0, 256, n5).astype(np.uint32) << 24)            # highest digit only (bit 23 clear: finite)
            bits[lbl == 8, 0] = 0x3f800000 + (rng.integers(0, 256, n8).astype(np.uint32) << 8)             # a middle digit only
            img[lbl == 2] = -7.25
            _paint(img, lbl, 6, [np.inf, np.inf], 0)
            _paint(img, lbl, 9, [np.nan], 0)
            return lbl, img, Q8
        return lbl, _image("u8", lbl.shape + (3,), 5113), (25, 50, 75)
    if name == "volume_u16":
        lbl = volume()
        return lbl, _image("u16", lbl.shape, 5120), Q5
    if name == "volume_f32_rgb":
        lbl = volume()
        img = _image("f32", lbl.shape + (3,), 5121)
        _paint(img, lbl, 4, [np.nan], 1)                                    # one object of several, one channel of three
        _paint(img, lbl, 6, [np.nan], 2)
        _paint(img, lbl, 9, [np.inf, np.inf], 0)
        return lbl, img, Q5
    if name == "diagonals_u8":
        lbl = diagonals()
        return lbl, _image("u8", lbl.shape, 5130), (50, 99.8)
    if name == "diagonals_u16_c2":
        lbl = diagonals()
        return lbl, _image("u16", lbl.shape + (2,), 5131), Q1
    if name == "empty_f32_c2":
        return np.zeros((4, 11, 13), np.int32) - 1, _image("f32", (4, 11, 13, 2), 5140), Q1
    if name == "empty_u8":
        return np.zeros((7, 9), np.int32), _image("u8", (7, 9), 5141), Q5
    raise KeyError(name)


NAMES = ("sizes_u16", "sizes_u8_ramp_rgb", "sizes_f32", "sizes_f32_q1", "huge_ids_u16", "chunks_u16", "chunks_f32_c1", "chunks_u8_rgb",
         "volume_u16", "volume_f32_rgb", "diagonals_u8", "diagonals_u16_c2", "empty_f32_c2", "empty_u8")
EMPTY = ("empty_f32_c2", "empty_u8")


def case(name):
    """(lbl, img, qs), the arrays read-only"""
    got = _cache.get(name)
    if got is None:
        lbl, img, qs = _build(name)
        for a in (lbl, img):
            a.setflags(write=False)
        got = _cache[name] = (lbl, img, qs)
    return got


def host(name):
    """the host route's table for the case (read-only, computed once)"""
    got = _host.get(name)
    if got is None:
        from stardist_amd.utils import measure_labels
        lbl, img, qs = case(name)
        got = measure_labels(lbl, img, percentiles=qs)
        for v in got.values():
            v.setflags(write=False)
        _host[name] = got
    return got


def q_names(qs):
    """the distinct column stems of the percentiles, in order"""
    out = []
    for q in qs:
        stem = "p%g_intensity" % float(q)
        if stem not in out:
            out.append(stem)
    return out


def percentile_keys(name):
    """the percentile columns of the case's table, in order"""
    lbl, img, qs = case(name)
    chan = img.ndim > lbl.ndim
    return [("%s-%d" % (stem, c)) if chan else stem for stem in q_names(qs) for c in range(img.shape[-1] if chan else 1)]


def percentile_block(table, name):
    """(n, C, number of distinct q) array of the percentile columns of a table of the case"""
    lbl, img, qs = case(name)
    chan = img.ndim > lbl.ndim
    C = img.shape[-1] if chan else 1
    return np.stack([np.stack([np.asarray(table[("%s-%d" % (stem, c)) if chan else stem]) for stem in q_names(qs)], axis=-1)
                     for c in range(C)], axis=1)


def same(a, b):
    """equal values (==) and equal NaN positions; a zero's sign is not compared"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and (a[~na] == b[~nb]).all())
