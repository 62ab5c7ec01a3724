"""Cases for stardist_amd.utils.measure_labels(hull=True), shared by tests/test_cpu_measure_hull.py (host route, brute force,
scikit-image golden, host harness of csrc/measure_hull.h), tests/test_gpu_measure_hull.py (the kernels) and
tests/golden/make_hull_golden.py: deterministic and small.  `case(name)` gives the label image and `host(name)` the host route's table
with hull=True, computed once per case and kept read-only.  `brute_force_mask` restates the definition of DESIGN.md section 3u the
long way round: all diamond points of all pixels, a monotone chain over the sorted points, half-plane tests over the whole box, all
pairs for F2 (numpy int64 on coordinates below 2^14, so every product is exact)."""
import numpy as np

MH_LDS_ROWS = 64                                  # restated from csrc/measure_hull.h (test_cpu_measure_hull.py checks the header)
TWO_PIXEL_OFFSETS = ((1, 2), (2, 1), (1, 3), (2, 3), (1, 1), (3, 5), (0, 4), (5, 0), (2, 4), (4, 6))
HULL_KEYS = ["convex_area", "solidity", "feret_diameter_max"]

_cache, _host = {}, {}


def _grid(masks, pitch, ids=None):
    """the masks as objects 1 .. n (or `ids`) of one image, each at the start of a cell of pitch x pitch pixels, the cells row by row
    in a square grid; nothing is left around the grid, so the first row and column of cells lie on the image border"""
    side = int(np.ceil(np.sqrt(len(masks))))
    a = np.zeros((side * pitch, side * pitch), np.int32)
    for k, m in enumerate(masks):
        y, x = k // side * pitch, k % side * pitch
        a[y:y + m.shape[0], x:x + m.shape[1]][m] = (k + 1) if ids is None else ids[k]
    return a


def patterns4x4():
    """the 65535 non-empty 4 x 4 patterns on a 5-pixel pitch, label = the pattern's number: 1280 x 1280"""
    ids = np.arange(1, 65536, dtype=np.int64)
    a = np.zeros((1280, 1280), np.int32)
    cy, cx = (ids - 1) // 256 * 5, (ids - 1) % 256 * 5
    for k in range(16):
        on = (ids >> k) & 1 == 1
        a[cy[on] + k // 4, cx[on] + k % 4] = ids[on]
    return a


def patterns4x4_shifted():
    """the same objects three rows down and two columns to the right in a 1283 x 1283 image: the odd row length moves the objects
    through every position of a wave's 64 and a workgroup's 256 consecutive pixels"""
    a = np.zeros((1283, 1283), np.int32)
    a[3:, 2:1282] = case("patterns4x4")
    return a


def random_mask_list():
    """random masks of 1 .. 13 x 1 .. 13 pixels at densities 0.15, 0.4 and 0.8 (non-empty; first and last row and column need not be
    occupied)"""
    rng = np.random.default_rng(7301)
    out = []
    for density in (0.15, 0.4, 0.8):
        for h in range(1, 14):
            for w in range(1, 14):
                m = rng.random((h, w)) < density
                if not m.any():
                    m[rng.integers(h), rng.integers(w)] = True
                out.append(m)
    return out


def ellipse_list():
    """40 rotated ellipses in boxes of up to 40 x 40"""
    rng = np.random.default_rng(7302)
    yy, xx = np.mgrid[:40, :40].astype(np.float64)
    out = []
    for _ in range(40):
        ry, rx, th = rng.uniform(1, 19.5), rng.uniform(1, 19.5), rng.uniform(0, np.pi)
        u = (yy - 19.5) * np.cos(th) + (xx - 19.5) * np.sin(th)
        v = -(yy - 19.5) * np.sin(th) + (xx - 19.5) * np.cos(th)
        m = (u / ry) ** 2 + (v / rx) ** 2 <= 1.0
        ys, xs = np.nonzero(m)
        out.append(m[ys.min():ys.max() + 1, xs.min():xs.max() + 1])
    return out


def two_pixel_list():
    """two pixels at each of TWO_PIXEL_OFFSETS, and the mirror image of each"""
    out = []
    for dy, dx in TWO_PIXEL_OFFSETS:
        m = np.zeros((dy + 1, dx + 1), bool)
        m[0, 0] = m[dy, dx] = True
        out += [m, m[:, ::-1].copy()]
    return out


def line_list():
    """single pixels, 1 x N and N x 1 lines (N = 2 .. 9, 64, 65), some with gaps"""
    out = [np.ones((1, 1), bool)]
    for n in (2, 3, 4, 5, 6, 7, 8, 9, 64, 65):
        row = np.ones((1, n), bool)
        out += [row, row.T.copy()]
        if n >= 4:
            gap = row.copy()
            gap[0, 1:n - 1:2] = False
            out += [gap, gap.T.copy()]
    return out


def split():
    """label 5 in two distant parts (a block top left, an L bottom right) with object 2 between them, inside 5's hull; and label 9 in
    two single pixels 70 rows apart, more rows than the LDS tier, with empty rows between"""
    a = np.zeros((90, 60), np.int32)
    a[2:6, 3:8] = 5
    a[70:80, 40:43] = 5
    a[78:80, 30:43] = 5
    a[30:45, 20:30] = 2
    a[5, 55] = 9
    a[75, 50] = 9
    return a


def border():
    """objects on the four borders and in the four corners of a 21 x 67 image, and one inside"""
    a = np.zeros((21, 67), np.int32)
    a[0, 0] = 1
    a[0, 66] = 2
    a[20, 0] = 3
    a[20, 66] = 4
    a[0:3, 10:30] = 5
    a[1, 12:20] = 0
    a[18:21, 30:60:2] = 6
    a[5:15, 0] = 7
    a[4:16:3, 66] = 8
    a[8:12, 20:40] = 11
    a[9:11, 22:30] = 12                                                     # inside 11's box, not 11
    return a


def gaps():
    """the two-pixel objects with ids 7, 14, 21, .. and a negative label beside them"""
    masks = two_pixel_list()
    a = _grid(masks, 8, ids=[7 * (k + 1) for k in range(len(masks))])
    a[-1, -1] = -4
    return a


def huge_ids():
    """the two-pixel objects with ids around 2^40 (int64): the routes compact them"""
    masks = two_pixel_list()
    return _grid(masks, 8).astype(np.int64) * 3 + np.where(_grid(masks, 8) > 0, 2 ** 40, 0)


def diagonal(n=5003):
    """a one-pixel diagonal of n rows in an n x (n + 2) image, label 3, with a single pixel of label 1 in a corner"""
    a = np.zeros((n, n + 2), np.int32)
    a[np.arange(n), np.arange(n) + 1] = 3
    a[n - 1, 0] = 1
    return a


_LABELS = {
    "patterns4x4": patterns4x4, "patterns4x4_shifted": patterns4x4_shifted,
    "random_masks": lambda: _grid(random_mask_list(), 14),
    "ellipses": lambda: _grid(ellipse_list(), 41),
    "two_pixels": lambda: _grid(two_pixel_list(), 8),
    "lines": lambda: _grid(line_list(), 66),
    "split": split, "border": border, "gaps": gaps, "huge_ids": huge_ids,
    "corners": lambda: np.array([[1, 0, 0, 0, 2], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [3, 0, 0, 0, 4]], np.int32),
    "empty": lambda: np.zeros((7, 9), np.int32) - 1,
    "diagonal": diagonal, "diagonal_t": lambda: diagonal().T.copy(),
    "whole": lambda: np.full((2048, 2048), 6, np.int32),
}
NAMES = tuple(_LABELS)
SMALL = ("random_masks", "ellipses", "two_pixels", "lines", "split", "border", "gaps", "huge_ids", "corners", "empty")
GOLDEN = ("random_masks", "ellipses", "two_pixels", "lines", "split", "border", "gaps")
MASK_LISTS = {"random_masks": random_mask_list, "ellipses": ellipse_list, "two_pixels": two_pixel_list, "lines": line_list}


def case(name):
    got = _cache.get(name)
    if got is None:
        got = _cache[name] = _LABELS[name]()
        got.setflags(write=False)
    return got


def host(name, **more):
    """the host route's table with hull=True (read-only, computed once per case and keyword set)"""
    key = (name, tuple(sorted(more.items())))
    got = _host.get(key)
    if got is None:
        from stardist_amd.utils import measure_labels
        got = _host[key] = measure_labels(case(name), hull=True, **more)
        for col in got.values():
            col.setflags(write=False)
    return got


def _diamonds(pixels):
    """the distinct diamond points (doubled coordinates, Python integers) of the pixels [(r, c)], sorted by y, then x"""
    return sorted({q for r, c in pixels for q in ((2 * r - 1, 2 * c), (2 * r + 1, 2 * c), (2 * r, 2 * c - 1), (2 * r, 2 * c + 1))})


def _hull(points):
    """Andrew's monotone chain over the sorted distinct points: the hull's vertices, once around"""
    def half(seq):
        st = []
        for p in seq:
            while len(st) >= 2 and (st[-1][0] - st[-2][0]) * (p[1] - st[-2][1]) - (st[-1][1] - st[-2][1]) * (p[0] - st[-2][0]) <= 0:
                st.pop()
            st.append(p)
        return st[:-1]
    return half(points) + half(points[::-1])


def brute_force_mask(mask):
    """(convex_area, F2) of the object `mask` (a boolean array that is the object's box): the hull of all diamond points, cross >= 0
    for every hull edge at every pixel centre of the box, all pairs of diamond points of the convex image"""
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    hull = np.array(_hull(_diamonds(zip(*(v.tolist() for v in np.nonzero(mask))))), np.int64)
    cy, cx = 2 * (np.arange(h * w, dtype=np.int64) // w), 2 * (np.arange(h * w, dtype=np.int64) % w)
    a, b = hull[None], np.roll(hull, -1, axis=0)[None]
    cross = (b[..., 0] - a[..., 0]) * (cx[:, None] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (cy[:, None] - a[..., 0])
    convex = (cross >= 0).all(axis=1)
    d = np.array(_diamonds(zip((cy[convex] // 2).tolist(), (cx[convex] // 2).tolist())), np.int64)
    f2 = 0
    for at in range(0, len(d), 512):
        part = d[at:at + 512]
        f2 = max(f2, int(((part[:, None, 0] - d[None, :, 0]) ** 2 + (part[:, None, 1] - d[None, :, 1]) ** 2).max()))
    return int(convex.sum()), f2


def brute_force(lbl):
    """{label: (convex_area, F2)} of every positive label of the 2D image, each over its bounding box"""
    lbl = np.asarray(lbl)
    out = {}
    for l in np.unique(lbl[lbl > 0]).tolist():
        ys, xs = np.nonzero(lbl == l)
        out[l] = brute_force_mask(lbl[ys.min():ys.max() + 1, xs.min():xs.max() + 1] == l)
    return out


def feret(f2):
    return np.sqrt(np.asarray(f2, np.int64).astype(np.float64) / 4.0)
