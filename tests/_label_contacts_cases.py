"""Cases of stardist_amd.utils.label_contacts and measure_labels(neighbors=), shared by tests/test_cpu_label_contacts.py,
tests/test_gpu_label_contacts.py and tests/golden/make_label_contacts_golden.py, and the brute-force statement of the definition the
tests compare with (plain loops over pixels and offsets).

    forward_offsets(nd, c)      the lexicographically positive offsets with at most c non-zero coordinates
    brute(a, c, background)     the contact table of the array a as three lists of Python ints, straight from the definition
    brute_neighbors(a, c)       {label: (neighbors, contact_objects, contact_background)} from the same loops
    SMALL                       small images (every dtype, degenerate shapes, wide ids): name -> array
    GOLDEN                      the names of SMALL whose edge sets tests/golden/label_contacts_reference.npz holds
    tile_shapes(nd), tiled(kind, shape)   the shapes around the tile extents of stardist_amd/csrc/label_edit.h and images on them
    windows_2d(), windows_3d()  all 3^9 3 x 3 windows and all 3^8 2 x 2 x 2 windows over {0, 1, 2}, each in a cell of its own
    balls()                     touching balls in a small volume
"""
import functools
import itertools
import os
import re
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constants():
    txt = open(os.path.join(ROOT, "stardist_amd", "csrc", "label_edit.h")).read()
    return {k: int(v) for k, v in re.findall(r"\b(LE_[A-Z_]+)\s*=\s*(\d+)", txt)}


K = header_constants()
TX, TY, TZ, VY = K["LE_TILE_X"], K["LE_TILE_Y"], K["LE_TILE_Z"], K["LE_VOL_TILE_Y"]


def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


# ----------------------------------------------------------------------------- the definition, by brute force

def forward_offsets(nd, c):
    return [o for o in itertools.product((-1, 0, 1), repeat=nd) if o > (0,) * nd and sum(1 for v in o if v) <= c]


def _contact_counts(a):
    """{number of non-zero coordinates of the offset: Counter of (min, max) over the contacts along such offsets}: one pass over the
    pixels and all forward offsets of full connectivity"""
    a = np.asarray(a)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    nd, shape = a.ndim, a.shape
    values = a.reshape(-1).tolist()
    strides = [int(np.prod(shape[d + 1:], dtype=np.int64)) for d in range(nd)]
    offs = [(o, sum(1 for v in o if v), sum(d * s for d, s in zip(o, strides))) for o in forward_offsets(nd, nd)]
    counts = {m: Counter() for m in range(1, nd + 1)}
    for p in itertools.product(*[range(n) for n in shape]):
        at = sum(v * s for v, s in zip(p, strides))
        here = values[at]
        for o, moved, step in offs:
            if all(0 <= v + d < n for v, d, n in zip(p, o, shape)):
                there = values[at + step]
                if here != there:
                    counts[moved][(min(here, there), max(here, there))] += 1
    return counts


_cache = {}


def _counts_of(a):
    key = (a.shape, str(a.dtype), a.tobytes())
    if key not in _cache:
        _cache[key] = _contact_counts(a)
    return _cache[key]


def brute(a, c, background):
    """(label_a, label_b, contacts): lists of Python ints, ascending by (label_a, label_b)"""
    total = Counter()
    for moved, cnt in _counts_of(np.ascontiguousarray(a)).items():
        if moved <= c:
            total.update(cnt)
    rows = sorted((lo, hi, n) for (lo, hi), n in total.items() if background or lo != 0)
    return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]


def brute_neighbors(a, c):
    """{label > 0 present: (neighbors, contact_objects, contact_background)}"""
    out = {int(l): [0, 0, 0] for l in np.unique(a) if l > 0}
    for lo, hi, n in zip(*brute(a, c, True)):
        if lo == 0:
            out[hi][2] += n
        else:
            for l in (lo, hi):
                out[l][0] += 1
                out[l][1] += n
    return {l: tuple(v) for l, v in out.items()}


def as_lists(table):
    """the three columns of a label_contacts result as lists of Python ints"""
    return tuple([int(v) for v in np.asarray(table[k]).tolist()] for k in ("label_a", "label_b", "contacts"))


# ----------------------------------------------------------------------------- small images

def _blobs(shape, n, seed, dtype=np.int32):
    """n seeds grown to a Voronoi partition, cut off 4 pixels from the seeds"""
    rng = np.random.RandomState(seed)
    pts = np.stack([rng.randint(0, s, n) for s in shape], axis=1)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).reshape(-1, 1, len(shape))
    d2 = ((grid - pts[None]) ** 2).sum(axis=-1)
    lab = (np.argmin(d2, axis=1) + 1).reshape(shape)
    lab[d2.min(axis=1).reshape(shape) > 16] = 0                            # farther than 4 pixels from every seed: background
    return lab.astype(dtype)


def _small():
    rng = np.random.RandomState(7)
    c = {}
    c["two_halves"] = np.repeat(np.array([[1, 2]], np.int32), 4, axis=0).repeat(3, axis=1)
    c["diagonal_only"] = np.array([[1, 0], [0, 2]], np.int32)
    c["anti_diagonal_only"] = np.array([[0, 1], [2, 0]], np.int32)
    c["checker"] = (np.indices((5, 6)).sum(axis=0) % 2 + 1).astype(np.uint8)
    c["noise_2d"] = rng.randint(0, 4, (9, 11)).astype(np.int16)
    c["noise_3d"] = rng.randint(0, 4, (4, 5, 6)).astype(np.int64)
    c["blobs_2d"] = _blobs((24, 31), 9, 1)
    c["blobs_3d"] = _blobs((6, 9, 11), 6, 2, np.uint16)
    c["blobs_uint8"] = _blobs((17, 13), 5, 3, np.uint8)
    c["one_label"] = np.full((5, 7), 3, np.int32)
    c["all_background"] = np.zeros((4, 6), np.int32)
    c["one_pixel"] = np.array([[5]], np.int32)
    c["one_row"] = np.array([[1, 1, 0, 2, 2, 3, 0, 0, 3]], np.int32)
    c["one_column"] = np.array([[1], [2], [2], [0], [4]], np.int32)
    c["one_plane"] = rng.randint(0, 3, (1, 5, 6)).astype(np.int32)
    c["thin_volume"] = rng.randint(0, 3, (5, 1, 4)).astype(np.int32)
    c["bool_mask"] = rng.rand(6, 7) > 0.5
    c["ring"] = np.pad(np.pad(np.full((2, 2), 2, np.int32), 2, constant_values=1), 1)
    c["wide_ids"] = np.array([[1, 2 ** 30, 2 ** 31 - 1], [2 ** 31 - 1, 1, 0]], np.int64)
    c["huge_ids"] = np.array([[3, 10 ** 12, 0], [10 ** 15, 3, 10 ** 12]], np.int64)
    c["far_corner_diagonals"] = np.zeros((6, 7), np.int32)
    c["far_corner_diagonals"][-1, -2], c["far_corner_diagonals"][-2, -1], c["far_corner_diagonals"][-1, 0], c["far_corner_diagonals"][0, -1] = 1, 2, 3, 4
    return {k: frozen(v) for k, v in c.items()}


SMALL = _small()
# scikit-image's RAG takes integer images; its graph has a node per value, 0 too
GOLDEN = ("two_halves", "diagonal_only", "anti_diagonal_only", "checker", "noise_2d", "noise_3d", "blobs_2d", "blobs_3d", "blobs_uint8",
          "one_row", "one_plane", "ring", "far_corner_diagonals")


# ----------------------------------------------------------------------------- images around the tile extents

def tile_shapes(nd):
    """every combination of tile extent - 1, the extent and + 1 per axis"""
    per_axis = [(TY, TX)] if nd == 2 else [(TZ, VY, TX)]
    return [tuple(s) for s in itertools.product(*[(n - 1, n, n + 1) for n in per_axis[0]])]


KINDS = ("blocks", "noise", "sparse")


@functools.lru_cache(maxsize=None)
def tiled(kind, shape):
    """blocks: boxes of 2 x 3 x 5 pixels with ids that differ between neighbours, so contacts straddle every tile face, edge and corner;
    noise: every pixel one of 0 .. 3; sparse: background but for single pixels and pairs, the image's last pixels among them"""
    rng = np.random.RandomState(len(shape) * 1000 + sum(shape))
    idx = np.indices(shape)
    z, (y, x) = (idx[0] if len(shape) == 3 else 0), idx[-2:]
    if kind == "blocks":
        a = 1 + (x // 5 + 7 * (y // 3) + 31 * (z // 2)) % 11
        a = np.where((x // 5 + y // 3 + z // 2) % 4 == 0, 0, a)
    elif kind == "noise":
        a = rng.randint(0, 4, shape)
    else:
        a = np.where(rng.rand(*shape) < 0.03, rng.randint(1, 9, shape), 0)
        a[tuple(-1 for _ in shape)] = 9
        a[tuple(-2 for _ in shape[:-1]) + (-2,)] = 8 if all(s > 1 for s in shape) else a[tuple(-1 for _ in shape)]
        a[tuple(-1 for _ in shape[:-1]) + (0,)] = 7
    return frozen(a.astype(np.int32))


# ----------------------------------------------------------------------------- all small windows

@functools.lru_cache(maxsize=None)
def windows_2d():
    """all 3^9 windows of 3 x 3 over {0, 1, 2}, window w in the 3 x 3 cell (w // 81, w % 81) of a (243 * 3, 81 * 3) image: the cells
    touch, which the definition does not mind"""
    w = np.arange(3 ** 9)
    digits = np.stack([(w // 3 ** k) % 3 for k in range(9)], axis=1).reshape(243, 81, 3, 3)
    return frozen(digits.transpose(0, 2, 1, 3).reshape(243 * 3, 81 * 3).astype(np.int32))


@functools.lru_cache(maxsize=None)
def windows_3d():
    """all 3^8 windows of 2 x 2 x 2 over {0, 1, 2}, in the cells of a (2, 81 * 2, 81 * 2) volume"""
    w = np.arange(3 ** 8)
    digits = np.stack([(w // 3 ** k) % 3 for k in range(8)], axis=1).reshape(81, 81, 2, 2, 2)
    return frozen(digits.transpose(2, 0, 3, 1, 4).reshape(2, 81 * 2, 81 * 2).astype(np.int32))


@functools.lru_cache(maxsize=None)
def balls():
    """five balls in a (12, 20, 70) volume, neighbours touching: the volume spans three tiles along z and y and two along x"""
    z, y, x = np.indices((12, 20, 70))
    a = np.zeros((12, 20, 70), np.int32)
    for k, (cz, cy, cx, r) in enumerate([(5, 9, 8, 6.5), (6, 10, 21, 6.5), (5, 9, 34, 6.5), (6, 10, 47, 6.5), (5, 9, 60, 6.5)], 1):
        d2 = (z - cz) ** 2 + (y - cy) ** 2 + (x - cx) ** 2
        a[(d2 <= r * r) & (a == 0)] = k
    return frozen(a)
