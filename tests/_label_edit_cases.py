"""Cases of stardist_amd.utils.find_boundaries, clear_border, remove_small_objects and select_labels, shared by
tests/test_cpu_label_edit.py, tests/test_gpu_label_edit.py and tests/golden/make_label_edit_golden.py, and the brute-force statements of
find_boundaries' and clear_border's definitions that the tests compare with (loops over pixels and offsets, no scipy morphology).

    FB                       small images of find_boundaries (every dtype, negative ids, degenerate shapes); fb_params(a) their arguments
    windows_image()          all 3^9 3 x 3 windows over {0, 1, 2}, each in a 5 x 5 cell of its own
    CB, RS, SL               cases of clear_border, remove_small_objects, select_labels: name -> (arguments, keyword arguments)
    tile_shapes(nd), tiled(kind, shape)   the shapes around the tile extents of stardist_amd/csrc/label_edit.h and images on them
"""
import functools
import itertools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("thick", "inner", "outer")


def header_constants():
    txt = open(os.path.join(ROOT, "stardist_amd", "csrc", "label_edit.h")).read()
    return {k: int(v) for k, v in re.findall(r"\b(LE_[A-Z_]+)\s*=\s*(\d+)", txt)}


K = header_constants()
TX, TY, TZ, VY = K["LE_TILE_X"], K["LE_TILE_Y"], K["LE_TILE_Z"], K["LE_VOL_TILE_Y"]


def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


# ----------------------------------------------------------------------------- the definitions, by brute force

def offsets(nd, c):
    return [o for o in itertools.product((-1, 0, 1), repeat=nd) if any(o) and sum(1 for v in o if v) <= c]


def brute_pixels(a, connectivity, mode, background):
    """find_boundaries as the definition reads, one pixel at a time (small images only)"""
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    top = int(np.iinfo(a.dtype).max)
    nd, shape = a.ndim, a.shape
    out = np.zeros(shape, bool)
    near, window = offsets(nd, connectivity), offsets(nd, nd) + [(0,) * nd]
    inside = lambda q: all(0 <= v < n for v, n in zip(q, shape))
    for p in np.ndindex(*shape):
        here = int(a[p])
        thick = any(int(a[q]) != here for q in (tuple(v + d for v, d in zip(p, o)) for o in near) if inside(q))
        if mode == "thick":
            out[p] = thick
        elif mode == "inner":
            out[p] = thick and here != background
        else:
            vals = [int(a[q]) for q in (tuple(v + d for v, d in zip(p, o)) for o in window) if inside(q)]
            adjacent = here != background and max(vals) != min(top if v == background else v for v in vals)
            out[p] = thick and (here == background or adjacent)
    return out


def brute_pixels_image(a, backgrounds):
    """find_boundaries of a 2D uint8 image for both connectivities, every mode and every background of `backgrounds`, in ONE loop over
    the pixels (each pixel's window is gathered once and every rule is read off it): {(connectivity, mode, background): bool image}"""
    assert a.ndim == 2 and a.dtype == np.uint8
    Y, X = a.shape
    rows = a.tolist()
    out = {(c, m, b): np.zeros(a.shape, bool) for c in (1, 2) for m in MODES for b in backgrounds}
    for y in range(Y):
        y0, y1 = max(y - 1, 0), min(y + 2, Y)
        for x in range(X):
            x0, x1 = max(x - 1, 0), min(x + 2, X)
            here = rows[y][x]
            window = [v for r in rows[y0:y1] for v in r[x0:x1]]
            cross = rows[y][x0:x1] + [rows[k][x] for k in range(y0, y1)]
            if min(window) == max(window):
                continue                                                    # one value: no rule marks the pixel
            thick = {1: min(cross) != max(cross), 2: True}
            for b in backgrounds:
                outer = here == b or max(window) != min(255 if v == b else v for v in window)
                for c in (1, 2):
                    if thick[c]:
                        out[(c, "thick", b)][y, x] = True
                        out[(c, "inner", b)][y, x] = here != b
                        out[(c, "outer", b)][y, x] = outer
    return out


def brute_shifts(a, connectivity, mode, background):
    """the same definition with the loop over the offsets outside and numpy over the pixels inside: for the large images"""
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    top = int(np.iinfo(a.dtype).max)
    nd, shape = a.ndim, a.shape
    wide = a.astype(object) if a.dtype == np.uint64 else a.astype(np.int64)
    raised = np.where(wide == background, top, wide)
    thick = np.zeros(shape, bool)
    hi, lo = wide.copy(), raised.copy()
    for o in offsets(nd, nd):
        here = tuple(slice(max(0, -d), n - max(0, d)) for d, n in zip(o, shape))
        there = tuple(slice(max(0, d), n - max(0, -d)) for d, n in zip(o, shape))
        if sum(1 for v in o if v) <= connectivity:
            thick[here] |= wide[there] != wide[here]
        hi[here] = np.maximum(hi[here], wide[there])
        lo[here] = np.minimum(lo[here], raised[there])
    is_bg = wide == background
    if mode == "thick":
        return thick
    if mode == "inner":
        return thick & ~is_bg
    return thick & (is_bg | (hi != lo))


def brute_components(a):
    """component image of a under full connectivity, 0 for the value 0, by a flood fill per pixel (small images only)"""
    comp = np.zeros(a.shape, np.int64)
    n = 0
    for p in np.ndindex(*a.shape):
        if a[p] == 0 or comp[p]:
            continue
        n += 1
        comp[p] = n
        stack = [p]
        while stack:
            q = stack.pop()
            for o in offsets(a.ndim, a.ndim):
                r = tuple(v + d for v, d in zip(q, o))
                if all(0 <= v < m for v, m in zip(r, a.shape)) and not comp[r] and a[r] == a[p]:
                    comp[r] = n
                    stack.append(r)
    return comp


def brute_clear_border(a, buffer_size=0, bgval=0, mask=None):
    comp = brute_components(a)
    ext = buffer_size + 1
    hit = set()
    for p in np.ndindex(*a.shape):
        outside = (not mask[p]) if mask is not None else any(v < ext or v >= n - ext for v, n in zip(p, a.shape))
        if outside:
            hit.add(int(comp[p]))
    out = a.copy()
    for p in np.ndindex(*a.shape):
        if int(comp[p]) in hit:
            out[p] = bgval
    return out


# ----------------------------------------------------------------------------- images

def blobs(shape, n, seed, dtype=np.int32, first=1, step=1, radius=(2, 6)):
    """n balls of random radius at random places, ids first, first + step, ...; later ones overwrite earlier ones, so objects touch"""
    rng = np.random.RandomState(seed)
    a = np.zeros(shape, np.int64)
    grid = np.ogrid[tuple(slice(0, s) for s in shape)]
    for k in range(n):
        c = [rng.randint(0, s) for s in shape]
        r = rng.randint(radius[0], radius[1] + 1)
        a[sum((g - v) ** 2 for g, v in zip(grid, c)) <= r * r] = first + k * step
    return a.astype(dtype)


def noise(shape, values, seed, dtype=np.int32):
    return np.asarray(values)[np.random.RandomState(seed).randint(0, len(values), size=shape)].astype(dtype)


FB = {
    "noise_u8": noise((9, 11), (0, 1, 2, 255), 1, np.uint8),
    "noise_i16_negative": noise((8, 7), (0, 1, -3, 5, 32767), 2, np.int16),
    "noise_i32": noise((7, 9), (0, 1, 2, 2 ** 31 - 1), 3, np.int32),
    "noise_i64": noise((6, 10), (0, 1, 7, 2 ** 40), 4, np.int64),
    "noise_i64_small": noise((6, 10), (0, 1, 7, -2), 14, np.int64),
    "mask": noise((9, 8), (0, 1), 5, np.uint8).astype(bool),
    "blobs": blobs((14, 17), 6, 6),
    "row": noise((1, 6), (0, 1, 2), 7, np.uint8),
    "column": noise((5, 1), (0, 1, 2), 8, np.int16),
    "single": np.array([[3]], np.int32),
    "slice_volume": noise((1, 4, 4), (0, 1, 2), 9, np.int32),
    "volume_u8": noise((4, 5, 6), (0, 1, 2, 255), 10, np.uint8),
    "volume_i16_negative": noise((3, 4, 5), (0, -1, 4), 11, np.int16),
    "volume_blobs": blobs((6, 9, 10), 5, 12, np.int64, radius=(1, 3)),
    "constant": np.full((5, 6), 4, np.int32),
}
FB = {k: frozen(v) for k, v in FB.items()}


def fb_params(a):
    """(connectivity, mode, background) of a find_boundaries case: every mode and connectivity, background 0 and another value (a
    negative one where the image has negative ids)"""
    other = -3 if (a.dtype.kind == "i" and (a < 0).any()) else 1
    return [(c, m, b) for c in range(1, a.ndim + 1) for m in MODES for b in (0, other)]


@functools.lru_cache(maxsize=None)
def windows_image():
    """every 3 x 3 window over the values {0, 1, 2}, each in the middle of a 5 x 5 cell of zeros: 141 x 140 cells -> (705, 700) uint8"""
    n = 3 ** 9
    rows, cols = 141, 140
    assert rows * cols >= n
    digits = (np.arange(n)[:, None] // 3 ** np.arange(9)[None, :]) % 3
    cells = np.zeros((rows * cols, 5, 5), np.uint8)
    cells[:n, 1:4, 1:4] = digits.reshape(n, 3, 3)
    return frozen(cells.reshape(rows, cols, 5, 5).transpose(0, 2, 1, 3).reshape(rows * 5, cols * 5))


def _two_components():
    a = np.zeros((12, 14), np.int32)
    a[0:3, 2:5] = 4                                                         # id 4 at the edge ...
    a[6:9, 6:9] = 4                                                         # ... and once more inside: only the first goes
    a[5:7, 10:12] = 9
    return a


def _diagonal_contact():
    a = np.zeros((10, 10), np.int32)
    a[0:3, 0:3] = 2
    a[3:6, 3:6] = 2                                                         # touches the first block at a corner: one component
    a[7:9, 1:3] = 2                                                         # the same id, apart
    a[6:8, 6:8] = 3                                                         # another id in diagonal contact with a 2: its own component
    return a


def _framed():
    a = np.zeros((13, 15), np.int32)
    a[:] = 5
    a[1:-1, 1:-1] = 0                                                       # the band of buffer_size 0 holds no background pixel
    a[4:7, 4:8] = 6
    a[8:11, 9:12] = 7
    return a


def _inner_objects():
    a = np.zeros((16, 18), np.int32)
    a[3:6, 3:7] = 1
    a[8:12, 9:14] = 2
    return a                                                                # the band of buffer_size 0, 1 holds only background


_CB_BLOBS = blobs((40, 70), 30, 21, radius=(2, 5))
_CB_VOLUME = blobs((7, 20, 70), 20, 22, radius=(1, 4))
_CB_MASK = np.random.RandomState(23).random_sample((40, 70)) < 0.97

# name -> (labels, keyword arguments)
CB = {
    "blobs": (_CB_BLOBS, {}),
    "blobs_buffer_1": (_CB_BLOBS, {"buffer_size": 1}),
    "blobs_buffer_largest": (_CB_BLOBS, {"buffer_size": 39}),
    "blobs_bgval_7": (_CB_BLOBS, {"bgval": 7}),
    "blobs_mask": (_CB_BLOBS, {"mask": _CB_MASK}),
    "blobs_mask_bgval_buffer_ignored": (_CB_BLOBS, {"mask": _CB_MASK, "bgval": 3, "buffer_size": 500}),
    "blobs_mask_all_true": (_CB_BLOBS, {"mask": np.ones((40, 70), bool), "bgval": 7}),
    "blobs_mask_all_false": (_CB_BLOBS, {"mask": np.zeros((40, 70), bool), "bgval": 7}),
    "blobs_u8": (_CB_BLOBS.astype(np.uint8), {"bgval": 255}),
    "blobs_i16_negative": (np.where(_CB_BLOBS % 3 == 1, -_CB_BLOBS, _CB_BLOBS).astype(np.int16), {"bgval": -7}),
    "blobs_i64": (_CB_BLOBS.astype(np.int64), {"buffer_size": 2}),
    "blobs_bool": (_CB_BLOBS > 0, {}),
    "two_components": (_two_components(), {}),
    "diagonal_contact": (_diagonal_contact(), {}),
    "framed_bgval_7": (_framed(), {"bgval": 7}),
    "framed_bgval_7_buffer_1": (_framed(), {"bgval": 7, "buffer_size": 1}),
    "inner_objects": (_inner_objects(), {"buffer_size": 1}),
    "inner_objects_bgval_7": (_inner_objects(), {"bgval": 7}),
    "volume": (_CB_VOLUME, {}),
    "volume_buffer_2_bgval": (_CB_VOLUME, {"buffer_size": 2, "bgval": 9}),
    "volume_buffer_largest": (_CB_VOLUME, {"buffer_size": 6}),
    "volume_mask": (_CB_VOLUME, {"mask": np.random.RandomState(24).random_sample((7, 20, 70)) < 0.99}),
    "slice_volume": (_CB_BLOBS[None], {}),
    "row": (noise((1, 9), (0, 1, 2), 25), {}),
    "single": (np.array([[4]], np.int32), {}),
}
CB = {k: (frozen(a), {kk: (frozen(v) if isinstance(v, np.ndarray) else v) for kk, v in kw.items()}) for k, (a, kw) in CB.items()}
CB_BRUTE = ("two_components", "diagonal_contact", "framed_bgval_7", "framed_bgval_7_buffer_1", "inner_objects", "inner_objects_bgval_7",
            "row", "single", "blobs_bgval_7", "blobs_mask", "blobs_buffer_largest")


def _split_id():
    a = np.zeros((12, 20), np.int32)
    a[1:3, 1:4] = 5                                                         # three pieces of 6 pixels, 18 together
    a[5:7, 8:11] = 5
    a[9:11, 15:18] = 5
    a[4:8, 1:4] = 2                                                         # 12 pixels in one piece
    a[0, 19] = 8
    return a


_RS_BLOBS = blobs((40, 70), 40, 31, radius=(1, 4))
_RS_VOLUME = blobs((7, 20, 70), 25, 32, radius=(1, 3))
_RS_MASK = np.random.RandomState(33).random_sample((30, 66)) < 0.45
_RS_MASK3 = np.random.RandomState(34).random_sample((5, 12, 66)) < 0.25

RS = {
    "split_id_kept": (_split_id(), {"min_size": 13}),
    "split_id_gone": (_split_id(), {"min_size": 19}),
    "blobs": (_RS_BLOBS, {"min_size": 30}),
    "blobs_default": (_RS_BLOBS, {}),
    "blobs_min_0": (_RS_BLOBS, {"min_size": 0}),
    "blobs_min_1": (_RS_BLOBS, {"min_size": 1}),
    "blobs_u8": (_RS_BLOBS.astype(np.uint8), {"min_size": 30}),
    "blobs_i16": (_RS_BLOBS.astype(np.int16), {"min_size": 20}),
    "blobs_i64": (_RS_BLOBS.astype(np.int64), {"min_size": 25}),
    "blobs_huge_ids": (np.where(_RS_BLOBS > 0, _RS_BLOBS.astype(np.int64) * 3 * 10 ** 9 + 17, 0), {"min_size": 30}),
    "volume": (_RS_VOLUME, {"min_size": 20}),
    "mask_c1": (_RS_MASK, {"min_size": 6, "connectivity": 1}),
    "mask_c2": (_RS_MASK, {"min_size": 6, "connectivity": 2}),
    "mask_min_1": (_RS_MASK, {"min_size": 1}),
    "mask3_c1": (_RS_MASK3, {"min_size": 4, "connectivity": 1}),
    "mask3_c2": (_RS_MASK3, {"min_size": 4, "connectivity": 2}),
    "mask3_c3": (_RS_MASK3, {"min_size": 4, "connectivity": 3}),
    "all_zero": (np.zeros((5, 6), np.int32), {"min_size": 3}),
    "mask_all_false": (np.zeros((5, 6), bool), {"min_size": 3}),
}
RS = {k: (frozen(a), kw) for k, (a, kw) in RS.items()}

_SL_BLOBS = blobs((40, 70), 25, 41, radius=(2, 5))
_SL_HUGE = np.where(_SL_BLOBS > 0, _SL_BLOBS.astype(np.int64) * 5 * 10 ** 9 + 3, 0)
_SL_IDS = np.unique(_SL_BLOBS)[1:]

# name -> (label image, ids, keyword arguments)
SL = {
    "some": (_SL_BLOBS, _SL_IDS[::2], {}),
    "some_invert": (_SL_BLOBS, _SL_IDS[::2], {"invert": True}),
    "some_relabel": (_SL_BLOBS, _SL_IDS[::3], {"relabel": True}),
    "some_invert_relabel": (_SL_BLOBS, _SL_IDS[::3], {"invert": True, "relabel": True}),
    "absent_ids": (_SL_BLOBS, np.array([3, 5, 1000, 10 ** 12, 0, -4], np.int64), {}),
    "absent_ids_relabel": (_SL_BLOBS, np.array([3, 5, 5, 1000, 10 ** 12, 0, -4], np.int64), {"relabel": True}),
    "empty_list": (_SL_BLOBS, np.zeros(0, np.int64), {}),
    "empty_list_invert_relabel": (_SL_BLOBS, np.zeros(0, np.int64), {"invert": True, "relabel": True}),
    "u8": (_SL_BLOBS.astype(np.uint8), _SL_IDS[1::2].astype(np.uint8), {}),
    "i16_relabel": (_SL_BLOBS.astype(np.int16), _SL_IDS[1::2], {"relabel": True}),
    "i64": (_SL_BLOBS.astype(np.int64), _SL_IDS[::2], {"invert": True}),
    "huge_ids": (_SL_HUGE, np.unique(_SL_HUGE)[1::2], {}),
    "huge_ids_invert": (_SL_HUGE, np.concatenate([np.unique(_SL_HUGE)[1::2], [12345]]), {"invert": True}),
    "huge_ids_relabel": (_SL_HUGE, np.unique(_SL_HUGE)[1::2], {"relabel": True}),
    "negative_values": (np.where(_SL_BLOBS % 4 == 1, -_SL_BLOBS, _SL_BLOBS), np.concatenate([_SL_IDS[::2], -_SL_IDS[:4]]), {}),
    "volume": (blobs((6, 20, 66), 12, 42, radius=(1, 4)), np.array([1, 4, 5, 9]), {"relabel": True}),
    "line": (noise((50,), (0, 1, 2, 3), 43), np.array([1, 3]), {}),
}
SL = {k: (frozen(a), frozen(w), kw) for k, (a, w, kw) in SL.items()}


def brute_select(a, wanted, invert=False, relabel=False):
    wanted = set(int(v) for v in wanted)
    out = np.zeros_like(a)
    kept = sorted(set(int(v) for v in a.reshape(-1) if v > 0 and ((int(v) in wanted) != invert)))
    new = {v: (k + 1 if relabel else v) for k, v in enumerate(kept)}
    flat, res = a.reshape(-1), out.reshape(-1)
    for i, v in enumerate(flat):
        if int(v) in new:
            res[i] = new[int(v)]
    return out


# ----------------------------------------------------------------------------- images around the tile extents (the device tests)

def tile_shapes(nd):
    """one more and one less than the tile extent along every axis, two tiles and one, and shapes smaller than a tile"""
    if nd == 2:
        return [(TY + 1, TX + 1), (TY - 1, TX - 1), (2 * TY + 1, 2 * TX + 1), (1, 1), (1, 70), (70, 1)]
    return [(TZ + 1, VY + 1, TX + 1), (TZ - 1, VY - 1, TX - 1), (2 * TZ + 1, 2 * VY + 1, 2 * TX + 1), (1, 1, 1), (2, 3, 4)]


@functools.lru_cache(maxsize=None)
def tiled(kind, shape):
    """an int32 image of `shape`: 'stripes' -- objects and stripes whose edges lie on the tile edges; 'faces' -- an object on every
    face and at every corner; 'noise' -- three ids at random, every pixel a boundary pixel; 'constant'"""
    nd = len(shape)
    tile = (TY, TX) if nd == 2 else (TZ, VY, TX)
    a = np.zeros(shape, np.int32)
    if kind == "stripes":
        for d, (n, t) in enumerate(zip(shape, tile)):
            idx = np.arange(n).reshape([-1 if k == d else 1 for k in range(nd)])
            a = a + ((idx // t) % 2 + 2 * (idx % t == t - 1)).astype(np.int32) * 3 ** d        # changes at, and one before, every tile edge
        a[tuple(slice(0, max(1, min(n, t) // 2)) for n, t in zip(shape, tile))] = 0
    elif kind == "faces":
        k = 1
        for d in range(nd):
            for side in (0, -1):
                at = [slice(n // 3, n // 3 + max(1, n // 3)) for n in shape]
                at[d] = slice(0, 2) if side == 0 else slice(-2, None)
                a[tuple(at)] = k
                k += 1
        for corner in itertools.product((0, -1), repeat=nd):
            a[corner] = k
            k += 1
    elif kind == "noise":
        a = noise(shape, (0, 1, 2), 51 + sum(shape))
    elif kind == "constant":
        a[:] = 3
    else:
        raise KeyError(kind)
    return frozen(a)


KINDS = ("stripes", "faces", "noise", "constant")


@functools.lru_cache(maxsize=None)
def balls():
    """touching balls in a 9 x 35 x 67 volume"""
    return frozen(blobs((9, 35, 67), 40, 61, radius=(3, 7)))
