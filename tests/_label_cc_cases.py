"""Cases of stardist_amd.utils.label_components, shared by tests/test_cpu_label_components.py and tests/test_gpu_label_components.py.
Shapes come from the tile constants of stardist_amd/csrc/label_cc.h, so that every case straddles tile borders with sizes that are no
multiple of a tile; each case is a few thousand to a few hundred thousand pixels.

    NAMES            every case
    case(name)       (image, background)
    dtypes(name)     the dtypes the case is run in (masks: bool, uint8, uint16, int32; multi-valued: the own one and the wider ones)
    connectivities(name)
    host(name, c)    (labels, n) of the host route at connectivity c, computed once, read-only
"""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constants():
    txt = open(os.path.join(ROOT, "stardist_amd", "csrc", "label_cc.h")).read()
    return {k: int(v) for k, v in re.findall(r"\b(LCC_[A-Z_]+)\s*=\s*(\d+)", txt)}


K = header_constants()
TX, TY, TZ, VY = K["LCC_TILE_X"], K["LCC_TILE_Y"], K["LCC_TILE_Z"], K["LCC_VOL_TILE_Y"]
IMAGE = (3 * TY + 5, 2 * TX + 7)                    # 3.2 x 2.1 tiles
VOLUME = (2 * TZ + 1, 3 * VY + 3, 2 * TX + 5)       # 2.2 x 3.4 x 2.1 tiles
MASK_DTYPES = ("bool", "uint8", "uint16", "int32")


def spiral(h, w):
    """a one-pixel-wide rectangular spiral from the corner inwards, one empty pixel between its turns"""
    a = np.zeros((h, w), bool)
    y = x = 0
    dy, dx = 0, 1
    a[0, 0] = True
    turns = 0
    while turns < 2:
        ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        free = 0 <= ny < h and 0 <= nx < w and not a[ny, nx] and not (0 <= fy < h and 0 <= fx < w and a[fy, fx])
        if free:
            y, x, turns = ny, nx, 0
            a[y, x] = True
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return a


def serpentine(h, w):
    a = np.zeros((h, w), bool)
    a[::2] = True
    a[1::4, -1] = True
    a[3::4, 0] = True
    return a


def u_shape(h, w):
    a = np.zeros((h, w), bool)
    a[:, 1] = a[:, w - 2] = a[-1, 1:w - 1] = True
    return a


def comb(h, w):
    """teeth in every other column that join only in the last row"""
    a = np.zeros((h, w), bool)
    a[:, ::2] = True
    a[-1] = True
    return a


def comb3d(d, h, w):
    """teeth along z, one per (even y, even x), that join only in the last plane"""
    a = np.zeros((d, h, w), bool)
    a[:, ::2, ::2] = True
    a[-1] = True
    return a


def checkerboard(shape):
    return (np.indices(shape).sum(axis=0) % 2) == 0


def diagonals(h, w):
    a = np.zeros((h, w), bool)
    y = np.arange(h)
    for k in range(0, w, 9):
        a[y, (y + k) % w] = True
    return a


def helix(d, h, w):
    """a curve that winds around the z axis, two turns, sampled densely"""
    a = np.zeros((d, h, w), bool)
    t = np.linspace(0, 1, 40 * (d + h + w))
    z = np.round(t * (d - 1)).astype(int)
    y = np.round((h - 1) / 2 * (1 + 0.95 * np.sin(4 * np.pi * t))).astype(int)
    x = np.round((w - 1) / 2 * (1 + 0.95 * np.cos(4 * np.pi * t))).astype(int)
    a[z, y, x] = True
    return a


def rings(d, h, w):
    """two interlocked square rings, one in the plane z = c, one in the plane y = cy, one empty pixel between them where they pass; a
    tooth of the first ring touches the second one diagonally (dy = dx = 1): two components at connectivity 1, one above"""
    a = np.zeros((d, h, w), bool)
    c, cy = d // 2, h // 2
    y0, y1, x0, x1 = 2, h - 3, 3, w // 2
    a[c, y0:y1 + 1, [x0, x1]] = True
    a[c, [y0, y1], x0:x1 + 1] = True
    z0, z1, xa, xb = 1, d - 2, x0 + 2, w - 4
    a[z0:z1 + 1, cy, [xa, xb]] = True
    a[[z0, z1], cy, xa:xb + 1] = True
    a[c, cy - 1, x0 + 1] = True
    return a


def random_mask(shape, density, seed):
    return np.random.RandomState(seed).random_sample(shape) < density


def blocks(shape, side, values, seed):
    """square blocks of `side` pixels, every block one of `values` at random: touching blocks of different values, one value in many
    separated blobs, equal neighbours merged"""
    rng = np.random.RandomState(seed)
    grid = [-(-n // side) for n in shape]
    picks = np.asarray(values)[rng.randint(0, len(values), grid)]
    for ax in range(len(shape)):
        picks = np.repeat(picks, side, axis=ax)
    return np.ascontiguousarray(picks[tuple(slice(0, n) for n in shape)])


def _cases():
    h, w = IMAGE
    d, vh, vw = VOLUME
    c = {}
    c["spiral"] = (spiral(h, w), 0)
    c["serpentine"] = (serpentine(h, w), 0)
    c["u_shape"] = (u_shape(h, w), 0)
    c["comb"] = (comb(h, w), 0)
    c["comb3d"] = (comb3d(d, vh, vw), 0)
    c["checkerboard"] = (checkerboard(IMAGE), 0)
    c["checkerboard3d"] = (checkerboard(VOLUME), 0)
    c["diagonals"] = (diagonals(h, w), 0)
    c["helix"] = (helix(3 * TZ + 2, 4 * VY + 1, 2 * TX + 9), 0)
    c["rings"] = (rings(d, vh, vw), 0)
    c["all_background"] = (np.zeros(IMAGE, bool), 0)
    c["all_foreground"] = (np.ones(IMAGE, bool), 0)
    c["all_foreground3d"] = (np.ones(VOLUME, bool), 0)
    c["single_pixel"] = (np.ones((1, 1), bool), 0)
    c["one_row"] = (random_mask((1, 3 * TX + 5), 0.7, 1), 0)
    c["one_column"] = (random_mask((3 * TY + 5, 1), 0.7, 2), 0)
    c["plane_as_volume"] = (random_mask((1, TY + 3, TX + 5), 0.55, 3), 0)
    c["empty"] = (np.zeros((0, 5), bool), 0)
    c["empty3d"] = (np.zeros((3, 0, 5), bool), 0)
    for density in (0.3, 0.5, 0.59, 0.7):
        c["random_%g" % density] = (random_mask((5 * TY + 3, 4 * TX + 9), density, int(density * 100)), 0)
    c["random_small_0.59"] = (random_mask((TY + 7, TX + 9), 0.59, 5), 0)
    c["random3d_0.3"] = (random_mask((3 * TZ + 1, 4 * VY + 3, 2 * TX + 5), 0.3, 7), 0)
    c["random3d_0.15"] = (random_mask((3 * TZ + 1, 4 * VY + 3, 2 * TX + 5), 0.15, 8), 0)
    c["blocks_u8"] = (blocks(IMAGE, 7, [0, 0, 1, 2, 3, 255], 11).astype(np.uint8), 0)
    c["blocks_u8_background_3"] = (c["blocks_u8"][0], 3)
    c["blocks_u8_background_absent"] = (c["blocks_u8"][0], 7)
    c["blocks_u16_high"] = (blocks(IMAGE, 5, [0, 1, 32768, 40000, 65535], 12).astype(np.uint16), 0)
    c["blocks_u16_background_65535"] = (c["blocks_u16_high"][0], 65535)
    c["blocks_i32_negative"] = (blocks(IMAGE, 6, [0, -1, -7, 5, 2 ** 31 - 1, -2 ** 31], 13).astype(np.int32), 0)
    c["blocks_i32_background_-7"] = (c["blocks_i32_negative"][0], -7)
    c["blocks3d_u8"] = (blocks(VOLUME, 3, [0, 0, 1, 2, 9], 14).astype(np.uint8), 0)
    c["labels_u16"] = (((np.arange(h)[:, None] // 13) * 40 + np.arange(w)[None, :] // 11 + 1).astype(np.uint16) * serpentine(h, w), 0)
    for img, _ in c.values():
        img.setflags(write=False)
    return c


_CASES = _cases()
NAMES = list(_CASES)
MASKS = [n for n in NAMES if _CASES[n][0].dtype == np.bool_]
MULTI = [n for n in NAMES if n not in MASKS]
EMPTY = ("empty", "empty3d")


def case(name):
    return _CASES[name]


def dtypes(name):
    own = _CASES[name][0].dtype.name
    return MASK_DTYPES if own == "bool" else {"uint8": ("uint8", "uint16", "int32"), "uint16": ("uint16", "int32"), "int32": ("int32",)}[own]


def connectivities(name):
    return tuple(range(1, _CASES[name][0].ndim + 1))


@functools.lru_cache(maxsize=None)
def host(name, connectivity):
    from stardist_amd.utils import label_components
    img, background = _CASES[name]
    lab, n = label_components(img, connectivity, background, return_num=True)
    lab.setflags(write=False)
    return lab, n


def per_value_oracle(img, connectivity, background):
    """scipy.ndimage.label per value, the components of all values sorted by their first pixel"""
    from scipy import ndimage
    structure = ndimage.generate_binary_structure(img.ndim, connectivity)
    firsts, parts = [], []
    for v in np.unique(img):
        if v == background:
            continue
        lab, n = ndimage.label(img == v, structure)
        if n:
            flat = lab.reshape(-1)
            where = np.flatnonzero(flat)
            _, first = np.unique(flat[where], return_index=True)
            firsts.append(where[first])
            parts.append(lab)
    out = np.zeros(img.shape, np.int32)
    if not parts:
        return out, 0
    order = np.argsort(np.concatenate(firsts))
    new_id = np.empty(len(order), np.int32)
    new_id[order] = np.arange(1, len(order) + 1)
    base = 0
    for lab in parts:
        n = int(lab.max())
        lut = np.concatenate([np.zeros(1, np.int32), new_id[base:base + n]])
        out += lut[lab]
        base += n
    return out, len(order)
