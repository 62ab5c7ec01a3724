"""Scenes and numpy statements shared by tests/test_cpu_relabel_points.py and tests/test_gpu_relabel_device.py: label images for the
per-object centroid sums and for star distances evaluated at given pixels only (csrc/relabel_star.hip).  All scenes are int32 and hold
ids with gaps; every array is built once per process and must not be written."""
import functools

import numpy as np

SHAPE_2D = (61, 130)          # rows wider than a wave of 64 pixels and no multiple of it
SHAPE_3D = (20, 37, 45)
SHAPE_WIDE = (40, 70000)      # one object over columns 60000 .. 69999: its sum of x is 2.6e10, past 2**32
SHAPE_U16 = (130, 130)        # large enough that the id 65543 needs no compaction (<= 4 * size + 1024)


def _disc(a, cy, cx, ry, rx, lab):
    yy, xx = np.ogrid[:a.shape[0], :a.shape[1]]
    a[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = lab


def _ball(a, c, r, lab):
    zz, yy, xx = np.ogrid[:a.shape[0], :a.shape[1], :a.shape[2]]
    a[((zz - c[0]) / r[0]) ** 2 + ((yy - c[1]) / r[1]) ** 2 + ((xx - c[2]) / r[2]) ** 2 <= 1.0] = lab


@functools.lru_cache(maxsize=None)
def multi2d():
    """discs and ellipses with non-sequential ids, two objects that touch, objects on three image borders and in a corner, a one-pixel
    object inside the image and one in the last pixel"""
    a = np.zeros(SHAPE_2D, np.int32)
    _disc(a, 14, 20, 9, 12, 3)
    _disc(a, 15, 44, 10, 11, 7)          # touches 3
    _disc(a, 40, 30, 14, 8, 12)
    _disc(a, 45, 80, 11, 25, 40)         # wider than a wave
    _disc(a, 2, 100, 6, 9, 41)           # cut by the top border
    _disc(a, 30, 128, 8, 6, 90)          # cut by the right border
    _disc(a, 60, 5, 5, 9, 91)            # bottom-left corner
    a[25, 70] = 200                      # one pixel
    a[60, 129] = 333                     # the last pixel: max_label is present only there
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ell():
    """an L whose centroid pixel is background"""
    a = np.zeros((40, 50), np.int32)
    a[5:35, 6:10] = 5
    a[31:35, 6:44] = 5
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ring_disc():
    """a ring (id 9) around a disc (id 4): both centroids fall on the same pixel, which belongs to the disc"""
    a = np.zeros((51, 53), np.int32)
    _disc(a, 25, 26, 20, 20, 9)
    _disc(a, 25, 26, 15, 15, 0)
    _disc(a, 25, 26, 8, 8, 4)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def u16_pair():
    """ids 7 and 65543 = 7 + 65536 side by side: two objects with two centroids, one object to a ray"""
    a = np.zeros(SHAPE_U16, np.int32)
    a[30:90, 20:60] = 7
    a[30:90, 60:100] = 65543
    a[100:120, 10:30] = 8
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def u16_zero():
    """id 65536 is an object with a centroid, and background to a ray"""
    a = np.zeros(SHAPE_U16, np.int32)
    a[20:60, 20:70] = 65536
    a[80:120, 40:100] = 2
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def wide():
    a = np.zeros(SHAPE_WIDE, np.int32)
    a[:, 60000:70000] = 2
    a[3:9, 100:400] = 1
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def one_pixel_image():
    a = np.full((1, 1), 1, np.int32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def full_image():
    """one object on every pixel: every atomic of the sums pass lands on one slot"""
    a = np.full((300, 300), 6, np.int32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def last_pixel():
    a = np.zeros(SHAPE_2D, np.int32)
    a[-1, -1] = 77
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def multi3d():
    """balls and a box with non-sequential ids, one on the volume's border, a one-voxel object, an L-shaped object"""
    a = np.zeros(SHAPE_3D, np.int32)
    _ball(a, (9, 12, 12), (6, 9, 9), 2)
    _ball(a, (10, 26, 30), (8, 8, 11), 5)
    _ball(a, (1, 30, 6), (4, 5, 5), 11)          # cut by the z = 0 face and the y border
    a[14:20, 2:8, 36:45] = 30                     # box in the far corner
    a[3, 3, 40] = 31                              # one voxel
    a[2:18, 16:19, 20:23] = 50                    # L: a bar along z ...
    a[15:18, 16:19, 2:23][a[15:18, 16:19, 2:23] == 0] = 50      # ... and one along x, where free
    a.setflags(write=False)
    return a


def scenes2d():
    return {"multi2d": multi2d(), "ell": ell(), "ring_disc": ring_disc(), "u16_pair": u16_pair(), "u16_zero": u16_zero()}


def scenes3d():
    return {"multi3d": multi3d()}


def centroid_scenes():
    """every scene the centroid rule is checked on (name -> int32 image)"""
    s = dict(scenes2d())
    s.update(scenes3d())
    s.update(wide=wide(), one_pixel_image=one_pixel_image(), full_image=full_image(), last_pixel=last_pixel())
    return s


def centroid_sums_np(lbl, top=None):
    """[top + 1][4] int64: pixel count, sum of z, of y, of x per label (z = 0 in 2D); slot 0 and absent labels 0.  np.bincount sums its
    weights in float64: every sum here is an integer below 2**53, so the float64 sum is exact."""
    a = np.asarray(lbl)
    top = int(a.max()) if top is None else int(top)
    flat = a.ravel().astype(np.int64)
    obj = (flat >= 1) & (flat <= top)
    idx = np.where(obj, flat, 0)
    out = np.zeros((top + 1, 4), np.int64)
    out[:, 0] = np.bincount(idx, minlength=top + 1)
    coords = np.unravel_index(np.arange(a.size, dtype=np.int64), a.shape)
    for d, c in enumerate(coords):
        col = 4 - a.ndim + d
        w = np.bincount(idx, weights=c.astype(np.int64), minlength=top + 1)
        assert (w < 2.0 ** 53).all()
        out[:, col] = w.astype(np.int64)
    out[0] = 0
    return out


def centroid_rule_np(lbl):
    """(labs, points) by the integer rule of _region_centroids_device: the labels present, ascending, and sums // count"""
    s = centroid_sums_np(lbl)
    labs = np.flatnonzero(s[:, 0])
    return labs.astype(np.int64), s[labs, 4 - np.asarray(lbl).ndim:] // s[labs, :1]


def probe_points(lbl, per_kind=6, seed=0):
    """(n, ndim) int64 pixels for the point rows: object pixels on each face of the image border, pixels of every object, background
    pixels, the first and the last pixel"""
    a = np.asarray(lbl)
    rng = np.random.default_rng(seed)
    pts = [np.zeros(a.ndim, np.int64), np.array(a.shape, np.int64) - 1]
    border = np.zeros(a.shape, bool)
    for ax in range(a.ndim):
        sl = [slice(None)] * a.ndim
        for at in (0, -1):
            sl[ax] = at
            border[tuple(sl)] = True
    for mask in [border & (a > 0), a == 0] + [a == v for v in np.unique(a[a > 0])]:
        where = np.argwhere(mask)
        if len(where):
            pts.extend(where[rng.choice(len(where), min(per_kind, len(where)), replace=False)])
    return np.ascontiguousarray(np.stack(pts).astype(np.int64))


def rays3d():
    from stardist_amd.rays3d import Rays_GoldenSpiral
    return Rays_GoldenSpiral(24, anisotropy=(2, 1, 1))
