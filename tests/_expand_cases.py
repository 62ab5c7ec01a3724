"""Cases of stardist_amd.utils.expand_labels / distance_transform, shared by tests/test_cpu_expand_labels.py and
tests/test_gpu_expand_labels.py, and a brute-force reference that states the definition of csrc/edt_feature.h literally.

    NAMES, SMALL, BIG   every case; those at or below BRUTE_LIMIT pixels (brute-forced); the larger ones (scipy is their reference)
    case(name)          the label image (read-only)
    spacings(name)      unit, dyadic, non-dyadic, one value per axis
    distances(name)     0, 1, 1.5, sqrt 2 and the float below it, 3, 6.5, one beyond the image diagonal
    brute(a, spacing, feature_is_zero=False)   (linear index of the nearest feature, distance) over all features, -1 / inf without one
    ambiguous(a, spacing)                      mask of the pixels whose minimal distance is reached by features of different labels
    reference(name, spacing)                   (index, distance), computed once: brute for SMALL, scipy for BIG
    ambiguous_case(name, spacing)              ambiguous() of a SMALL case, from the pass that made its reference
    expanded(a, index, dist, distance)         the expand_labels result that follows from a reference
    as_int32(a)                                the labels as the C entry points take them
    bounded(index, dist, max_distance)         the reference under a search bound
"""
import functools

import numpy as np

BRUTE_LIMIT = 5000
THREADS = 256                                                               # EDTF_THREADS: one workgroup covers this many pixels
SQRT2 = float(np.sqrt(2.0))


def _discs(shape, n, rmin, rmax, seed, dtype=np.int32):
    """n discs / balls of random centre and radius, painted in order: later ones overwrite (overlap) or touch earlier ones"""
    rng = np.random.RandomState(seed)
    a = np.zeros(shape, dtype)
    for i in range(n):
        c = [rng.uniform(0, s - 1) for s in shape]
        r = rng.uniform(rmin, rmax)
        box = tuple(slice(max(int(ci - r), 0), int(ci + r) + 2) for ci in c)
        grid = np.meshgrid(*[np.arange(s)[b] for s, b in zip(shape, box)], indexing="ij")
        a[box][sum((g - ci) ** 2 for g, ci in zip(grid, c)) <= r * r] = i + 1
    return a


discs = _discs                                                              # for the tests at scale: a nuclei-like image of any size


def _points(shape, n, seed, top=None):
    rng = np.random.RandomState(seed)
    a = np.zeros(shape, np.int32)
    flat = rng.choice(a.size, n, replace=False)
    a.reshape(-1)[flat] = np.arange(1, n + 1) if top is None else top - np.arange(n)
    return a


def _lattice(shape, pitch=4):
    """single-pixel labels, all different, on a lattice of even pitch: every midpoint between two of them is an integer pixel"""
    a = np.zeros(shape, np.int32)
    sl = tuple(slice(1, None, pitch) for _ in shape)
    a[sl] = np.arange(1, a[sl].size + 1).reshape(a[sl].shape)
    return a


def _one(shape, at, label=7):
    a = np.zeros(shape, np.int32)
    a[at] = label
    return a


# widths that are no multiple of 64; every axis spans more than one workgroup of THREADS consecutive pixels
IMAGE, VOLUME = (37, 131), (7, 19, 37)
_MAKERS = {
    "discs": lambda: _discs(IMAGE, 14, 3, 9, 1),
    "points": lambda: _points((41, 97), 25, 2),
    "lattice": lambda: _lattice((33, 67)),
    "corner": lambda: _one(IMAGE, (0, 0)),
    "far_corner": lambda: _one(IMAGE, (IMAGE[0] - 1, IMAGE[1] - 1)),
    "no_feature": lambda: np.zeros((9, 70), np.int32),
    "all_labelled": lambda: (np.random.RandomState(3).randint(1, 6, (9, 70))).astype(np.int32),
    "one_row": lambda: _points((1, 300), 9, 4),
    "one_column": lambda: _points((300, 1), 9, 5),
    "single_pixel": lambda: np.full((1, 1), 5, np.int32),
    "single_background_pixel": lambda: np.zeros((1, 1), np.int32),
    "high_labels": lambda: _points((29, 83), 30, 6, top=2 ** 31 - 1),
    "discs_u8": lambda: _discs(IMAGE, 14, 3, 9, 7, np.uint8) * np.uint8(17),
    "discs_u16": lambda: _discs(IMAGE, 14, 3, 9, 8, np.uint16) * np.uint16(4681),
    "discs_i64": lambda: _discs(IMAGE, 14, 3, 9, 9, np.int64) + (_discs(IMAGE, 14, 3, 9, 9, np.int64) > 0) * (2 ** 40),
    "balls": lambda: _discs(VOLUME, 10, 2, 5, 10),
    "points3d": lambda: _points((6, 17, 45), 20, 11),
    "lattice3d": lambda: _lattice((9, 13, 21)),
    "corner3d": lambda: _one(VOLUME, (0, 0, 0)),
    "far_corner3d": lambda: _one(VOLUME, tuple(n - 1 for n in VOLUME)),
    "no_feature3d": lambda: np.zeros((3, 5, 70), np.int32),
    "all_labelled3d": lambda: (np.random.RandomState(12).randint(1, 6, (3, 5, 70))).astype(np.int32),
    "plane_as_volume": lambda: _discs((30, 70), 6, 3, 8, 13).reshape(1, 30, 70),
    "balls_u16": lambda: _discs(VOLUME, 10, 2, 5, 14, np.uint16) * np.uint16(6553),
    "discs_big": lambda: _discs((150, 333), 120, 3, 9, 15),
    "balls_big": lambda: _discs((12, 70, 150), 150, 2, 6, 16),
}
NAMES = tuple(_MAKERS)
RANDOMISED = ("discs", "points", "discs_u8", "discs_u16", "discs_i64", "balls", "points3d", "balls_u16", "high_labels")
DISCS = ("discs", "discs_u8", "discs_u16", "discs_i64", "balls", "balls_u16")
TIED = ("lattice", "lattice3d") + DISCS                                     # must contain ties between different labels
NO_FEATURE = ("no_feature", "no_feature3d", "single_background_pixel")
EMPTY_SHAPES = ((0, 5), (4, 0), (0, 3, 4), (2, 0, 4), (2, 3, 0))


@functools.lru_cache(maxsize=None)
def case(name):
    a = np.ascontiguousarray(_MAKERS[name]())
    a.setflags(write=False)
    return a


SMALL = tuple(n for n in NAMES if case(n).size <= BRUTE_LIMIT)
BIG = tuple(n for n in NAMES if n not in SMALL)


def spacings(name):
    return ((1.0, 1.0), (2.0, 0.5), (1.3, 0.7)) if case(name).ndim == 2 else ((1.0, 1.0, 1.0), (2.0, 1.0, 0.5), (1.3, 0.7, 1.1))


def distances(name):
    beyond = float(np.ceil(2.0 * np.sqrt(sum(n * n for n in case(name).shape)))) + 1.0      # the largest spacing is 2
    return (0.0, 1.0, 1.5, SQRT2, float(np.nextafter(SQRT2, 0)), 3.0, 6.5, beyond)


def _squared(p, q, spacing):
    """D of the definition for coordinate arrays p (n, 1, nd) and q (1, m, nd): terms t = s * d; t * t, summed first axis first, each
    numpy operation rounding on its own"""
    total = None
    for ax, s in enumerate(spacing):
        t = np.float64(s) * (q[..., ax] - p[..., ax]).astype(np.float64)
        t = t * t
        total = t if total is None else total + t
    return total


def _brute(a, spacing, feature_is_zero):
    a = np.asarray(a)
    assert a.size <= BRUTE_LIMIT and len(spacing) == a.ndim
    feature = (a == 0) if feature_is_zero else (a != 0)
    index, dist, amb = np.full(a.size, -1, np.int32), np.full(a.size, np.inf), np.zeros(a.size, bool)
    if feature.any():
        q = np.argwhere(feature)
        q = q[np.lexsort([q[:, ax] for ax in range(a.ndim)])]               # primary key: the last axis, then the one before it
        labels = a[tuple(q.T)].astype(np.int64)
        lin = np.ravel_multi_index(tuple(q.T), a.shape).astype(np.int32)
        p = np.argwhere(np.ones(a.shape, bool))
        for lo in range(0, len(p), 256):
            D = _squared(p[lo:lo + 256, None, :], q[None, :, :], spacing)
            first = D.argmin(axis=1)                                        # the first minimum: the smallest key among equals
            best = D[np.arange(len(first)), first]
            index[lo:lo + 256], dist[lo:lo + 256] = lin[first], np.sqrt(best)
            tied = D == best[:, None]
            amb[lo:lo + 256] = np.where(tied, labels[None, :], labels.max()).min(axis=1) != np.where(tied, labels[None, :], labels.min()).max(axis=1)
    return index.reshape(a.shape), dist.reshape(a.shape), amb.reshape(a.shape)


def brute(a, spacing, feature_is_zero=False):
    return _brute(a, spacing, feature_is_zero)[:2]


def ambiguous(a, spacing):
    return _brute(a, spacing, False)[2]


def scipy_reference(a, spacing, feature_is_zero=False):
    """(linear index, distance) from scipy.ndimage.distance_transform_edt, -1 / inf for an image without features"""
    from scipy.ndimage import distance_transform_edt
    a = np.asarray(a)
    background = (a != 0) if feature_is_zero else (a == 0)
    if background.all():
        return np.full(a.shape, -1, np.int32), np.full(a.shape, np.inf)
    dist, idx = distance_transform_edt(background, sampling=spacing, return_indices=True)
    return np.ravel_multi_index(tuple(idx), a.shape).astype(np.int32), dist


@functools.lru_cache(maxsize=None)
def _brute_case(name, spacing):
    out = _brute(case(name), spacing, False)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, spacing):
    if name in SMALL:
        return _brute_case(name, spacing)[:2]
    index, dist = scipy_reference(case(name), spacing)
    index.setflags(write=False)
    dist.setflags(write=False)
    return index, dist


def ambiguous_case(name, spacing):
    """ambiguous() of a SMALL case, from the same brute-force pass as its reference"""
    return _brute_case(name, spacing)[2]


def bounded(index, dist, max_distance):
    far = ~(dist <= max_distance)
    return np.where(far, np.int32(-1), index), np.where(far, np.inf, dist)


def as_int32(a):
    """the labels as int32 with their order kept: the image itself where it fits, else the ranks of its values"""
    if int(a.max(initial=0)) < 2 ** 31:
        return np.ascontiguousarray(a.astype(np.int32))
    u, inv = np.unique(a, return_inverse=True)
    assert u[0] == 0
    return np.ascontiguousarray(inv.reshape(a.shape).astype(np.int32))


def expanded(a, index, dist, distance):
    near = (dist <= distance) & (index >= 0)
    out = np.zeros_like(a)
    out[near] = a.reshape(-1)[index[near]]
    return out
