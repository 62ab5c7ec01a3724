"""Scenes for group_matching_labels (frames of a time lapse / slices of a stack), shared by the CPU and the GPU tests, and the two
host-side references both compare with: the host function itself and the composition of sparse_overlap lists (independent of the
kernels).  No scene has two optimal assignments that tie exactly: sizes and shifts differ from object to object."""
import numpy as np

CRITERIA = ("iou", "iot", "iop")
THRESHS = (1e-10, 0.3, 0.5, 0.7)


def discs(shape, n, seed, rmin=3, rmax=9):
    """n discs (balls in 3D) at random centres, painted in id order (later ones cover earlier ones)"""
    rng = np.random.RandomState(seed)
    y = np.zeros(shape, np.int32)
    for i in range(1, n + 1):
        r = rng.randint(rmin, rmax)
        c = [rng.randint(0, s) for s in shape]
        sl = tuple(slice(max(0, ci - r), min(s, ci + r + 1)) for ci, s in zip(c, shape))
        g = np.ogrid[sl]
        y[sl][sum((gi - ci) ** 2 for gi, ci in zip(g, c)) < r * r] = i
    return y


def rename(y, rng, spread=7):
    """the same objects under permuted, non-sequential ids"""
    ids = np.unique(y[y > 0])
    lut = np.zeros(int(y.max()) + 1, np.int64)
    lut[ids] = rng.permutation(len(ids)) * spread + rng.randint(1, spread)
    return lut[y].astype(y.dtype)


def moving(seed, shape=(96, 128), n=60, frames=5):
    """frame k + 1 = frame k rolled by up to 3 px, one object dropped, ids permuted and spread"""
    rng = np.random.RandomState(100 + seed)
    ys = [discs(shape, n, seed)]
    for _ in range(frames - 1):
        y = np.roll(ys[-1], tuple(int(v) for v in rng.randint(-3, 4, len(shape))), axis=tuple(range(len(shape))))
        present = np.unique(y[y > 0])
        y = np.where(y == present[rng.randint(len(present))], 0, y)
        ys.append(rename(y, rng).astype(np.int32))
    return ys


def docstring_scene():
    from stardist_amd.data import test_image_nuclei_2d
    _y = test_image_nuclei_2d(return_mask=True)[1]
    return np.stack([_y, 2 * np.roll(_y, 10)], axis=0)


def with_background():
    """an all-background frame in the middle and at the end: the objects after the gap are all new"""
    ys = moving(11, frames=4)
    return [ys[0], ys[1], np.zeros_like(ys[0]), ys[2], ys[3], np.zeros_like(ys[0])]


def split_and_merge():
    """object 3 splits into 8 and 9 (unequal parts, each reaching outside the parent by a different amount), then 8, 9 and the neighbour 4
    merge into 5; discs move around them"""
    ys = []
    for k in range(3):
        y = np.roll(discs((80, 120), 25, 21), (k, 2 * k), axis=(0, 1)) * 10
        y[20:60, 30:100] = 0
        ys.append(y)
    ys[0][25:50, 40:70] = 3
    ys[0][30:48, 74:92] = 4
    ys[1][24:50, 39:52] = 8
    ys[1][27:52, 54:72] = 9
    ys[1][31:48, 75:93] = 4
    ys[2][26:49, 41:90] = 5
    return ys


def volumes():
    return moving(32, shape=(20, 40, 48), n=30, frames=3)


def big_ids():
    """frame 0 carries ids just below 2**31 - 1 (the fresh ids that follow still fit int32); an int64 stack"""
    ys = moving(41, shape=(64, 80), n=20, frames=3)
    first = np.where(ys[0] > 0, 2 ** 31 - 1 - 100 - 3 * ys[0].astype(np.int64), 0)
    return np.stack([first] + [y.astype(np.int64) for y in ys[1:]])


def scenes():
    """name -> stack (ndarray) or list of frames"""
    out = {"docstring": docstring_scene(), "background": with_background(), "split_merge": split_and_merge(), "volumes": volumes(),
           "big_ids": big_ids()}
    for seed in range(6):
        ys = moving(seed)
        out["moving%d" % seed] = ys if seed % 2 else np.stack(ys)                   # list and ndarray input
    out["moving_uint16"] = [y.astype(np.uint16) for y in moving(8)]
    out["moving_int64"] = np.stack(moving(7)).astype(np.int64)
    return out


def compose(ys, thresh, criterion):
    """group_matching_labels from sparse_overlap lists of the raw frames, all on the host: independent of both kernels"""
    from stardist_amd import matching_sparse as S
    lists = [S.sparse_overlap(a, b) for a, b in zip(ys[:-1], ys[1:])]
    return S.lookup_tables(ys, S.group_tables_from_overlaps(lists, int(np.max(ys[0])), thresh, criterion))


def _timing_tool():
    """tools/time_group_matching.py as a module: the timing scene has one definition, the tool's"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "time_group_matching.py")
    spec = importlib.util.spec_from_file_location("_time_group_matching", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def lattice_stack(frames=8, size=2048):
    """the scene of tools/time_group_matching.py, from the tool's own generator: `frames` frames of size^2 lattice discs (at 2048: the first
    12 756 of the lattice's 14 161), each frame the one before shifted by 1-2 px with 5 objects removed"""
    return _timing_tool().lattice_stack(frames, size)
