"""Scenes for fill_label_holes, shared by tests/test_cpu_fill_holes.py (host harness of csrc/fill_holes.h) and
tests/test_gpu_fill_holes.py (the kernels): deterministic by seed, small, int32 unless a case says otherwise.  The reference of every
comparison is stardist_amd.utils.fill_label_holes on the numpy array; `expected(name, a)` computes it once per scene and keeps it."""
import itertools

import numpy as np

FH_LDS_WORDS = 16384                 # restated from csrc/fill_holes.h (test_cpu_fill_holes.py checks the header against it)
FH_WAVE_WORDS = 1024                 # likewise: planes up to this size go to single-wave workgroups
N_RANDOM = 40
WORD_WIDTHS = (31, 32, 33, 63, 64, 65, 97)

_expected = {}


def expected(name, a):
    """the host function's result for the scene `name` (read-only, computed once)"""
    got = _expected.get(name)
    if got is None:
        from stardist_amd.utils import fill_label_holes
        got = fill_label_holes(a)
        got.setflags(write=False)
        _expected[name] = got
    return got


def _dist(shape, centre):
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return np.sqrt(sum((g - c) ** 2 for g, c in zip(grids, centre)))


def random_scene(seed):
    """discs, rings / shells, peppered discs and cut-open rings, later objects painted over earlier ones (so objects sit in the holes of
    others); ids permuted with gaps; every fifth scene has one label negated; scenes 0-23 are 2D (up to 70 x 90), 24-39 3D (up to
    24 x 30 x 40), and some have an extent of 1"""
    rng = np.random.default_rng(1000 + seed)
    if seed < 24:
        shape = (int(rng.integers(20, 71)), int(rng.integers(20, 91)))
        if seed % 8 == 3:
            shape = (1, shape[1])
        if seed % 8 == 6:
            shape = (shape[0], 1)
    else:
        shape = (int(rng.integers(6, 25)), int(rng.integers(10, 31)), int(rng.integers(10, 41)))
        if seed % 8 == 3:
            shape = (1,) + shape[1:]
        if seed % 8 == 6:
            shape = shape[:2] + (1,)
    n_obj = int(rng.integers(3, 13))
    ids = rng.permutation(np.arange(1, 4 * n_obj + 1))[:n_obj]
    a = np.zeros(shape, np.int32)
    for lab in ids:
        centre = [rng.uniform(-1, n) for n in shape]
        r = rng.uniform(2.0, 0.45 * max(shape))
        d = _dist(shape, centre)
        kind = int(rng.integers(0, 4))
        if kind == 0:                                   # disc
            m = d <= r
        elif kind == 1:                                 # ring / shell
            m = (d <= r) & (d >= r - rng.uniform(1.0, 2.5))
        elif kind == 2:                                 # peppered disc
            m = (d <= r) & (rng.random(shape) > 0.12)
        else:                                           # ring cut open along the last axis
            m = (d <= r) & (d >= r - rng.uniform(1.0, 2.5))
            grids = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
            slit = grids[-1] > centre[-1]
            for g, c in zip(grids[:-1], centre[:-1]):
                slit &= np.abs(g - c) < 1.0
            m &= ~slit
        a[m] = lab
    if seed % 5 == 0:
        present = np.unique(a[a > 0])
        if len(present):
            a[a == present[len(present) // 2]] *= -1
    return a


def _ring(n, lo, hi, lab, a=None, centre=None):
    a = np.zeros((n, n), np.int32) if a is None else a
    d = _dist(a.shape, centre or ((n - 1) / 2.0,) * 2)
    a[(d <= hi) & (d >= lo)] = lab
    return a


def spiral(open_mouth, n=64, lab=4, offset=(3, 5)):
    """an n x n block of `lab` with a one-pixel spiral corridor of (n - 2) // 4 turns carved into it (walls one pixel thick), set at
    `offset` in an image a little larger; with open_mouth the corridor's outer end breaks through the block's first row"""
    b = np.full((n, n), lab, np.int32)
    o = 1
    while n - 1 - 2 * o >= 3:
        hi = n - 1 - o
        b[o, o:hi + 1] = 0
        b[hi, o:hi + 1] = 0
        b[o:hi + 1, o] = 0
        b[o:hi + 1, hi] = 0
        b[o + 1, o] = lab                               # the ring is cut below its first corner ...
        if n - 1 - 2 * (o + 2) >= 3:
            b[o + 2, o + 1] = 0                         # ... and its far end leads into the next ring
        o += 2
    if open_mouth:
        b[0, 1] = 0
    a = np.zeros((n + 6, n + 9), np.int32)
    a[offset[0]:offset[0] + n, offset[1]:offset[1] + n] = b
    return a


def hand_2d():
    """name -> scene"""
    out = {}
    for side in range(4):                               # cavity reaches a border: stays open
        a = _ring(21, 6.0, 8.5, 3, centre=[(4.0, 10.0), (16.0, 10.0), (10.0, 4.0), (10.0, 16.0)][side])
        out["cavity_reaches_border_%d" % side] = a
    a = np.zeros((12, 14), np.int32)                    # object on the border, cavity closed: filled
    a[0:7, 3:10] = 6
    a[1:5, 5:8] = 0
    out["ring_on_border_closed"] = a
    out["smaller_id_erased"] = np.array([[0, 0, 0, 0, 0, 0, 0], [0, 5, 5, 5, 5, 5, 0], [0, 5, 0, 2, 0, 5, 0], [0, 5, 5, 5, 5, 5, 0],
                                         [0, 0, 0, 0, 0, 0, 0]], np.int32)
    out["larger_id_kept"] = np.array([[0, 0, 0, 0, 0], [0, 1, 1, 1, 0], [0, 1, 7, 1, 0], [0, 1, 1, 1, 0], [0, 0, 0, 0, 0]], np.int32)
    for order in itertools.permutations((2, 5, 9)):
        a = np.zeros((41, 41), np.int32)
        for (lo, hi), lab in zip(((16.0, 18.5), (9.0, 11.5), (3.0, 5.5)), order):
            _ring(41, lo, hi, lab, a)
        out["concentric_%d%d%d" % order] = a
    a = np.zeros((9, 9), np.int32)                      # the cavity meets the outside only across a corner
    a[2:7, 2:7] = 8
    a[3:6, 3:6] = 0
    a[2, 2] = 0
    out["diagonal_leak"] = a
    a = np.zeros((210, 215), np.int32)                  # planes of 2 * 200 * 7 words: beyond FH_WAVE_WORDS, within FH_LDS_WORDS
    _ring(0, 92.0, 99.6, 30, a, centre=(104.5, 107.0))
    _ring(0, 20.0, 24.0, 12, a, centre=(80.0, 90.0))
    _ring(0, 6.0, 9.0, 45, a, centre=(130.0, 120.0))
    out["ring_200"] = a
    out["spiral_closed"] = spiral(False)
    out["spiral_open"] = spiral(True)
    return out


def word_boundary(width, leak, closed):
    """a 7-row block of label 3, `width` wide, starting at column 5: a chamber at one end and a one-pixel corridor along the middle row
    to the other end, where it leaves the block (leak 'right': chamber left, corridor open at the last column; 'left': mirrored) --
    or stops one pixel short (closed)"""
    b = np.full((7, width), 3, np.int32)
    b[2:5, 1:4] = 0
    b[3, 1:width - 1] = 0
    if not closed:
        b[3, width - 1] = 0
    if leak == "left":
        b = b[:, ::-1]
    a = np.zeros((11, width + 9), np.int32)
    a[2:9, 5:5 + width] = b
    return a


def word_boundary_cases():
    return {"words_%d_%s_%s" % (w, leak, "closed" if closed else "open"): word_boundary(w, leak, closed)
            for w in WORD_WIDTHS for leak in ("left", "right") for closed in (False, True)}


def _cube_shell(shape=(11, 12, 13), lo=2, hi=8, lab=5):
    a = np.zeros(shape, np.int32)
    a[lo:hi + 1, lo:hi + 1, lo:hi + 1] = lab
    a[lo + 1:hi, lo + 1:hi, lo + 1:hi] = 0
    return a


def volumes():
    out = {}
    shape = (16, 18, 20)
    d = _dist(shape, (7.5, 8.5, 9.5))
    a = np.zeros(shape, np.int32)
    a[(d <= 6.0) & (d >= 4.0)] = 3
    a[(d <= 1.5)] = 2                                   # a smaller id inside the cavity
    out["shell_closed"] = a
    for axis in range(3):
        for far in (False, True):
            c = [7.5, 8.5, 9.5]
            c[axis] = shape[axis] - 1 - 1.0 if far else 1.0
            d = _dist(shape, c)
            a = np.zeros(shape, np.int32)
            a[(d <= 6.0) & (d >= 4.0)] = 3
            out["shell_cut_axis%d_%s" % (axis, "far" if far else "near")] = a
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in (9, 24, 24)], indexing="ij")
    a = np.zeros((9, 24, 24), np.int32)
    a[(np.sqrt((y - 11.5) ** 2 + (x - 11.5) ** 2) - 7.0) ** 2 + (z - 4.0) ** 2 <= 2.5 ** 2] = 4
    out["torus"] = a
    a = _cube_shell()
    a[2, 5, 5] = 0
    out["shell_pinhole"] = a
    a = _cube_shell()
    a[2, 2, 5] = 0                                      # a voxel of an edge: the cavity meets the outside only diagonally
    out["shell_diagonal_leak"] = a
    return out


def budget_scene(opened):
    """a ring whose 520-row, 17-word box needs 2 * 520 * 17 = 17680 words, just over FH_LDS_WORDS; small objects inside and around"""
    a = np.zeros((520, 530), np.int32)
    d = _dist(a.shape, (259.5, 264.5))
    a[(d <= 259.9) & (d >= 250.0)] = 60
    if opened:
        a[258:261, 264:] = np.where(a[258:261, 264:] == 60, 0, a[258:261, 264:])
    rng = np.random.default_rng(7)
    for k in range(30):
        cy, cx = rng.uniform(5, 515), rng.uniform(5, 525)
        r = rng.uniform(3, 12)
        dd = _dist(a.shape, (cy, cx))
        m = (dd <= r) & (dd >= r - 2.0) & (a == 0)
        a[m] = 1 + 3 * k if k % 2 else 41 + 3 * k
    return a


def many_objects(seed=3):
    """about 6000 labels of 1 to 9 pixels on a 3 x 3 grid of cells in 256 x 256, every sixth a full ring with a one-pixel hole"""
    rng = np.random.default_rng(seed)
    a = np.zeros((256, 256), np.int32)
    cells = [(i, j) for i in range(85) for j in range(85)]
    pick = rng.permutation(len(cells))[:6000]
    ids = rng.permutation(np.arange(1, 9001))[:6000]
    for k, (c, lab) in enumerate(zip(pick, ids)):
        i, j = cells[c]
        if k % 6 == 0:
            m = np.ones((3, 3), bool)
            m[1, 1] = False
        else:
            m = rng.random((3, 3)) < 0.6
            m[int(rng.integers(0, 3)), int(rng.integers(0, 3))] = True
        a[3 * i:3 * i + 3, 3 * j:3 * j + 3][m] = lab
    return a


def all_int32_scenes():
    """name -> scene, everything above but the budget scenes (which the callers take on their own: they are the large ones)"""
    out = {"random_%02d" % s: random_scene(s) for s in range(N_RANDOM)}
    out.update(hand_2d())
    out.update(word_boundary_cases())
    out.update(volumes())
    out["many_objects"] = many_objects()
    return out
