"""Cases of stardist_amd.augment, shared by tests/test_cpu_augment.py (the host harness of csrc/augment.h) and
tests/test_gpu_augment.py (the kernel).  A case is a batch: inputs (B, *shape), one params dict per sample, all different.

    NAMES               every case, '<shape>-<what>'
    case(name)          (x float32 (B, *shape), y int32 (B, *shape), params_list), read-only
    reference(name)     (x', y') = Compose.apply_host per sample, stacked; computed once
    packed(name)        (flags, table, disp) as sd_augment_batch_device takes them: Compose.table and the control grids zoomed on the host
    same(a, b)          equal, NaN matching NaN by position
    constant_warp(name) / has_warp(name)
    inside_fraction(name)   share of the batch's output pixels whose coordinates lie inside the patch on every axis
"""
import functools
import math

import numpy as np

from stardist_amd import augment as A

B = 3
SHAPES = [(5, 7), (33, 33), (32, 48), (1, 8), (4, 6, 6), (3, 8, 8)]
TRAINING_SHAPE = (256, 256)              # with B = 4


def _tag(shape):
    return "x".join(str(n) for n in shape)


def _inputs(shape, n, hard, seed):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1, 2, size=(n,) + shape).astype(np.float32)
    # labels: blocks of 2 - 3 pixels with many ids, a fifth of them background
    idx = np.indices(shape)
    blocks = sum((idx[d] // (2 + d % 2)) * (7 ** d) for d in range(len(shape)))
    y = np.stack([np.where((blocks + b) % 5 == 0, 0, blocks * 3 + b + 1) for b in range(n)]).astype(np.int32)
    if hard:
        flat = x.reshape(n, -1)
        for b in range(n):
            pos = rng.choice(flat.shape[1], size=min(4, flat.shape[1]), replace=False)
            flat[b, pos] = [np.inf, -np.inf, np.nan, np.inf][:len(pos)]
        y = np.where(y % 4 == 1, -y, y)
        y = np.where(y % 4 == 2, 2 ** 31 - 1 - y, y).astype(np.int32)
    return x, y


def _flip(shape, b):
    nd = len(shape)
    a0, a1 = nd - 2, nd - 1
    perm, flip = list(range(nd)), [False] * nd
    if shape[a0] == shape[a1] and b > 0:
        perm[a0], perm[a1] = a1, a0
    flip[a0], flip[a1] = b in (0, 2), b in (1, 2)
    return {"perm": tuple(perm), "flip": tuple(flip)}


def _matrix(shape, angle, zoom):
    nd = len(shape)
    a0, a1 = nd - 2, nd - 1
    M = np.eye(nd)
    cs, sn = math.cos(angle) / zoom, math.sin(angle) / zoom
    M[a0, a0], M[a0, a1], M[a1, a0], M[a1, a1] = cs, -sn, sn, cs
    return M


def _grid(shape, amount, seed):
    nd = len(shape)
    rng = np.random.RandomState(seed)
    gshape = tuple(5 if d >= nd - 2 else 1 for d in range(nd))
    grid = (amount * rng.uniform(-1, 1, size=(2,) + gshape)).astype(np.float32)
    if shape[nd - 2] == 1:
        grid[0] = 0                                             # an axis of extent 1: any displacement leaves it in constant mode
    return grid


def _warp(shape, mode, M=None, o=None, shift=None, grid=None):
    nd = len(shape)
    M = np.eye(nd) if M is None else M
    o = A.Warp.offset(M, shape) if o is None else np.asarray(o, np.float64)
    if shift is not None:
        o = o + np.asarray(shift, np.float64)
    return {"M": M, "o": o, "grid": grid, "axes": (nd - 2, nd - 1), "mode": mode}


def _intensity(b):
    return {"scale": np.float32([0.6, 1.37, 2.0][b % 3]), "shift": np.float32([-0.2, 0.013, 0.2][b % 3])}


def _noise(b, seed):
    rng = np.random.RandomState(seed)
    return {"sigma": np.float32([0.5, 0.02, 0.0][b % 3]), "key": tuple(int(v) for v in rng.randint(0, 2 ** 32, size=2, dtype=np.uint64)),
            "sample": b}


def _warps(shape, seed):
    """the Warp cases of one shape: name -> (mode, [params of sample b])"""
    nd = len(shape)
    n = np.array(shape, np.float64)
    flat = shape[nd - 2] == 1                                   # an axis of extent 1: any rotation leaves it in constant mode
    angles = [0.0, 0.0, 0.0] if flat else [0.3, -1.2, 2.5]
    zooms = [1.3, 0.7, 0.9]
    plane = np.array([0.0] * (nd - 2) + [0.0 if flat else 1.0, 1.0])    # the axes the offsets of the cases below move along
    out = {}
    for mode in ("reflect", "constant"):
        out["rot-" + mode] = (mode, [_warp(shape, mode, _matrix(shape, angles[b], zooms[b])) for b in range(B)])
        # identity, coordinates exactly on the edges: -0.5, 0, n - 1, n - 0.5
        out["edges_a-" + mode] = (mode, [_warp(shape, mode, o=v) for v in (-0.5 * plane, 0 * n, (n - 1) * plane)])
        out["edges_b-" + mode] = (mode, [_warp(shape, mode, o=v) for v in ((n - 0.5) * plane, 0.5 * plane, 0 * n)])
        # most of the patch leaves: a rotation about a corner (a shift along the long axis for the flat shape)
        far = [_warp(shape, mode, _matrix(shape, 0.0 if flat else 0.5 + 0.2 * b, 1.0), shift=(0.26 + 0.03 * b) * n * plane) for b in range(B)]
        out["far-" + mode] = (mode, far)
        out["elastic-" + mode] = (mode, [_warp(shape, mode, grid=_grid(shape, 3.0, seed + b)) for b in range(B)])
        out["elastic_affine-" + mode] = (mode, [_warp(shape, mode, _matrix(shape, angles[b] / 2, 0.8 + 0.1 * b), grid=_grid(shape, 2.0, seed + 10 + b))
                                                for b in range(B)])
    # several periods away
    out["periods-reflect"] = ("reflect", [_warp(shape, "reflect", shift=v) for v in (5 * n, -5 * n, (5 * n + 0.25) * plane)])
    return out


def _build():
    cases = {}
    for k, shape in enumerate(SHAPES):
        tag, seed = _tag(shape), 100 * k
        plain, hard = _inputs(shape, B, False, seed), _inputs(shape, B, True, seed + 1)
        flips = [_flip(shape, b) for b in range(B)]
        cases[tag + "-flip"] = plain + ([{"flip": f} for f in flips],)
        cases[tag + "-flip-hard"] = hard + ([{"flip": f} for f in flips],)
        if shape == (32, 48):                                   # flips only: the extents differ
            continue
        cases[tag + "-intensity"] = hard + ([{"intensity": _intensity(b)} for b in range(B)],)
        cases[tag + "-noise"] = plain + ([{"noise": _noise(b, seed + b)} for b in range(B)],)
        warps = _warps(shape, seed)
        for name, (mode, ws) in warps.items():
            cases["%s-warp-%s" % (tag, name)] = plain + ([{"warp": w} for w in ws],)
        for name in ("edges_a-constant", "edges_b-constant", "edges_a-reflect", "rot-reflect"):
            cases["%s-warp-%s-hard" % (tag, name)] = hard + ([{"warp": w} for w in warps[name][1]],)
        for mode in ("reflect", "constant"):
            ws = warps["elastic_affine-" + mode][1]
            chain = [{"flip": flips[b], "warp": ws[b], "intensity": _intensity(b), "noise": _noise(b + 1, seed + 5 + b)} for b in range(B)]
            cases["%s-chain-%s" % (tag, mode)] = plain + (chain,)
            cases["%s-chain-%s-hard" % (tag, mode)] = hard + (chain,)
    # the training size
    shape = TRAINING_SHAPE
    aug = A.Compose([A.FlipRot90(), A.Warp(elastic_grid=5, elastic_amount=4.0), A.IntensityScaleShift(), A.AdditiveNoise()])
    state = np.random.get_state()                               # drawn as training draws, without touching the caller's stream
    np.random.seed(7)
    cases[_tag(shape) + "-chain-training"] = _inputs(shape, 4, False, 999) + ([aug.draw(shape) for _ in range(4)],)
    np.random.set_state(state)
    for x, y, _ in cases.values():
        x.setflags(write=False)
        y.setflags(write=False)
    return cases


_CASES = _build()
NAMES = list(_CASES)


def case(name):
    return _CASES[name]


def has_warp(name):
    return "warp" in _CASES[name][2][0]


def constant_warp(name):
    return has_warp(name) and _CASES[name][2][0]["warp"]["mode"] == "constant"


@functools.lru_cache(maxsize=None)
def reference(name):
    x, y, params = case(name)
    outs = [A.Compose.apply_host(x[b], y[b], params[b]) for b in range(len(params))]
    rx, ry = np.stack([np.asarray(o[0], np.float32) for o in outs]), np.stack([np.asarray(o[1], np.int32) for o in outs])
    rx.setflags(write=False)
    ry.setflags(write=False)
    return rx, ry


@functools.lru_cache(maxsize=None)
def packed(name):
    from stardist_amd.utils import zoom_linear
    x, y, params = case(name)
    shape = x.shape[1:]
    flags, tab, grids = A.Compose.table(params, shape)
    disp = None
    if grids is not None:
        zoom = A.Warp.zoom_factors(grids.shape[2:], shape)
        disp = np.ascontiguousarray(np.stack([zoom_linear(g, zoom) for g in grids]), np.float32)
        assert disp.shape == (len(params), 2) + shape
    return flags, tab, disp


def inside_fraction(name):
    x, y, params = case(name)
    shape = x.shape[1:]
    inside = 0
    for p in params:
        c = A.Warp.coordinates(p["warp"], shape)
        ok = np.ones(shape, bool)
        for d, n in enumerate(shape):
            ok &= (c[d] >= 0) & (c[d] <= n - 1)
        inside += int(ok.sum())
    return inside / float(x.size)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]))
