"""CPU: stardist_amd.augment -- the Philox4x32-10 known answers (numpy form, a scalar form written here, the header's), the statistics
of the Irwin-Hall noise, the host route against numpy / scipy written out, the draw stream, a host build of csrc/augment.h
(tests/host/augment_check.cpp) against the host route on every case of tests/_augment_cases.py -- as a shared library and as a
stand-alone program under the address and undefined-behaviour sanitizers -- and the CPU fallback of TrainData2D / TrainData3D.
Every comparison is ==, NaN matching NaN by position."""
import ctypes
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import _augment_cases as C
from stardist_amd import augment as A

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "augment_check.cpp")

KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox_scalar(counter, key):
    """Philox4x32-10 on Python integers"""
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return tuple(c)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("augment") / "libaugment_check.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so], check=True)
    l = ctypes.CDLL(so)
    l.aug_batch.restype = l.aug_sample_bytes.restype = ctypes.c_int
    l.aug_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                            ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    l.aug_philox.argtypes = [ctypes.c_void_p] * 3
    return l


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def harness(lib, name):
    x, y, params = C.case(name)
    flags, tab, disp = C.packed(name)
    shape = (ctypes.c_int * 3)(*x.shape[1:])
    ox, oy = np.full(x.shape, -7, np.float32), np.full(y.shape, -7, np.int32)
    rc = lib.aug_batch(ptr(x), ptr(y), x.shape[0], x.ndim - 1, ctypes.cast(shape, ctypes.c_void_p), flags, ptr(tab), ptr(disp),
                       0 if disp is None else disp.shape[1], ptr(ox), ptr(oy))
    return rc, ox, oy


# ---- the generator ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter, key, want", KNOWN)
def test_philox_known_answers_numpy_and_scalar(counter, key, want):
    assert philox_scalar(counter, key) == want
    assert tuple(int(w) for w in A.philox4x32_10(counter, key)) == want
    # vectorised: the same block among others
    ctr = [np.array([1, c, 2], np.uint64) for c in counter]
    out = A.philox4x32_10(ctr, key)
    assert tuple(int(w[1]) for w in out) == want and out[0].dtype == np.uint32


@pytest.mark.parametrize("counter, key, want", KNOWN)
def test_philox_known_answers_header(lib, counter, key, want):
    c, k, out = np.array(counter, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
    lib.aug_philox(ptr(c), ptr(k), ptr(out))
    assert tuple(int(w) for w in out) == want


def test_numpy_philox_equals_scalar_on_random_blocks():
    rng = np.random.RandomState(3)
    ctr = rng.randint(0, 2 ** 32, size=(4, 64), dtype=np.uint64)
    key = tuple(int(v) for v in rng.randint(0, 2 ** 32, size=2, dtype=np.uint64))
    out = A.philox4x32_10(list(ctr), key)
    for j in range(64):
        assert tuple(int(w[j]) for w in out) == philox_scalar([int(v) for v in ctr[:, j]], key)


def test_noise_statistics():
    n = 2 ** 20
    g = A.irwin_hall_noise(n, (0x12345678, 0x9abcdef0), sample=1)
    assert g.dtype == np.float64 and np.array_equal(g * 2.0 ** 32, np.round(g * 2.0 ** 32))
    assert abs(g.mean()) <= 6 / math.sqrt(n)
    assert abs(g.var() - 1) <= 6 * math.sqrt(1.9 / n)             # kurtosis of 12 terms: 2.9
    assert np.all(np.abs(g) < 6)
    # another sample word, another key word: other noise
    assert not np.array_equal(g[:64], A.irwin_hall_noise(64, (0x12345678, 0x9abcdef0), sample=2))
    assert not np.array_equal(g[:64], A.irwin_hall_noise(64, (0x12345679, 0x9abcdef0), sample=1))
    # pixels past 2^32 use the high counter word
    far = A.irwin_hall_noise(4, (5, 6), first=2 ** 32)
    words = sum(sum(philox_scalar((0, 1, 0, blk), (5, 6))) for blk in range(3))
    assert far[0] == (words - (6 * 2 ** 32 - 6)) * 2.0 ** -32


# ---- the host route ------------------------------------------------------------------------------------------------------------------
def test_flip_rot90_is_transpose_and_flip():
    rng = np.random.RandomState(0)
    for shape in [(6, 6), (5, 7), (3, 4, 4), (3, 4, 5)]:
        x, y = rng.rand(*shape).astype(np.float32), rng.randint(0, 9, shape).astype(np.int32)
        seen = set()
        for seed in range(40):
            np.random.seed(seed)
            p = A.FlipRot90().draw(shape)
            seen.add((p["perm"], p["flip"]))
            gx, gy = A.FlipRot90.apply_host(x, y, p)
            flipped = tuple(d for d in range(len(shape)) if p["flip"][d])
            assert np.array_equal(gx, np.flip(np.transpose(x, p["perm"]), flipped)) and np.array_equal(gy, np.flip(np.transpose(y, p["perm"]), flipped))
            assert gx.shape == shape
            nd = len(shape)
            if shape[nd - 2] != shape[nd - 1]:
                assert p["perm"] == tuple(range(nd))
            assert all(not f for f in p["flip"][:nd - 2]) and p["perm"][:nd - 2] == tuple(range(nd - 2))      # the default plane
        assert len(seen) == (8 if shape[-1] == shape[-2] else 4)


@pytest.mark.parametrize("mode", ["reflect", "constant"])
@pytest.mark.parametrize("shape", [(9, 11), (4, 7, 6)])
def test_warp_apply_host_is_scipy_written_out(shape, mode):
    from scipy import ndimage
    rng = np.random.RandomState(1)
    x, y = rng.rand(*shape).astype(np.float32), rng.randint(0, 50, shape).astype(np.uint16)
    np.random.seed(5)
    w = A.Warp(elastic_grid=3, elastic_amount=1.5, mode=mode)
    p = w.draw(shape)
    nd = len(shape)
    a0, a1 = nd - 2, nd - 1
    # the matrix: a rotation and an isotropic zoom in the plane, identity elsewhere; o = centre - M centre
    sub = p["M"][np.ix_([a0, a1], [a0, a1])]
    zoom = 1 / math.sqrt(abs(np.linalg.det(sub)))
    assert 0.8 <= zoom <= 1.25 and np.allclose(sub @ sub.T * zoom ** 2, np.eye(2))
    assert np.array_equal(np.delete(np.delete(p["M"], [a0, a1], 0), [a0, a1], 1), np.eye(nd - 2))
    centre = (np.array(shape) - 1) / 2
    assert np.allclose(p["M"] @ centre + p["o"], centre, atol=1e-12)
    assert p["grid"].dtype == np.float32 and p["grid"].shape == (2,) + tuple(3 if d >= nd - 2 else 1 for d in range(nd))
    assert np.abs(p["grid"]).max() <= 1.5
    # the coordinates, one rounding per operation, and the two scipy calls
    disp = ndimage.zoom(p["grid"], (1.0,) + tuple(n / g for n, g in zip(shape, p["grid"].shape[1:])), order=1)
    assert disp.shape == (2,) + shape
    idx = np.indices(shape).astype(np.float64)
    coords = []
    for d in range(nd):
        c = p["o"][d] + p["M"][d][0] * idx[0]
        for e in range(1, nd):
            c = c + p["M"][d][e] * idx[e]
        if d >= nd - 2:
            c = c + disp[d - (nd - 2)].astype(np.float64)
        coords.append(c)
    gx, gy = w.apply_host(x, y, p)
    assert gx.dtype == np.float32 and gy.dtype == np.int32
    assert np.array_equal(gx, ndimage.map_coordinates(x, coords, output=np.float32, order=1, mode=mode, cval=0))
    assert np.array_equal(gy, ndimage.map_coordinates(y, coords, output=np.int32, order=0, mode=mode, cval=0))
    assert not np.array_equal(gx, x)


def test_warp_raises_where_the_control_grid_does_not_zoom_to_the_patch():
    assert A.Warp.zoom_factors((1, 5, 5), (4, 6, 6)) == (1.0, 4.0, 1.2, 1.2)
    with pytest.raises(ValueError):
        A.Warp.zoom_factors((5, 5), (5,))
    import stardist_amd.utils as U
    real = U._zoom_out_shape
    U._zoom_out_shape = lambda shape, zoom: tuple(n + 1 for n in real(shape, zoom))
    try:
        with pytest.raises(ValueError):
            A.Warp.zoom_factors((5, 5), (7, 9))
    finally:
        U._zoom_out_shape = real


def test_intensity_and_noise_arithmetic():
    rng = np.random.RandomState(2)
    x, y = rng.rand(6, 5).astype(np.float32), np.arange(30, dtype=np.int32).reshape(6, 5)
    p = {"scale": np.float32(1.37), "shift": np.float32(-0.11)}
    gx, gy = A.IntensityScaleShift.apply_host(x, y, p)
    want = np.array([np.float32(np.float32(v) * np.float32(1.37)) + np.float32(-0.11) for v in x.ravel()], np.float32).reshape(x.shape)
    assert gx.dtype == np.float32 and np.array_equal(gx, want) and gy is y
    q = {"sigma": np.float32(0.3), "key": (11, 12), "sample": 2}
    gx, gy = A.AdditiveNoise.apply_host(x, y, q)
    g = A.irwin_hall_noise(30, (11, 12), 2)
    want = np.array([np.float32(v) + np.float32(np.float32(0.3) * np.float32(n)) for v, n in zip(x.ravel(), g)], np.float32).reshape(x.shape)
    assert gx.dtype == np.float32 and np.array_equal(gx, want) and gy is y


def test_compose_order_and_errors():
    ops = [A.AdditiveNoise(), A.IntensityScaleShift(), A.Warp(), A.FlipRot90()]
    c = A.Compose(ops)
    assert [type(o) for o in c.ops] == [A.FlipRot90, A.Warp, A.IntensityScaleShift, A.AdditiveNoise]
    for op in ops:
        with pytest.raises(ValueError):
            A.Compose(ops + [type(op)()])
    with pytest.raises(ValueError):
        A.Compose([lambda x, y: (x, y)])
    # the chain is the four steps in that order
    rng = np.random.RandomState(4)
    x, y = rng.rand(8, 8).astype(np.float32), rng.randint(0, 9, (8, 8)).astype(np.int32)
    np.random.seed(1)
    p = c.draw(x.shape)
    assert list(p) == ["flip", "warp", "intensity", "noise"]
    wx, wy = A.FlipRot90.apply_host(x, y, p["flip"])
    wx, wy = A.Warp.apply_host(wx, wy, p["warp"])
    wx, _ = A.IntensityScaleShift.apply_host(wx, wy, p["intensity"])
    wx, _ = A.AdditiveNoise.apply_host(wx, wy, p["noise"])
    gx, gy = c.apply_host(x, y, p)
    assert np.array_equal(gx, wx) and np.array_equal(gy, wy)


OPS = {"flip": lambda: A.FlipRot90(), "warp": lambda: A.Warp(), "elastic": lambda: A.Warp(elastic_grid=4, elastic_amount=2.0),
       "intensity": lambda: A.IntensityScaleShift(), "noise": lambda: A.AdditiveNoise(),
       "chain": lambda: A.Compose([A.FlipRot90(), A.Warp(elastic_grid=4, elastic_amount=1.0), A.IntensityScaleShift(), A.AdditiveNoise()])}


@pytest.mark.parametrize("what", list(OPS))
def test_draw_stream(what):
    def state_after(fn, seed):
        np.random.seed(seed)
        fn()
        return np.random.get_state()

    def same_state(a, b):
        return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]

    aug = OPS[what]()
    for shape in [(8, 8), (8, 12), (4, 8, 8)]:
        x, y = np.zeros(shape, np.float32), np.zeros(shape, np.int32)
        for seed in range(5):
            assert same_state(state_after(lambda: aug(x, y), seed), state_after(lambda: aug.draw(shape), seed))
    # the number of draws: that of so many uniforms, whatever the extents and the values drawn
    count = {}
    for shape in [(8, 8), (8, 12), (20, 4), (4, 8, 8), (5, 8, 12)]:
        for seed in range(5):
            after = state_after(lambda: aug.draw(shape), seed)
            k = 0
            np.random.seed(seed)
            while not same_state(np.random.get_state(), after):
                np.random.uniform()
                k += 1
                assert k < 1000
            count.setdefault(len(shape), set()).add(k)
    assert all(len(v) == 1 for v in count.values())
    if what != "elastic" and what != "chain":
        assert count[2] == count[3]                  # the default plane has two axes in 2D and 3D; only a control grid's size is per nd


# ---- the header ------------------------------------------------------------------------------------------------------------------------
def test_table_row_layout(lib):
    assert lib.aug_sample_bytes() == A._SAMPLE_DTYPE.itemsize == 168


@pytest.mark.parametrize("name", C.NAMES)
def test_host_build_of_the_header_equals_apply_host(lib, name):
    rc, ox, oy = harness(lib, name)
    wx, wy = C.reference(name)
    assert rc == 0
    assert C.same(ox, wx), (np.argwhere(~((ox == wx) | (np.isnan(ox) & np.isnan(wx))))[:5])
    assert C.same(oy, wy)


@pytest.mark.parametrize("name", [n for n in C.NAMES if C.has_warp(n)])
def test_warp_cases_do_not_pass_trivially(name):
    x, y, params = C.case(name)
    wx, wy = C.reference(name)
    if C.constant_warp(name):
        inside = C.inside_fraction(name)
        assert inside >= 1 / 3 and 1 - inside >= 0.05, inside
    assert len(set(np.unique(wy).tolist()) - {0}) >= 3
    assert not C.same(wx, x)


def test_hard_cases_hold_what_they_should():
    for name in C.NAMES:
        x, y, _ = C.case(name)
        if name.endswith("-hard"):
            assert np.isnan(x).any() and np.isinf(x).any() and (y < 0).any() and (y > 2 ** 31 - 200).any()
            if "edges" in name and "1x8" not in name:
                assert np.isnan(C.reference(name)[0]).sum() > np.isnan(x).sum() - 3 * 1       # 0 * inf at a zero-weight neighbour
    assert any(p["noise"]["sigma"] == 0 for p in C.case("5x7-noise")[2])
    assert C.case("256x256-chain-training")[0].shape == (4, 256, 256)


def test_entry_checks_of_the_harness(lib):
    x, y, params = C.case("5x7-flip")
    flags, tab, _ = C.packed("5x7-flip")
    shape = (ctypes.c_int * 3)(5, 7, 0)
    ox, oy = np.zeros_like(x), np.zeros_like(y)

    def run(tab=tab, B=3, nd=2, shape=shape, flags=flags, n_disp=0, disp=None, ox=ox):
        return lib.aug_batch(ptr(x), ptr(y), B, nd, ctypes.cast(shape, ctypes.c_void_p), flags, ptr(tab), ptr(disp), n_disp, ptr(ox), ptr(oy))

    assert run() == 0
    for field, value in (("base", 35), ("base", -1), ("step", 8), ("comp", 0)):
        bad = tab.copy()
        bad[field][1] = value
        assert run(tab=bad) == -1, field
    assert run(B=0) == -1 and run(nd=4) == -1 and run(flags=16) == -1 and run(ox=x) == -1
    assert run(shape=(ctypes.c_int * 3)(5, 0, 0)) == -1
    assert run(n_disp=2, disp=np.zeros((3, 2, 5, 7), np.float32)) == -1          # a displacement field without a Warp


def test_stand_alone_sanitizer_build_passes_every_case(tmp_path):
    exe, cases = str(tmp_path / "augment_check"), str(tmp_path / "cases.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DAUGMENT_CHECK_MAIN", SRC, "-o", exe], check=True)
    with open(cases, "wb") as f:
        for name in C.NAMES:
            x, y, _ = C.case(name)
            flags, tab, disp = C.packed(name)
            wx, wy = C.reference(name)
            shape = tuple(x.shape[1:]) + (0,) * (4 - x.ndim)
            f.write(struct.pack("<7i", x.shape[0], x.ndim - 1, *shape, flags, 0 if disp is None else disp.shape[1]))
            f.write(tab.tobytes() + x.tobytes() + y.tobytes() + (b"" if disp is None else disp.tobytes()) + wx.tobytes() + wy.tobytes())
    r = subprocess.run([exe, cases], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d records, 0 bad" % len(C.NAMES) in r.stdout


# ---- training data -------------------------------------------------------------------------------------------------------------------------
def _dataset(shape, n=3, seed=0):
    rng = np.random.RandomState(seed)
    X = [rng.rand(*shape).astype(np.float32) for _ in range(n)]
    Y = [(rng.rand(*shape) * 6).astype(np.uint16) for _ in range(n)]
    return X, Y


@pytest.mark.parametrize("nd", [2, 3])
def test_cpu_device_falls_back_to_apply_host(nd):
    import torch
    from stardist_amd.training import TrainData2D
    from stardist_amd.training3d import TrainData3D
    aug = A.Compose([A.FlipRot90(), A.Warp(elastic_grid=4, elastic_amount=1.0), A.IntensityScaleShift(), A.AdditiveNoise()])
    if nd == 2:
        X, Y = _dataset((40, 40))
        make = lambda a: TrainData2D(X, Y, batch_size=2, n_rays=8, length=4, patch_size=(32, 32), grid=(2, 2), augmenter=a)
    else:
        from stardist_amd.rays3d import Rays_GoldenSpiral
        X, Y = _dataset((10, 20, 20))
        make = lambda a: TrainData3D(X, Y, batch_size=2, rays=Rays_GoldenSpiral(8), length=4, patch_size=(8, 16, 16), grid=(1, 2, 2), augmenter=a)
    capable, plain = make(aug), make(lambda x, y: aug(x, y))
    assert not capable.augments_on("cpu") and capable.augments_on("cuda:0") and not plain.augments_on("cuda:0")
    np.random.seed(11)
    got = [capable.patches(i, torch.device("cpu")) for i in range(2)]
    state = np.random.get_state()
    np.random.seed(11)
    want = [plain.patches(i, torch.device("cpu")) for i in range(2)]
    assert np.array_equal(state[1], np.random.get_state()[1]) and state[2] == np.random.get_state()[2]
    for (gx, gy), (wx, wy) in zip(got, want):
        assert gx.dtype == torch.float32 and gx.shape[0] == 2 and torch.equal(gx, wx)
        assert len(gy) == 2 and all(np.array_equal(a, b) for a, b in zip(gy, wy))
    # and it is augmented: not the patches of no augmenter
    np.random.seed(11)
    assert not torch.equal(make(None).patches(0, torch.device("cpu"))[0], want[0][0])


@pytest.mark.parametrize("nd", [2, 3])
def test_draw_only_draws_where_the_augmenter_is_called(nd):
    """sample(i, draw_only=True) leaves np.random where sample(i) leaves it, and its params applied on the host give sample(i)"""
    from stardist_amd.training import TrainData2D
    from stardist_amd.training3d import TrainData3D
    aug = A.Compose([A.FlipRot90(), A.Warp(elastic_grid=4, elastic_amount=1.0), A.IntensityScaleShift(), A.AdditiveNoise()])
    if nd == 2:
        X, Y = _dataset((40, 40))
        data = TrainData2D(X, Y, batch_size=2, n_rays=8, length=4, patch_size=(32, 32), augmenter=aug, foreground_prob=0.5)
    else:
        from stardist_amd.rays3d import Rays_GoldenSpiral
        X, Y = _dataset((10, 20, 20))
        data = TrainData3D(X, Y, batch_size=2, rays=Rays_GoldenSpiral(8), length=4, patch_size=(8, 16, 16), augmenter=aug, foreground_prob=0.5)
    np.random.seed(3)
    want = [data.sample(i) for i in range(3)]
    state = np.random.get_state()
    data.index_map.clear()
    np.random.seed(3)
    for i in range(3):
        Xr, Yr, params = data.sample(i, draw_only=True)
        for b in range(2):
            gx, gy = aug.apply_host(Xr[b], Yr[b], params[b])
            assert np.array_equal(gx, want[i][0][b]) and np.array_equal(gy, want[i][1][b])
    assert np.array_equal(state[1], np.random.get_state()[1]) and state[2] == np.random.get_state()[2]
