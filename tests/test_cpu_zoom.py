"""CPU: the arithmetic of the device zoom (csrc/zoom_linear.h through tests/host/zoom_check.cpp, with the tables of
stardist_amd.utils._zoom_axis_table) against scipy.ndimage.zoom(order=1) bit for bit; zoom_linear on host input; and the routing of
predict_instances(scale=) on a CPU model.

Three things scipy does that a plain "floor, 1 - x, x" interpolation does not, each pinned below:
  * the second weight is 1 - (1 - x), not x (test_second_weight_is_one_minus_the_first);
  * (m - 1) * ((n - 1) / (m - 1)) can round past n - 1, and scipy then writes 0 for the last index (test_coordinate_rounded_past_the_edge);
  * at the far edge scipy reads the mirrored sample with weight 0, so a non-finite pixel there spreads (test_non_finite_pixels_spread_as_in_scipy)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from scipy.ndimage import zoom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}

F2 = (0.25, 0.5, 1 / 3, 1.5, 2.0, 3.0, (0.73, 1.31))
FLOAT_CASES = [((37, 53), f) for f in F2] + [((64, 64), f) for f in F2] + \
              [((1, 40), f) for f in (2.0, 3.0, (1, 0.5), (1, 1 / 3), (1.0, 1.31))] + \
              [((9, 17, 13), f) for f in (0.25, 0.5, 1 / 3, 2.0, 3.0, (2.2, 0.5, 0.5))]
INT_CASES = [((37, 53), 0.5), ((37, 53), 2.0), ((37, 53), 1 / 3), ((37, 53), (0.73, 1.31)), ((9, 17, 13), 0.5),
             ((9, 17, 13), (2.2, 0.5, 0.5)), ((20, 24, 3), (0.5, 1.5, 1)), ((64, 64), 3.0)]
RANGES = {"unit": (0.0, 1.0), "signed": (-1000.0, 1000.0), "counts": (0.0, 65535.0)}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("zoomlin") / "libzoomlin.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                    os.path.join(ROOT, "tests", "host", "zoom_check.cpp"), "-o", so], check=True)
    l = ctypes.CDLL(so)
    l.zl_zoom.restype = ctypes.c_int
    l.zl_zoom.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int]
    return l


def harness_zoom(lib, a, factors, wide=0):
    """the shipped arithmetic on a host array: tables from the product's builder, elements from the shared header"""
    from stardist_amd.utils import _zoom_axis_table, _zoom_out_shape
    out_shape = _zoom_out_shape(a.shape, factors)
    assert out_shape is not None
    tabs = [_zoom_axis_table(n, m) for n, m in zip(a.shape, out_shape)]
    i0, w0, w1 = (np.ascontiguousarray(np.concatenate([t[j] for t in tabs])) for j in range(3))
    assert i0.dtype == np.int32 and w0.dtype == np.float64 and w1.dtype == np.float64
    a = np.ascontiguousarray(a)
    out = np.empty(out_shape, a.dtype)
    ins, outs = np.asarray(a.shape, np.int32), np.asarray(out_shape, np.int32)
    rc = lib.zl_zoom(a.ctypes.data, out.ctypes.data, DT[a.dtype], a.ndim, ins.ctypes.data, outs.ctypes.data, i0.ctypes.data,
                     w0.ctypes.data, w1.ctypes.data, wide)
    assert rc == 0
    return out


def same_bits(got, want):
    """equal shapes, dtypes and bits; a NaN matches a NaN (its sign and payload depend on the machine that made it)"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype != np.float32:
        return np.array_equal(got, want)
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn])


def data(shape, lo, hi, seed):
    return (np.random.default_rng(seed).random(shape) * (hi - lo) + lo).astype(np.float32)


@pytest.mark.parametrize("rng_name", sorted(RANGES))
def test_harness_equals_scipy_float32(lib, rng_name):
    lo, hi = RANGES[rng_name]
    for k, (shape, f) in enumerate(FLOAT_CASES):
        a = data(shape, lo, hi, k)
        want = zoom(a, f, order=1)
        assert np.isfinite(want).all()
        assert same_bits(harness_zoom(lib, a, f), want), (shape, f)
    assert same_bits(harness_zoom(lib, data((37, 53), lo, hi, 99), (0.73, 1.31), wide=1), zoom(data((37, 53), lo, hi, 99), (0.73, 1.31), order=1))


def test_harness_equals_scipy_channels(lib):
    a = data((20, 24, 3), -5.0, 5.0, 7)
    assert same_bits(harness_zoom(lib, a, (0.5, 1.5, 1)), zoom(a, (0.5, 1.5, 1), order=1))
    b = np.ascontiguousarray(np.moveaxis(a, -1, 0))
    assert same_bits(harness_zoom(lib, b, (1, 0.5, 1.5)), zoom(b, (1, 0.5, 1.5), order=1))
    c = data((2, 5, 6, 3), 0.0, 1.0, 8)                                    # rank 4: a 3D image with channels
    assert same_bits(harness_zoom(lib, c, (2.0, 0.6, 1.5, 1)), zoom(c, (2.0, 0.6, 1.5, 1), order=1))
    d = data((17,), 0.0, 1.0, 9)
    assert same_bits(harness_zoom(lib, d, 2.5), zoom(d, 2.5, order=1))


@pytest.mark.parametrize("dtype", (np.uint8, np.uint16))
def test_harness_equals_scipy_integers(lib, dtype):
    top = np.iinfo(dtype).max
    for k, (shape, f) in enumerate(INT_CASES):
        a = np.random.default_rng(k).integers(0, top + 1, shape).astype(dtype)
        a.flat[0], a.flat[-1] = 0, top
        assert same_bits(harness_zoom(lib, a, f), zoom(a, f, order=1)), (shape, f)
    # 0 and the maximum only: sums that land on k + 0.5 and on the maximum itself
    b = (np.random.default_rng(5).integers(0, 2, (37, 53)) * top).astype(dtype)
    for f in (0.5, 2.0, (0.73, 1.31)):
        assert same_bits(harness_zoom(lib, b, f), zoom(b, f, order=1)), f


def test_output_extent_one_and_half_way_extents(lib):
    a = data((3, 40), 0.0, 1.0, 1)
    got = harness_zoom(lib, a, (0.3, 1))                                   # round(0.9) = 1 row: ratio 1, the first source row
    assert got.shape == (1, 40) and same_bits(got, zoom(a, (0.3, 1), order=1))
    b = data((5, 7), 0.0, 1.0, 2)
    got = harness_zoom(lib, b, 0.5)                                        # 2.5 -> 2 and 3.5 -> 4: Python's round, halves to even
    assert got.shape == (2, 4) and same_bits(got, zoom(b, 0.5, order=1))


def test_second_weight_is_one_minus_the_first(lib):
    """3 -> 141 rows: x = 1/70 and the like, where 1 - (1 - x) != x in float64 and the float32 result shows it"""
    from stardist_amd.utils import _zoom_axis_table
    i0, w0, w1 = _zoom_axis_table(3, 141)
    cc = np.arange(141, dtype=np.float64) * (np.float64(2) / np.float64(140))
    assert np.array_equal(w1, 1.0 - w0) and not np.array_equal(w1, cc - np.floor(cc))
    a = data((3, 40), 0.0, 100.0, 3)
    assert same_bits(harness_zoom(lib, a, (47.0, 1.0)), zoom(a, (47.0, 1.0), order=1))


def test_coordinate_rounded_past_the_edge(lib):
    """4 -> 188 samples: 187 * (3 / 187) > 3 in float64; scipy takes the last coordinate for outside the array and writes 0"""
    from stardist_amd.utils import _zoom_axis_table
    pairs = [(n, m) for n in range(2, 40) for m in range(2, 400) if np.float64(m - 1) * (np.float64(n - 1) / np.float64(m - 1)) > n - 1]
    assert (4, 188) in pairs
    for n, m in pairs[:3] + pairs[-3:]:
        i0 = _zoom_axis_table(n, m)[0]
        assert i0[-1] == -1 and (i0[:-1] >= 0).all() and i0[:-1].max() <= n - 1
        a = data((n, 3), 1.0, 2.0, n * m)
        f = (m / n, 1)
        want = zoom(a, f, order=1)
        assert want.shape == (m, 3) and (want[-1] == 0).all() and (want[:-1] > 0).all()
        assert same_bits(harness_zoom(lib, a, f), want), (n, m)
        u = (a * 100).astype(np.uint8)
        assert same_bits(harness_zoom(lib, u, f), zoom(u, f, order=1)), (n, m)


def test_non_finite_pixels_spread_as_in_scipy(lib):
    """an inf or NaN makes NaN of every output that reads it with weight 0: along an axis of factor 1 (scipy interpolates there too) and,
    at the far edge, through the mirrored sample n - 2"""
    a = data((20, 24, 3), 0.0, 1.0, 4)
    a[4, 6, 1] = np.inf
    a[11, 2, 0] = np.nan
    with np.errstate(invalid="ignore"):
        want = zoom(a, (0.5, 1.5, 1), order=1)
    assert np.isnan(want[2, 9, 2])                                          # channel 2 reads channel 1 as its mirrored neighbour
    assert same_bits(harness_zoom(lib, a, (0.5, 1.5, 1)), want)
    rng = np.random.default_rng(11)
    for shape, f in (((37, 53), 0.5), ((37, 53), (0.73, 1.31)), ((9, 17, 13), (2.2, 0.5, 0.5)), ((5, 9), (1, 1)), ((3, 20, 24), (1, 2.0, 1 / 3))):
        b = data(shape, -1.0, 1.0, 5)
        for _ in range(6):
            at = tuple(int(rng.integers(0, n)) if rng.random() < 0.5 else int(rng.choice([0, n - 1, max(n - 2, 0)])) for n in shape)
            b[at] = rng.choice([np.inf, -np.inf, np.nan])
        with np.errstate(invalid="ignore"):
            want = zoom(b, f, order=1)
        assert same_bits(harness_zoom(lib, b, f), want), (shape, f)


def test_out_shape_is_scipys_or_none():
    from stardist_amd.utils import _zoom_out_shape
    for shape, f in FLOAT_CASES + [((5, 7), 0.5), ((3, 40), (0.3, 1)), ((7, 9), np.float64(1.5)), ((7, 9), (2, np.int64(3)))]:
        assert _zoom_out_shape(shape, f) == zoom(np.zeros(shape, np.uint8), f, order=0).shape
    assert _zoom_out_shape((1, 40), 0.25) is None                           # empty output
    assert _zoom_out_shape((4, 4), (2.0,)) is None and _zoom_out_shape((4, 4), "2") is None
    assert _zoom_out_shape((4, 4), np.float32(0.3)) is None                 # n * float32 rounds in float32: scipy's business
    assert _zoom_out_shape((2,) * 5, 2.0) is None and _zoom_out_shape((4, 4), float("nan")) is None


def test_zoom_linear_on_host_input_is_scipy(monkeypatch):
    import torch
    from scipy import ndimage
    from stardist_amd.utils import zoom_linear
    a = data((20, 24, 3), 0.0, 1.0, 6)
    got = zoom_linear(a, (0.5, 1.5, 1))
    assert isinstance(got, np.ndarray) and same_bits(got, zoom(a, (0.5, 1.5, 1), order=1))
    calls = []
    real = ndimage.zoom
    monkeypatch.setattr(ndimage, "zoom", lambda x, z, **kw: calls.append((x.dtype, kw)) or real(x, z, **kw))
    for x in (a.astype(np.float64), a.astype(np.int32), (a * 255).astype(np.uint8)):
        got = zoom_linear(x, 2.0)
        assert got.dtype == x.dtype and np.array_equal(got, real(x, 2.0, order=1))
    # tensors the kernel does not serve (here: host tensors, of a served and of an unserved dtype) take scipy and come back as tensors
    for x in (a, a.astype(np.float64)):
        got = zoom_linear(torch.from_numpy(x), (0.5, 1.5, 1))
        assert isinstance(got, torch.Tensor) and got.device.type == "cpu" and np.array_equal(got.numpy(), real(x, (0.5, 1.5, 1), order=1))
    assert len(calls) == 5 and all(kw == dict(order=1) for _, kw in calls)


def test_empty_output_is_left_to_scipy():
    """an output extent of 0 is scipy's to answer: its error where it raises one, its empty array where it does not (1.15 does not)"""
    import torch
    from stardist_amd.utils import zoom_linear
    a = np.zeros((1, 40), np.float32)
    try:
        want = zoom(a, 0.25, order=1)
    except Exception as e:                                                  # noqa: BLE001 -- whatever this scipy raises
        want = e
    for x in (a, torch.from_numpy(a)):
        if isinstance(want, Exception):
            with pytest.raises(type(want)) as got:
                zoom_linear(x, 0.25)
            assert str(got.value) == str(want)
        else:
            got = zoom_linear(x, 0.25)
            assert tuple(got.shape) == want.shape == (0, 10) and str(got.dtype).endswith("float32")
    with pytest.raises(RuntimeError):
        zoom_linear(a, (2.0,))                                              # scipy: sequence argument must have length equal to input rank


def test_cpu_model_still_calls_scipy(monkeypatch):
    from scipy import ndimage
    from stardist_amd.models import Config2D, StarDist2D
    m = StarDist2D(Config2D(n_rays=8, unet_n_depth=1, unet_n_filter_base=4, n_channel_in=2), basedir=None, device="cpu")
    img = np.random.RandomState(1).uniform(0, 1, (40, 56, 2)).astype(np.float32)
    seen, calls = {}, []
    real = ndimage.zoom

    def fake_sparse(x, **kw):
        seen["x"] = x
        yield (np.zeros(0, np.float32), np.zeros((0, 8), np.float32), np.zeros((0, 2), int))
    monkeypatch.setattr(m, "_predict_sparse_generator", fake_sparse)
    monkeypatch.setattr(m, "_instances_from_prediction", lambda shape, prob, dist, **kw: ("labels", {}))
    monkeypatch.setattr(ndimage, "zoom", lambda x, z, **kw: calls.append((z, kw)) or real(x, z, **kw))
    m.predict_instances(img, scale=(0.5, 1.5, 1))
    assert calls == [((0.5, 1.5, 1), dict(order=1))]
    assert isinstance(seen["x"], np.ndarray) and np.array_equal(seen["x"], real(img, (0.5, 1.5, 1), order=1))
    assert m._zoom_on_device(img) and m._zoom_on_device(img.astype(np.uint16)) and not m._zoom_on_device(img.astype(np.float64))
    assert not m._zoom_on_device(img.astype(">f4").astype(">u2")) and not m._zoom_on_device(img[None, None, None])
