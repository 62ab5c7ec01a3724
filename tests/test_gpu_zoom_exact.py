"""GPU: stardist_amd.utils.zoom_linear (csrc/zoom.hip) against scipy.ndimage.zoom(order=1), computed on this machine, bit for bit; and
predict_instances(scale=) / predict_instances_iter(scale=) on the device path against the host path, with scipy's zoom made to raise.

The arithmetic itself is compared with scipy on the CPU as well (tests/test_cpu_zoom.py, through the shared header)."""
import os
import sys

import numpy as np
import pytest
from scipy.ndimage import zoom

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(got, want):
    """equal shapes, dtypes and bits; a NaN matches a NaN (its sign and payload depend on the machine that made it)"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype != np.float32:
        return np.array_equal(got, want)
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn])


def data(shape, seed, lo=-100.0, hi=1000.0):
    return (np.random.default_rng(seed).random(shape) * (hi - lo) + lo).astype(np.float32)


def device_zoom(a, f):
    import torch
    from stardist_amd.utils import zoom_linear
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    out = zoom_linear(t, f)
    assert out.is_cuda and out.dtype == t.dtype and out.is_contiguous()
    return out.cpu().numpy()


CASES = [((37, 53), 0.5), ((37, 53), 2.0), ((37, 53), 1 / 3), ((37, 53), (0.73, 1.31)),
         ((9, 17, 13), 0.5), ((9, 17, 13), (2.2, 0.5, 0.5)),
         ((20, 24, 3), (0.5, 1.5, 1)), ((3, 20, 24), (1, 0.5, 1.5)),
         ((3, 40), (0.3, 1)),                      # output extent 1
         ((5, 7), 0.5),                            # 2.5 -> 2, 3.5 -> 4
         ((3, 40), (47.0, 1.0)),                   # weights where 1 - (1 - x) != x
         ((4, 3), (47.0, 1)),                      # 4 -> 188: the last coordinate rounds past the edge, scipy writes 0 there
         ((2, 5, 6, 3), (2.0, 0.6, 1.5, 1)), ((17,), 2.5)]


@pytest.mark.parametrize("shape,f", CASES)
def test_kernel_equals_scipy_float32(shape, f):
    a = data(shape, len(shape) * 100 + shape[0])
    if shape == (20, 24, 3):
        chw = np.ascontiguousarray(np.moveaxis(a, -1, 0))                   # "the same data channels-first"
        assert same_bits(device_zoom(chw, (1, 0.5, 1.5)), zoom(chw, (1, 0.5, 1.5), order=1))
    assert same_bits(device_zoom(a, f), zoom(a, f, order=1))


@pytest.mark.parametrize("dtype", (np.uint8, np.uint16))
def test_kernel_equals_scipy_integers(dtype):
    top = np.iinfo(dtype).max
    for k, (shape, f) in enumerate((((37, 53), 0.5), ((37, 53), (0.73, 1.31)), ((9, 17, 13), (2.2, 0.5, 0.5)), ((4, 3), (47.0, 1)))):
        a = np.random.default_rng(k).integers(0, top + 1, shape).astype(dtype)
        a.flat[0], a.flat[-1] = 0, top
        assert same_bits(device_zoom(a, f), zoom(a, f, order=1)), (shape, f)
    b = (np.random.default_rng(5).integers(0, 2, (37, 53)) * top).astype(dtype)      # 0 and the maximum only
    assert same_bits(device_zoom(b, 2.0), zoom(b, 2.0, order=1))


def test_non_finite_pixels_spread_as_in_scipy():
    a = data((20, 24, 3), 4, 0.0, 1.0)
    a[4, 6, 1] = np.inf
    a[11, 2, 0] = np.nan
    a[19, 23, 2] = -np.inf
    with np.errstate(invalid="ignore"):
        want = zoom(a, (0.5, 1.5, 1), order=1)
    assert np.isnan(want[2, 9, 2])
    assert same_bits(device_zoom(a, (0.5, 1.5, 1)), want)


def test_non_contiguous_view_and_repeatability():
    import torch
    from stardist_amd.utils import zoom_linear
    big = data((40, 70), 3)
    t = torch.from_numpy(big).to("cuda:0")
    for view_t, view_a in ((t[::2, 3:-5], big[::2, 3:-5]), (t.T, big.T)):
        assert not view_t.is_contiguous()
        got = zoom_linear(view_t, (0.73, 1.31))
        assert same_bits(got.cpu().numpy(), zoom(view_a, (0.73, 1.31), order=1))
        again = zoom_linear(view_t, (0.73, 1.31))
        assert got.data_ptr() != again.data_ptr() and torch.equal(got.view(torch.int32), again.view(torch.int32))
    assert torch.equal(t, torch.from_numpy(big).to("cuda:0"))               # the input is left as it was


def test_more_than_one_sweep_of_the_grid():
    """1500 x 1500 by 2.0: 9 M output elements, several times the threads of one launch, so the grid-stride loop iterates"""
    a = data((1500, 1500), 8, 0.0, 1.0)
    assert same_bits(device_zoom(a, 2.0), zoom(a, 2.0, order=1))


def test_unserved_tensors_take_scipy_and_stay_on_the_device():
    import torch
    from stardist_amd.utils import zoom_linear
    a = data((20, 24), 6).astype(np.float64)
    got = zoom_linear(torch.from_numpy(a).to("cuda:0"), 1.5)
    assert got.is_cuda and got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), zoom(a, 1.5, order=1))
    empty = zoom_linear(torch.zeros((1, 40), device="cuda:0"), 0.25)         # what scipy answers for an empty output (no error in 1.15)
    assert tuple(empty.shape) == zoom(np.zeros((1, 40), np.float32), 0.25, order=1).shape


# ------------------------------------------------------------------------------------------------- predict_instances(scale=)
@pytest.fixture(scope="module")
def model2d():
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from oracle import synth
    from stardist_amd.models import Config2D, StarDist2D
    dev = torch.device("cuda:0")
    model = StarDist2D(Config2D(n_rays=32), basedir=None, device=dev, seed=0)
    bench.calibrate_heads(model, torch.from_numpy(synth.s2d_nuclei_image(256, 256, seed=1)).to(dev))
    return model


@pytest.fixture(scope="module")
def model3d():
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from oracle import synth
    from stardist_amd.models import Config3D, StarDist3D
    dev = torch.device("cuda:0")
    model = StarDist3D(Config3D(rays=32), basedir=None, device=dev, seed=0)
    model.thresholds = dict(prob=0.5, nms=0.3)
    bench.calibrate_heads(model, torch.from_numpy(synth.s3d_nuclei_image(64, seed=0)).to(dev), frac=0.009, radius=8.5, noise=0.03)
    return model


def zoom_must_not_run(*args, **kwargs):
    raise AssertionError("scipy.ndimage.zoom was called on the device path")


def assert_same_result(got, want, min_objects=1):
    (labels, res), (labels_w, res_w) = got, want
    assert labels.dtype == labels_w.dtype and np.array_equal(labels, labels_w)
    assert set(res) == set(res_w) and len(res_w["prob"]) >= min_objects
    compared = 0
    for key, v in res_w.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(res[key], v), key
            compared += 1
    assert compared >= 3


def both_paths(model, monkeypatch, img, **kwargs):
    """(device path with scipy's zoom forbidden, host path) of one predict_instances call"""
    from scipy import ndimage
    with monkeypatch.context() as mp:
        mp.setattr(model, "_zoom_on_device", lambda img: False)             # the host path: the scipy line, as before
        want = model.predict_instances(img, **kwargs)
    with monkeypatch.context() as mp:
        mp.setattr(ndimage, "zoom", zoom_must_not_run)
        got = model.predict_instances(img, **kwargs)
    return got, want


@pytest.mark.parametrize("scale", (0.5, 2.0, (0.34, 1.47)))
def test_predict_instances_scale_2d(model2d, monkeypatch, scale):
    import torch
    from oracle import synth
    from stardist_amd.utils import PercentileNormalizer
    x = synth.s2d_nuclei_image(192, 256, seed=2)
    assert x.dtype == np.float32
    got, want = both_paths(model2d, monkeypatch, x, scale=scale)
    assert_same_result(got, want)
    assert got[0].shape == x.shape
    # the same call equals predicting the zoomed image, brought back to the input's grid
    s = np.asarray((scale, scale) if np.isscalar(scale) else scale)
    _, res_z = model2d.predict_instances(zoom(x, tuple(s), order=1))
    assert np.array_equal(got[1]["prob"], res_z["prob"]) and np.allclose(got[1]["points"] * s.reshape(1, 2), res_z["points"])
    got_t, _ = both_paths(model2d, monkeypatch, torch.from_numpy(x).to(model2d.device), scale=scale)
    assert_same_result(got_t, want)
    raw = np.clip(x * 20000 + 3000, 0, 65535).astype(np.uint16)
    got_u, want_u = both_paths(model2d, monkeypatch, raw, scale=scale, normalizer=PercentileNormalizer(1, 99.8))
    assert_same_result(got_u, want_u)


@pytest.mark.parametrize("scale", (0.5, (1.0, 1.5, 0.75)))
def test_predict_instances_scale_3d(model3d, monkeypatch, scale):
    import torch
    from oracle import synth
    from stardist_amd.utils import PercentileNormalizer
    x = synth.s3d_nuclei_image(64, seed=1)
    got, want = both_paths(model3d, monkeypatch, x, scale=scale)
    assert_same_result(got, want)
    assert got[0].shape == x.shape
    got_t, _ = both_paths(model3d, monkeypatch, torch.from_numpy(x).to(model3d.device), scale=scale)
    assert_same_result(got_t, want)
    raw = np.clip(x * 20000 + 3000, 0, 65535).astype(np.uint16)
    got_u, want_u = both_paths(model3d, monkeypatch, raw, scale=scale, normalizer=PercentileNormalizer(1, 99.8))
    assert_same_result(got_u, want_u, min_objects=0)


def test_predict_instances_iter_with_scale(model2d, monkeypatch):
    from oracle import synth
    from scipy import ndimage
    imgs = [synth.s2d_nuclei_image(160, 192, seed=s) for s in (3, 4, 5)]
    with monkeypatch.context() as mp:
        mp.setattr(model2d, "_zoom_on_device", lambda img: False)
        want = [model2d.predict_instances(im, scale=(0.8, 1.25)) for im in imgs]
    uploads = []
    real = model2d.predict_instances
    with monkeypatch.context() as mp:
        mp.setattr(ndimage, "zoom", zoom_must_not_run)
        mp.setattr(model2d, "predict_instances", lambda img, **kw: uploads.append(type(img).__module__) or real(img, **kw))
        got = list(model2d.predict_instances_iter(iter(imgs), scale=(0.8, 1.25)))
    assert len(got) == 3 and all(u.startswith("torch") for u in uploads)     # the overlapped upload, not the plain loop
    for g, w in zip(got, want):
        assert_same_result(g, w)


def test_predict_instances_iter_with_scale_leaves_other_dtypes_to_scipy(model2d):
    """a float64 image has no kernel: it stays a host array, scipy resamples it, and the result is the plain call's"""
    from oracle import synth
    imgs = [synth.s2d_nuclei_image(160, 192, seed=3), synth.s2d_nuclei_image(160, 192, seed=4).astype(np.float64)]
    want = [model2d.predict_instances(im, scale=(0.8, 1.25)) for im in imgs]
    got = list(model2d.predict_instances_iter(iter(imgs), scale=(0.8, 1.25)))
    for g, w in zip(got, want):
        assert_same_result(g, w)
