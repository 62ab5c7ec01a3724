"""GPU: normalisation on the device (csrc/normalize.hip through stardist_amd.utils.normalize / normalize_mi_ma and the normaliser classes)
against the host functions of this package on the same input.  Every comparison is np.array_equal (NaN cases: equal NaN positions):
the percentiles are exact order statistics with numpy's interpolation and the rescale is the host expression, so there is no tolerance."""
import ctypes
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (2,), (1000, 1003), (2048, 2048), (64, 128, 130)]
PAIRS = [(1, 99.8), (3, 99.8), (0, 100), (2, 50), (50, 50)]


def families(dtype, shape, seed):
    """name -> array: uniform, heavily tied, constant, saturated (uint16), negative, +-inf, -0.0, subnormal (float32)"""
    n = int(np.prod(shape))
    rng = np.random.default_rng(seed + n)
    out = {}
    if dtype == np.uint8:
        out["uniform"] = rng.integers(0, 256, n, dtype=np.uint8)
        out["tied"] = rng.integers(7, 10, n, dtype=np.uint8)
        out["constant"] = np.full(n, 200, np.uint8)
    elif dtype == np.uint16:
        out["uniform"] = rng.integers(0, 65536, n).astype(np.uint16)
        out["tied"] = (rng.integers(0, 4, n) * 257).astype(np.uint16)
        out["constant"] = np.full(n, 1234, np.uint16)
        sat = rng.integers(100, 5000, n).astype(np.uint16)
        sat[: n // 3] = 65535                                   # a saturated block, as a burnt-out region of an image is
        sat[rng.random(n) < 0.05] = 65535
        out["saturated"] = sat
    else:
        out["uniform"] = rng.random(n, dtype=np.float32)
        out["tied"] = rng.integers(0, 5, n).astype(np.float32) * np.float32(0.25)
        out["constant"] = np.full(n, 3.5, np.float32)
        out["negative"] = (rng.standard_normal(n) * 1e3).astype(np.float32)
        inf = rng.standard_normal(n).astype(np.float32)
        inf[rng.random(n) < 0.05] = np.inf
        inf[rng.random(n) < 0.05] = -np.inf
        out["inf"] = inf
        zero = rng.integers(-1, 2, n).astype(np.float32)
        zero[rng.random(n) < 0.3] = -0.0
        out["negzero"] = zero
        sub = (rng.integers(-50, 50, n).astype(np.float32) * np.float32(1e-42)).astype(np.float32)
        sub[rng.random(n) < 0.2] = np.float32(1e-30)
        out["subnormal"] = sub
    return {k: v.reshape(shape) for k, v in out.items()}


def _same(got, want):
    """np.array_equal with equal NaN positions"""
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(np.isnan(got), np.isnan(want)) and \
        np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _percentiles(t, qs, n_seg=1):
    from stardist_amd.utils import _interp_mode, _percentiles_device
    return _percentiles_device(t, qs, n_seg, _interp_mode(t, qs[0])).cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_percentiles_and_normalize_equal_host(dtype, shape):
    import torch
    from stardist_amd.utils import normalize
    for name, x in families(dtype, shape, seed=len(shape)).items():
        t = _dev(x)
        for k, (pmin, pmax) in enumerate(PAIRS):
            with np.errstate(invalid="ignore"):
                want_p = np.asarray([np.percentile(x, pmin), np.percentile(x, pmax)]).astype(np.float32)
                got_p = _percentiles(t, (pmin, pmax))[0]
                assert _same(got_p, want_p), (name, pmin, pmax, got_p, want_p)
                for clip in (False, True):
                    want = normalize(x, pmin, pmax, clip=clip)
                    got = normalize(t, pmin, pmax, clip=clip)
                    assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.float32
                    assert _same(got.cpu().numpy(), want), (name, pmin, pmax, clip)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_per_channel(dtype):
    from stardist_amd.utils import normalize
    for shape, axis in (((301, 257, 3), (0, 1)), ((9, 40, 50, 2), (0, 1, 2))):
        for name, x in families(dtype, shape, seed=7).items():
            t = _dev(x)
            for pmin, pmax in PAIRS[:3]:
                with np.errstate(invalid="ignore"):
                    want_p = np.stack([np.percentile(x, pmin, axis=axis), np.percentile(x, pmax, axis=axis)], -1).astype(np.float32)
                    assert _same(_percentiles(t, (pmin, pmax), n_seg=shape[-1]), want_p), (name, shape, pmin, pmax)
                    assert _same(normalize(t, pmin, pmax, axis=axis, clip=True).cpu().numpy(), normalize(x, pmin, pmax, axis=axis, clip=True))


def test_nan_and_fallbacks():
    import torch
    from stardist_amd.utils import normalize, normalize_mi_ma
    rng = np.random.default_rng(11)
    x = rng.random((300, 310), dtype=np.float32)
    x[123, 45] = np.nan
    got = normalize(_dev(x), 1, 99.8).cpu().numpy()
    want = normalize(x, 1, 99.8)
    assert np.isnan(want).all() and _same(got, want)
    assert np.isnan(_percentiles(_dev(x), (1, 99.8))).all()
    x3 = rng.random((50, 60, 2), dtype=np.float32)
    x3[3, 4, 1] = -np.nan                                      # one channel only
    assert _same(normalize(_dev(x3), 1, 99.8, axis=(0, 1)).cpu().numpy(), normalize(x3, 1, 99.8, axis=(0, 1)))
    # dtypes and axes outside the kernels: the host path, same values, device tensor out
    for a, kw in ((rng.random((40, 50)), {}), (rng.integers(-500, 500, (40, 50)).astype(np.int32), {}),
                  (rng.random((40, 50), dtype=np.float32), dict(axis=0)), (rng.integers(0, 999, (20, 30)).astype(np.uint16), dict(dtype=np.float64))):
        got = normalize(_dev(a), 1, 99.8, **kw)
        want = normalize(a, 1, 99.8, **kw)
        assert torch.is_tensor(got) and got.is_cuda and _same(got.cpu().numpy(), want)
    u = rng.integers(0, 60000, (64, 70)).astype(np.uint16)
    for mi, ma in ((100, 50000.5), (np.float32(3), np.float32(2000)), (np.asarray([[7.25]]), np.asarray([[30000.0]]))):
        for clip in (False, True):
            assert _same(normalize_mi_ma(_dev(u), mi, ma, clip=clip).cpu().numpy(), normalize_mi_ma(u, mi, ma, clip=clip))
    # numpy in: numpy out from the host path, as before
    out = normalize(u, 1, 99.8)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32


def test_more_than_2_24_elements():
    """4200 x 4200 float32 (1.76e7 > 2^24 elements): single-precision counting or 32-bit positions cannot pass; numpy's own float32
    virtual index (numpy >= 2.0) is followed, whatever ranks it names"""
    from stardist_amd.utils import normalize
    x = np.random.default_rng(5).random((4200, 4200), dtype=np.float32)
    x[:1400] = np.float32(0.75)                                 # a third of the image on one value: counts above 2^22 in one bin
    t = _dev(x)
    want_p = np.asarray([np.percentile(x, 1), np.percentile(x, 99.8)]).astype(np.float32)
    assert _same(_percentiles(t, (1, 99.8))[0], want_p)
    assert _same(normalize(t, 1, 99.8).cpu().numpy(), normalize(x, 1, 99.8))


def test_q_as_numpy_scalar_and_three_percentiles():
    """np.float64 / numpy integer q: numpy interpolates float32 data in float64 (they are not weak scalars), and so does the device;
    np.float32 q has no device path and takes the host's.  Three percentiles in one call (the entry point's upper limit)."""
    import torch
    from stardist_amd.utils import PercentileNormalizer, normalize
    x = np.random.default_rng(5).standard_normal((317, 631)).astype(np.float32)
    t = _dev(x)
    assert np.float32(np.percentile(x, 99.8)) != np.float32(np.percentile(x, np.float64(99.8))) or int(np.__version__.split(".")[0]) < 2
    for pmin, pmax in ((np.float64(1), np.float64(99.8)), (np.int64(1), np.float64(99.8)), (np.float32(1), np.float32(99.8)), (1, np.float64(99.8)),
                       (1, 99.8)):
        got = normalize(t, pmin, pmax)
        assert torch.is_tensor(got) and got.is_cuda and _same(got.cpu().numpy(), normalize(x, pmin, pmax)), (type(pmin), type(pmax))
    nz = PercentileNormalizer(np.float64(1), np.float64(99.8))
    assert _same(nz.before_device(t, "YX").cpu().numpy(), PercentileNormalizer(np.float64(1), np.float64(99.8)).before(x, "YX"))
    for a in (x, (np.abs(x) * 9000).astype(np.uint16), (np.abs(x) * 60).astype(np.uint8)):
        for qs in ((1, 50, 99.8), (0, 100, 37.3), (50, 50, 50)):
            with np.errstate(invalid="ignore"):
                want = np.asarray([np.percentile(a, q) for q in qs]).astype(np.float32)
            assert _same(_percentiles(_dev(a), qs)[0], want), (a.dtype, qs)


def test_entry_points_return_before_the_device_is_done():
    """no host synchronisation inside the two entry points: with a long-running kernel in front of them on the stream, both return while
    that kernel is still running (the event recorded behind it has not completed)"""
    import torch
    from stardist_amd.utils import normalize
    t = _dev(np.random.default_rng(8).integers(0, 65536, (1024, 1024)).astype(np.uint16))
    f = _dev(np.random.default_rng(9).random((1024, 1024), dtype=np.float32))
    a, b = normalize(t, 1, 99.8), normalize(f, 1, 99.8)           # first calls: workspace, code objects, output blocks in torch's cache
    torch.cuda.synchronize()
    del a, b
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); torch.cuda._sleep(1_000_000); e1.record()       # how long a spin of 10^6 device clock ticks lasts here
    e1.synchronize()
    ticks = int(1_000_000 * 400.0 / max(e0.elapsed_time(e1), 1e-3))
    busy = torch.cuda.Event()
    torch.cuda._sleep(ticks)                                      # about 0.4 s of device time
    busy.record()
    a, b = normalize(t, 1, 99.8), normalize(f, 1, 99.8)
    still_running = not busy.query()
    torch.cuda.synchronize()
    assert still_running, "the entry points waited for the device"
    assert _same(a.cpu().numpy(), normalize(t.cpu().numpy(), 1, 99.8)) and _same(b.cpu().numpy(), normalize(f.cpu().numpy(), 1, 99.8))


def test_entry_points_twice_same_bits():
    import torch
    from stardist_amd.lib import _native as N
    rng = np.random.default_rng(6)
    for x, code in ((rng.integers(0, 65536, (1500, 1501)).astype(np.uint16), 1), (rng.standard_normal((1500, 1501)).astype(np.float32), 2),
                    (rng.integers(0, 256, (1500, 1501), dtype=np.uint8), 0)):
        t = _dev(x)
        q = (ctypes.c_double * 2)(1.0, 99.8)
        res = []
        for _ in range(2):
            p = torch.full((2,), -1.0, dtype=torch.float32, device=t.device)
            o = torch.full(t.shape, -1.0, dtype=torch.float32, device=t.device)
            N.dcall(t, "sd_percentiles_device", ctypes.c_void_p(t.data_ptr()), code, t.numel(), 1, ctypes.cast(q, ctypes.c_void_p), 2, 1,
                    ctypes.c_void_p(p.data_ptr()))
            N.dcall(t, "sd_normalize_mi_ma_device", ctypes.c_void_p(t.data_ptr()), code, t.numel(), 1, ctypes.c_void_p(p.data_ptr()),
                    ctypes.c_void_p(p.data_ptr() + 4), float(np.float32(1e-20)), 0, ctypes.c_void_p(o.data_ptr()))
            res.append((p.cpu().numpy(), o.cpu().numpy()))
        assert res[0][0].tobytes() == res[1][0].tobytes() and res[0][1].tobytes() == res[1][1].tobytes()
        assert _same(res[0][1], __import__("stardist_amd.utils", fromlist=["normalize"]).normalize(x, 1, 99.8))
    # arguments the entry point refuses
    t = _dev(np.zeros(8, np.float32))
    p = torch.zeros(2, dtype=torch.float32, device=t.device)
    for bad in ((ctypes.c_double * 2)(1.0, 101.0), (ctypes.c_double * 2)(float("nan"), 5.0)):
        with pytest.raises(N.NativeError):
            N.dcall(t, "sd_percentiles_device", ctypes.c_void_p(t.data_ptr()), 2, 8, 1, ctypes.cast(bad, ctypes.c_void_p), 2, 1, ctypes.c_void_p(p.data_ptr()))
    with pytest.raises(N.NativeError):
        N.dcall(t, "sd_percentiles_device", ctypes.c_void_p(t.data_ptr()), 5, 8, 1, ctypes.cast(q, ctypes.c_void_p), 2, 1, ctypes.c_void_p(p.data_ptr()))


# ----------------------------------------------------------------------------- through the models
def _raw(img, seed):
    """a raw uint16 camera image of a synthetic float image: offset, gain, a few saturated pixels"""
    rng = np.random.default_rng(seed)
    a = np.clip(img.astype(np.float64) * 3000 + 120 + rng.normal(0, 3, img.shape), 0, 65535)
    a[rng.random(img.shape) < 1e-4] = 65535
    return a.astype(np.uint16)


def _model(kind):
    import torch
    import bench
    from oracle import synth
    from stardist_amd.models import Config2D, Config3D, StarDist2D, StarDist3D
    from stardist_amd.utils import normalize
    dev = torch.device("cuda:0")
    if kind == "YX":
        raws = [_raw(synth.s2d_nuclei_image(256, 320, seed=s), s) for s in (1, 2, 3)]
        m = StarDist2D(Config2D(n_rays=32), basedir=None, device=dev, seed=0)
        bench.calibrate_heads(m, torch.from_numpy(normalize(raws[0], 1, 99.8)).to(dev))
        axis = None
    elif kind == "YXC":
        raws = [np.stack([_raw(synth.s2d_nuclei_image(256, 320, seed=s + c), s + c) // (c + 1) for c in range(3)], -1) for s in (1, 2, 3)]
        m = StarDist2D(Config2D(n_rays=32, n_channel_in=3), basedir=None, device=dev, seed=0)
        bench.calibrate_heads(m, torch.from_numpy(normalize(raws[0], 1, 99.8, axis=(0, 1))).to(dev))
        axis = (0, 1)
    else:
        raws = [_raw(synth.s3d_nuclei_image(64, seed=s), s) for s in (1, 2, 3)]
        m = StarDist3D(Config3D(rays=96), basedir=None, device=dev, seed=0)
        m.thresholds = dict(prob=0.5, nms=0.3)
        bench.calibrate_heads(m, torch.from_numpy(normalize(raws[0], 1, 99.8)).to(dev), frac=0.02, radius=8.5, noise=0.03)
        axis = None
    return m, raws, axis


def _same_instances(a, b, keys):
    (la, ra), (lb, rb) = a, b
    assert np.array_equal(la, lb)
    for k in keys:
        assert np.array_equal(ra[k], rb[k]), k


@pytest.mark.parametrize("kind", ["YX", "YXC", "ZYX"])
def test_predict_instances_with_normalizer_equals_host_normalize(kind):
    """raw uint16 host image + PercentileNormalizer, the same image as a device tensor, and the host-normalised image: identical label
    images and coord / points / prob (3D: dist in coord's place); the same through predict_instances_iter over three images"""
    import torch
    from stardist_amd.utils import PercentileNormalizer, normalize
    m, raws, axis = _model(kind)
    keys = ("coord", "points", "prob") if kind != "ZYX" else ("dist", "points", "prob")
    want = [m.predict_instances(normalize(r, 1, 99.8, axis=axis)) for r in raws]
    assert len(want[0][1]["prob"]) > 5
    nz = PercentileNormalizer(1, 99.8)
    for r, w in zip(raws, want):
        _same_instances(m.predict_instances(r, normalizer=nz), w, keys)
        _same_instances(m.predict_instances(torch.as_tensor(r, device=m.device), normalizer=nz), w, keys)
    assert torch.is_tensor(nz.mi) and nz.mi.is_cuda                      # the bounds stayed on the device
    mi = np.percentile(raws[-1], 1, axis=axis, keepdims=True).astype(np.float32)
    assert np.array_equal(nz.mi.cpu().numpy().reshape(mi.shape), mi)
    m.__dict__.pop("_upload_ring", None)
    got = list(m.predict_instances_iter(iter(raws), normalizer=PercentileNormalizer(1, 99.8)))
    assert len(got) == 3
    # the prefetch path was taken (its page-locked staging ring holds the RAW dtype), not the plain loop
    assert any(k == (raws[0].shape, raws[0].dtype.str) for k in m.__dict__.get("_upload_ring", {})), m.__dict__.get("_upload_ring", {}).keys()
    # a host image of a dtype without kernel is normalised on the host and uploaded once: same result
    _same_instances(m.predict_instances(raws[0].astype(np.float64), normalizer=nz), want[0], keys)
    assert isinstance(nz.mi, np.ndarray)
    for g, w in zip(got, want):
        _same_instances(g, w, keys)

    class Foreign(object):                                                # any other object with csbdeep's protocol: the host path
        do_after = False

        def before(self, x, axes):
            assert isinstance(x, np.ndarray)
            return normalize(x, 1, 99.8, axis=tuple(d for d, a in enumerate(axes) if a != "C"))
    _same_instances(m.predict_instances(raws[0], normalizer=Foreign()), want[0], keys)


def test_predict_instances_big_with_fixed_bounds():
    from stardist_amd.utils import MiMaNormalizer, normalize_mi_ma
    m, raws, _ = _model("YX")
    raw = np.tile(raws[0], (2, 2))
    mi, ma = np.percentile(raw, 1), np.percentile(raw, 99.8)
    kw = dict(axes="YX", block_size=256, min_overlap=64, context=64, show_progress=False)
    lw, rw = m.predict_instances_big(normalize_mi_ma(raw, mi, ma), **kw)
    lg, rg = m.predict_instances_big(raw, normalizer=MiMaNormalizer(mi, ma), **kw)
    assert len(rw["prob"]) > 5 and np.array_equal(lw, lg)
    for k in ("coord", "points", "prob"):
        assert np.array_equal(rw[k], rg[k])


def test_no_host_synchronisation_in_predict_setup():
    """torch's sync debug mode raises no warning while _predict_setup normalises a raw device tensor.  That mode sees torch's own calls
    only, not the two entry points (called through ctypes): those hold no synchronising call by construction -- csrc/normalize.hip has
    no stream / device synchronise and no copy to the host, which tests/test_cpu_normalize.py checks on the source."""
    import torch
    from stardist_amd.utils import PercentileNormalizer
    m, raws, _ = _model("YX")
    t = torch.as_tensor(raws[0], device=m.device)
    nz = PercentileNormalizer(1, 99.8)
    m._predict_setup(t, None, nz, None)                                    # first call: allocations, code objects
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            x = m._predict_setup(t, None, nz, None)[0]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert x.dtype == torch.float32 and x.is_cuda
    assert not [w for w in seen if "synchroniz" in str(w.message).lower()], [str(w.message) for w in seen]
