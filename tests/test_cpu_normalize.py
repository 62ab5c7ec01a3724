"""CPU: the host-checkable half of the device normalisation (csrc/select_rank.h through tests/host/select_rank_check.cpp) against numpy,
the normaliser classes of stardist_amd.utils on numpy arrays, and "numpy in -> numpy out, unchanged" for normalize / normalize_mi_ma."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DT = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}
SIZES = (1, 2, 63, 64, 65, 10 ** 6)
QS = (0, 1, 3, 50, 99.8, 100)
NUMPY_2 = int(np.__version__.split(".")[0]) >= 2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("selrank") / "libselrank.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                    os.path.join(ROOT, "tests", "host", "select_rank_check.cpp"), "-o", so], check=True)
    l = ctypes.CDLL(so)
    l.sr_select.restype = None
    l.sr_select.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    l.sr_percentile.restype = None
    l.sr_percentile.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                ctypes.c_void_p, ctypes.c_void_p]
    return l


def families(n, seed=0):
    """name -> array of n elements: the data families of the issue, for the three element types"""
    rng = np.random.default_rng(seed + n)
    out = {}
    out["u8_uniform"] = rng.integers(0, 256, n, dtype=np.uint8)
    out["u8_tied"] = rng.integers(7, 10, n, dtype=np.uint8)
    out["u8_constant"] = np.full(n, 200, np.uint8)
    out["u16_uniform"] = rng.integers(0, 65536, n).astype(np.uint16)
    out["u16_tied"] = (rng.integers(0, 4, n) * 257).astype(np.uint16)
    out["u16_constant"] = np.full(n, 1234, np.uint16)
    sat = rng.integers(100, 5000, n).astype(np.uint16)
    sat[rng.random(n) < 1 / 3] = 65535
    out["u16_saturated"] = sat
    out["f32_uniform"] = rng.random(n, dtype=np.float32)
    out["f32_tied"] = rng.integers(0, 5, n).astype(np.float32) * np.float32(0.25)
    out["f32_constant"] = np.full(n, 3.5, np.float32)
    out["f32_negative"] = (rng.standard_normal(n) * 1e3).astype(np.float32)
    inf = rng.standard_normal(n).astype(np.float32)
    inf[rng.random(n) < 0.05] = np.inf
    inf[rng.random(n) < 0.05] = -np.inf
    out["f32_inf"] = inf
    zero = rng.integers(-1, 2, n).astype(np.float32)
    zero[rng.random(n) < 0.3] = -0.0
    out["f32_negzero"] = zero
    sub = (rng.integers(-50, 50, n).astype(np.float32) * np.float32(1e-42)).astype(np.float32)
    sub[rng.random(n) < 0.2] = np.float32(1e-30)
    out["f32_subnormal"] = sub
    return out


def interp_f32(x):
    """numpy >= 2.0 keeps a Python-scalar q in the dtype of float data: float32 index and interpolation for float32"""
    return int(NUMPY_2 and x.dtype == np.float32)


def ranks_of(n):
    r = {0, min(1, n - 1), n // 2, max(n - 2, 0), n - 1}
    for q in QS:
        v = q / 100 * (n - 1)
        r.add(int(np.floor(v)))
        r.add(min(int(np.floor(v)) + 1, n - 1))
    return sorted(r)


def test_key_order_and_round_trip(lib):
    """the float32 key sorts like the value (with -0.0 below +0.0) and selecting every rank returns the sorted array"""
    x = np.array([-np.inf, -3.5, -1e-42, -0.0, 0.0, 1e-42, 1e-30, 2.0, np.inf], np.float32)
    ranks = np.arange(len(x), dtype=np.int64)
    for perm_seed in range(3):
        p = np.random.default_rng(perm_seed).permutation(len(x))
        xs = np.ascontiguousarray(x[p])
        vals = np.empty(len(x), np.float64)
        lib.sr_select(xs.ctypes.data, 2, len(xs), ranks.ctypes.data, len(ranks), vals.ctypes.data)
        assert np.array_equal(vals.astype(np.float32), x)
        assert np.array_equal(np.signbit(vals), np.signbit(x))


@pytest.mark.parametrize("n", SIZES)
def test_selected_rank_equals_partition(lib, n):
    for name, x in families(n).items():
        ranks = np.asarray(ranks_of(n), np.int64)
        want = np.partition(x, ranks)[ranks].astype(np.float64)
        for lo in range(0, len(ranks), 6):                       # the device carries at most 6 ranks per call; so does this check
            rr = np.ascontiguousarray(ranks[lo:lo + 6])
            got = np.empty(len(rr), np.float64)
            lib.sr_select(x.ctypes.data, DT[x.dtype], n, rr.ctypes.data, len(rr), got.ctypes.data)
            assert np.array_equal(got, want[lo:lo + 6]), (name, n, rr, got, want[lo:lo + 6])


@pytest.mark.parametrize("n", SIZES)
def test_percentile_equals_numpy_bit_for_bit(lib, n):
    """float32(np.percentile(x, q)) -- the cast normalize_mi_ma applies -- from the header's ranks and interpolation"""
    for name, x in families(n).items():
        for lo in range(0, len(QS), 3):
            qs = QS[lo:lo + 3]
            q = np.asarray(qs, np.float64)
            got = np.empty(len(q), np.float32)
            ranks = np.empty(2 * len(q), np.int64)
            lib.sr_percentile(x.ctypes.data, DT[x.dtype], n, q.ctypes.data, len(q), interp_f32(x), got.ctypes.data, ranks.ctypes.data)
            with np.errstate(invalid="ignore"):
                want = np.asarray([np.percentile(x, v) for v in qs]).astype(np.float32)
            # np.array_equal: equal values, i.e. equal bits but for the sign of a zero (numpy's partition does not order -0.0 and +0.0)
            # and the NaN that inf - inf gives in numpy's interpolation as in ours
            assert np.array_equal(got, want, equal_nan=True), (name, n, qs, got, want)


def test_percentile_float64_interpolation_of_float32(lib):
    """q given as numpy float64: numpy interpolates float32 data in float64 and the result is rounded to float32 afterwards"""
    x = np.random.default_rng(5).standard_normal(100003).astype(np.float32)
    qs = (1.0, 99.8)
    q = np.asarray(qs, np.float64)
    got = np.empty(2, np.float32)
    ranks = np.empty(4, np.int64)
    lib.sr_percentile(x.ctypes.data, 2, len(x), q.ctypes.data, 2, 0, got.ctypes.data, ranks.ctypes.data)
    want = np.asarray([np.percentile(x, np.float64(v)) for v in qs]).astype(np.float32)
    assert np.array_equal(got, want)


def test_large_n_ranks_follow_numpy(lib):
    """more than 2^24 elements: the float32 virtual index numpy >= 2.0 uses is not the exact one; the ranks asked for must be numpy's"""
    n = 4200 * 4200
    x = np.random.default_rng(1).random(n, dtype=np.float32)
    q = np.asarray([1.0, 99.8], np.float64)
    got = np.empty(2, np.float32)
    ranks = np.empty(4, np.int64)
    lib.sr_percentile(x.ctypes.data, 2, n, q.ctypes.data, 2, interp_f32(x), got.ctypes.data, ranks.ctypes.data)
    want = np.asarray([np.percentile(x, 1), np.percentile(x, 99.8)]).astype(np.float32)
    assert np.array_equal(got, want), (got, want, ranks)


# ----------------------------------------------------------------------------- the Python surface on numpy arrays
def _host_normalize_mi_ma(x, mi, ma, clip=False, eps=1e-20, dtype=np.float32):
    """the expression of stardist_amd/utils.py before the device path existed (csbdeep.utils.normalize_mi_ma)"""
    if dtype is not None:
        x = x.astype(dtype, copy=False)
        mi = dtype(mi) if np.isscalar(mi) else mi.astype(dtype, copy=False)
        ma = dtype(ma) if np.isscalar(ma) else ma.astype(dtype, copy=False)
        eps = dtype(eps)
    x = (x - mi) / (ma - mi + eps)
    if clip:
        x = np.clip(x, 0, 1)
    return x


def _host_normalize(x, pmin=3, pmax=99.8, axis=None, clip=False, eps=1e-20, dtype=np.float32):
    mi = np.percentile(x, pmin, axis=axis, keepdims=True)
    ma = np.percentile(x, pmax, axis=axis, keepdims=True)
    return _host_normalize_mi_ma(x, mi, ma, clip=clip, eps=eps, dtype=dtype)


def test_numpy_in_numpy_out_unchanged():
    from stardist_amd.utils import normalize, normalize_mi_ma
    rng = np.random.default_rng(2)
    for x in (rng.integers(0, 4000, (40, 50)).astype(np.uint16), rng.random((9, 20, 21), dtype=np.float32), rng.integers(0, 255, (30, 31, 3), dtype=np.uint8),
              rng.random((16, 16))):
        for kw in (dict(), dict(pmin=1, pmax=99.8, clip=True), dict(pmin=0, pmax=100, axis=(0, 1)), dict(dtype=None)):
            got, want = normalize(x, **kw), _host_normalize(x, **kw)
            assert isinstance(got, np.ndarray) and got.dtype == want.dtype and np.array_equal(got, want)
        got, want = normalize_mi_ma(x, 3, 200.5, clip=True), _host_normalize_mi_ma(x, 3, 200.5, clip=True)
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.parametrize("axes,shape", [("YX", (33, 47)), ("YXC", (33, 47, 3)), ("ZYX", (5, 20, 21)), ("ZYXC", (5, 20, 21, 2))])
def test_percentile_normalizer_before_equals_normalize(axes, shape):
    from stardist_amd.utils import PercentileNormalizer, normalize
    x = np.random.default_rng(3).integers(0, 60000, shape).astype(np.uint16)
    axis = tuple(d for d, a in enumerate(axes) if a != "C")
    nz = PercentileNormalizer(1, 99.8)
    got = nz.before(x, axes)
    assert got.dtype == np.float32 and np.array_equal(got, normalize(x, 1, 99.8, axis=axis))
    assert nz.mi.dtype == np.float32 and nz.mi.shape == tuple(s if a == "C" else 1 for s, a in zip(shape, axes))
    got = PercentileNormalizer(2, 50, clip=True).before(x, axes)
    assert np.array_equal(got, normalize(x, 2, 50, axis=axis, clip=True))
    assert PercentileNormalizer().pmin == 2 and PercentileNormalizer().pmax == 99.8 and PercentileNormalizer().do_after is True


def test_normalizer_after_and_fixed_bounds():
    from stardist_amd.utils import MiMaNormalizer, NoNormalizer, PercentileNormalizer, normalize_mi_ma
    # an affine example that float32 carries exactly: values k / 4 with percentiles 0 and 100 -> mi = 2, ma = 10
    x = (np.arange(8, 41, dtype=np.float32) / 4).reshape(3, 11)
    nz = PercentileNormalizer(0, 100, eps=0)
    y = nz.before(x, "YX")
    assert float(nz.mi.ravel()[0]) == 2.0 and float(nz.ma.ravel()[0]) == 10.0
    mean, scale = nz.after(y, y * 0 + 0.5, "YX")
    assert np.array_equal(mean, x) and np.array_equal(scale, np.full_like(x, 4.0))
    assert nz.after(y, None, "YX")[1] is None
    off = PercentileNormalizer(0, 100, do_after=False)
    off.before(x, "YX")
    assert off.do_after is False
    with pytest.raises(ValueError):
        off.after(y, None, "YX")
    with pytest.raises(ValueError):
        PercentileNormalizer(50, 20)
    u = np.random.default_rng(4).integers(0, 4000, (20, 30)).astype(np.uint16)
    mm = MiMaNormalizer(10, 3000.5, clip=True)
    assert np.array_equal(mm.before(u, "YX"), normalize_mi_ma(u, 10, 3000.5, clip=True))
    m2, s2 = MiMaNormalizer(2.0, 10.0).after(y, None, "YX")
    assert np.array_equal(m2, x) and s2 is None
    no = NoNormalizer()
    assert no.before(u, "YX") is u and no.do_after is False
    with pytest.raises(ValueError):
        no.after(u, None, "YX")


def test_entry_points_hold_no_synchronising_call():
    """the device path of a prediction stays asynchronous: csrc/normalize.hip neither synchronises a stream or the device nor copies
    to the host (the percentiles stay in device memory, where the rescale reads them)"""
    src = open(os.path.join(ROOT, "stardist_amd", "csrc", "normalize.hip")).read()
    for word in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "hipEventSynchronize", "hipHostMalloc"):
        assert word not in src, word


def test_interp_mode_follows_numpy_scalar_rules(lib):
    """utils._interp_mode picks the precision np.percentile works in for this q: Python int / float are weak scalars (float32 for float32
    data under numpy >= 2.0); np.float64 -- a subclass of Python float -- and numpy integers are not (float64); anything else has no
    device path.  Checked against np.percentile itself on data where the two precisions give different float32 results."""
    import torch
    from stardist_amd.utils import _interp_mode
    f32, u16 = torch.zeros(4, dtype=torch.float32), torch.zeros(4, dtype=torch.uint16)
    weak = int(NUMPY_2)
    assert _interp_mode(f32, 99.8) == weak and _interp_mode(f32, 1) == weak
    assert _interp_mode(f32, np.float64(99.8)) == 0 and _interp_mode(f32, np.int64(3)) == 0 and _interp_mode(f32, np.uint8(3)) == 0
    for q in (99.8, 1, np.float64(99.8), np.int64(3)):
        assert _interp_mode(u16, q) == 0
    for q in (True, np.bool_(True), np.float32(99.8), np.float16(50), np.asarray(99.8), [1.0], "1", None):
        assert _interp_mode(f32, q) is None and _interp_mode(u16, q) is None
    x = np.random.default_rng(5).standard_normal(100003).astype(np.float32)
    differ = 0
    for q in (99.8, np.float64(99.8), 1, np.int64(1), 37.3, np.float64(37.3)):
        got = np.empty(2, np.float32)
        ranks = np.empty(4, np.int64)
        qq = np.asarray([float(q), float(q)], np.float64)
        lib.sr_percentile(x.ctypes.data, 2, len(x), qq.ctypes.data, 2, _interp_mode(torch.from_numpy(x), q), got.ctypes.data, ranks.ctypes.data)
        assert got[0] == np.float32(np.percentile(x, q)), (q, type(q))
        lib.sr_percentile(x.ctypes.data, 2, len(x), qq.ctypes.data, 2, 1 - _interp_mode(torch.from_numpy(x), q), got.ctypes.data, ranks.ctypes.data)
        differ += int(got[0] != np.float32(np.percentile(x, q)))
    assert differ > 0 or not NUMPY_2          # the case is real: the other precision gives other bits for some of these
