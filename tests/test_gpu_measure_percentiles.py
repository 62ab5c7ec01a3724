"""GPU: stardist_amd.utils.measure_labels(percentiles=) on device input (csrc/measure_rank.hip) against the host route, on the cases of
tests/_percentile_cases.py, exactly (== and equal NaN positions): every calling form, shape=True together with percentiles, the C entry
point's table against the host harness of csrc/measure_rank.h, its NaN rows and argument checks, repeatability, a chunk workspace that
runs out of slots, and offsets past 2^31."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _percentile_cases as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPE_CODE = {"uint8": 0, "uint16": 1, "float32": 2}
NUMPY_2 = int(np.__version__.split(".")[0]) >= 2
_vp, _i = ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def harness_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("measure_rank") / "libmeasure_rank.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host", "measure_rank_check.cpp"),
                    "-o", so], check=True)
    l = ctypes.CDLL(so)
    l.mr_percentiles.restype = _i
    l.mr_percentiles.argtypes = [_vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp]
    return l


def measure(*a, **kw):
    from stardist_amd.utils import measure_labels
    return measure_labels(*a, **kw)


def check_against_host(name, got):
    """a numpy table of the device route against the host route's: keys, dtypes, shapes; the percentile columns and the integer-typed
    columns exactly (the other float columns are tests/test_gpu_measure.py's)"""
    want = P.host(name)
    assert list(got) == list(want)
    for k in want:
        assert isinstance(got[k], np.ndarray) and got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
    for k in P.percentile_keys(name):
        assert P.same(got[k], want[k]), (name, k)
    for k in want:
        if k.startswith(("label", "area", "bbox-", "min_intensity", "max_intensity")):
            assert np.array_equal(got[k], want[k], equal_nan=True), (name, k)


@pytest.mark.parametrize("name", P.NAMES)
def test_tensors_in_tensors_out(torch, name):
    lbl, img, qs = P.case(name)
    t, x = torch.as_tensor(lbl, device="cuda"), torch.as_tensor(img, device="cuda")
    keep = t.clone(), x.clone()
    got = measure(t, x, percentiles=qs, as_tensors=True)
    assert all(isinstance(v, torch.Tensor) and v.device == t.device and v.dim() == 1 and v.is_contiguous() for v in got.values())
    assert torch.equal(t, keep[0]) and torch.equal(x.view(torch.uint8), keep[1].view(torch.uint8))                    # inputs unchanged
    check_against_host(name, {k: v.cpu().numpy() for k, v in got.items()})


@pytest.mark.parametrize("name", P.NAMES)
def test_numpy_in_with_device_numpy_out(torch, name):
    lbl, img, qs = P.case(name)
    check_against_host(name, measure(lbl, img, percentiles=qs, device="cuda"))


@pytest.mark.parametrize("name", P.NAMES)
def test_shape_together_with_percentiles(torch, name):
    lbl, img, qs = P.case(name)
    both = measure(lbl, img, shape=True, percentiles=qs, device="cuda")
    shape_only = measure(lbl, img, shape=True, device="cuda")
    plain = measure(lbl, img, device="cuda")
    pk = P.percentile_keys(name)
    extra = [k for k in shape_only if k not in plain]
    assert extra and list(both) == list(plain) + pk + extra                 # after the intensity columns, before the shape columns
    for k in shape_only:
        assert both[k].dtype == shape_only[k].dtype and both[k].tobytes() == shape_only[k].tobytes(), k
    want = P.host(name)
    for k in pk:
        assert both[k].dtype == want[k].dtype and P.same(both[k], want[k]), k


def entry(torch, lbl, img, qs, top=None, fill=-3.0, interp=None):
    """the (top + 1, C, n_q) float64 table of the C entry point as a numpy array; it starts as `fill`"""
    from stardist_amd.lib import _native as N
    lab = torch.as_tensor(np.ascontiguousarray(np.maximum(lbl, 0), np.int32), device="cuda")
    x = torch.as_tensor(np.ascontiguousarray(img), device="cuda")
    C = 1 if img.ndim == lbl.ndim else img.shape[-1]
    top = int(lab.max()) if top is None else top
    zyx = ((1,) + lbl.shape) if lbl.ndim == 2 else lbl.shape
    boxes = torch.empty((top + 1, 6), dtype=torch.int32, device="cuda")
    out = torch.full((top + 1, C, len(qs)), fill, dtype=torch.float64, device="cuda")
    q = (ctypes.c_double * len(qs))(*[float(v) for v in qs])
    vp = lambda a: ctypes.c_void_p(a.data_ptr())
    N.dcall(lab, "sd_label_boxes_device", vp(lab), *zyx, top, vp(boxes))
    N.dcall(lab, "sd_label_percentiles_device", vp(lab), *zyx, top, vp(boxes), vp(x), DTYPE_CODE[img.dtype.name], C, ctypes.cast(q, _vp), len(qs),
            (1 if NUMPY_2 else 0) if interp is None else interp, vp(out))
    return out.cpu().numpy()


def harness(lib, lbl, img, qs, top, interp=None):
    lab = np.ascontiguousarray(np.maximum(lbl, 0), np.int32)
    img = np.ascontiguousarray(img)
    C = 1 if img.ndim == lbl.ndim else img.shape[-1]
    q = np.array([float(v) for v in qs], np.float64)
    out = np.full((top + 1, C, len(q)), -3.0, np.float64)
    zyx = ((1,) + lbl.shape) if lbl.ndim == 2 else lbl.shape
    assert lib.mr_percentiles(lab.ctypes.data, *zyx, top, img.ctypes.data, DTYPE_CODE[img.dtype.name], C, q.ctypes.data, len(q),
                              (1 if NUMPY_2 else 0) if interp is None else interp, -1, -1, out.ctypes.data, None) == 0
    return out


@pytest.mark.parametrize("name", [n for n in P.NAMES if n != "huge_ids_u16"])
def test_entry_point_table_equals_the_harness(torch, harness_lib, name):
    """the C entry point on a table filled with -3, with three ids beyond the largest label: row 0 and absent rows hold NaN, every
    other row is the host harness's (both interpolation modes for float32), and a second call gives the same bits"""
    lbl, img, qs = P.case(name)
    top = int(max(lbl.max(), 0)) + 3
    modes = (0, 1) if img.dtype == np.float32 else (0,)
    for interp in modes:
        got = entry(torch, lbl, img, qs, top=top, interp=interp)
        want = harness(harness_lib, lbl, img, qs, top, interp=interp)
        present = np.unique(lbl[lbl > 0])
        absent = np.setdiff1d(np.arange(top + 1), present)
        assert 0 in absent and top in absent and np.isnan(got[absent]).all()
        assert not (got == -3.0).any() and P.same(got, want), (name, interp)
        again = entry(torch, lbl, img, qs, top=top, interp=interp)
        assert got.tobytes() == again.tobytes() or (np.isnan(got).any() and P.same(got, again))
    if name not in P.EMPTY:
        labels = P.host(name)["label"]
        block = P.percentile_block(P.host(name), name)
        stems = P.q_names(qs)
        cols = [stems.index("p%g_intensity" % float(q)) for q in qs]
        table = entry(torch, lbl, img, qs)
        assert P.same(table[labels].astype(block.dtype), block[:, :, cols])


def test_same_bits_after_the_workspace_has_grown(torch):
    lbl, img, qs = P.case("chunks_f32_c1")
    one = entry(torch, lbl, img, qs)
    big = np.zeros((3000, 3100), np.int32)
    big[5:2990, 7:3000] = 1
    big[10:20, 10:30] = 2
    filler = entry(torch, big, np.arange(big.size, dtype=np.uint32).reshape(big.shape).astype(np.uint16), (50,))
    assert np.isfinite(filler[1:]).all()
    two = entry(torch, lbl, img, qs)
    assert P.same(one, two) and one[~np.isnan(one)].tobytes() == two[~np.isnan(two)].tobytes()


@pytest.mark.parametrize("name", ["diagonals_u8", "diagonals_u16_c2"])
def test_exhausted_chunk_workspace_falls_back(torch, name):
    """more multi-chunk objects than the chunk workspace has slots (sized from the header's capacity): the rest are worked off by the
    block tier and the table is still the host route's"""
    lbl, img, qs = P.case(name)
    want = P.host(name)
    C = 1 if img.ndim == lbl.ndim else img.shape[-1]
    assert len(want["label"]) * C > P.MR_CHUNK_SLOTS
    sizes = (want["bbox-2"] - want["bbox-0"]) * (want["bbox-3"] - want["bbox-1"])
    assert (sizes > P.MS_CHUNK_PIXELS).all()
    got = measure(torch.as_tensor(lbl, device="cuda"), torch.as_tensor(img, device="cuda"), percentiles=qs)
    check_against_host(name, got)


def test_bad_arguments(torch):
    from stardist_amd.lib import _native as N
    t = torch.zeros((4, 5), dtype=torch.int32, device="cuda")
    img = torch.ones((4, 5), dtype=torch.float32, device="cuda")
    boxes = torch.zeros((3, 6), dtype=torch.int32, device="cuda")
    out = torch.full((3, 1, 2), 7.0, dtype=torch.float64, device="cuda")
    p, x, b, o = (ctypes.c_void_p(a.data_ptr()) for a in (t, img, boxes, out))
    q = (ctypes.c_double * 9)(25.0, 50.0, 1, 2, 3, 4, 5, 6, 7)
    qp = ctypes.cast(q, _vp)
    fn = N.lib().sd_label_percentiles_device
    good = [p, 1, 4, 5, 2, b, x, 2, 1, qp, 2, 1, o]
    bad = [(0, None), (1, 0), (2, -1), (3, 0), (4, -1), (5, None), (6, None), (7, 3), (7, -1), (8, 0), (8, 65), (9, None), (10, 0), (10, 9), (12, None)]
    for at, value in bad:
        args = list(good)
        args[at] = value
        assert fn(*args, N.current_stream()) == -1, at
        assert "sd_label_percentiles" in N.lib().sd_last_error().decode()
    for wrong in (-0.5, 100.5, float("nan"), float("inf"), -float("inf")):
        qq = (ctypes.c_double * 2)(50.0, wrong)
        args = list(good)
        args[9] = ctypes.cast(qq, _vp)
        assert fn(*args, N.current_stream()) == -1, wrong
        assert "percentiles" in N.lib().sd_last_error().decode()
    args = list(good)
    args[1:4] = [2 ** 10, 2 ** 21, 2 ** 10]                                 # more than 2^40 pixels, Z * Y beyond int
    assert fn(*args, N.current_stream()) == -1
    torch.cuda.synchronize()
    assert (out == 7).all()                                                 # nothing was launched
    assert N.lib().sd_label_boxes_device(p, 1, 4, 5, 2, b, N.current_stream()) == 0
    assert fn(*good, N.current_stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                           # no objects: every row is NaN


def test_offsets_past_2_31(torch):
    """32769 x 65537 int32 labels made on the device, objects of every tier in the last rows (flat offsets beyond 2^31), uint8 image;
    expected values from np.percentile on the crop of the last rows, on those objects only"""
    Y, X, tail = 32769, 65537, 12
    assert (Y - 1) * X > 2 ** 31
    rng = np.random.default_rng(5160)
    crop = np.zeros((tail, X), np.int32)
    for y, x, l in [(2, 5, 1), (1, 30000, 2), (4, 65520, 3), (7, 65528, 5)]:
        crop[y:y + 5, x:x + 7] = l
    crop[0:tail, 40000:40200] = 9                                           # 12 x 200 pixels: the block tier
    xs = np.arange(1000, 7000)
    crop[xs * tail // 7000, xs] = 10                                        # a thin line in a box of 12 x 6000 pixels: the chunked tier
    crop[tail - 1, X - 1] = 11                                              # the image's last pixel
    assert tail * 200 > P.MR_SORT_KEYS and tail * 6000 > P.MS_CHUNK_PIXELS
    crop_img = rng.integers(0, 256, crop.shape, dtype=np.uint8)
    lbl = torch.zeros((Y, X), dtype=torch.int32, device="cuda")
    img = torch.zeros((Y, X), dtype=torch.uint8, device="cuda")
    lbl[Y - tail:] = torch.as_tensor(crop, device="cuda")
    img[Y - tail:] = torch.as_tensor(crop_img, device="cuda")
    qs = (0, 25, 50, 99.8, 100)
    got = {k: v.cpu().numpy() for k, v in measure(lbl, img, percentiles=qs, as_tensors=True).items()}
    del lbl, img
    assert got["label"].tolist() == [1, 2, 3, 5, 9, 10, 11]
    for q in qs:
        want = np.array([np.percentile(crop_img[crop == l], float(q)) for l in got["label"]], np.float64)
        assert got["p%g_intensity" % q].dtype == np.float64 and np.array_equal(got["p%g_intensity" % q], want), q
