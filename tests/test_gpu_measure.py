"""GPU: stardist_amd.utils.measure_labels on device input (csrc/measure.hip with the box and centroid-sum kernels) against the host
route, on the cases of tests/_measure_cases.py: every integer-typed column, the centroids, min, max and the mean of integer images
exactly; float sums bit for bit where every partial sum is exact and within the derived bounds (tests/_measure_cases.sum_bounds)
otherwise; both calling forms, repeatability, the C entry point's sentinel rows and argument checks, and offsets past 2^31."""
import ctypes

import numpy as np
import pytest

import _measure_cases as C

pytestmark = pytest.mark.gpu

INTENSITY = ("sum_intensity", "mean_intensity", "min_intensity", "max_intensity", "std_intensity")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def measure(*a, **kw):
    from stardist_amd.utils import measure_labels
    return measure_labels(*a, **kw)


def check_against_host(name, got):
    """a numpy table of the device route against the host route's"""
    want = C.host(name)
    lbl, img = C.case(name)
    assert list(got) == list(want) == C.case_keys(name)
    for k in want:
        assert isinstance(got[k], np.ndarray) and got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
    for k in want:
        if k.startswith(("label", "area", "bbox-", "centroid-", "min_intensity", "max_intensity")):
            assert np.array_equal(got[k], want[k], equal_nan=True), (name, k)
    if img is None or not len(want["label"]):
        return
    if img.dtype != np.float32:
        for k in want:
            assert np.array_equal(got[k], want[k]), (name, k)               # exact sums: every derived column is the host's too
    elif name == "non_finite":
        v = img.astype(np.float64)
        for k in want:
            assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])) and np.array_equal(np.isinf(got[k]), np.isinf(want[k])), k
        fine = np.isfinite(want["std_intensity"])
        bound = np.array([(lbl == l).sum() * 2.0 ** -52 * np.abs(v[lbl == l]).sum() for l in want["label"][fine]])
        assert fine.sum() == len(fine) - 3 and (np.abs(got["sum_intensity"][fine] - want["sum_intensity"][fine]) <= bound).all()
    else:
        C.check_float_columns(name, got, exact=name in C.FLOAT_EXACT)


@pytest.mark.parametrize("name", C.NAMES)
def test_tensors_in_tensors_out(torch, name):
    lbl, img = C.case(name)
    t = torch.as_tensor(lbl, device="cuda")
    x = None if img is None else torch.as_tensor(img, device="cuda")
    keep = t.clone(), (None if x is None else x.clone())
    got = measure(t, x, as_tensors=True)
    assert all(isinstance(v, torch.Tensor) and v.device == t.device and v.dim() == 1 and v.is_contiguous() for v in got.values())
    assert torch.equal(t, keep[0]) and (x is None or torch.equal(x.view(torch.uint8), keep[1].view(torch.uint8)))      # inputs unchanged
    check_against_host(name, {k: v.cpu().numpy() for k, v in got.items()})


@pytest.mark.parametrize("name", C.NAMES)
def test_numpy_in_with_device_numpy_out(torch, name):
    lbl, img = C.case(name)
    check_against_host(name, measure(lbl, img, device="cuda"))


def test_other_calling_forms(torch):
    lbl, img = C.case("2d_u16")
    t = torch.as_tensor(lbl, device="cuda")
    check_against_host("2d_u16", measure(t, img))                            # an image that is elsewhere is moved to the labels
    check_against_host("2d_u16", measure(t, torch.from_numpy(img.copy())))
    check_against_host("2d_u16", measure(torch.from_numpy(lbl.copy()), img, device="cuda"))
    check_against_host("2d_u16", measure(t.to(torch.int64), torch.as_tensor(img, device="cuda")))
    tr = torch.as_tensor(np.ascontiguousarray(lbl.T), device="cuda").T      # views that are not contiguous
    xr = torch.as_tensor(np.ascontiguousarray(img.T), device="cuda").T
    assert not tr.is_contiguous() and not xr.is_contiguous()
    check_against_host("2d_u16", measure(tr, xr))
    # dtypes the kernels do not take: through the host code, back as asked
    wide = measure(t, torch.as_tensor(img.astype(np.float64), device="cuda"), as_tensors=True)
    assert all(v.is_cuda for v in wide.values()) and wide["min_intensity"].dtype == torch.float64
    host = C.host("2d_u16")
    assert np.array_equal(wide["label"].cpu().numpy(), host["label"]) and np.array_equal(wide["max_intensity"].cpu().numpy(), host["max_intensity"])
    with pytest.raises(ValueError, match="integer"):
        measure(t.to(torch.float32), img)
    with pytest.raises(ValueError, match="2D or 3D"):
        measure(torch.zeros((2, 3, 4, 5), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="shape"):
        measure(t, torch.zeros((67, 130), device="cuda"))
    e = measure(torch.zeros((0, 5), dtype=torch.int32, device="cuda"), as_tensors=True)
    assert all(v.shape == (0,) and v.is_cuda for v in e.values())


@pytest.mark.parametrize("name", C.FLOAT_RANDOM + ("non_finite",))
def test_two_calls_give_the_same_bits(torch, name):
    lbl, img = C.case(name)
    t, x = torch.as_tensor(lbl, device="cuda"), torch.as_tensor(img, device="cuda")
    one = measure(t, x, as_tensors=True)
    filler = measure(torch.as_tensor(C.case("chunked_f32_random")[0], device="cuda"), as_tensors=True)     # other work in between
    two = measure(t.clone(), x.clone(), as_tensors=True)
    assert len(filler["label"]) > 0
    for k in one:
        a, b = one[k].cpu().numpy(), two[k].cpu().numpy()
        assert a.tobytes() == b.tobytes() or (name == "non_finite" and np.array_equal(a, b, equal_nan=True)), k


def tables(torch, lbl, img, top=None, fill=None):
    """(boxes, sums (top + 1, C, 2), minmax (top + 1, C, 2)) of the C entry points as numpy arrays; the output tables start as `fill`"""
    from stardist_amd.lib import _native as N
    lab = torch.as_tensor(np.ascontiguousarray(np.maximum(lbl, 0), np.int32), device="cuda")
    x = torch.as_tensor(np.ascontiguousarray(img), device="cuda")
    C_ = 1 if img.ndim == lbl.ndim else img.shape[-1]
    top = int(lab.max()) if top is None else top
    code = {"uint8": 0, "uint16": 1, "float32": 2}[img.dtype.name]
    zyx = ((1,) + lbl.shape) if lbl.ndim == 2 else lbl.shape
    boxes = torch.empty((top + 1, 6), dtype=torch.int32, device="cuda")
    sums = torch.full((top + 1, C_, 2), float("nan") if fill is None else fill, dtype=torch.float64, device="cuda")
    mm = torch.full((top + 1, C_, 2), float("nan") if fill is None else fill, dtype=torch.float32, device="cuda")
    if code != 2:
        sums, mm = sums.view(torch.int64), mm.view(torch.int32)             # the NaNs' bits
    vp = lambda a: ctypes.c_void_p(a.data_ptr())
    N.dcall(lab, "sd_label_boxes_device", vp(lab), *zyx, top, vp(boxes))
    N.dcall(lab, "sd_label_intensity_stats_device", vp(lab), *zyx, top, vp(boxes), vp(x), code, C_, vp(sums) if code != 2 else None,
            vp(sums) if code == 2 else None, vp(mm))
    return boxes.cpu().numpy(), sums.cpu().numpy(), mm.cpu().numpy()


@pytest.mark.parametrize("name", C.FLOAT_EXACT + C.FLOAT_RANDOM + ("2d_u8_rgb", "chunked_u16"))
def test_entry_point_tables_and_sentinel_rows(torch, name):
    """the C entry point on NaN-filled tables, with three ids beyond the largest label: absent rows hold the documented sentinel; the
    sums of squares of the float cases against math.fsum (bit for bit on the exact cases)"""
    lbl, img = C.case(name)
    want = C.host(name)
    top = int(lbl.max()) + 3
    _, sums, mm = tables(torch, lbl, img, top=top)
    rows = want["label"]
    absent = np.setdiff1d(np.arange(top + 1), rows)
    assert 0 in absent and top in absent and len(absent) > 10
    assert (sums[absent] == 0).all()
    if img.dtype == np.float32:
        assert np.isposinf(mm[absent][..., 0]).all() and np.isneginf(mm[absent][..., 1]).all()
    else:
        assert (mm[absent][..., 0] == 2 ** 31 - 1).all() and (mm[absent][..., 1] == -2 ** 31).all()
    S, S2 = sums[rows][..., 0], sums[rows][..., 1]
    chan = img.ndim > lbl.ndim
    col = lambda key: np.stack([want["%s-%d" % (key, c)] for c in range(S.shape[1])], axis=1) if chan else want[key][:, None]
    assert np.array_equal(mm[rows][..., 0], col("min_intensity")) and np.array_equal(mm[rows][..., 1], col("max_intensity"))
    if img.dtype != np.float32:
        planes = img.reshape(lbl.shape + (-1,)).astype(np.int64)
        assert np.array_equal(S, col("sum_intensity"))
        assert np.array_equal(S2, np.stack([(planes[lbl == l] ** 2).sum(axis=0) for l in rows]))
        return
    o = C.float_oracle(name)
    if name in C.FLOAT_EXACT:
        assert np.array_equal(S, o["S"]) and np.array_equal(S2, o["S2"])
    else:
        bS, bS2 = C.sum_bounds(o)
        assert (np.abs(S - o["S"]) <= bS).all() and (np.abs(S2 - o["S2"]) <= bS2).all()


def test_integer_sums_beyond_2_53(torch):
    lbl, img = C.case("all_65535")
    _, sums, mm = tables(torch, lbl, img)
    n = 1500 * 1500
    assert n * 65535 ** 2 > 2 ** 53 and int(np.float64(2 ** 53 + 65535 ** 2)) != 2 ** 53 + 65535 ** 2      # float64 partial sums round
    assert sums[1, 0].tolist() == [n * 65535, n * 65535 ** 2] and mm[1, 0].tolist() == [65535, 65535]


def test_bad_arguments(torch):
    from stardist_amd.lib import _native as N
    t = torch.zeros((4, 5), dtype=torch.int32, device="cuda")
    img = torch.ones((4, 5), dtype=torch.float32, device="cuda")
    boxes = torch.zeros((3, 6), dtype=torch.int32, device="cuda")
    fs = torch.full((3, 1, 2), 7.0, dtype=torch.float64, device="cuda")
    mm = torch.full((3, 1, 2), 7.0, dtype=torch.float32, device="cuda")
    p, x, b, f, m = (ctypes.c_void_p(a.data_ptr()) for a in (t, img, boxes, fs, mm))
    fn = N.lib().sd_label_intensity_stats_device
    good = [p, 1, 4, 5, 2, b, x, 2, 1, None, f, m]
    bad = {0: None, 1: 0, 2: -1, 3: 0, 4: -1, 5: None, 6: None, 7: 3, 8: 0, 10: None, 11: None}
    for at, value in bad.items():
        args = list(good)
        args[at] = value
        assert fn(*args, N.current_stream()) == -1, at
        assert "sd_label_intensity_stats" in N.lib().sd_last_error().decode()
    for extra in ({7: -1}, {8: 65}, {7: 0}, {7: 1}):                        # an integer dtype needs the int64 table
        args = list(good)
        for at, value in extra.items():
            args[at] = value
        assert fn(*args, N.current_stream()) == -1
    torch.cuda.synchronize()
    assert (fs == 7).all() and (mm == 7).all()                              # nothing was launched
    assert N.lib().sd_label_boxes_device(p, 1, 4, 5, 2, b, N.current_stream()) == 0
    assert fn(*good, N.current_stream()) == 0
    torch.cuda.synchronize()
    assert (fs == 0).all() and torch.isinf(mm).all()                        # no objects: every row is the sentinel


def test_offsets_past_2_31(torch):
    """32769 x 65537 int32 labels made on the device, a few small objects in the last rows (flat offsets beyond 2^31), uint8 image;
    expected values from the host route on the crop of the last rows"""
    Y, X, tail = 32769, 65537, 12
    assert (Y - 1) * X > 2 ** 31
    rng = np.random.default_rng(4160)
    crop = np.zeros((tail, X), np.int32)
    spots = [(2, 5, 1), (1, 30000, 2), (4, 65520, 3), (7, 65528, 5), (0, 40000, 9)]
    for y, x, l in spots:
        crop[y:y + 5, x:x + 7] = l
    crop[tail - 1, X - 1] = 11                                              # the image's last pixel
    crop_img = rng.integers(0, 256, crop.shape, dtype=np.uint8)
    lbl = torch.zeros((Y, X), dtype=torch.int32, device="cuda")
    img = torch.zeros((Y, X), dtype=torch.uint8, device="cuda")
    lbl[Y - tail:] = torch.as_tensor(crop, device="cuda")
    img[Y - tail:] = torch.as_tensor(crop_img, device="cuda")
    got = {k: v.cpu().numpy() for k, v in measure(lbl, img, as_tensors=True).items()}
    del lbl, img
    want = measure(crop, crop_img)
    assert want["label"].tolist() == [1, 2, 3, 5, 9, 11] and want["area"].tolist() == [35] * 5 + [1]
    for k in want:
        shift = (Y - tail) if k in ("bbox-0", "bbox-2", "centroid-0") else 0
        assert np.array_equal(got[k], want[k] + shift), k
