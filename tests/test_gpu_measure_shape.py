"""GPU: stardist_amd.utils.measure_labels(shape=True) on device input (csrc/measure_shape.hip with the box and centroid-sum kernels)
against the host route on the cases of tests/_shape_cases.py: every column with ==, the raw integer tables of the 65535 4 x 4 patterns
against a vectorised numpy oracle; tensors in and out (== but for the two columns that call atan2 / pow, which may differ by the two
maths libraries' rounding); the two C entry points on sentinel-filled tables, twice with other work in between, with ids beyond
max_label and with bad arguments; the other calling forms; offsets past 2^31."""
import ctypes

import numpy as np
import pytest

import _measure_cases as M
import _shape_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def measure(*a, **kw):
    from stardist_amd.utils import measure_labels
    return measure_labels(*a, **kw)


def libm_close(a, b):
    """the rule for orientation and the 3D equivalent_diameter: 1e-14 of max(|a|, |b|, 1) -- 45 ulp, above the 6 and 16 ulp the OpenCL
    conformance limits allow a device atan2 and pow, plus the host library's 1"""
    return (np.abs(a - b) <= 1e-14 * np.maximum(np.maximum(np.abs(a), np.abs(b)), 1)).all()


def check_against_host(name, got, exact_libm):
    want = S.host(name)
    nd = S.case(name).ndim
    assert list(got) == list(want) == M.keys(nd) + S.shape_keys(nd)
    for k in want:
        assert isinstance(got[k], np.ndarray) and got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (name, k)
        if not exact_libm and (k == "orientation" or (k == "equivalent_diameter" and nd == 3)):
            assert libm_close(got[k], want[k]), (name, k)
        else:
            assert np.array_equal(got[k], want[k]), (name, k)


@pytest.mark.parametrize("name", S.NAMES)
def test_numpy_in_with_device_numpy_out(torch, name):
    """the raw columns come back in one copy and the columns are derived by numpy: every column is the host route's"""
    check_against_host(name, measure(S.case(name), shape=True, device="cuda"), exact_libm=True)


@pytest.mark.parametrize("name", S.NAMES)
def test_tensors_in_tensors_out(torch, name):
    t = torch.as_tensor(S.case(name), device="cuda")
    keep = t.clone()
    got = measure(t, shape=True, as_tensors=True)
    assert all(isinstance(v, torch.Tensor) and v.device == t.device and v.dim() == 1 and v.is_contiguous() for v in got.values())
    assert torch.equal(t, keep)                                             # the input is unchanged
    check_against_host(name, {k: v.cpu().numpy() for k, v in got.items()}, exact_libm=False)


def entry_points(torch, lbl, top=None, fill=-3):
    """(m2 (top + 1, 6), counts (top + 1, 18) or None for a volume) of the two C entry points as numpy arrays; the tables start as `fill`"""
    from stardist_amd.lib import _native as N
    lab = torch.as_tensor(np.ascontiguousarray(lbl.astype(np.int64).clip(-1, 2 ** 31 - 1), np.int32), device="cuda")
    top = int(lab.max()) if top is None else top
    zyx = ((1,) + tuple(lab.shape)) if lab.dim() == 2 else tuple(lab.shape)
    vp = lambda a: ctypes.c_void_p(a.data_ptr())
    boxes = torch.empty((top + 1, 6), dtype=torch.int32, device="cuda")
    m2 = torch.full((top + 1, 6), fill, dtype=torch.int64, device="cuda")
    N.dcall(lab, "sd_label_boxes_device", vp(lab), *zyx, top, vp(boxes))
    N.dcall(lab, "sd_label_moment_sums_device", vp(lab), *zyx, top, vp(boxes), vp(m2))
    counts = None
    if lab.dim() == 2:
        counts = torch.full((top + 1, 18), fill, dtype=torch.int64, device="cuda")
        N.dcall(lab, "sd_label_contour_counts_device", vp(lab), *lab.shape, top, vp(counts))
    return m2.cpu().numpy(), None if counts is None else counts.cpu().numpy()


def test_all_4x4_patterns_against_the_vector_oracle(torch):
    lbl = S.case("patterns4x4")
    labels, m2_want, counts_want = S.vector_oracle(lbl)
    assert len(labels) == 65535
    m2, counts = entry_points(torch, lbl)
    assert (m2[0] == 0).all() and (counts[0] == 0).all()
    assert np.array_equal(m2[labels], m2_want) and np.array_equal(counts[labels], counts_want)
    got = measure(torch.as_tensor(lbl, device="cuda"), shape=True)
    assert np.array_equal(got["label"], labels)
    h = counts_want[:, 2:]
    assert np.array_equal(got["euler_number"], h[:, 8] - h[:, 6] - h[:, 14]) and got["euler_number"].min() < 0 < got["euler_number"].max()
    n = counts_want[:, :3].astype(np.float64)
    assert np.array_equal(got["perimeter"], n[:, 0] + n[:, 1] * np.sqrt(2) + n[:, 2] * ((1 + np.sqrt(2)) / 2))


@pytest.mark.parametrize("name", ("small_2d", "small_3d", "chunked", "blobs2d", "blobs3d", "edges-2+1", "edges+2-1", "row", "column", "one_pixel"))
def test_entry_points_write_every_row_and_repeat(torch, name):
    """sentinel-filled tables, three ids beyond the largest label; called twice with an unrelated larger call in between: the same
    bits, the rows of absent labels 0, the rows present the host route's"""
    lbl = S.case(name)
    raw = S.raw(name)
    top = int(lbl.max()) + 3
    one = entry_points(torch, lbl, top=top, fill=-3)
    filler = entry_points(torch, S.case("patterns4x4"), fill=7)            # 1536 x 1536: larger than every case here
    two = entry_points(torch, lbl, top=top, fill=2 ** 62)
    assert filler[0].any() and S.case("patterns4x4").size > lbl.size
    rows = raw["label"]
    absent = np.setdiff1d(np.arange(top + 1), rows)
    assert 0 in absent and top in absent
    for a, b, want in zip(one, two, (raw["m2"], raw.get("contour"))):
        if want is None:
            assert a is None and b is None
            continue
        assert a.tobytes() == b.tobytes()
        assert (a[absent] == 0).all() and np.array_equal(a[rows], want)


def test_ids_above_max_label_are_background(torch):
    lbl = S.case("edges-1+2")
    top = 20
    want = S.brute_force(np.where(lbl <= top, lbl, 0))
    m2, counts = entry_points(torch, lbl, top=top)
    assert sorted(want) == [l for l in range(top + 1) if counts[l].any()] and len(want) > 10
    for l, (wm, wc) in want.items():
        assert m2[l].tolist() == wm and counts[l].tolist() == wc


def test_bad_arguments(torch):
    from stardist_amd.lib import _native as N
    t = torch.zeros((4, 5), dtype=torch.int32, device="cuda")
    boxes = torch.zeros((3, 6), dtype=torch.int32, device="cuda")
    m2 = torch.full((3, 6), 7, dtype=torch.int64, device="cuda")
    counts = torch.full((3, 18), 7, dtype=torch.int64, device="cuda")
    p, b, m, c = (ctypes.c_void_p(a.data_ptr()) for a in (t, boxes, m2, counts))
    moments, contour = N.lib().sd_label_moment_sums_device, N.lib().sd_label_contour_counts_device
    good = [p, 1, 4, 5, 2, b, m]
    for at, value in {0: None, 1: 0, 2: -1, 3: 0, 4: -1, 5: None, 6: None}.items():
        args = list(good)
        args[at] = value
        assert moments(*args, N.current_stream()) == -1, at
        assert "sd_label_moment_sums" in N.lib().sd_last_error().decode()
    good2 = [p, 4, 5, 2, c]
    for at, value in {0: None, 1: 0, 2: -3, 3: -1, 4: None}.items():
        args = list(good2)
        args[at] = value
        assert contour(*args, N.current_stream()) == -1, at
        assert "sd_label_contour_counts" in N.lib().sd_last_error().decode()
    torch.cuda.synchronize()
    assert (m2 == 7).all() and (counts == 7).all()                          # nothing was launched
    assert N.lib().sd_label_boxes_device(p, 1, 4, 5, 2, b, N.current_stream()) == 0
    assert moments(*good, N.current_stream()) == 0 and contour(*good2, N.current_stream()) == 0
    torch.cuda.synchronize()
    assert (m2 == 0).all() and (counts == 0).all()                          # no objects: every row is written, as 0


def test_other_calling_forms(torch):
    """the forms of test_gpu_measure.py::test_other_calling_forms, with shape=True"""
    lbl, img = M.case("2d_u16")
    want = dict(M.host("2d_u16"))
    want.update({k: S.host("small_2d")[k] for k in S.shape_keys(2)})

    def check(got):
        assert list(got) == list(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    t = torch.as_tensor(lbl, device="cuda")
    check(measure(t, img, shape=True))                                      # an image that is elsewhere is moved to the labels
    check(measure(t, torch.from_numpy(img.copy()), shape=True))
    check(measure(torch.from_numpy(lbl.copy()), img, shape=True, device="cuda"))
    check(measure(t.to(torch.int64), torch.as_tensor(img, device="cuda"), shape=True))
    tr = torch.as_tensor(np.ascontiguousarray(lbl.T), device="cuda").T      # views that are not contiguous
    xr = torch.as_tensor(np.ascontiguousarray(img.T), device="cuda").T
    assert not tr.is_contiguous() and not xr.is_contiguous()
    check(measure(tr, xr, shape=True))
    # ids that need compaction: the device route reports the originals and the same shapes
    huge = measure(torch.as_tensor(S.case("huge_ids"), device="cuda"), shape=True)
    assert np.array_equal(huge["label"], M.huge_ids()[2])
    assert all(np.array_equal(huge[k], S.host("small_2d")[k]) for k in huge if k != "label")
    # dtypes the kernels do not take: through the host code, back as asked
    wide = measure(t, torch.as_tensor(img.astype(np.float64), device="cuda"), shape=True, as_tensors=True)
    assert all(v.is_cuda for v in wide.values()) and list(wide) == list(want)
    assert np.array_equal(wide["perimeter"].cpu().numpy(), want["perimeter"]) and np.array_equal(wide["euler_number"].cpu().numpy(), want["euler_number"])
    with pytest.raises(ValueError, match="integer"):
        measure(t.to(torch.float32), img, shape=True)
    with pytest.raises(ValueError, match="2D or 3D"):
        measure(torch.zeros((2, 3, 4, 5), dtype=torch.int32, device="cuda"), shape=True)
    with pytest.raises(ValueError, match="shape"):
        measure(t, torch.zeros((67, 130), device="cuda"), shape=True)
    for shape_ in ((0, 5), (0, 4, 5)):
        e = measure(torch.zeros(shape_, dtype=torch.int32, device="cuda"), shape=True, as_tensors=True)
        assert list(e) == M.keys(len(shape_)) + S.shape_keys(len(shape_))
        assert all(v.shape == (0,) and v.is_cuda for v in e.values()) and e["extent"].dtype == torch.float64
        assert len(shape_) == 3 or e["euler_number"].dtype == torch.int64
    plain = measure(t)                                                      # without shape: today's table
    assert list(plain) == M.keys(2) and all(np.array_equal(plain[k], M.host("2d_none")[k]) for k in plain)


def test_offsets_past_2_31(torch):
    """46349 x 46351 int32 labels made on the device -- past 2^31 pixels and, with (pixels) x (largest extent)^2 = 2^62.1, still a call
    shape=True accepts -- a few small objects in the last rows (flat offsets beyond 2^31); expected values from the host route on the
    crop of the last rows"""
    Y, X, tail = 46349, 46351, 12
    assert (Y - tail) * X > 2 ** 31 and Y * X * max(Y, X) ** 2 < 2 ** 63
    crop = np.zeros((tail, X), np.int32)
    for y, x, l in [(2, 5, 1), (1, 30000, 2), (4, 46330, 3), (7, 46340, 5), (0, 40000, 9)]:
        crop[y:y + 5, x:x + 7] = l
    crop[6, 46333] = 0                                                      # a hole
    crop[4, 7] = crop[5, 8] = 0                                             # a dent with a diagonal
    crop[tail - 1, X - 1] = 11                                              # the image's last pixel
    lbl = torch.zeros((Y, X), dtype=torch.int32, device="cuda")
    lbl[Y - tail:] = torch.as_tensor(crop, device="cuda")
    got = {k: v.cpu().numpy() for k, v in measure(lbl, shape=True, as_tensors=True).items()}
    del lbl
    # the crop starts at a row that is no multiple of the tile height, so its tiles are not the big image's: the tables must not care
    assert (Y - tail) % S.MSH_TILE_Y != 0
    want = measure(crop, shape=True)
    assert want["label"].tolist() == [1, 2, 3, 5, 9, 11]
    for k in want:
        shift = (Y - tail) if k in ("bbox-0", "bbox-2", "centroid-0") else 0
        if k == "orientation":
            assert libm_close(got[k], want[k]), k
        else:
            assert np.array_equal(got[k], want[k] + shift), k
