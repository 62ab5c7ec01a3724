"""GPU: stardist_amd.utils.measure_labels(hull=True) on device input (csrc/measure_hull.hip with the box and centroid-sum kernels)
against the host route on the cases of tests/_hull_cases.py, every column with ==: the 65535 4 x 4 patterns and the same image shifted
through the positions of a wave and a workgroup, objects taller than the LDS tier (a 5003-row diagonal, its transpose, an object that
fills a 2048 x 2048 image), corners, a split label, labels inside another's hull, negative labels, ids with gaps and ids that need
compaction; tensors in and out; the C entry point on a sentinel-filled table, twice with other work in between, with ids beyond
max_label and with bad arguments; hull together with shape, percentiles and neighbors; offsets past 2^31."""
import ctypes

import numpy as np
import pytest

import _hull_cases as H
import _measure_cases as M
import _shape_cases as S

pytestmark = pytest.mark.gpu

NEIGHBOR_KEYS = ["neighbors", "contact_objects", "contact_background"]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def measure(*a, **kw):
    from stardist_amd.utils import measure_labels
    return measure_labels(*a, **kw)


def check_against_host(name, got):
    want = H.host(name)
    assert list(got) == list(want) == M.keys(2) + H.HULL_KEYS
    for k in want:
        assert isinstance(got[k], np.ndarray) and got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (name, k)
        assert np.array_equal(got[k], want[k]), (name, k)


@pytest.mark.parametrize("name", H.SMALL + ("patterns4x4", "diagonal", "diagonal_t", "whole"))
def test_numpy_in_with_device_numpy_out(torch, name):
    """the raw columns come back in one copy and the columns are derived by numpy: every column is the host route's"""
    check_against_host(name, measure(H.case(name), hull=True, device="cuda"))


def test_the_patterns_shifted_through_the_waves(torch):
    """the hull columns do not change when an object moves; label and area neither, the boxes by the shift"""
    want = H.host("patterns4x4")
    got = measure(torch.as_tensor(H.case("patterns4x4_shifted"), device="cuda"), hull=True)
    assert list(got) == list(want)
    for k in ["label", "area"] + H.HULL_KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    for k, shift in (("bbox-0", 3), ("bbox-1", 2), ("bbox-2", 3), ("bbox-3", 2)):
        assert np.array_equal(got[k], want[k] + shift), k


@pytest.mark.parametrize("name", ("random_masks", "ellipses", "split", "border", "gaps", "huge_ids", "corners", "empty", "diagonal"))
def test_tensors_in_tensors_out(torch, name):
    t = torch.as_tensor(H.case(name), device="cuda")
    keep = t.clone()
    got = measure(t, hull=True, as_tensors=True)
    assert all(isinstance(v, torch.Tensor) and v.device == t.device and v.dim() == 1 and v.is_contiguous() for v in got.values())
    assert torch.equal(t, keep)                                             # the input is unchanged
    assert got["convex_area"].dtype == torch.int64 and got["solidity"].dtype == got["feret_diameter_max"].dtype == torch.float64
    check_against_host(name, {k: v.cpu().numpy() for k, v in got.items()})


def entry_point(torch, lbl, top=None, fill=-3):
    """the table (top + 1, 2) of sd_label_hull_device as a numpy array; it starts as `fill`"""
    from stardist_amd.lib import _native as N
    lab = torch.as_tensor(np.ascontiguousarray(lbl.astype(np.int64).clip(-1, 2 ** 31 - 1), np.int32), device="cuda")
    top = int(lab.max()) if top is None else top
    vp = lambda a: ctypes.c_void_p(a.data_ptr())
    boxes = torch.empty((top + 1, 6), dtype=torch.int32, device="cuda")
    table = torch.full((top + 1, 2), fill, dtype=torch.int64, device="cuda")
    N.dcall(lab, "sd_label_boxes_device", vp(lab), 1, *lab.shape, top, vp(boxes))
    N.dcall(lab, "sd_label_hull_device", vp(lab), *lab.shape, top, vp(boxes), vp(table))
    return table.cpu().numpy()


def integers(table):
    f2 = np.rint(table["feret_diameter_max"] ** 2 * 4).astype(np.int64)
    assert np.array_equal(H.feret(f2), table["feret_diameter_max"])
    return np.stack([table["convex_area"], f2], axis=1)


@pytest.mark.parametrize("name", ("random_masks", "ellipses", "lines", "split", "border", "gaps", "corners"))
def test_entry_point_writes_every_row_and_repeats(torch, name):
    """a sentinel-filled table, three ids beyond the largest label; called twice with an unrelated larger call in between: the same
    bits, the rows of absent labels 0, the rows present the host route's"""
    lbl = H.case(name)
    want = H.host(name)
    top = int(lbl.max()) + 3
    one = entry_point(torch, lbl, top=top, fill=-3)
    filler = entry_point(torch, H.case("lines"), fill=7)
    two = entry_point(torch, lbl, top=top, fill=2 ** 62)
    assert filler.any()
    rows = want["label"]
    absent = np.setdiff1d(np.arange(top + 1), rows)
    assert 0 in absent and top in absent
    assert one.tobytes() == two.tobytes()
    assert (one[absent] == 0).all() and np.array_equal(one[rows], integers(want))


def test_two_calls_give_identical_bits(torch):
    t = torch.as_tensor(H.case("ellipses"), device="cuda")
    a = measure(t, hull=True, as_tensors=True)
    measure(torch.as_tensor(H.case("random_masks"), device="cuda"), hull=True)
    b = measure(t, hull=True, as_tensors=True)
    assert all(torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)) for k in a)


def test_ids_above_max_label_are_background(torch):
    lbl = H.case("border")
    top = 6
    want = H.brute_force(np.where(lbl <= top, lbl, 0))
    out = entry_point(torch, lbl, top=top)
    assert sorted(want) == [l for l in range(top + 1) if out[l].any()]
    assert all(tuple(out[l]) == want[l] for l in want)


def test_bad_arguments(torch):
    from stardist_amd.lib import _native as N
    t = torch.zeros((4, 5), dtype=torch.int32, device="cuda")
    boxes = torch.zeros((3, 6), dtype=torch.int32, device="cuda")
    table = torch.full((3, 2), 7, dtype=torch.int64, device="cuda")
    p, b, h = (ctypes.c_void_p(a.data_ptr()) for a in (t, boxes, table))
    hull = N.lib().sd_label_hull_device
    good = [p, 4, 5, 2, b, h]
    for at, value in ((0, None), (1, 0), (1, 2 ** 30), (2, -1), (2, 2 ** 30), (3, -1), (4, None), (5, None)):
        args = list(good)
        args[at] = value
        assert hull(*args, N.current_stream()) == -1, at
        assert "sd_label_hull" in N.lib().sd_last_error().decode()
    torch.cuda.synchronize()
    assert (table == 7).all()                                               # nothing was launched
    assert N.lib().sd_label_boxes_device(p, 1, 4, 5, 2, b, N.current_stream()) == 0
    assert hull(*good, N.current_stream()) == 0
    torch.cuda.synchronize()
    assert (table == 0).all()                                               # no objects: every row is written, as 0


def test_hull_with_shape_percentiles_and_neighbors(torch):
    lbl, img = M.case("2d_u8_rgb")
    lbl = np.maximum(lbl, 0)                                                # neighbors= refuses the case's negative label
    kw = dict(shape=True, hull=True, percentiles=(50, 99.8), neighbors=2)
    want = measure(lbl, img, **kw)
    keys = list(want)
    at = keys.index("convex_area")
    assert keys[at:] == H.HULL_KEYS + NEIGHBOR_KEYS and keys[at - 1] == S.shape_keys(2)[-1]
    t, x = torch.as_tensor(lbl, device="cuda"), torch.as_tensor(img, device="cuda")
    for got in (measure(t, x, **kw), {k: v.cpu().numpy() for k, v in measure(t, x, as_tensors=True, **kw).items()}, measure(lbl, img, device="cuda", **kw)):
        assert list(got) == keys
        for k in keys:
            assert got[k].dtype == want[k].dtype, k
            if k == "orientation":
                assert (np.abs(got[k] - want[k]) <= 1e-14 * np.maximum(np.abs(want[k]), 1)).all()      # atan2: as tests/test_gpu_measure_shape.py
            else:
                assert np.array_equal(got[k], want[k]), k
    plain = measure(t, x, shape=True, percentiles=(50, 99.8), neighbors=2)     # without hull: today's table
    assert list(plain) == [k for k in keys if k not in H.HULL_KEYS]


def test_other_calling_forms(torch):
    lbl = H.case("ellipses")
    want = H.host("ellipses")

    def check(got, want=want):
        assert list(got) == list(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    t = torch.as_tensor(lbl, device="cuda")
    check(measure(torch.from_numpy(lbl.copy()), hull=True, device="cuda"))
    check(measure(t.to(torch.int64), hull=True))
    tr = torch.as_tensor(np.ascontiguousarray(lbl.T), device="cuda").T      # a view that is not contiguous
    assert not tr.is_contiguous()
    check(measure(tr, hull=True))
    check(measure(t - (t == 0).to(torch.int32) * 5, hull=True))              # a negative background
    huge = measure(torch.as_tensor(H.case("huge_ids"), device="cuda"), hull=True)      # ids that need compaction: the originals come back
    check(huge, H.host("huge_ids"))
    assert huge["label"].min() > 2 ** 40
    with pytest.raises(ValueError, match="hull=True takes a 2D"):
        measure(torch.zeros((3, 4, 5), dtype=torch.int32, device="cuda"), hull=True)
    e = measure(torch.zeros((0, 5), dtype=torch.int32, device="cuda"), hull=True, as_tensors=True)
    assert list(e) == M.keys(2) + H.HULL_KEYS and all(v.shape == (0,) and v.is_cuda for v in e.values())
    assert e["convex_area"].dtype == torch.int64 and e["solidity"].dtype == torch.float64
    plain = measure(t)                                                      # without hull: today's table
    assert list(plain) == M.keys(2) and all(np.array_equal(plain[k], want[k]) for k in plain)


def test_offsets_past_2_31(torch):
    """46349 x 46351 int32 labels made on the device, a few objects in the last rows (flat offsets beyond 2^31); expected values from
    the host route on the crop of the last rows"""
    Y, X, tail = 46349, 46351, 12
    assert (Y - tail) * X > 2 ** 31
    free = torch.cuda.mem_get_info()[0]
    if free < 5 * 4 * Y * X:
        pytest.skip("needs %.0f GB of free device memory, %.0f are free" % (5 * 4 * Y * X / 1e9, free / 1e9))
    crop = np.zeros((tail, X), np.int32)
    for y, x, l in [(2, 5, 1), (1, 30000, 2), (4, 46330, 3), (7, 46340, 5), (0, 40000, 9)]:
        crop[y:y + 5, x:x + 7] = l
    crop[4, 7] = crop[5, 8] = crop[4, 8] = 0                                # a dent
    crop[3, 46320] = 3                                                      # a part of its own, ten columns away
    crop[tail - 1, X - 1] = 11                                              # the image's last pixel
    lbl = torch.zeros((Y, X), dtype=torch.int32, device="cuda")
    lbl[Y - tail:] = torch.as_tensor(crop, device="cuda")
    got = {k: v.cpu().numpy() for k, v in measure(lbl, hull=True, as_tensors=True).items()}
    del lbl
    want = measure(crop, hull=True)
    assert want["label"].tolist() == [1, 2, 3, 5, 9, 11] and (want["solidity"] < 1).sum() >= 2
    for k in ["label", "area"] + H.HULL_KEYS:
        assert np.array_equal(got[k], want[k]), k
    for k in ("bbox-0", "bbox-1", "bbox-2", "bbox-3"):
        assert np.array_equal(got[k], want[k] + ((Y - tail) if k in ("bbox-0", "bbox-2") else 0)), k
