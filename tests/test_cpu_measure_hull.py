"""CPU: stardist_amd.utils.measure_labels(hull=True) on host input.  The two integers per object (convex_area, F2) against a brute-force
statement of the definition (all diamond points, a monotone chain over the sorted points, half-plane tests over the whole box, all
pairs), on every non-empty 4 x 4 pattern and on random masks, ellipses, two-pixel objects, lines, split labels, border objects and ids
with gaps; the three columns against scikit-image 0.18.3's regionprops_table (tests/golden/hull_reference.npz) with ==; the per-object
code of the kernels (csrc/measure_hull.h through tests/host/measure_hull_check.cpp, everything visited in two orders) against the host
route with ==; keys, order, dtypes, errors and host tensors.  Cases: tests/_hull_cases.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _hull_cases as H
import _measure_cases as M
import _shape_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "measure_hull_check.cpp")
_vp, _i = ctypes.c_void_p, ctypes.c_int
NEIGHBOR_KEYS = ["neighbors", "contact_objects", "contact_background"]


def measure(*a, **kw):
    from stardist_amd.utils import measure_labels
    return measure_labels(*a, **kw)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "hull_reference.npz"))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("measure_hull") / "libmeasure_hull.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", so], check=True)
    l = ctypes.CDLL(so)
    l.mh_lds_rows.restype = l.mh_max_extent.restype = l.mh_label_hull.restype = _i
    l.mh_label_hull.argtypes = [_vp, _i, _i, _i, _vp, _i]
    return l


def integers(table):
    """(convex_area, F2) of a table's rows: F2 back from feret_diameter_max = sqrt(F2 / 4), exact while F2 < 2^52"""
    f2 = np.rint(table["feret_diameter_max"] ** 2 * 4).astype(np.int64)
    assert np.array_equal(H.feret(f2), table["feret_diameter_max"])
    return table["convex_area"], f2


def test_constants_are_the_header_s(lib):
    from stardist_amd import label_ops
    txt = open(os.path.join(ROOT, "stardist_amd", "csrc", "measure_hull.h")).read()
    assert re.findall(r"\bMH_LDS_ROWS\s*=\s*(\d+)", txt) == [str(H.MH_LDS_ROWS)] and lib.mh_lds_rows() == H.MH_LDS_ROWS
    assert lib.mh_max_extent() == label_ops._HULL_MAX_EXTENT == 2 ** 30


def test_cases_are_what_they_say():
    p = H.case("patterns4x4")
    assert p.shape == (1280, 1280) and len(np.unique(p)) == 65536 and p.max() == 65535
    for l, rows in ((0xF99F, ("1111", "1001", "1001", "1111")), (0x8421, ("1000", "0100", "0010", "0001")), (0x9009, ("1001", "0000", "0000", "1001"))):
        y, x = (l - 1) // 256 * 5, (l - 1) % 256 * 5
        assert ["".join(str(int(v == l)) for v in row) for row in p[y:y + 4, x:x + 4]] == list(rows)
    assert np.array_equal(H.case("patterns4x4_shifted")[3:, 2:1282], p) and H.case("patterns4x4_shifted").shape == (1283, 1283)
    assert len(H.random_mask_list()) == 3 * 13 * 13 and {m.shape for m in H.random_mask_list()} == {(h, w) for h in range(1, 14) for w in range(1, 14)}
    assert len(H.two_pixel_list()) == 2 * len(H.TWO_PIXEL_OFFSETS) and all(m.sum() == 2 or m.shape == (1, 1) for m in H.two_pixel_list())
    s = H.case("split")
    ys = np.nonzero(s == 5)[0]
    assert set(np.unique(s)) == {0, 2, 5, 9} and ys.max() - ys.min() > H.MH_LDS_ROWS and not (s[10:65] == 5).any()
    t = H.host("split")
    assert t["convex_area"][1] > t["area"][1] + t["area"][0]               # object 2 lies in 5's hull and counts
    d = H.case("diagonal")
    assert d.shape[0] > 4 * H.MH_LDS_ROWS and (d == 3).sum() == d.shape[0] and H.case("whole").shape == (2048, 2048)
    assert (H.case("gaps") < 0).any() and H.case("huge_ids").max() > 2 ** 40 and H.case("huge_ids").dtype == np.int64
    b = H.case("border")
    assert b[0, 0] and b[0, -1] and b[-1, 0] and b[-1, -1] and b[0].any() and b[-1].any() and b[:, 0].any() and b[:, -1].any()


@pytest.mark.parametrize("name", H.SMALL)
def test_host_route_equals_the_definition(name):
    lbl = H.case(name)
    t = H.host(name)
    want = H.brute_force(lbl)
    assert t["label"].tolist() == sorted(want)
    assert t["convex_area"].dtype == np.int64 and t["solidity"].dtype == t["feret_diameter_max"].dtype == np.float64
    assert t["convex_area"].tolist() == [want[l][0] for l in sorted(want)]
    assert np.array_equal(t["feret_diameter_max"], H.feret([want[l][1] for l in sorted(want)]))
    assert np.array_equal(integers(t)[1], np.array([want[l][1] for l in sorted(want)], np.int64))
    assert np.array_equal(t["solidity"], t["area"].astype(np.float64) / t["convex_area"].astype(np.float64))


def test_host_route_equals_the_definition_on_every_4x4_pattern():
    t = H.host("patterns4x4")
    assert t["label"].tolist() == list(range(1, 65536))
    area, f2 = integers(t)
    bits = (np.arange(1, 65536)[:, None] >> np.arange(16)) & 1 == 1
    seen = set()
    for v, m in enumerate(bits.reshape(-1, 4, 4), 1):
        ys, xs = np.nonzero(m)
        want = H.brute_force_mask(m[ys.min():ys.max() + 1, xs.min():xs.max() + 1])
        assert (int(area[v - 1]), int(f2[v - 1])) == want, (v, want)
        seen.add(want)
    assert (16, 4 * 16 + 4 * 9) in seen and (1, 4) in seen and len(seen) > 50


def test_pixel_centres_on_a_hull_edge_belong_to_the_convex_image():
    """two pixels at offset (2, 1): the hull's edges (0, -1) - (4, 1) and (0, 1) - (4, 3) pass exactly through the centres (2, 0) and
    (2, 2) of the middle row, which count (cross == 0), as in scikit-image (the golden holds this case and its mirror).  The hull is at
    least one pixel wide at the height of every row's centres between its first and last row (it is that wide at both ends and
    convex), so no row in between is empty."""
    lbl = np.zeros((3, 2), np.int32)
    lbl[0, 0] = lbl[2, 1] = 1
    for a in (lbl, lbl[:, ::-1], lbl.T):
        t = measure(np.ascontiguousarray(a), hull=True)
        assert t["convex_area"].tolist() == [4] and t["solidity"].tolist() == [0.5]
        assert t["feret_diameter_max"].tolist() == [np.sqrt((6 * 6 + 2 * 2) / 4.0)]
    for name in H.SMALL + ("patterns4x4",):
        assert (H.host(name)["convex_area"] >= H.host(name)["bbox-2"] - H.host(name)["bbox-0"]).all()    # a pixel in every row


@pytest.mark.parametrize("name", H.GOLDEN)
def test_columns_equal_scikit_image(golden, name):
    g = lambda key: golden["%s/%s" % (name, key)]
    assert str(golden["skimage_version"]) == "0.18.3"
    assert np.array_equal(H.case(name), g("lbl"))                            # the generator still makes the case the golden was made for
    t = H.host(name)
    assert np.array_equal(t["label"], g("label")) and np.array_equal(t["area"], g("area")) and len(t["label"]) > 0
    for k in H.HULL_KEYS:
        assert t[k].dtype == g(k).dtype and np.array_equal(t[k], g(k)), k


def harness(lib, lbl, top=None, backwards=0):
    lab = np.ascontiguousarray(lbl.astype(np.int64).clip(-1, 2 ** 31 - 1), np.int32)
    top = int(max(lab.max(), 0)) if top is None else top
    out = np.full((top + 1, 2), -3, np.int64)
    assert lib.mh_label_hull(lab.ctypes.data, *lab.shape, top, out.ctypes.data, backwards) == 0
    return out


@pytest.mark.parametrize("name", [n for n in H.SMALL if n not in ("huge_ids", "empty")] + ["patterns4x4", "diagonal", "diagonal_t", "whole"])
def test_harness_equals_host_route(lib, name):
    """the per-object code of the kernels, forwards and backwards: every row written, absent rows 0, present rows the host's"""
    lbl = H.case(name)
    t = H.host(name)
    rows = t["label"]
    area, f2 = integers(t)
    for backwards in (0, 1):
        out = harness(lib, lbl, backwards=backwards)
        absent = np.setdiff1d(np.arange(len(out)), rows)
        assert 0 in absent and (out[absent] == 0).all()
        assert np.array_equal(out[rows, 0], area) and np.array_equal(out[rows, 1], f2)


def test_harness_ids_above_max_label_are_background_and_bad_arguments(lib):
    lbl = H.case("border")
    top = 6
    want = H.brute_force(np.where(lbl <= top, lbl, 0))
    out = harness(lib, lbl, top=top)
    assert sorted(want) == [l for l in range(top + 1) if out[l].any()]
    assert all(tuple(out[l]) == want[l] for l in want)
    assert lib.mh_label_hull(None, 4, 4, 1, out.ctypes.data, 0) == -1
    assert lib.mh_label_hull(lbl.ctypes.data, 2 ** 30, 1, 1, out.ctypes.data, 0) == -1


def test_stand_alone_sanitizer_build_passes(tmp_path):
    exe = str(tmp_path / "measure_hull_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMEASURE_HULL_CHECK_MAIN",
                    SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def combos():
    lbl, img = M.case("2d_u8_rgb")
    lbl = np.maximum(lbl, 0)                                                # neighbors= refuses the case's negative label
    for with_img in (False, True):
        for shape in (False, True):
            for pct in (None, (50, 99.8)):
                for nb in (None, 1, 2):
                    if pct and not with_img:
                        continue
                    kw = dict(shape=shape, percentiles=pct, neighbors=nb)
                    yield lbl, (img if with_img else None), kw


def expected_keys(lbl, img, kw, hull):
    keys = M.keys(lbl.ndim) if img is None else M.case_keys("2d_u8_rgb")
    if kw["percentiles"]:
        keys = keys + ["p%g_intensity-%d" % (q, c) for q in kw["percentiles"] for c in range(img.shape[-1])]
    keys = keys + (S.shape_keys(lbl.ndim) if kw["shape"] else []) + (H.HULL_KEYS if hull else [])
    return keys + (NEIGHBOR_KEYS if kw["neighbors"] is not None else [])


def test_without_hull_the_table_is_today_s_and_the_order_with_it():
    """for every combination of img / shape / percentiles / neighbors: without hull (absent or False) the columns, their order and
    dtypes are the documented ones and equal the same columns of the call with hull=True, which adds its three after the shape columns
    and before the neighbour columns"""
    for lbl, img, kw in combos():
        plain, off, full = measure(lbl, img, **kw), measure(lbl, img, hull=False, **kw), measure(lbl, img, hull=True, **kw)
        assert list(plain) == list(off) == expected_keys(lbl, img, kw, False), kw
        assert list(full) == expected_keys(lbl, img, kw, True), kw
        for k in plain:
            assert plain[k].dtype == off[k].dtype == full[k].dtype, k
            assert np.array_equal(plain[k], full[k], equal_nan=True) and np.array_equal(plain[k], off[k], equal_nan=True), k
        for k in H.HULL_KEYS:
            assert np.array_equal(full[k], measure(lbl, hull=True)[k]), k


def test_without_hull_the_native_calls_are_today_s(monkeypatch):
    """the two halves are called without a hull keyword unless hull=True: what runs for today's calls is what ran before"""
    from stardist_amd import label_ops
    seen = []
    real = label_ops._measure_raw_host
    monkeypatch.setattr(label_ops, "_measure_raw_host", lambda *a, **k: seen.append(sorted(k)) or real(*a, **k))
    monkeypatch.setattr(label_ops, "_hull_raw_host", lambda *a, **k: pytest.fail("the hull code ran"))
    lbl = H.case("border")
    measure(lbl)
    measure(lbl, hull=False, shape=True)
    assert seen == [[], ["shape"]]


def test_an_empty_table_has_empty_hull_columns():
    for lbl in (H.case("empty"), np.zeros((0, 5), np.int32)):
        t = measure(lbl, hull=True)
        assert list(t) == M.keys(2) + H.HULL_KEYS
        assert [(t[k].shape, t[k].dtype) for k in H.HULL_KEYS] == [((0,), np.int64), ((0,), np.float64), ((0,), np.float64)]


def test_argument_errors(monkeypatch):
    from stardist_amd import label_ops
    monkeypatch.setattr(label_ops, "_measure_raw_host", lambda *a, **k: pytest.fail("something ran"))
    monkeypatch.setattr(label_ops, "_measure_raw_device", lambda *a, **k: pytest.fail("something ran"))
    one = np.zeros(1, np.int32)
    for dev in (None, "cuda"):
        with pytest.raises(ValueError, match="hull=True takes a 2D"):
            measure(np.zeros((3, 4, 5), np.int32), hull=True, device=dev)
        for shape in ((2 ** 30, 1), (1, 2 ** 30), (2 ** 30 + 5, 2)):
            with pytest.raises(ValueError, match="2\\^30"):
                measure(np.lib.stride_tricks.as_strided(one, shape=shape, strides=(0, 0)), hull=True, device=dev)
        with pytest.raises(ValueError, match="2D or 3D"):
            measure(np.zeros(7, np.int32), hull=True, device=dev)
    with pytest.raises(TypeError):
        measure(np.zeros((4, 5), np.int32), None, False, True)              # keyword only


def test_an_extent_just_below_the_limit_is_taken(monkeypatch):
    from stardist_amd import label_ops
    monkeypatch.setattr(label_ops, "_measure_raw_host", lambda *a, **k: (_ for _ in ()).throw(KeyError("reached")))
    with pytest.raises(KeyError, match="reached"):
        measure(np.lib.stride_tricks.as_strided(np.zeros(1, np.int32), shape=(2 ** 30 - 1, 1), strides=(0, 0)), hull=True)


@pytest.mark.parametrize("name", ("random_masks", "ellipses", "split", "gaps", "huge_ids", "empty"))
def test_host_tensors_against_numpy(name):
    """as_tensors=True on host tensors: the hull columns are + - * / sqrt of the integers, so == on every one"""
    import torch
    want = H.host(name)
    got = measure(torch.from_numpy(H.case(name).copy()), hull=True, as_tensors=True)
    assert list(got) == list(want)
    for k in want:
        assert isinstance(got[k], torch.Tensor) and got[k].device.type == "cpu" and got[k].dim() == 1
        assert got[k].numpy().dtype == want[k].dtype and np.array_equal(got[k].numpy(), want[k]), k


def test_the_abi_lists_the_entry_point():
    from stardist_amd.lib import _native
    header = open(os.path.join(ROOT, "include", "stardist_hip.h")).read()
    assert "sd_label_hull_device" in _native.SIGNATURES and re.search(r"\bint sd_label_hull_device\(", header)
    assert len(_native.SIGNATURES["sd_label_hull_device"][1]) == 7
