"""CPU: stardist_amd.utils.measure_labels on host input -- against an oracle written here from scipy.ndimage, against scikit-image
0.18's regionprops_table (tests/golden/measure_reference.npz), against math.fsum for the float sums -- and the summation order of the
device pass (csrc/measure.h through tests/host/measure_check.cpp: chunks, per-lane sums, the cross-lane tree) against the host route:
exactly for integers and for float data whose partial sums are exact, within the derived bounds otherwise.  Cases: tests/_measure_cases.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import _measure_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i = ctypes.c_void_p, ctypes.c_int
DTYPE_CODE = {"uint8": 0, "uint16": 1, "float32": 2}


def measure(*a, **kw):
    from stardist_amd.utils import measure_labels
    return measure_labels(*a, **kw)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("measure") / "libmeasure.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host", "measure_check.cpp"), "-o", so], check=True)
    l = ctypes.CDLL(so)
    l.ms_chunk_pixels.restype = _i
    l.ms_wave_pixels.restype = _i
    l.ms_stats.restype = _i
    l.ms_stats.argtypes = [_vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp]
    return l


def harness(lib, lbl, img):
    """(sums (top + 1, C, 2), minmax (top + 1, C, 2), most chunks of a box) of the host harness: the tables of the C entry point"""
    lab = np.ascontiguousarray(np.maximum(lbl, 0), np.int32)
    img = np.ascontiguousarray(img)
    C_ = 1 if img.ndim == lbl.ndim else img.shape[-1]
    top = int(lab.max())
    code = DTYPE_CODE[img.dtype.name]
    sums = np.full((top + 1, C_, 2), -3, np.float64 if code == 2 else np.int64)
    mm = np.full((top + 1, C_, 2), -3, np.float32 if code == 2 else np.int32)
    chunks = ctypes.c_int(0)
    zyx = ((1,) + lbl.shape) if lbl.ndim == 2 else lbl.shape
    rc = lib.ms_stats(lab.ctypes.data, *zyx, top, img.ctypes.data, code, C_, sums.ctypes.data if code != 2 else None,
                      sums.ctypes.data if code == 2 else None, mm.ctypes.data, ctypes.addressof(chunks))
    assert rc == 0
    return sums, mm, chunks.value


def columns(table, key, name):
    """(n, C) array of an intensity column of the case's table"""
    lbl, img = C.case(name)
    if img.ndim == lbl.ndim:
        return np.asarray(table[key])[:, None]
    return np.stack([table["%s-%d" % (key, c)] for c in range(img.shape[-1])], axis=1)


def test_constants_are_the_header_s(lib):
    txt = open(os.path.join(ROOT, "stardist_amd", "csrc", "measure.h")).read()
    assert re.findall(r"\bMS_CHUNK_PIXELS\s*=\s*(\d+)", txt) == [str(C.MS_CHUNK_PIXELS)] and lib.ms_chunk_pixels() == C.MS_CHUNK_PIXELS
    assert re.findall(r"\bMS_WAVE_PIXELS\s*=\s*(\d+)", txt) == [str(C.MS_WAVE_PIXELS)] and lib.ms_wave_pixels() == C.MS_WAVE_PIXELS


def test_cases_are_what_they_say():
    a = C.small_2d()
    present = np.unique(a[a > 0])
    assert a.shape == (67, 131) and 35 <= len(present) <= 45 and (a < 0).any() and len(present) < present.max() / 2      # gaps
    h = C.host("2d_none")
    assert (h["area"] == 1).sum() >= 1
    on_border = (h["bbox-0"] == 0) | (h["bbox-1"] == 0) | (h["bbox-2"] == 67) | (h["bbox-3"] == 131)
    assert on_border.sum() >= 5
    boxes = np.stack([h["bbox-%d" % k] for k in range(4)], axis=1)
    inside = [(boxes[:, 0] < b[0]) & (boxes[:, 1] < b[1]) & (boxes[:, 2] > b[2]) & (boxes[:, 3] > b[3]) for b in boxes]
    assert np.any(inside)                                                   # a box strictly inside another one: the ring's
    v = C.host("3d_none")
    assert C.small_3d().shape == (9, 33, 70) and 12 <= len(v["label"]) <= 16 and ((v["bbox-3"] - v["bbox-0"]) == 1).any()
    f = C.chunked()
    box_rows = C.MS_CHUNK_PIXELS // f.shape[1]
    t = C.host("chunked_u16")
    frame = list(t["label"]).index(7)
    assert [t["bbox-%d" % k][frame] for k in range(4)] == [0, 0, f.shape[0], f.shape[1]]
    assert f.shape[0] // box_rows >= 3 and f.shape[0] % box_rows != 0 and 550 < f.shape[0] < 650
    areas = t["area"] * 1
    assert ((t["bbox-2"] - t["bbox-0"]) * (t["bbox-3"] - t["bbox-1"]) > C.MS_WAVE_PIXELS).sum() == 2 and len(areas) > 25
    assert C.case("2d_u8_rgb")[1].strides[0] % 2 == 1
    lbl, img = C.case("all_65535")
    assert lbl.size * 65535 ** 2 > 2 ** 53


def scipy_oracle(lbl, img):
    """label, area, boxes, centroid and, per channel, sum / min / max / population variance from scipy.ndimage and per-object numpy"""
    lab = np.maximum(lbl, 0)
    found = ndimage.find_objects(lab)
    labels = np.array([k for k, s in enumerate(found, 1) if s is not None], np.int64)
    out = {"label": labels, "area": ndimage.sum_labels(np.ones(lab.shape, np.int64), lab, labels).astype(np.int64)}
    boxes = [found[k - 1] for k in labels]
    for d in range(lab.ndim):
        out["bbox-%d" % d] = np.array([b[d].start for b in boxes], np.int64)
        out["bbox-%d" % (d + lab.ndim)] = np.array([b[d].stop for b in boxes], np.int64)
    com = np.array(ndimage.center_of_mass(np.ones(lab.shape), lab, labels), np.float64).reshape(len(labels), lab.ndim)
    for d in range(lab.ndim):
        out["centroid-%d" % d] = com[:, d]
    if img is not None:
        planes = img.reshape(lbl.shape + (-1,))
        for c in range(planes.shape[-1]):
            p = planes[..., c]
            out["sum-%d" % c] = ndimage.sum_labels(p, lab, labels)
            out["min-%d" % c] = ndimage.minimum(p, lab, labels)
            out["max-%d" % c] = ndimage.maximum(p, lab, labels)
            out["var-%d" % c] = np.array([np.var(p[lab == k].astype(np.float64)) for k in labels])
    return out


@pytest.mark.parametrize("name", [n for n in C.NAMES if n not in ("non_finite", "huge_ids_u16", "empty_none", "empty_f32")])
def test_host_route_equals_scipy_oracle(name):
    lbl, img = C.case(name)
    got, want = C.host(name), scipy_oracle(lbl, img)
    assert list(got) == C.case_keys(name)
    for key in ["label", "area"] + [k for k in got if k.startswith(("bbox-", "centroid-"))]:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    if img is None:
        return
    n = got["area"].astype(np.float64)
    for c in range(columns(got, "sum_intensity", name).shape[1]):
        S, mn, mx = (columns(got, k, name)[:, c] for k in ("sum_intensity", "min_intensity", "max_intensity"))
        mean, std = (columns(got, k, name)[:, c] for k in ("mean_intensity", "std_intensity"))
        assert np.array_equal(mn, want["min-%d" % c]) and np.array_equal(mx, want["max-%d" % c])
        assert np.array_equal(mean, S.astype(np.float64) / n)
        if name in C.INTEGER:
            assert S.dtype == mn.dtype == mx.dtype == np.int64
            if name != "all_65535":                                         # scipy sums in float64: exact below 2^53
                assert np.array_equal(S, want["sum-%d" % c].astype(np.int64))
            # two-pass variance of numpy against sum2 / n - mean^2: both within a few roundings of mean^2 + var
            assert np.allclose(std * std, want["var-%d" % c], rtol=0, atol=64 * 2.0 ** -53 * (mean * mean + want["var-%d" % c]).max())
        else:
            assert S.dtype == np.float64 and mn.dtype == mx.dtype == np.float32
    if name in C.FLOAT_EXACT or name in C.FLOAT_RANDOM:
        C.check_float_columns(name, got, exact=name in C.FLOAT_EXACT)


def test_host_route_equals_scikit_image_golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "measure_reference.npz"))
    for nd, names in (("2d", ("2d_u16", "2d_u8_rgb")), ("3d", ("3d_u16", "3d_u8"))):
        assert np.array_equal(C.case(names[0])[0], g[nd + "/lbl"])          # the generator still makes the case the golden was made for
        got = C.host(names[0])
        for key in [k for k in got if k.startswith(("label", "area", "bbox-", "centroid-"))]:
            want = g["%s/%s" % (nd, key)]
            assert np.array_equal(got[key], want) and got[key].dtype == (np.float64 if key.startswith("centroid") else np.int64), key
        for name in names:
            assert np.array_equal(C.case(name)[1], g[name + "/img"])
            mean = columns(C.host(name), "mean_intensity", name)
            for c in range(mean.shape[1]):
                assert np.array_equal(mean[:, c], g["%s/mean_intensity-%d" % (name, c)]), (name, c)


def test_integer_sums_are_exact_beyond_2_53():
    t = C.host("all_65535")
    n = 1500 * 1500
    assert t["area"].tolist() == [n] and t["sum_intensity"].tolist() == [n * 65535]
    assert t["mean_intensity"].tolist() == [65535.0] and t["min_intensity"].tolist() == t["max_intensity"].tolist() == [65535]
    assert t["std_intensity"].tolist() == [float(np.sqrt(max(0.0, np.float64(n * 65535 ** 2) / np.float64(n) - 65535.0 ** 2)))]


@pytest.mark.parametrize("name", [n for n in C.NAMES if C.case(n)[1] is not None and n not in ("huge_ids_u16", "empty_f32")])
def test_harness_equals_host_route(lib, name):
    """the device's order of additions with plain loops: integers, min, max and exact float data bit for bit; random float data within
    the bounds; sentinel rows for absent labels"""
    lbl, img = C.case(name)
    sums, mm, chunks = harness(lib, lbl, img)
    want = C.host(name)
    rows = want["label"]
    absent = np.setdiff1d(np.arange(sums.shape[0]), rows)
    assert 0 in absent and (sums[absent] == 0).all()
    if img.dtype == np.float32:
        assert np.isposinf(mm[absent][..., 0]).all() and np.isneginf(mm[absent][..., 1]).all()
    else:
        assert (mm[absent][..., 0] == 2 ** 31 - 1).all() and (mm[absent][..., 1] == -2 ** 31).all()
    assert chunks >= (3 if name.startswith("chunked") or name == "all_65535" else 1)
    S, S2 = sums[rows][..., 0], sums[rows][..., 1]
    assert np.array_equal(mm[rows][..., 0], columns(want, "min_intensity", name), equal_nan=True)
    assert np.array_equal(mm[rows][..., 1], columns(want, "max_intensity", name), equal_nan=True)
    if name in C.INTEGER:
        assert np.array_equal(S, columns(want, "sum_intensity", name))
        planes = img.reshape(lbl.shape + (-1,)).astype(np.int64)
        for k, l in enumerate(rows):
            assert S2[k].tolist() == [int(x) for x in (planes[lbl == l] ** 2).sum(axis=0)]
    elif name == "non_finite":
        host_sum = columns(want, "sum_intensity", name)
        assert np.array_equal(np.isnan(S), np.isnan(host_sum)) and np.array_equal(np.isinf(S), np.isinf(host_sum))
        assert np.isnan(S).sum() == 2 and np.isposinf(S).sum() == 1 and np.isnan(S2).sum() == 1 and np.isposinf(S2).sum() == 2
    else:
        n = want["area"][:, None].astype(np.float64)
        with np.errstate(all="ignore"):
            mean = S / n
            table = dict(want)
            for c in range(S.shape[1]):
                suffix = ("-%d" % c) if img.ndim > lbl.ndim else ""
                table["sum_intensity" + suffix] = np.ascontiguousarray(S[:, c])
                table["mean_intensity" + suffix] = np.ascontiguousarray(mean[:, c])
                table["std_intensity" + suffix] = np.sqrt(np.maximum(0.0, S2[:, c] / n[:, 0] - mean[:, c] * mean[:, c]))
        C.check_float_columns(name, table, exact=name in C.FLOAT_EXACT, sums2=S2)


def test_non_finite_pixels_as_numpy():
    lbl, img, what = C.non_finite()
    t = C.host("non_finite")
    row = {l: list(t["label"]).index(l) for l in what}
    (a, b, c) = list(what)
    for key in ("sum_intensity", "mean_intensity", "min_intensity", "max_intensity", "std_intensity"):
        assert np.isnan(t[key][row[a]]), key                                # a NaN pixel
    assert t["sum_intensity"][row[b]] == np.inf and t["mean_intensity"][row[b]] == np.inf and t["max_intensity"][row[b]] == np.inf
    assert np.isfinite(t["min_intensity"][row[b]]) and np.isnan(t["std_intensity"][row[b]])     # inf - inf
    assert np.isnan(t["sum_intensity"][row[c]]) and t["min_intensity"][row[c]] == -np.inf and t["max_intensity"][row[c]] == np.inf
    others = np.setdiff1d(np.arange(len(t["label"])), list(row.values()))
    assert all(np.isfinite(t[k][others]).all() for k in t)
    for l, k in row.items():                                                # numpy's own answers
        v = img[lbl == l]
        with np.errstate(all="ignore"):
            assert np.array_equal([t["min_intensity"][k], t["max_intensity"][k]], [v.min(), v.max()], equal_nan=True)
            assert np.isnan(t["sum_intensity"][k]) == np.isnan(v.astype(np.float64).sum())


def test_huge_ids_report_the_originals():
    lbl, old, new = C.huge_ids()
    got, small = C.host("huge_ids_u16"), C.host("2d_u16")
    assert lbl.dtype == np.int64 and new.max() == 2 ** 40 and np.array_equal(small["label"], old)
    assert got["label"].dtype == np.int64 and np.array_equal(got["label"], new)
    for key in small:
        if key != "label":
            assert np.array_equal(got[key], small[key]), key


def test_no_objects_gives_empty_columns_of_the_right_types():
    for name, nd in (("empty_none", 2), ("empty_f32", 3)):
        t = C.host(name)
        assert list(t) == C.case_keys(name) and all(v.shape == (0,) for v in t.values())
        assert all(t[k].dtype == np.int64 for k in t if k.startswith(("label", "area", "bbox")))
        assert all(t[k].dtype == np.float64 for k in t if k.startswith(("centroid", "sum", "mean", "std")))
        assert all(t[k].dtype == np.float32 for k in t if k.startswith(("min", "max")))
    u = measure(np.zeros((5, 6), np.uint8), np.zeros((5, 6), np.uint16))
    assert u["sum_intensity"].dtype == u["min_intensity"].dtype == np.int64 and u["mean_intensity"].dtype == np.float64


def test_host_input_takes_the_host_code_and_errors_come_first(monkeypatch):
    from stardist_amd import _route, label_ops
    monkeypatch.setattr(label_ops, "_measure_raw_device", lambda *a, **k: pytest.fail("device path taken"))
    monkeypatch.setattr(_route, "_device_labels", lambda *a, **k: pytest.fail("labels uploaded"))
    lbl, img = C.case("2d_u16")
    for other in (lbl.astype(np.int64), np.maximum(lbl, 0).astype(np.uint8), lbl.tolist()):
        got = measure(other, img)
        assert all(np.array_equal(got[k], C.host("2d_u16")[k]) for k in got)
    wide = measure(lbl, img.astype(np.float64))                             # a dtype the kernels do not take: still measured
    assert wide["min_intensity"].dtype == np.float64 and np.array_equal(wide["min_intensity"], C.host("2d_u16")["min_intensity"])
    assert np.array_equal(measure(lbl, img.astype(np.int32))["sum_intensity"], C.host("2d_u16")["sum_intensity"])
    for dev in (None, "cuda"):                                              # the same errors, before anything runs, on both routes
        with pytest.raises(ValueError, match="2D or 3D"):
            measure(np.zeros(7, np.int32), device=dev)
        with pytest.raises(ValueError, match="2D or 3D"):
            measure(np.zeros((2, 3, 4, 5), np.int32), np.zeros((9, 9)), device=dev)
        with pytest.raises(ValueError, match="shape"):
            measure(lbl, img[:-1], device=dev)
        with pytest.raises(ValueError, match="shape"):
            measure(lbl, img[..., None, None], device=dev)
        with pytest.raises(ValueError, match="shape"):
            measure(C.small_3d(), img, device=dev)
    with pytest.raises(ValueError, match="integer"):
        measure(lbl.astype(np.float32), img)
    import stardist_amd
    assert not hasattr(stardist_amd, "measure_labels")                      # the top-level names mirror the reference's exports


def test_host_tensors_and_as_tensors():
    import torch
    lbl, img = C.case("2d_f32_random_c2")
    want = C.host("2d_f32_random_c2")
    got = measure(torch.from_numpy(lbl.copy()), torch.from_numpy(img.copy()), as_tensors=True)
    assert list(got) == list(want)
    for k in want:
        assert isinstance(got[k], torch.Tensor) and got[k].device.type == "cpu" and got[k].dim() == 1
        assert got[k].numpy().dtype == want[k].dtype and np.array_equal(got[k].numpy(), want[k]), k
    plain = measure(torch.from_numpy(lbl.copy()), img)
    assert all(isinstance(plain[k], np.ndarray) and np.array_equal(plain[k], want[k]) for k in want)
    e = measure(np.zeros((3, 3), np.int32), as_tensors=True)
    assert all(isinstance(v, torch.Tensor) and v.shape == (0,) for v in e.values())
