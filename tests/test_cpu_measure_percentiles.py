"""CPU: stardist_amd.utils.measure_labels(percentiles=) on host input -- against a brute-force statement of the definition (np.sort and
the interpolation written out here), against np.percentile per object -- and the per-object code of the device pass (csrc/measure_rank.h
through tests/host/measure_rank_check.cpp: the sort tier's staging and network, the digit passes of the block tier, the chunk
histograms merged into a slot) against the host route.  Every comparison is exact: == and equal NaN positions.  Cases:
tests/_percentile_cases.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _percentile_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "measure_rank_check.cpp")
_vp, _i = ctypes.c_void_p, ctypes.c_int
DTYPE_CODE = {"uint8": 0, "uint16": 1, "float32": 2}
NUMPY_2 = int(np.__version__.split(".")[0]) >= 2


def measure(*a, **kw):
    from stardist_amd.utils import measure_labels
    return measure_labels(*a, **kw)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("measure_rank") / "libmeasure_rank.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so], check=True)
    l = ctypes.CDLL(so)
    for name in ("mr_sort_keys", "mr_rank_keys", "mr_chunk_slots", "mr_chunk_pixels", "mr_max_q", "mr_percentiles"):
        getattr(l, name).restype = _i
    l.mr_percentiles.argtypes = [_vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp]
    return l


def harness(lib, name, force=-1, slots=-1):
    """((top + 1, C, n_q) table of the host harness -- the table of the C entry point --, objects per tier) for the case"""
    lbl, img, qs = P.case(name)
    lab = np.ascontiguousarray(np.maximum(lbl, 0), np.int32)
    img = np.ascontiguousarray(img)
    C = 1 if img.ndim == lbl.ndim else img.shape[-1]
    top = int(lab.max())
    q = np.array([float(v) for v in qs], np.float64)
    out = np.full((top + 1, C, len(q)), -3.0, np.float64)
    tiers = np.zeros(3, np.int32)
    zyx = ((1,) + lbl.shape) if lbl.ndim == 2 else lbl.shape
    rc = lib.mr_percentiles(lab.ctypes.data, *zyx, top, img.ctypes.data, DTYPE_CODE[img.dtype.name], C, q.ctypes.data, len(q),
                            1 if NUMPY_2 else 0, force, slots, out.ctypes.data, tiers.ctypes.data)
    assert rc == 0
    return out, tiers.tolist()


def host_block(name):
    """(labels, (n, C, n_q) array of the host route's percentile columns with a column per q given, duplicates included)"""
    lbl, img, qs = P.case(name)
    t = P.host(name)
    block = P.percentile_block(t, name)
    stems = P.q_names(qs)
    return t["label"], block[:, :, [stems.index("p%g_intensity" % float(q)) for q in qs]]


def test_constants_are_the_header_s(lib):
    txt = open(os.path.join(ROOT, "stardist_amd", "csrc", "measure_rank.h")).read()
    assert re.findall(r"\bMR_SORT_KEYS\s*=\s*(\d+)", txt) == [str(P.MR_SORT_KEYS)] and lib.mr_sort_keys() == P.MR_SORT_KEYS
    assert re.findall(r"\bMR_RANK_KEYS\s*=\s*(\d+)", txt)[:1] == [str(P.MR_RANK_KEYS)] and lib.mr_rank_keys() == P.MR_RANK_KEYS
    assert re.findall(r"\bMR_CHUNK_SLOTS\s*=\s*(\d+)", txt) == [str(P.MR_CHUNK_SLOTS)] and lib.mr_chunk_slots() == P.MR_CHUNK_SLOTS
    assert re.findall(r"\bMR_MAX_Q\s*=\s*(\d+)", txt) == [str(P.MR_MAX_Q)] and lib.mr_max_q() == P.MR_MAX_Q
    assert lib.mr_chunk_pixels() == P.MS_CHUNK_PIXELS
    from stardist_amd import label_ops
    assert label_ops._MAX_PERCENTILES == P.MR_MAX_Q


def test_cases_are_what_they_say():
    t = P.host("sizes_u16")
    area = dict(zip(t["label"].tolist(), t["area"].tolist()))
    assert [area[l] for l in (3, 7, 8, 20, 21, 22, 40, 41, 45)] == [1, 2, 3, 63, 64, 65, 257, P.MR_SORT_KEYS, P.MR_SORT_KEYS + 1]
    box = lambda t, l: [int(t["bbox-%d" % k][t["label"].tolist().index(l)]) for k in range(len([k for k in t if k.startswith("bbox-")]))]
    assert box(t, 50) == box(t, 51) and area[50] + area[51] == 16 * 40
    assert len(t["label"]) < t["label"].max() / 2                           # gaps
    c = P.host("chunks_u16")
    pixels = lambda t, l: int(np.prod(np.subtract(box(t, l)[len(box(t, l)) // 2:], box(t, l)[:len(box(t, l)) // 2])))
    carea = dict(zip(c["label"].tolist(), c["area"].tolist()))
    assert pixels(c, 2) == P.MS_CHUNK_PIXELS and pixels(c, 3) == P.MS_CHUNK_PIXELS + 256
    assert pixels(c, 5) > P.MS_CHUNK_PIXELS and carea[5] == 270 and pixels(c, 6) == carea[6] + 12 > P.MS_CHUNK_PIXELS
    assert box(c, 8) == box(c, 9) and pixels(c, 8) > P.MR_SORT_KEYS
    v = P.host("volume_u16")
    assert pixels(v, 4) > P.MS_CHUNK_PIXELS and pixels(v, 9) > P.MR_SORT_KEYS and box(v, 4)[3] - box(v, 4)[0] == 5
    d = P.host("diagonals_u8")
    assert len(d["label"]) > P.MR_CHUNK_SLOTS and all(pixels(d, l) > P.MS_CHUNK_PIXELS for l in (1, len(d["label"])))
    lbl, img, _ = P.case("sizes_u16")
    assert {0, 65535} <= set(img[lbl == 41].tolist())
    lbl, img, _ = P.case("sizes_f32")
    assert (np.abs(img[np.isfinite(img) & (img != 0)]) < 2.0 ** -126).any() and (np.abs(img[np.isfinite(img)]) > 2.0 ** 100).any() and (img < 0).any()
    assert len(P.Q8) == P.MR_MAX_Q and len(set(float(q) for q in P.Q8)) == P.MR_MAX_Q - 1
    assert P.case("huge_ids_u16")[0].max() == 2 ** 40


def brute(v, q, f32):
    """the definition: the sorted values, numpy's virtual index (n - 1) q / 100, its two neighbours and weight, and numpy's _lerp; in
    float32 for float32 data under numpy >= 2.0 (f32), else in float64 (float32 data: rounded at the end)"""
    if np.isnan(v).any():
        return np.float32(np.nan) if v.dtype == np.float32 else np.float64(np.nan)
    s = np.sort(v)
    n = len(s)
    ft = np.float32 if f32 else np.float64
    vi = ft(n - 1) * (ft(q) / ft(100))
    lo = int(np.floor(vi))
    hi = lo + 1
    if vi >= n - 1:
        lo = hi = n - 1
        t = ft(vi) - ft(-1)                                                 # numpy takes the weight against index -1 here
    else:
        t = ft(vi - ft(lo))
    hi = min(hi, n - 1)
    a, b = s[lo], s[hi]
    with np.errstate(all="ignore"):
        if v.dtype.kind in "iu":
            d = np.float64(b - a)                                           # in the integer type: b >= a
            a, b = np.float64(a), np.float64(b)
        else:
            a, b = ft(a), ft(b)
            d = b - a
        res = b - d * (ft(1) - t) if t >= 0.5 else a + d * t
    return np.float32(res) if v.dtype == np.float32 else np.float64(res)


@pytest.mark.parametrize("name", [n for n in P.NAMES if n not in P.EMPTY and n != "huge_ids_u16"])
def test_host_route_equals_the_definition_and_numpy(name):
    lbl, img, qs = P.case(name)
    labels, block = host_block(name)
    assert np.array_equal(labels, np.unique(lbl[lbl > 0]))
    planes = img.reshape(lbl.shape + (-1,))
    f32 = img.dtype == np.float32 and NUMPY_2
    assert block.dtype == (np.float32 if img.dtype == np.float32 else np.float64)
    with np.errstate(all="ignore"):
        for k, l in enumerate(labels):
            v = planes[lbl == l]
            for c in range(v.shape[1]):
                for j, q in enumerate(qs):
                    got = block[k, c, j]
                    want = np.percentile(v[:, c], float(q))
                    mine = brute(v[:, c], float(q), f32)
                    assert P.same(got, block.dtype.type(want)) and P.same(got, mine), (name, l, c, q, got, want, mine)


@pytest.mark.parametrize("force", [-1, 1, 2])
@pytest.mark.parametrize("name", [n for n in P.NAMES if n not in P.EMPTY and n != "huge_ids_u16"])
def test_harness_equals_host_route(lib, name, force):
    """every object in the tier of its box, every object through the block tier, every object through the chunked tier while slots last"""
    lbl, img, qs = P.case(name)
    out, tiers = harness(lib, name, force)
    labels, block = host_block(name)
    absent = np.setdiff1d(np.arange(out.shape[0]), labels)
    assert 0 in absent and np.isnan(out[absent]).all()
    assert P.same(out[labels].astype(block.dtype), block) and P.same(out[labels], block.astype(np.float64)), name
    if force == -1 and name.startswith(("chunks", "volume")):
        assert all(tiers), tiers
    if name.startswith("diagonals") and force != 1:                         # more multi-chunk objects than slots: the rest fall back
        C = 1 if img.ndim == lbl.ndim else img.shape[-1]
        assert tiers == [0, len(labels) - P.MR_CHUNK_SLOTS // C, P.MR_CHUNK_SLOTS // C]
    if force == 1:
        assert tiers[0] == tiers[2] == 0


def test_harness_with_few_slots_and_the_other_interpolation(lib):
    for name in ("chunks_f32_c1", "volume_f32_rgb"):
        labels, block = host_block(name)
        out, tiers = harness(lib, name, force=2, slots=4)
        assert tiers[2] >= 1 and tiers[1] >= 3 and P.same(out[labels].astype(np.float32), block)
    # interp_f32 = 0: float64 interpolation rounded at the end -- what np.percentile gives for q as a float64 array element
    lbl, img, qs = P.case("sizes_f32")
    lab = np.ascontiguousarray(lbl)
    q = np.array([25.0, 99.8], np.float64)
    out = np.zeros((int(lab.max()) + 1, 1, 2))
    assert lib.mr_percentiles(lab.ctypes.data, 1, *lbl.shape, int(lab.max()), img.ctypes.data, 2, 1, q.ctypes.data, 2, 0, -1, -1, out.ctypes.data, None) == 0
    with np.errstate(all="ignore"):
        for l in np.unique(lbl[lbl > 0]):
            want = np.percentile(img[lbl == l].astype(np.float64), q).astype(np.float32)
            assert P.same(out[l, 0].astype(np.float32), want), l


def test_harness_bad_arguments(lib):
    lab, img, q, out = np.zeros((4, 5), np.int32), np.zeros((4, 5), np.float32), np.array([50.0]), np.zeros((1, 1, 1))
    good = [lab.ctypes.data, 1, 4, 5, 0, img.ctypes.data, 2, 1, q.ctypes.data, 1, 1, -1, -1, out.ctypes.data, None]
    assert lib.mr_percentiles(*good) == 0 and np.isnan(out).all()
    for at, value in ((0, None), (1, 0), (3, -1), (4, -1), (5, None), (6, 3), (7, 0), (8, None), (9, 0), (9, P.MR_MAX_Q + 1), (13, None)):
        args = list(good)
        args[at] = value
        assert lib.mr_percentiles(*args) == -1, at
    for bad in (-0.5, 100.5, np.nan, np.inf):
        qq = np.array([bad])
        args = list(good)
        args[8] = qq.ctypes.data
        assert lib.mr_percentiles(*args) == -1, bad


def test_stand_alone_sanitizer_build_passes(tmp_path):
    """the harness as a program of its own under AddressSanitizer and UBSan: a scene with a one-pixel object, a NaN, infinities, every
    tier forced and natural, against std::sort"""
    exe = str(tmp_path / "measure_rank_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DMEASURE_RANK_CHECK_MAIN", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("ok") == 3 and "WRONG" not in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("name", P.NAMES)
def test_column_names_order_and_dtypes(name):
    lbl, img, qs = P.case(name)
    t = P.host(name)
    plain = measure(lbl, img)
    keys = list(t)
    pk = P.percentile_keys(name)
    assert keys == list(plain) + pk                                         # after the intensity columns
    assert all(k.startswith("p") and "_intensity" in k for k in pk)
    for k in pk:
        assert t[k].dtype == (np.float32 if img.dtype == np.float32 else np.float64) and t[k].shape == t["label"].shape
    for k in plain:
        assert np.array_equal(t[k], plain[k], equal_nan=True) and t[k].dtype == plain[k].dtype
    with_shape = measure(lbl, img, shape=True, percentiles=qs)
    shape_only = measure(lbl, img, shape=True)
    extra = [k for k in shape_only if k not in plain]
    assert list(with_shape) == list(plain) + pk + extra and extra      # ... and before the shape columns
    assert all(np.array_equal(with_shape[k], shape_only[k], equal_nan=True) for k in shape_only)
    assert all(P.same(with_shape[k], t[k]) for k in pk)


def test_names_follow_percent_g():
    lbl, img, _ = P.case("sizes_u16")
    t = measure(lbl, img, percentiles=[50, 99.8, np.float64(2.5), np.int32(7), 1e-3, 100])
    assert [k for k in t if k.startswith("p")] == ["p50_intensity", "p99.8_intensity", "p2.5_intensity", "p7_intensity", "p0.001_intensity",
                                                  "p100_intensity"]
    rgb = measure(*P.case("sizes_u8_ramp_rgb")[:2], percentiles=(50,))
    assert [k for k in rgb if k.startswith("p")] == ["p50_intensity-0", "p50_intensity-1", "p50_intensity-2"]
    c1 = measure(lbl, img[..., None], percentiles=(50,))
    assert "p50_intensity-0" in c1 and P.same(c1["p50_intensity-0"], t["p50_intensity"])
    assert P.same(t["p100_intensity"], t["max_intensity"].astype(np.float64)) and t["p50_intensity"].dtype == np.float64


def test_no_objects_gives_empty_columns_of_the_right_types():
    for name, dt in (("empty_f32_c2", np.float32), ("empty_u8", np.float64)):
        t = P.host(name)
        pk = P.percentile_keys(name)
        assert pk and all(t[k].shape == (0,) and t[k].dtype == dt for k in pk)
        assert list(t)[-len(pk):] == pk


def test_huge_ids_report_the_originals():
    lbl, old, new = P.huge_ids()
    got, small = P.host("huge_ids_u16"), measure(*P.case("sizes_u16")[:2], percentiles=P.Q5)
    assert lbl.dtype == np.int64 and np.array_equal(small["label"], old) and np.array_equal(got["label"], new)
    assert all(P.same(got[k], small[k]) for k in small if k != "label")


def test_value_errors_come_before_anything_runs(monkeypatch):
    from stardist_amd import _route, label_ops
    monkeypatch.setattr(label_ops, "_measure_raw_device", lambda *a, **k: pytest.fail("device path taken"))
    monkeypatch.setattr(label_ops, "_measure_raw_host", lambda *a, **k: pytest.fail("host path taken"))
    monkeypatch.setattr(_route, "_device_labels", lambda *a, **k: pytest.fail("labels uploaded"))
    lbl, img, _ = P.case("sizes_u16")
    for dev in (None, "cuda"):
        with pytest.raises(ValueError, match="img"):
            measure(lbl, percentiles=(50,), device=dev)
        for bad in ((-0.001,), (100.0001,), (50, 101), (np.nan,), (np.inf,), (50, -np.inf), (), tuple(range(9)), [1] * 9):
            with pytest.raises(ValueError, match="percentiles"):
                measure(lbl, img, percentiles=bad, device=dev)
        with pytest.raises(ValueError, match="percentiles"):
            measure(lbl, img, percentiles=50, device=dev)


def test_none_is_the_call_without_the_keyword():
    for name in ("sizes_f32", "volume_f32_rgb", "chunks_u8_rgb"):
        lbl, img, _ = P.case(name)
        a, b = measure(lbl, img), measure(lbl, img, percentiles=None)
        assert list(a) == list(b) and all(np.array_equal(a[k], b[k], equal_nan=True) and a[k].dtype == b[k].dtype for k in a)
        a, b = measure(lbl, img, shape=True), measure(lbl, img, shape=True, percentiles=None)
        assert list(a) == list(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def test_host_input_makes_no_native_call(monkeypatch):
    from stardist_amd import _route, label_ops
    from stardist_amd.lib import _native
    monkeypatch.setattr(label_ops, "_measure_raw_device", lambda *a, **k: pytest.fail("device path taken"))
    monkeypatch.setattr(_route, "_device_labels", lambda *a, **k: pytest.fail("labels uploaded"))
    monkeypatch.setattr(_native, "dcall", lambda *a, **k: pytest.fail("native call"))
    monkeypatch.setattr(_native, "lib", lambda *a, **k: pytest.fail("library loaded"))
    lbl, img, qs = P.case("sizes_f32")
    want = P.host("sizes_f32")
    for other in (lbl.astype(np.int64), lbl.tolist()):
        got = measure(other, img, percentiles=qs)
        assert list(got) == list(want) and all(P.same(got[k], want[k]) for k in got)
    wide = measure(lbl, img.astype(np.float64), percentiles=(50,))          # a dtype the kernels do not take: numpy's result type
    assert wide["p50_intensity"].dtype == np.float64
    i32 = measure(lbl, P.case("sizes_u16")[1].astype(np.int32), percentiles=(25,))
    assert i32["p25_intensity"].dtype == np.float64 and P.same(i32["p25_intensity"], P.host("sizes_u16")["p25_intensity"])


def test_host_tensors_and_as_tensors():
    import torch
    for name in ("sizes_f32", "volume_f32_rgb", "sizes_u8_ramp_rgb"):
        lbl, img, qs = P.case(name)
        want = P.host(name)
        got = measure(torch.from_numpy(lbl.copy()), torch.from_numpy(img.copy()), percentiles=qs, as_tensors=True)
        assert list(got) == list(want)
        for k in want:
            assert isinstance(got[k], torch.Tensor) and got[k].device.type == "cpu" and got[k].dim() == 1
            assert got[k].numpy().dtype == want[k].dtype and P.same(got[k].numpy(), want[k]), k
        plain = measure(torch.from_numpy(lbl.copy()), img, percentiles=qs)
        assert all(isinstance(plain[k], np.ndarray) and P.same(plain[k], want[k]) for k in want)
        mixed = measure(lbl, img, percentiles=qs, shape=True, as_tensors=True)
        assert all(isinstance(v, torch.Tensor) for v in mixed.values()) and all(P.same(mixed[k].numpy(), want[k]) for k in want)
    e = measure(np.zeros((3, 3), np.int32), np.zeros((3, 3), np.float32), percentiles=(50,), as_tensors=True)
    assert e["p50_intensity"].shape == (0,) and e["p50_intensity"].dtype == torch.float32
