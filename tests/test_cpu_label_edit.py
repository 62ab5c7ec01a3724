"""CPU: stardist_amd.utils.find_boundaries, clear_border, remove_small_objects and select_labels on host input -- against scikit-image
0.18.3 (tests/golden/label_edit_reference.npz), against brute-force statements of the definitions (tests/_label_edit_cases.py: loops over
pixels and offsets, no scipy morphology), find_boundaries exhaustively over all 3^9 3 x 3 windows of three values -- and the per-pixel
rules of the device pass (csrc/label_edit.h through tests/host/label_edit_check.cpp: tiles with their halo, the border band, the clear
pass) against the host routes, as a stand-alone program built plain and under the address and undefined-behaviour sanitizers.  All
comparisons are exact.

One case departs from the golden file on purpose: mode "outer" on an int64 image.  scikit-image raises the background to 2^63 - 1 and
scipy filters in float64, where that is 2^63; what the conversion back gives is the platform's choice (x86: -2^63, which makes every
object pixel with a background pixel in a whole line of its window a boundary).  The host route applies the stated rule, which does not
depend on the dtype; the test checks that it marks nothing scikit-image does not and differs only at such pixels."""
import os
import struct
import subprocess
import warnings

import numpy as np
import pytest

import _label_edit_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "label_edit_check.cpp")
MODE_CODE = {"thick": 0, "inner": 1, "outer": 2}


def U():
    from stardist_amd import utils
    return utils


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "label_edit_reference.npz"))


def zyx(shape):
    return ((1,) + tuple(shape)) if len(shape) == 2 else tuple(shape)


def test_the_four_names_are_public():
    import stardist_amd
    from stardist_amd import label_ops, utils
    for name in ("find_boundaries", "clear_border", "remove_small_objects", "select_labels"):
        assert getattr(utils, name) is getattr(label_ops, name) and not hasattr(stardist_amd, name)


@pytest.mark.parametrize("name", sorted(C.FB))
def test_find_boundaries_host_equals_golden_equals_brute_force(golden, name):
    img = C.FB[name]
    assert np.array_equal(img, golden["fb/%s/img" % name]) and img.dtype == golden["fb/%s/img" % name].dtype
    for c, mode, background in C.fb_params(img):
        got = U().find_boundaries(img, c, mode, background)
        want = golden["fb/%s/c%d_%s_b%d" % (name, c, mode, background)]
        brute = C.brute_pixels(img, c, mode, background)
        assert got.dtype == np.bool_ and got.shape == img.shape, (name, c, mode, background)
        assert np.array_equal(got, brute) and np.array_equal(C.brute_shifts(img, c, mode, background), brute), (name, c, mode, background)
        if img.dtype == np.int64 and mode == "outer":                       # the module docstring's exception
            window = C.brute_shifts((img == background).astype(np.uint8), img.ndim, "thick", 0) | (img == background)
            assert not (got & ~want).any() and not ((got != want) & ~window).any() and not ((got != want) & (img == background)).any()
        else:
            assert np.array_equal(got, want), (name, c, mode, background)
    assert np.array_equal(U().find_boundaries(img, mode="subpixel"), golden["fb/%s/subpixel" % name])
    assert np.array_equal(U().find_boundaries(img), golden["fb/%s/c1_thick_b0" % name])         # the defaults
    assert np.array_equal(U().find_boundaries(img.tolist()), U().find_boundaries(np.asarray(img.tolist())))


def test_find_boundaries_cases_cover_what_they_should():
    kinds = set(a.dtype.name for a in C.FB.values())
    assert {"uint8", "int16", "int32", "int64", "bool"} <= kinds
    assert any((a < 0).any() for a in C.FB.values() if a.dtype.kind == "i") and any(a.ndim == 3 for a in C.FB.values())
    assert {(1, 6), (5, 1), (1, 4, 4)} <= set(a.shape for a in C.FB.values())
    assert int(C.FB["noise_i64"].max()) > 2 ** 31 and int(C.FB["noise_i32"].max()) == 2 ** 31 - 1 and int(C.FB["noise_u8"].max()) == 255
    for a in C.FB.values():
        assert {b for _, _, b in C.fb_params(a)} in ({0, 1}, {0, -3}) and {c for c, _, _ in C.fb_params(a)} == set(range(1, a.ndim + 1))


def test_find_boundaries_all_3x3_windows():
    w = C.windows_image()
    assert w.shape == (705, 700) and w.dtype == np.uint8
    centres = w.reshape(141, 5, 140, 5)[:, 1:4, :, 1:4].transpose(0, 2, 1, 3).reshape(-1, 9)[:3 ** 9]
    assert len(np.unique(centres, axis=0)) == 3 ** 9                        # every window once
    brute = C.brute_pixels_image(w, (0, 1))                                 # a loop over the pixels of the whole image
    assert len(brute) == 12
    for (c, mode, background), want in brute.items():
        got = U().find_boundaries(w, c, mode, background)
        assert np.array_equal(got, want), (c, mode, background)
        assert np.array_equal(C.brute_shifts(w, c, mode, background), want), (c, mode, background)
    # the one-loop statement is the generic per-pixel one (on a part of the image: that loop is slow)
    part = w[:40, :45]
    for key, want in C.brute_pixels_image(part, (0,)).items():
        assert np.array_equal(want, C.brute_pixels(part, *key)), key
    for c in (1, 2):
        for mode in C.MODES:
            assert np.array_equal(C.brute_shifts(part, c, mode, 0), C.brute_pixels(part, c, mode, 0))


def test_find_boundaries_arguments_and_routing(monkeypatch):
    import torch
    from stardist_amd import label_ops
    monkeypatch.setattr(label_ops, "_find_boundaries_device", lambda *a, **k: pytest.fail("device path taken"))
    img = C.FB["blobs"]
    want = U().find_boundaries(img, 2, "inner")
    t = U().find_boundaries(torch.from_numpy(img.copy()), 2, "inner")       # a host tensor: the host code, a host tensor out
    assert isinstance(t, torch.Tensor) and t.dtype == torch.bool and t.device.type == "cpu" and np.array_equal(t.numpy(), want)
    for bad in (0, 3, -1, 1.5, "1", True):
        with pytest.raises(ValueError, match="connectivity"):
            U().find_boundaries(img, bad)
    with pytest.raises(ValueError, match="mode"):
        U().find_boundaries(img, 1, "thin")
    for dev in (None, "cuda"):
        with pytest.raises(ValueError, match="connectivity"):
            U().find_boundaries(img, 3, device=dev)
    sub = U().find_boundaries(img, mode="subpixel", device="cuda")          # subpixel: the host code on every input
    assert isinstance(sub, np.ndarray) and sub.shape == (27, 33) and sub.dtype == np.bool_
    assert U().find_boundaries(np.zeros((0, 4), np.int32)).shape == (0, 4)
    big = C.FB["noise_i64"]                                                 # values beyond int32: the host code, whatever device= says
    monkeypatch.setattr(label_ops.N, "require_device", lambda: None)
    monkeypatch.setattr(label_ops, "_int32_values_device", lambda x, device: None if int(np.abs(x).max()) >= 2 ** 31 else pytest.fail("fits"))
    assert np.array_equal(U().find_boundaries(big, 1, "outer", device="cuda"), U().find_boundaries(big, 1, "outer"))


def test_find_boundaries_device_route_gets_background_and_sentinel(monkeypatch):
    from stardist_amd import label_ops
    seen = []

    def fake(lab, connectivity, mode, background, sentinel):
        seen.append((lab, connectivity, mode, background, sentinel))
        raise RuntimeError("stop")
    monkeypatch.setattr(label_ops, "_find_boundaries_device", fake)
    monkeypatch.setattr(label_ops.N, "require_device", lambda: None)
    monkeypatch.setattr(label_ops, "_int32_values_device", lambda x, device: x)
    for dt, top in (("bool", 255), ("uint8", 255), ("int8", 127), ("int16", 32767), ("uint16", 65535), ("int32", 2 ** 31 - 1),
                    ("uint32", 2 ** 32 - 1), ("int64", 2 ** 63 - 1)):
        with pytest.raises(RuntimeError, match="stop"):
            U().find_boundaries(np.zeros((3, 4), dt), 2, "outer", 1.0, device="cuda")
        assert seen[-1][1:] == (2, "outer", 1, top), dt
    n = len(seen)
    for kw in ({"background": 0.5}, {"mode": "subpixel"}):                  # the host code
        assert not U().find_boundaries(np.zeros((3, 4), np.uint8), device="cuda", **kw).any()
    assert not U().find_boundaries(np.zeros((3, 4), np.uint64), device="cuda").any() and not U().find_boundaries(np.zeros(5, np.uint8), device="cuda").any()
    assert len(seen) == n


@pytest.mark.parametrize("name", sorted(C.CB))
def test_clear_border_host_equals_golden_and_brute_force(golden, name):
    img, kw = C.CB[name]
    assert np.array_equal(img, golden["cb/%s/img" % name]) and img.dtype == golden["cb/%s/img" % name].dtype
    if "mask" in kw:
        assert np.array_equal(kw["mask"], golden["cb/%s/mask" % name])
    keep = img.copy()
    got = U().clear_border(img, **kw)
    assert got.dtype == img.dtype and got.shape == img.shape and np.array_equal(got, golden["cb/%s/out" % name]), name
    assert np.array_equal(img, keep) and got is not img
    if name in C.CB_BRUTE:
        assert np.array_equal(got, C.brute_clear_border(img, **kw)), name


def test_clear_border_cases_are_what_they_say():
    cb = lambda name: U().clear_border(*C.CB[name][:1], **C.CB[name][1])
    two = C.CB["two_components"][0]
    out = cb("two_components")
    assert (out[0:3, 2:5] == 0).all() and (out[6:9, 6:9] == 4).all() and (out[5:7, 10:12] == 9).all()       # only the piece at the edge goes
    diag = C.CB["diagonal_contact"][0]
    out = cb("diagonal_contact")
    assert (out[3:6, 3:6] == 0).all() and (out[7:9, 1:3] == 2).all() and (out[6:8, 6:8] == 3).all() and (diag[3:6, 3:6] == 2).all()
    framed = C.CB["framed_bgval_7"][0]
    out = cb("framed_bgval_7")                                              # no background pixel in the band: the background stays 0
    assert (out[framed == 5] == 7).all() and (out[framed == 0] == 0).all() and (out[framed == 6] == 6).all()
    out = cb("framed_bgval_7_buffer_1")                                     # now there is one: every background pixel becomes 7
    assert (out[framed == 0] == 7).all() and (out[framed == 5] == 7).all() and (out[framed == 6] == 6).all()
    inner = C.CB["inner_objects"][0]
    assert np.array_equal(cb("inner_objects"), inner)                       # a band of background only, bgval 0: nothing changes
    out = cb("inner_objects_bgval_7")
    assert (out[inner == 0] == 7).all() and np.array_equal(out[inner > 0], inner[inner > 0])
    blobs = C.CB["blobs"][0]
    assert np.array_equal(cb("blobs_mask_all_true"), blobs) and (cb("blobs_mask_all_false") == 7).all()
    assert 0 < (cb("blobs") > 0).sum() < (blobs > 0).sum() and (cb("blobs_buffer_1") > 0).sum() < (cb("blobs") > 0).sum()
    assert C.CB["blobs_buffer_largest"][1]["buffer_size"] == min(blobs.shape) - 1 and C.CB["volume_buffer_largest"][1]["buffer_size"] == 6
    assert cb("blobs_bool").dtype == np.bool_ and (C.CB["blobs_i16_negative"][0] < 0).any()


def test_clear_border_errors_and_routing(monkeypatch):
    import torch
    from stardist_amd import label_ops
    monkeypatch.setattr(label_ops, "_clear_border_device", lambda *a, **k: pytest.fail("device path taken"))
    img = C.CB["blobs"][0]
    for dev in (None, "cuda"):                                              # before anything runs, on both routes
        with pytest.raises(ValueError, match="buffer size"):
            U().clear_border(img, buffer_size=40, device=dev)
        with pytest.raises(ValueError, match="buffer_size"):
            U().clear_border(img, buffer_size=-1, device=dev)
        with pytest.raises(TypeError, match="bool"):
            U().clear_border(img, mask=np.ones(img.shape, np.uint8), device=dev)
        with pytest.raises(AssertionError, match="same shape"):
            U().clear_border(img, mask=np.ones((40, 69), bool), device=dev)
    assert np.array_equal(U().clear_border(img, buffer_size=40, mask=np.ones(img.shape, bool)), img)          # with a mask any buffer_size
    t = U().clear_border(torch.from_numpy(img.copy()), 1, 7, torch.from_numpy(C.CB["blobs_mask"][1]["mask"].copy()))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.int32 and np.array_equal(t.numpy(), U().clear_border(img, 1, 7, C.CB["blobs_mask"][1]["mask"]))
    assert np.array_equal(U().clear_border(img.tolist()), U().clear_border(img))
    wide = img.astype(np.int64)                                             # a bgval the kernels do not take: the host code
    assert np.array_equal(U().clear_border(wide, bgval=2 ** 40, device="cuda"), U().clear_border(wide, bgval=2 ** 40))
    assert (U().clear_border(wide, bgval=2 ** 40) == 2 ** 40).any()


@pytest.mark.parametrize("name", sorted(C.RS))
def test_remove_small_objects_host_equals_golden(golden, name):
    img, kw = C.RS[name]
    keep = img.copy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = U().remove_small_objects(img, **kw)
    assert got.dtype == img.dtype and got.shape == img.shape and np.array_equal(img, keep) and got is not img
    if "rs/%s/out" % name in golden.files:
        assert np.array_equal(img, golden["rs/%s/img" % name]) and np.array_equal(got, golden["rs/%s/out" % name]), name
    else:                                                                   # ids that scikit-image's bincount cannot take: per id, by hand
        assert name == "blobs_huge_ids"
        want = img.copy()
        for v in np.unique(img):
            if (img == v).sum() < kw["min_size"]:
                want[img == v] = 0
        assert np.array_equal(got, want) and 0 < (got > 0).sum() < (img > 0).sum()


def test_remove_small_objects_cases_are_what_they_say():
    from scipy import ndimage
    rs = lambda name: U().remove_small_objects(C.RS[name][0], **C.RS[name][1])
    split = C.RS["split_id_kept"][0]
    assert ndimage.label(split == 5)[1] == 3 and (split == 5).sum() == 18
    out = rs("split_id_kept")                                               # every piece is below 13, together they are not: kept
    assert (out[split == 5] == 5).all() and (out[split == 2] == 0).all() and out[0, 19] == 0
    assert (rs("split_id_gone") == 0).all()
    for c in (2, 7, None):                                                  # an integer image: the connectivity plays no part, as there
        assert np.array_equal(U().remove_small_objects(split, 13, c), out)
    assert np.array_equal(rs("blobs_min_0"), C.RS["blobs"][0]) and np.array_equal(rs("blobs_min_1"), C.RS["blobs"][0])
    m = C.RS["mask_c1"][0]
    a, b = rs("mask_c1"), rs("mask_c2")
    assert a.dtype == np.bool_ and (a & ~m).sum() == 0 and a.sum() < b.sum() < m.sum()         # diagonal joins make larger components
    assert rs("mask3_c1").sum() < rs("mask3_c2").sum() <= rs("mask3_c3").sum() < C.RS["mask3_c1"][0].sum()
    assert np.array_equal(rs("mask_min_1"), m)
    for dev in (None, "cuda"):
        with pytest.raises(ValueError, match="Negative value labels"):
            U().remove_small_objects(np.array([[1, -1], [2, 2]], np.int32), 2, device=dev)
        with pytest.raises(ValueError, match="bool or integer"):
            U().remove_small_objects(np.zeros((3, 3), np.float32), device=dev)
        with pytest.raises(ValueError, match="connectivity"):
            U().remove_small_objects(m, 3, 3, device=dev)
    with pytest.warns(UserWarning, match="Only one label"):
        U().remove_small_objects(np.ones((3, 3), np.int32), 2)


@pytest.mark.parametrize("name", sorted(C.SL))
def test_select_labels_host_equals_brute_force(name):
    import torch
    lbl, wanted, kw = C.SL[name]
    keep = lbl.copy()
    got = U().select_labels(lbl, wanted, **kw)
    assert got.dtype == lbl.dtype and got.shape == lbl.shape and np.array_equal(got, C.brute_select(lbl, wanted, **kw)), name
    assert np.array_equal(lbl, keep) and got is not lbl
    assert np.array_equal(U().select_labels(lbl, wanted.tolist(), **kw), got)
    if lbl.dtype != np.uint16:
        t = U().select_labels(torch.from_numpy(lbl.copy()), torch.from_numpy(wanted.copy()), **kw)
        assert isinstance(t, torch.Tensor) and t.device.type == "cpu" and np.array_equal(t.numpy(), got)


def test_select_labels_cases_are_what_they_say():
    sl = lambda name: U().select_labels(C.SL[name][0], C.SL[name][1], **C.SL[name][2])
    lbl, wanted, _ = C.SL["some"]
    out = sl("some")
    assert set(np.unique(out)) == {0} | set(wanted.tolist()) and np.array_equal(out[out > 0], lbl[out > 0])
    inv = sl("some_invert")
    assert np.array_equal((out > 0) | (inv > 0), lbl > 0) and not ((out > 0) & (inv > 0)).any()
    rel = sl("some_relabel")
    kept = np.unique(lbl[np.isin(lbl, C.SL["some_relabel"][1])])
    assert list(np.unique(rel)) == list(range(len(kept) + 1))
    for k, v in enumerate(kept):                                            # ascending id order
        assert (rel[lbl == v] == k + 1).all()
    assert set(np.unique(sl("absent_ids"))) == {0, 3, 5} and set(np.unique(sl("absent_ids_relabel"))) == {0, 1, 2}
    assert not sl("empty_list").any() and np.array_equal(sl("empty_list_invert_relabel") > 0, lbl > 0)
    huge = C.SL["huge_ids"][0]
    assert int(huge.max()) > 2 ** 31 and set(np.unique(sl("huge_ids"))) == {0} | set(C.SL["huge_ids"][1].tolist())
    assert (sl("negative_values") >= 0).all()
    with pytest.raises(ValueError, match="integer"):
        U().select_labels(np.zeros((3, 3), np.float32), [1])
    with pytest.raises(ValueError, match="integers"):
        U().select_labels(lbl, [1.5])


def test_select_labels_filters_by_a_measure_labels_table():
    from stardist_amd.utils import measure_labels
    lbl = C.SL["some"][0]
    table = measure_labels(lbl)
    out = U().select_labels(lbl, table["label"][table["area"] > 50])
    sizes = np.bincount(lbl.reshape(-1))
    assert set(np.unique(out)) == {0} | set(int(v) for v in np.nonzero(sizes > 50)[0] if v > 0)


# ----------------------------------------------------------------------------- the device pass's rules on the host

def records():
    """[(head, tail, arrays)]: the cases as label_edit_check.cpp reads them, with the host routes' results"""
    from stardist_amd.utils import label_components
    recs = []
    fb = [(a, p) for a in C.FB.values() if a.ndim in (2, 3) and np.abs(a.astype(object)).max() < 2 ** 31 for p in C.fb_params(a)]
    for nd in (2, 3):
        for shape in C.tile_shapes(nd):
            for k, kind in enumerate(C.KINDS):
                a = C.tiled(kind, shape)
                fb += [(a, (c, mode, k % 2)) for c in range(1, nd + 1) for mode in C.MODES]
    fb += [(C.windows_image(), (c, mode, b)) for c in (1, 2) for mode in C.MODES for b in (0, 1)]
    fb += [(C.balls(), (c, "outer", 0)) for c in (1, 2, 3)] + [(C.balls()[4:5], (3, "outer", 0)), (C.balls()[4], (2, "outer", 0))]
    for a, (c, mode, background) in fb:
        want = U().find_boundaries(a, c, mode, background)
        top = 255 if a.dtype == np.bool_ else int(np.iinfo(a.dtype).max)
        recs.append(((0,) + zyx(a.shape) + (c, MODE_CODE[mode]), (background, top), [a.astype(np.int32), want.astype(np.uint8)]))
    for name, (a, kw) in sorted(C.CB.items()):
        val = a.astype(np.int32)
        key = label_components(val, a.ndim)
        arrays = [val, key] + ([kw["mask"].astype(np.uint8)] if "mask" in kw else []) + [U().clear_border(a, **kw).astype(np.int32)]
        recs.append(((1,) + zyx(a.shape) + (a.ndim, -1 if "mask" in kw else kw.get("buffer_size", 0)), (int(kw.get("bgval", 0)), a.size + 1), arrays))
    for name, (a, kw) in sorted(C.RS.items()):
        if name == "blobs_huge_ids" or kw.get("min_size", 64) == 0:
            continue
        val = a.astype(np.int32)
        key = label_components(a, kw.get("connectivity", 1)) if a.dtype == np.bool_ else val
        flags = (np.bincount(key.reshape(-1)) < kw.get("min_size", 64)).astype(np.uint8)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = U().remove_small_objects(a, **kw).astype(np.int32)
        recs.append(((2,) + zyx(a.shape) + (0, 0), (0, len(flags)), [val, key, flags, want]))
    return recs


@pytest.fixture(scope="module")
def records_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("label_edit") / "records.bin")
    recs = records()
    with open(path, "wb") as f:
        for head, tail, arrays in recs:
            f.write(struct.pack("<6i2q", *[int(v) for v in head + tail]))
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
    return path, len(recs)


def test_constants_are_the_header_s():
    k = C.header_constants()
    assert (C.TX, C.TY, C.TZ, C.VY) == (k["LE_TILE_X"], k["LE_TILE_Y"], k["LE_TILE_Z"], k["LE_VOL_TILE_Y"])
    assert C.TY * C.TX == C.TZ * C.VY * C.TX == k["LE_TILE_PIXELS"] and k["LE_TILE_PIXELS"] % k["LE_THREADS"] == 0
    cells = max((C.TY + 2) * (C.TX + 2), (C.TZ + 2) * (C.VY + 2) * (C.TX + 2))
    assert 4 * cells <= 64 * 1024                                           # the LDS of a workgroup


def test_harness_equals_host_routes(records_file, tmp_path):
    path, n = records_file
    exe = str(tmp_path / "label_edit_check")
    subprocess.run(["g++", "-O2", "-std=c++17", SRC, "-o", exe], check=True)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert n > 300 and "%d records, 0 bad" % n in r.stdout


def test_stand_alone_sanitizer_build_passes_every_case(records_file, tmp_path):
    path, n = records_file
    exe = str(tmp_path / "label_edit_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe], check=True)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d records, 0 bad" % n in r.stdout


def test_harness_notices_a_wrong_result(records_file, tmp_path):
    path, n = records_file
    exe, broken = str(tmp_path / "label_edit_check"), str(tmp_path / "broken.bin")
    subprocess.run(["g++", "-O2", "-std=c++17", SRC, "-o", exe], check=True)
    data = bytearray(open(path, "rb").read())
    data[-1] ^= 1                                                           # the last expected value of the last record
    open(broken, "wb").write(bytes(data))
    r = subprocess.run([exe, broken], capture_output=True, text=True)
    assert r.returncode == 1 and "%d records, 1 bad" % n in r.stdout
