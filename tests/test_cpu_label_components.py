"""CPU: stardist_amd.utils.label_components on host input -- against scipy.ndimage.label (masks), against scipy.ndimage.label per value
(multi-valued images), against scikit-image 0.18's skimage.measure.label (tests/golden/label_components_reference.npz) -- and the four
phases of the device pass (csrc/label_cc.h through tests/host/label_cc_check.cpp: tiles, local arrays, border merge, flatten, number)
against the host route, in two visiting orders, and once more under the address and undefined-behaviour sanitizers as a stand-alone
program.  All comparisons are exact.  Cases: tests/_label_cc_cases.py."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import _label_cc_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "label_cc_check.cpp")
_vp, _i = ctypes.c_void_p, ctypes.c_int
DTYPE_CODE = {"bool": 0, "uint8": 0, "uint16": 1, "int32": 3}


def label(*a, **kw):
    from stardist_amd.utils import label_components
    return label_components(*a, **kw)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("label_cc") / "liblabel_cc.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", so], check=True)
    l = ctypes.CDLL(so)
    for name in ("lcc_tile_x", "lcc_tile_y", "lcc_tile_z", "lcc_vol_tile_y", "lcc_tile_pixels"):
        getattr(l, name).restype = _i
    l.lcc_label.restype = _i
    l.lcc_label.argtypes = [_vp, _i, _i, _i, _i, _i, ctypes.c_longlong, _i, _vp, _vp]
    return l


def zyx(shape):
    return ((1,) + tuple(shape)) if len(shape) == 2 else tuple(shape)


def harness(lib, img, connectivity, background, reversed_order):
    a = np.ascontiguousarray(img)
    out = np.full(a.shape, -5, np.int32)
    n = ctypes.c_int(-1)
    rc = lib.lcc_label(a.ctypes.data, DTYPE_CODE[a.dtype.name], *zyx(a.shape), connectivity, int(background), int(reversed_order), out.ctypes.data,
                       ctypes.addressof(n))
    assert rc == 0, rc                                                      # -2: a write broke par[p] <= p
    return out, n.value


def test_constants_are_the_header_s(lib):
    k = C.header_constants()
    assert (lib.lcc_tile_x(), lib.lcc_tile_y(), lib.lcc_tile_z(), lib.lcc_vol_tile_y(), lib.lcc_tile_pixels()) == \
        (k["LCC_TILE_X"], k["LCC_TILE_Y"], k["LCC_TILE_Z"], k["LCC_VOL_TILE_Y"], k["LCC_TILE_PIXELS"]) == (C.TX, C.TY, C.TZ, C.VY, k["LCC_TILE_PIXELS"])
    assert C.TY * C.TX == C.TZ * C.VY * C.TX == k["LCC_TILE_PIXELS"] and 2 * 4 * k["LCC_TILE_PIXELS"] <= 64 * 1024       # the LDS of a workgroup


def count(name, c):
    img, background = C.case(name)
    return ndimage.label(img != background, ndimage.generate_binary_structure(img.ndim, c))[1]


def test_cases_are_what_they_say():
    for name in C.NAMES:
        img, _ = C.case(name)
        assert img.dtype.name in DTYPE_CODE and img.flags["C_CONTIGUOUS"] and img.size <= 400000, name
        if name not in C.EMPTY + ("single_pixel", "one_row", "one_column", "plane_as_volume", "random_small_0.59"):
            tile = (C.TY, C.TX) if img.ndim == 2 else (C.TZ, C.VY, C.TX)
            assert all(n > 2 * t and n % t for n, t in zip(img.shape, tile)), name      # several tiles, a partial last one
            assert img.size >= 3000, name
    for name in ("spiral", "serpentine", "u_shape", "comb", "comb3d"):
        assert [count(name, c) for c in C.connectivities(name)] == [1] * C.case(name)[0].ndim, name
    sp = C.case("spiral")[0]
    assert (sp.sum(axis=1) > 0).all() and 0.4 < sp.mean() < 0.6             # it fills the image: it crosses every tile border
    assert not C.case("comb")[0][:-1, 1::2].any() and not C.case("comb3d")[0][:-1, 1::2].any()
    for name in ("checkerboard", "checkerboard3d"):
        nd = C.case(name)[0].ndim
        assert [count(name, c) for c in (1, nd)] == [(C.case(name)[0].size + 1) // 2, 1]
    assert count("diagonals", 1) == C.case("diagonals")[0].sum() and count("diagonals", 2) < 40
    assert [count("rings", c) for c in (1, 2, 3)] == [2, 1, 1]
    h = [count("helix", c) for c in (1, 2, 3)]
    assert h[0] > h[1] >= h[2] == 1
    assert not C.case("all_background")[0].any() and C.case("all_foreground")[0].all() and C.case("all_foreground3d")[0].all()
    assert C.case("single_pixel")[0].shape == (1, 1) and C.case("one_row")[0].shape[0] == 1 and C.case("one_column")[0].shape[1] == 1
    assert C.case("plane_as_volume")[0].shape[0] == 1 and C.case("empty")[0].size == 0 and C.case("empty3d")[0].ndim == 3
    big = C.host("random_0.59", 2)[0]
    assert np.bincount(big.reshape(-1))[1:].max() > 0.5 * C.case("random_0.59")[0].sum()      # one component spans the image
    u8, i32, u16 = C.case("blocks_u8")[0], C.case("blocks_i32_negative")[0], C.case("blocks_u16_high")[0]
    assert (i32 < 0).any() and i32.min() == -2 ** 31 and i32.max() == 2 ** 31 - 1 and (u16 > 2 ** 15).sum() > 1000 and u16.max() == 65535
    for v in (1, 2, 3, 255):                                                # one value in several separated blobs
        assert ndimage.label(u8 == v)[1] > 3
    assert (u8[:, 1:] != u8[:, :-1])[(u8[:, 1:] != 0) & (u8[:, :-1] != 0)].sum() > 20         # touching objects of different values
    assert C.case("blocks_u8_background_3")[1] == 3 and not (u8 == 7).any() and C.case("blocks_u8_background_absent")[1] == 7
    assert C.case("blocks_i32_background_-7")[1] == -7 and C.case("blocks_u16_background_65535")[1] == 65535


@pytest.mark.parametrize("name", C.MASKS)
def test_host_route_equals_scipy_on_masks(name):
    img, _ = C.case(name)
    for c in C.connectivities(name):
        got, n = C.host(name, c)
        want, m = ndimage.label(img, ndimage.generate_binary_structure(img.ndim, c))
        assert got.dtype == np.int32 and got.shape == img.shape and n == m and np.array_equal(got, want), (name, c)
        for dt in ("uint8", "int32"):                                       # a mask of another dtype: the same components
            again, k = label(img.astype(dt), c, return_num=True)
            assert k == n and again.dtype == np.int32 and np.array_equal(again, got), (name, c, dt)


@pytest.mark.parametrize("name", C.MULTI)
def test_host_route_equals_per_value_oracle(name):
    img, background = C.case(name)
    for c in C.connectivities(name):
        got, n = C.host(name, c)
        want, m = C.per_value_oracle(img, c, background)
        assert got.dtype == np.int32 and n == m == got.max() and np.array_equal(got, want), (name, c)
        assert np.array_equal(got == 0, img == background)


def test_host_route_equals_scikit_image_golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "label_components_reference.npz"))
    names = sorted(set(k.split("/")[0] for k in g.files))
    assert len(names) >= 12 and any(n in C.MULTI for n in names) and any(C.case(n)[0].ndim == 3 for n in names)
    for name in names:
        img, background = C.case(name)
        assert np.array_equal(img, g[name + "/img"]) and img.dtype == g[name + "/img"].dtype and int(g[name + "/background"]) == background
        for c in C.connectivities(name):
            got, n = C.host(name, c)
            assert n == int(g["%s/c%d/n" % (name, c)]) and np.array_equal(got, g["%s/c%d/labels" % (name, c)]), (name, c)


@pytest.mark.parametrize("name", [n for n in C.NAMES if n not in C.EMPTY])
def test_harness_equals_host_route_in_both_orders(lib, name):
    img, background = C.case(name)
    for c in C.connectivities(name):
        want, n = C.host(name, c)
        for dt in C.dtypes(name):
            for rev in (False, True):
                got, m = harness(lib, img.astype(dt), c, background, rev)
                assert m == n and np.array_equal(got, want), (name, c, dt, rev)
    if img.ndim == 2:                                                       # Z = 1 with the 3D offsets: the rule for connectivity 2
        got, m = harness(lib, img, 3, background, False)
        assert m == C.host(name, 2)[1] and np.array_equal(got, C.host(name, 2)[0])


def test_harness_argument_checks(lib):
    a = np.ones((4, 4), np.uint8)
    out = np.zeros((4, 4), np.int32)
    n = ctypes.c_int(0)
    ok = lambda *args: lib.lcc_label(*args, out.ctypes.data, ctypes.addressof(n))
    assert ok(a.ctypes.data, 0, 1, 4, 4, 1, 0, 0) == 0
    assert ok(None, 0, 1, 4, 4, 1, 0, 0) == ok(a.ctypes.data, 2, 1, 4, 4, 1, 0, 0) == ok(a.ctypes.data, 0, 0, 4, 4, 1, 0, 0) == -1
    assert ok(a.ctypes.data, 0, 1, 4, 4, 0, 0, 0) == ok(a.ctypes.data, 0, 1, 4, 4, 4, 0, 0) == ok(a.ctypes.data, 0, 2, 2 ** 15, 2 ** 15, 1, 0, 0) == -1


def test_stand_alone_sanitizer_build_passes_every_case(tmp_path):
    exe, cases = str(tmp_path / "label_cc_check"), str(tmp_path / "cases.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DLABEL_CC_CHECK_MAIN", SRC,
                    "-o", exe], check=True)
    records = 0
    with open(cases, "wb") as f:
        for name in C.NAMES:
            if name in C.EMPTY:
                continue
            img, background = C.case(name)
            for c in C.connectivities(name):
                want, n = C.host(name, c)
                for dt in (C.dtypes(name)[0], C.dtypes(name)[-1]):
                    a = np.ascontiguousarray(img.astype(dt))
                    f.write(struct.pack("<6iq", DTYPE_CODE[dt], *zyx(a.shape), c, n, background))
                    f.write(a.tobytes())
                    f.write(np.ascontiguousarray(want, "<i4").tobytes())
                    records += 1
    r = subprocess.run([exe, cases], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d records, 0 bad" % records in r.stdout


def test_arguments_and_routing(monkeypatch):
    import torch
    from stardist_amd import label_ops
    monkeypatch.setattr(label_ops, "_label_components_device", lambda *a, **k: pytest.fail("device path taken"))
    img, _ = C.case("blocks_u8")
    want, n = C.host("blocks_u8", 2)
    assert np.array_equal(label(img), want) and np.array_equal(label(img, None, None), want)       # None: ndim, background 0
    assert np.array_equal(label(img.tolist()), want)
    lab, k = label(img.astype(np.int64), return_num=True)
    assert k == n and type(k) is int and lab.dtype == np.int32 and np.array_equal(lab, want)
    assert np.array_equal(label(img.astype(np.float64) / 2, background=0.0), want)                 # a dtype the kernels do not take
    assert np.array_equal(label(img, 1), C.host("blocks_u8", 1)[0])
    t = label(torch.from_numpy(img.copy()), 2)                              # a host tensor: the host code, a host tensor out
    assert isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.device.type == "cpu" and np.array_equal(t.numpy(), want)
    t, k = label(torch.from_numpy(img.astype(np.int64)), 2, return_num=True)
    assert k == n and np.array_equal(t.numpy(), want)
    for bad in (0, 3, -1, 1.5, "2", True):
        with pytest.raises(ValueError, match="Connectivity"):
            label(img, bad)
    with pytest.raises(ValueError, match="Connectivity"):
        label(C.case("rings")[0], 4)
    for dev in (None, "cuda"):                                              # the same errors, before anything runs, on both routes
        with pytest.raises(ValueError, match="2D or 3D"):
            label(np.zeros(7, np.uint8), device=dev)
        with pytest.raises(ValueError, match="2D or 3D"):
            label(np.zeros((2, 3, 4, 5), np.uint8), device=dev)
        with pytest.raises(ValueError, match="Connectivity"):
            label(img, 3, device=dev)
    for name in C.EMPTY:
        e, k = label(C.case(name)[0], return_num=True)
        assert e.shape == C.case(name)[0].shape and e.dtype == np.int32 and k == 0
    import stardist_amd
    assert not hasattr(stardist_amd, "label_components")                    # the top-level names mirror the reference's exports


def test_device_route_is_taken_for_the_kernel_dtypes(monkeypatch):
    from stardist_amd import label_ops
    seen = []

    def fake(img, connectivity, background, device):
        seen.append((str(img.dtype), connectivity, background, device))
        raise RuntimeError("stop")
    monkeypatch.setattr(label_ops, "_label_components_device", fake)
    for dt in ("bool", "uint8", "uint16", "int32"):
        with pytest.raises(RuntimeError, match="stop"):
            label(np.zeros((3, 4), dt), device="cuda", background=np.int64(2))
    assert seen == [(dt, 2, 2, "cuda") for dt in ("bool", "uint8", "uint16", "int32")]
    for dt in ("int64", "float32", "int8"):                                # the host code, numpy out
        assert label(np.ones((3, 4), dt), device="cuda").max() == 1
    assert label(np.ones((3, 4), np.uint8), background=0.5, device="cuda").max() == 1
    assert len(seen) == 4
