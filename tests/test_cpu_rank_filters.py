"""CPU: stardist_amd.rank_filters on host input -- the five filters and the four morphology functions against scipy.ndimage with == on
every NaN-free case, against a loop over the definition (tests/_rank_filter_cases.py: explicit index maps, sorted() per window, the
NaN rule) on every case, the argument rules -- and the per-element rules of the device passes (csrc/rank_filter.h through
tests/host/rank_filter_check.cpp) against the host route, as a stand-alone program built plain and under the address and
undefined-behaviour sanitizers.  All comparisons are exact."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _rank_filter_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "rank_filter_check.cpp")
CASES = C.cases()
NAMES = C.FILTERS + C.MORPHOLOGY


def U():
    from stardist_amd import utils
    return utils


def test_the_names_are_public():
    import stardist_amd
    from stardist_amd import rank_filters, utils
    for name in NAMES:
        assert getattr(utils, name) is getattr(rank_filters, name) and not hasattr(stardist_amd, name)


def test_the_cases_cover_what_they_should():
    fns = {c[0] for c in CASES.values()}
    assert fns == set(NAMES) and len(CASES) > 350
    assert {c[1].dtype.type for c in CASES.values()} == set(C.DTYPES)
    assert {c[2].get("mode", "reflect") for c in CASES.values()} == set(C.MODES)
    assert sum(C.has_nan(c[1]) for c in CASES.values()) >= 15
    assert {c[1].shape for c in CASES.values()} >= {(67, 131), (5, 70, 33), (1, 1), (1, 40), (40, 1), (5, 6)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_scipy_and_the_definition(name):
    import scipy.ndimage as ndi
    fn, img, kw = CASES[name]
    keep = img.copy()
    got = getattr(U(), fn)(img, **kw)
    assert np.array_equal(img, keep, equal_nan=img.dtype.kind == "f") and got.flags["C_CONTIGUOUS"]
    if not C.has_nan(img):
        with np.errstate(all="ignore"):
            assert C.same(got, getattr(ndi, fn)(img, **kw))
    assert C.same(got, C.brute(fn, img, **kw))


@pytest.mark.parametrize("fn", C.MORPHOLOGY)
def test_morphology_equals_scipy_with_size_and_with_footprint(fn):
    import scipy.ndimage as ndi
    rng = np.random.RandomState(3)
    for dtype in C.DTYPES:
        img = C.noise((23, 37), dtype, 11)
        for size in ((3, 3), (4, 4), (2, 5), (4, 3), (1, 6)):
            fp = rng.rand(*size) > 0.4
            fp[0, 0] = True
            for mode in C.MODES:
                cval = C.a_cval(dtype)
                assert C.same(getattr(U(), fn)(img, size, mode=mode, cval=cval), getattr(ndi, fn)(img, size=size, mode=mode, cval=cval))
                assert C.same(getattr(U(), fn)(img, footprint=fp, mode=mode, cval=cval), getattr(ndi, fn)(img, footprint=fp, mode=mode, cval=cval))


def test_the_nan_rule_and_the_cases_are_what_they_say():
    a = np.zeros((9, 9), np.float32)
    a[4, 4] = np.nan
    for fn in ("minimum_filter", "maximum_filter", "median_filter"):
        got = getattr(U(), fn)(a, 3)
        assert np.argwhere(np.isnan(got)).tolist() == [[y, x] for y in (3, 4, 5) for x in (3, 4, 5)]
    ell = C.footprints()["ell"]                                             # 4 x 3, window rows y - 2 .. y + 1, columns x - 1 .. x + 1
    got = U().maximum_filter(a, footprint=ell)
    assert sorted(map(tuple, np.argwhere(np.isnan(got)))) == sorted({(4 + 2 - dy, 4 + 1 - dx) for dy, dx in np.argwhere(ell)})
    assert np.isnan(U().grey_opening(a, 3)).sum() == 25 and np.isnan(U().white_tophat(a, 3)).sum() == 25
    corner = np.zeros((6, 6), np.float32)
    corner[0, 0] = np.nan
    assert np.isnan(U().median_filter(corner, 5)).sum() == 9 and np.isnan(U().median_filter(corner, 5, mode="mirror")).sum() == 9
    assert np.isnan(U().median_filter(corner, 5, mode="constant", cval=1.0)).sum() == 9
    inf = np.zeros((5, 5), np.float32)
    inf[2, 2] = np.inf
    assert np.isinf(U().white_tophat(inf, 3)[2, 2]) and np.isnan(U().white_tophat(np.full((5, 5), np.inf, np.float32), 3)).all()
    u = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert U().white_tophat(u, 3, mode="constant", cval=255)[0, 0] == 1     # numpy's wrap, as scipy has it
    assert U().minimum_filter(u, (1, 4), origin=(0, -2)).tolist()[0] == [0, 1, 2, 1] and U().minimum_filter(u, (1, 4), origin=(0, 1)).tolist()[0] == [0] * 4


def test_inputs_of_other_kinds(monkeypatch):
    import torch
    from stardist_amd import rank_filters
    monkeypatch.setattr(rank_filters, "_device_plan", lambda *a, **k: pytest.fail("device path taken"))
    img = C.noise((20, 30), np.float32, 2)
    want = U().median_filter(img, 3)
    got = U().median_filter(torch.from_numpy(img), 3)                        # a host tensor: the host code, a tensor back
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and C.same(got.numpy(), want)
    assert C.same(U().median_filter(np.asfortranarray(img), 3), want) and C.same(U().median_filter(img[::-1][::-1], 3), want)
    mask = torch.from_numpy(img > 0)
    got = U().white_tophat(mask, 3)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.bool and C.same(got.numpy(), U().white_tophat(img > 0, 3))
    assert C.same(U().minimum_filter(img, footprint=torch.ones(3, 3, dtype=torch.bool)), U().minimum_filter(img, 3))
    empty = np.zeros((0, 5), np.uint8)
    assert U().median_filter(empty, 3).shape == (0, 5)


def test_argument_errors(monkeypatch):
    from stardist_amd import rank_filters
    monkeypatch.setattr(rank_filters, "_device_plan", lambda *a, **k: pytest.fail("device work before the argument checks"))
    monkeypatch.setattr(rank_filters.R, "to_device_tensor", lambda *a, **k: pytest.fail("device work before the argument checks"))
    img = C.noise((12, 15), np.float32, 2)
    u8 = C.noise((12, 15), np.uint8, 2)
    calls = {fn: (lambda a, _f=fn, **k: getattr(U(), _f)(a, **k)) for fn in NAMES}
    calls["rank_filter"] = lambda a, **k: U().rank_filter(a, k.pop("rank", 1), **k)
    calls["percentile_filter"] = lambda a, **k: U().percentile_filter(a, k.pop("percentile", 40), **k)
    for fn, call in calls.items():
        for dev in (None, "cuda"):
            for dtype in (np.float64, np.int32, np.int8, np.float16, np.uint32):
                with pytest.raises(TypeError, match="bool, uint8, uint16 or float32"):
                    call(np.zeros((4, 5), dtype), size=3, device=dev)
            for shape in ((5,), (2, 3, 4, 5)):
                with pytest.raises(ValueError, match="2D or 3D"):
                    call(np.zeros(shape, np.float32), size=3, device=dev)
            with pytest.raises(ValueError, match="2\\^32 - 1 pixels"):
                call(np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), (2 ** 16, 2 ** 16), (0, 0)), size=3, device=dev)
            for kw in (dict(), dict(size=3, footprint=np.ones((3, 3), bool))):
                with pytest.raises(ValueError, match="exactly one of size and footprint"):
                    call(img, device=dev, **kw)
            for bad in (0, -1, 1.5, (3,), (3, 3, 3), (3, 0), "3", True):
                with pytest.raises(ValueError, match="size"):
                    call(img, size=bad, device=dev)
            for bad in (np.zeros((3, 3), bool), np.ones(3, bool), np.ones((3, 3, 3), bool), np.ones((3, 3), np.float32)):
                with pytest.raises(ValueError, match="footprint"):
                    call(img, footprint=bad, device=dev)
            for bad in ("wrap", "grid-wrap", "grid-constant", "Reflect", ("reflect", "nearest"), None, 0):
                with pytest.raises(ValueError, match="mode"):
                    call(img, size=3, mode=bad, device=dev)
            for bad in (np.nan, "0", None, 1e39, 0.1):                      # 0.1 is no float32
                with pytest.raises(ValueError, match="cval"):
                    call(img, size=3, mode="constant", cval=bad, device=dev)
            for bad in (-1, 256, 1.5, np.inf, -np.inf, np.nan):
                with pytest.raises(ValueError, match="cval"):
                    call(u8, size=3, cval=bad, device=dev)
            for bad in (2, -1, 0.5):
                with pytest.raises(ValueError, match="cval"):
                    call(u8 > 100, size=3, cval=bad, device=dev)
            with pytest.raises(ValueError, match="cval"):
                call(u8.astype(np.uint16), size=3, cval=65536, device=dev)
            assert call(img, size=3, mode="constant", cval=0.5).shape == img.shape and call(u8 > 100, size=3, cval=True).dtype == bool
    for fn in C.FILTERS:
        for dev in (None, "cuda"):
            for size, bad in ((4, 2), (4, -3), (5, 3), (5, -3), ((4, 5), (2, 0)), ((4, 5), (0, -3)), (3, (0,)), (3, (0, 0, 0)), (3, 0.5), (3, True)):
                with pytest.raises(ValueError, match="origin"):
                    calls[fn](img, size=size, origin=bad, device=dev)
            with pytest.raises(ValueError, match="origin"):
                calls[fn](img, footprint=C.footprints()["ell"], origin=(2, 0), device=dev)
    for fn in C.MORPHOLOGY:
        with pytest.raises(TypeError):
            calls[fn](img, size=3, origin=0)
    for dev in (None, "cuda"):
        for bad in (9, -10, 1.0, "1", None, True):
            with pytest.raises(ValueError, match="rank"):
                U().rank_filter(img, bad, size=3, device=dev)
        for bad in (100.5, -100.5, np.nan, "50", None):
            with pytest.raises(ValueError, match="percentile"):
                U().percentile_filter(img, bad, size=3, device=dev)


# ----------------------------------------------------------------------------- the device passes' rules on the host

_CODE = {"bool": 0, "uint8": 0, "uint16": 1, "float32": 2}
_OP = {"min": 0, "max": 1, "rank": 2}


def call_record(fn, img, kw):
    """bytes as rank_filter_check.cpp reads them: the plan of one call, the image and the host route's result"""
    from stardist_amd import rank_filters as RF
    nd, name = img.ndim, img.dtype.name
    plan, fuse, mode, cval = RF._plan(fn, nd, name, kw.get("size"), kw.get("footprint"), kw.get("mode", "reflect"), kw.get("cval", 0),
                                      kw.get("origin", 0), kw.get("rank"), kw.get("percentile"))
    if fuse is not None and name == "bool":
        fuse = "xor"
    pad = lambda v, fill: (fill,) * (3 - nd) + tuple(v)
    out = struct.pack("<5i3qd", 0, _CODE[name], RF._MODES[mode], RF._FUSE[fuse], len(plan), *pad(img.shape, 1), float(cval))
    for op, rank, extent, fp, origin in plan:
        offsets = np.argwhere(np.ones(extent, bool) if fp is None else fp).astype(np.int32)
        offsets = np.concatenate([np.zeros((len(offsets), 3 - nd), np.int32), offsets], axis=1)
        out += struct.pack("<10i", _OP[op], rank, len(offsets), int(fp is None), *pad(extent, 1), *pad(origin, 0)) + np.ascontiguousarray(offsets).tobytes()
    want = getattr(U(), fn)(img, **kw)
    return out + np.ascontiguousarray(img).tobytes() + want.tobytes()


def predicate_records():
    """the caps and the tier boundaries as stardist_amd.rank_filters states them, for the header to agree with"""
    from stardist_amd import rank_filters as RF
    recs = [struct.pack("<8i", 1, 2, RF._LDS_BYTES, RF.MAX_WINDOW, RF.MAX_FOOTPRINT, 0, 0, 1)]
    for dtype in (np.uint8, np.uint16, np.float32):
        b = np.dtype(dtype).itemsize
        for size in (1, 2, 160, 161, 162, 352, 353, 354, 736, 737, 738, 1025):
            for last in (0, 1):
                recs.append(struct.pack("<8i", 1, 0, b, size, last, 0, 0, int(RF.box_window_in_lds(dtype, size, bool(last)))))
        for nd, extents in ((2, [(1, s, s) for s in range(1, 200, 7)] + [(1, 1, 1025), (1, 1025, 1), (1, 98, 98), (1, 99, 98)]),
                            (3, [(s, s, s) for s in range(1, 40, 3)] + [(1, 1, 1025), (1025, 1, 1), (9, 60, 2)])):
            for e in extents:
                recs.append(struct.pack("<8i", 1, 1, b, int(nd == 3), *e, int(RF.footprint_window_in_lds(nd, dtype, e[3 - nd:]))))
    return recs


def records():
    return [call_record(*CASES[name]) for name in sorted(CASES)] + predicate_records()


@pytest.fixture(scope="module")
def records_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("rank_filters") / "records.bin")
    recs = records()
    with open(path, "wb") as f:
        f.write(b"".join(recs))
    return path, recs


def test_tier_boundaries_are_where_the_documents_say():
    from stardist_amd import rank_filters as RF
    for dtype, top in ((np.uint8, 737), (np.bool_, 737), (np.uint16, 353), (np.float32, 161)):
        assert RF.box_window_in_lds(dtype, top, False) and not RF.box_window_in_lds(dtype, top + 1, False)
        assert RF.box_window_in_lds(dtype, RF.MAX_WINDOW, True)
    assert RF.footprint_window_in_lds(2, np.float32, (81, 65)) and not RF.footprint_window_in_lds(2, np.float32, (82, 65))
    assert RF.footprint_window_in_lds(3, np.uint16, (13, 13, 33)) and not RF.footprint_window_in_lds(3, np.uint16, (13, 14, 33))


def test_harness_equals_host_route(records_file, tmp_path):
    path, recs = records_file
    exe = str(tmp_path / "rank_filter_check")
    subprocess.run(["g++", "-O2", "-std=c++17", SRC, "-o", exe], check=True)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert len(recs) > 500 and "%d records, 0 bad" % len(recs) in r.stdout
    assert int(r.stdout.split(",")[-1].split()[0]) > 1000000                # and it went over the pixels


def test_stand_alone_sanitizer_build_passes_every_case(records_file, tmp_path):
    path, recs = records_file
    exe = str(tmp_path / "rank_filter_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe], check=True)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d records, 0 bad" % len(recs) in r.stdout


def test_harness_notices_a_wrong_result(records_file, tmp_path):
    path, recs = records_file
    exe, broken = str(tmp_path / "rank_filter_check"), str(tmp_path / "broken.bin")
    subprocess.run(["g++", "-O2", "-std=c++17", SRC, "-o", exe], check=True)
    data = bytearray(open(path, "rb").read())
    data[len(recs[0]) - 1] ^= 1                                             # the last element of the first call record
    data[-4] ^= 1                                                           # what the last predicate should give
    open(broken, "wb").write(bytes(data))
    r = subprocess.run([exe, broken], capture_output=True, text=True)
    assert r.returncode == 1 and "%d records, 2 bad" % len(recs) in r.stdout
