"""CPU: stardist_amd.utils.measure_labels(shape=True) on host input.  The raw integer columns (second-order coordinate sums, contour
classes, 2 x 2 configuration histogram) against a brute-force statement of their definitions in Python integers; the derived columns
against scikit-image 0.18.3's regionprops_table (tests/golden/shape_reference.npz) within bounds that follow from the golden's own
rounding error; the eigenvalues against numpy.linalg.eigvalsh; the per-pixel code of the kernels (csrc/measure_shape.h through
tests/host/measure_shape_check.cpp, tiles visited in two orders) against the host route, exactly; keys, errors and host tensors.
Cases: tests/_shape_cases.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _measure_cases as M
import _shape_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "measure_shape_check.cpp")
_vp, _i = ctypes.c_void_p, ctypes.c_int


def measure(*a, **kw):
    from stardist_amd.utils import measure_labels
    return measure_labels(*a, **kw)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "shape_reference.npz"))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("measure_shape") / "libmeasure_shape.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", so], check=True)
    l = ctypes.CDLL(so)
    for name in ("msh_tile_y", "msh_tile_x", "msh_halo"):
        getattr(l, name).restype = _i
    l.msh_moment_sums.restype = l.msh_contour_counts.restype = _i
    l.msh_moment_sums.argtypes = [_vp, _i, _i, _i, _i, _vp, _i]
    l.msh_contour_counts.argtypes = [_vp, _i, _i, _i, _vp, _i]
    return l


def test_constants_are_the_header_s(lib):
    txt = open(os.path.join(ROOT, "stardist_amd", "csrc", "measure_shape.h")).read()
    assert re.findall(r"\bMSH_TILE_Y\s*=\s*(\d+)", txt) == [str(S.MSH_TILE_Y)] and lib.msh_tile_y() == S.MSH_TILE_Y
    assert re.findall(r"\bMSH_TILE_X\s*=\s*(\d+)", txt) == [str(S.MSH_TILE_X)] and lib.msh_tile_x() == S.MSH_TILE_X
    assert re.findall(r"\bMSH_HALO\s*=\s*(\d+)", txt) == [str(S.MSH_HALO)] and lib.msh_halo() == S.MSH_HALO


def test_cases_are_what_they_say():
    assert S.case("patterns3x3").shape == (115, 115) and len(np.unique(S.case("patterns3x3"))) == 512
    p = S.case("patterns4x4")
    assert p.shape == (1536, 1536) and p.max() == 65535
    assert len(np.unique(p)) == 65536
    for l, rows in ((0xF99F, ("1111", "1001", "1001", "1111")), (0x8421, ("1000", "0100", "0010", "0001")), (0x9009, ("1001", "0000", "0000", "1001"))):
        y, x = (l - 1) // 256 * 6, (l - 1) % 256 * 6                        # a ring (a hole), a diagonal chain, four separate pixels
        cell = p[y:y + 6, x:x + 6]
        assert (cell[[0, 5]] == 0).all() and (cell[:, [0, 5]] == 0).all() and set(np.unique(cell)) == {0, l}
        assert ["".join(str(int(v > 0)) for v in row) for row in cell[1:5, 1:5]] == list(rows)
    assert S.case("blobs2d").shape == (200, 260) and 60 <= len(S.host("blobs2d")["label"]) <= 100
    assert S.case("blobs3d").shape == (48, 70, 64) and 60 <= len(S.host("blobs3d")["label"]) <= 100
    assert max(S.host(n)["area"].max() for n in S.GOLDEN) <= 10 ** 4        # what the golden tolerances assume
    ys, xs = set(), set()
    for name in S.EDGES:
        a = S.case(name)
        ys.add(a.shape[0] % S.MSH_TILE_Y)
        xs.add(a.shape[1] % S.MSH_TILE_X)
        t = S.host(name)
        Y, X = a.shape
        assert a[0, 0] and a[0, X - 1] and a[Y - 1, 0] and a[Y - 1, X - 1]   # the four corners
        thin = lambda lo, hi, on: ((t[hi] - t[lo] == 1) & on & (t["area"] >= 5)).any()
        assert thin("bbox-0", "bbox-2", t["bbox-0"] == 0) and thin("bbox-0", "bbox-2", t["bbox-2"] == Y)         # one-pixel lines
        assert thin("bbox-1", "bbox-3", t["bbox-1"] == 0) and thin("bbox-1", "bbox-3", t["bbox-3"] == X)
        for ty in range(S.MSH_TILE_Y, Y, S.MSH_TILE_Y):                     # an object across every tile edge and on every tile corner
            for tx in range(0, X, S.MSH_TILE_X):
                seg = slice(tx + 3, min(tx + S.MSH_TILE_X, X) - 3)
                assert tx + 40 > X or ((a[ty - 1, seg] == a[ty, seg]) & (a[ty, seg] > 0)).any()
                assert tx == 0 or a[ty - 1, tx - 1] == a[ty, tx] > 0
        for tx in range(S.MSH_TILE_X, X, S.MSH_TILE_X):
            for ty in range(0, Y, S.MSH_TILE_Y):
                seg = slice(ty + 3, min(ty + S.MSH_TILE_Y, Y) - 3)
                assert ty + 12 > Y or ((a[seg, tx - 1] == a[seg, tx]) & (a[seg, tx] > 0)).any()
    assert ys == {S.MSH_TILE_Y - 2, S.MSH_TILE_Y - 1, 1, 2} and xs == {S.MSH_TILE_X - 2, S.MSH_TILE_X - 1, 1, 2}
    assert (S.case("small_2d") < 0).any() and S.case("huge_ids").max() == 2 ** 40


@pytest.mark.parametrize("name", S.SMALL)
def test_raw_columns_equal_the_definitions(name):
    lbl = S.case(name)
    raw = S.raw(name)
    want = S.brute_force(lbl)
    assert raw["label"].tolist() == sorted(want) and raw["m2"].dtype == np.int64 and raw["m2"].shape == (len(want), 6)
    assert ("contour" in raw) == (lbl.ndim == 2)
    for k, l in enumerate(raw["label"].tolist()):
        m2, counts = want[l]
        assert raw["m2"][k].tolist() == m2, (name, l)
        if counts is not None:
            assert raw["contour"][k].tolist() == counts, (name, l)
    if lbl.ndim == 2 and len(want) and name != "huge_ids":                  # (the oracle keeps a table row per id)
        labels, m2, counts = S.vector_oracle(lbl)                           # the oracle of the GPU test states the same
        assert np.array_equal(labels, raw["label"]) and np.array_equal(m2, raw["m2"]) and np.array_equal(counts, raw["contour"])


def test_huge_ids_and_the_negative_label():
    small, huge = S.raw("small_2d"), S.raw("huge_ids")
    assert np.array_equal(huge["label"], M.huge_ids()[2]) and np.array_equal(small["label"], M.huge_ids()[1])
    for key in ("m2", "contour"):
        assert np.array_equal(small[key], huge[key])
    lbl = S.case("small_2d")
    negative = int(-lbl.min())
    assert negative not in small["label"]                                   # background, and "not l" for its neighbours
    t, u = S.host("small_2d"), S.host("huge_ids")
    assert all(np.array_equal(t[k], u[k]) for k in t if k != "label")


def mod_pi(d):
    return np.abs((d + np.pi / 2) % np.pi - np.pi / 2)


@pytest.mark.parametrize("name", S.GOLDEN)
def test_derived_columns_against_scikit_image(golden, name):
    """Tolerances: every golden object has at most 10^4 pixels, so scikit-image's float sums are within n 2^-52 ~ 2.3e-12 of exact,
    relative to the trace; the bounds below leave a factor of 40 and more above that"""
    g = lambda key: golden["%s/%s" % (name, key)]
    lbl = S.case(name)
    assert np.array_equal(lbl, g("lbl"))                                    # the generator still makes the case the golden was made for
    t = S.host(name)
    nd = lbl.ndim
    assert list(t) == M.keys(nd) + S.shape_keys(nd)
    assert np.array_equal(t["label"], g("label")) and np.array_equal(t["area"], g("area"))
    assert all(t[k].dtype == (np.int64 if k == "euler_number" else np.float64) for k in S.shape_keys(nd))
    trace = sum(g("inertia_tensor-%d-%d" % (d, d)) for d in range(nd))
    for k in S.shape_keys(nd):
        if k.startswith("inertia_tensor"):
            assert (np.abs(t[k] - g(k)) <= 1e-10 * trace).all(), k
    for k in ("major_axis_length", "minor_axis_length"):
        assert (np.abs(t[k] - g(k)) <= 1e-10 * g(k)).all(), k
    assert (np.abs(t["equivalent_diameter"] - g("equivalent_diameter")) <= 1e-15 * g("equivalent_diameter")).all()
    assert np.array_equal(t["extent"], g("extent"))
    if nd == 3:
        return
    assert (np.abs(t["eccentricity"] ** 2 - g("eccentricity") ** 2) <= 4e-10).all()
    for k in ("perimeter", "perimeter_crofton"):
        assert (np.abs(t[k] - g(k)) <= 1e-14 * g(k)).all(), k
    assert t["euler_number"].dtype == np.int64 and np.array_equal(t["euler_number"], g("euler_number"))
    # orientation, modulo pi.  Where this table's a - c == 0 the documented rule holds exactly.  Where only scikit-image's own a - c
    # is 0 (its sums rounded differently) the golden holds 0.18.3's branch value, 90 degrees from the limit of the general formula, so
    # such a row is compared with the rule too, within the bound.  Every other row is compared with the golden within the bound.
    a, b, c = t["inertia_tensor-0-0"], t["inertia_tensor-0-1"], t["inertia_tensor-1-1"]
    branch = a - c == 0
    assert np.array_equal(t["orientation"][branch], np.where(b[branch] < 0, np.pi / 4, -np.pi / 4))
    theirs = ~branch & (g("inertia_tensor-0-0") - g("inertia_tensor-1-1") == 0)
    want = np.where(theirs, np.where(g("inertia_tensor-0-1") < 0, np.pi / 4, -np.pi / 4), g("orientation"))
    with np.errstate(all="ignore"):
        bound = 3e-10 * (a + c) / np.hypot(2 * b, c - a)
    compared = ~branch & (bound <= 1e-6)
    assert (~branch & ~compared).sum() <= 0.1 * len(a)
    assert (mod_pi(t["orientation"] - want)[compared] <= bound[compared]).all()
    print(name, "orientation rows: %d in the a == c branch, %d only in scikit-image's, %d compared, %d left out"
          % (branch.sum(), theirs.sum(), compared.sum(), (~branch & ~compared).sum()))
    # the rows whose reference is the rule and not the golden are few and known: one of the 511 patterns (0b11111010), none elsewhere
    assert theirs.sum() == (1 if name == "patterns3x3" else 0)
    if name == "patterns3x3":
        assert t["label"][theirs].tolist() == [0b11111010] and compared[theirs].all()
    if name == "small_2d":
        assert branch.sum() == 6 and len(a) == 39


def test_orientation_of_the_diagonals():
    """two 3-pixel diagonal objects pin both signs of the a - c == 0 branch: the limit of the general formula, 90 degrees from 0.18.3"""
    lbl = np.zeros((5, 9), np.int32)
    for k in range(3):
        lbl[1 + k, 1 + k] = 1                                               # down and to the right: rows and columns grow together
        lbl[1 + k, 7 - k] = 2
    t = measure(lbl, shape=True)
    assert (t["inertia_tensor-0-0"] == t["inertia_tensor-1-1"]).all()
    assert t["inertia_tensor-0-1"][0] < 0 < t["inertia_tensor-0-1"][1]
    assert t["orientation"].tolist() == [np.pi / 4, -np.pi / 4]
    assert t["eccentricity"].tolist() == [1.0, 1.0] and t["minor_axis_length"].tolist() == [0.0, 0.0]
    assert t["euler_number"].tolist() == [1, 1] and t["perimeter"].tolist() == [np.sqrt(2)] * 2      # the middle pixel: (a, d) = (0, 2)
    # the general formula next to the branch: with one more pixel beside an end a != c, and the angles stay near the branch's
    lbl[3, 4] = 1
    lbl[3, 6] = 2
    near = measure(lbl, shape=True)
    assert (near["inertia_tensor-0-0"] != near["inertia_tensor-1-1"]).all()
    assert abs(near["orientation"][0] - np.pi / 4) < 0.35 and abs(near["orientation"][1] + np.pi / 4) < 0.35


@pytest.mark.parametrize("name", S.GOLDEN + S.EDGES)
def test_eigenvalues_against_eigvalsh(name):
    t = S.host(name)
    nd = S.case(name).ndim
    T = np.stack([np.stack([t["inertia_tensor-%d-%d" % (i, j)] for j in range(nd)], axis=-1) for i in range(nd)], axis=-2)
    want = np.maximum(np.linalg.eigvalsh(T)[:, ::-1], 0)
    trace = np.trace(T, axis1=1, axis2=2)
    for k in range(nd):
        assert (np.abs(t["inertia_tensor_eigvals-%d" % k] - want[:, k]) <= 1e-12 * trace).all(), k
    lam = np.stack([t["inertia_tensor_eigvals-%d" % k] for k in range(nd)], axis=1)
    assert (lam >= 0).all() and (np.diff(lam, axis=1) <= 0).all()            # clipped, descending


def harness(lib, lbl, top=None, backwards=0):
    lab = np.ascontiguousarray(lbl.astype(np.int64).clip(-1, 2 ** 31 - 1), np.int32)
    top = int(max(lab.max(), 0)) if top is None else top
    zyx = ((1,) + lab.shape) if lab.ndim == 2 else lab.shape
    m2 = np.full((top + 1, 6), -3, np.int64)
    assert lib.msh_moment_sums(lab.ctypes.data, *zyx, top, m2.ctypes.data, backwards) == 0
    counts = None
    if lab.ndim == 2:
        counts = np.full((top + 1, 18), -3, np.int64)
        assert lib.msh_contour_counts(lab.ctypes.data, *lab.shape, top, counts.ctypes.data, backwards) == 0
    return m2, counts


@pytest.mark.parametrize("name", [n for n in S.SMALL if n != "huge_ids"])
def test_harness_equals_host_route(lib, name):
    """the per-pixel code of the kernels over tiles, forwards and backwards: every row written, absent rows 0, present rows the host's"""
    lbl = S.case(name)
    raw = S.raw(name)
    rows = raw["label"]
    for backwards in (0, 1):
        m2, counts = harness(lib, lbl, backwards=backwards)
        absent = np.setdiff1d(np.arange(len(m2)), rows)
        assert 0 in absent and (m2[absent] == 0).all() and np.array_equal(m2[rows], raw["m2"])
        if counts is not None:
            assert (counts[absent] == 0).all() and np.array_equal(counts[rows], raw["contour"])


def test_harness_ids_above_max_label_are_background(lib):
    lbl = S.case("edges-2+1")
    top = 20
    want = S.brute_force(np.where(lbl <= top, lbl, 0))
    m2, counts = harness(lib, lbl, top=top)
    assert sorted(want) == [l for l in range(top + 1) if counts[l].any()]
    for l, (wm, wc) in want.items():
        assert m2[l].tolist() == wm and counts[l].tolist() == wc
    assert lib.msh_contour_counts(None, 4, 4, 1, counts.ctypes.data, 0) == -1 and lib.msh_moment_sums(None, 1, 4, 4, 1, m2.ctypes.data, 0) == -1


def test_stand_alone_sanitizer_build_passes(tmp_path):
    exe = str(tmp_path / "measure_shape_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMEASURE_SHAPE_CHECK_MAIN",
                    SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("name", S.NAMES)
def test_without_shape_the_table_is_today_s(name):
    lbl = S.case(name)
    plain, full = measure(lbl), S.host(name)
    assert list(plain) == list(measure(lbl, shape=False)) == M.keys(lbl.ndim)
    assert list(full) == M.keys(lbl.ndim) + S.shape_keys(lbl.ndim)
    for k in plain:
        assert plain[k].dtype == full[k].dtype and np.array_equal(plain[k], full[k]), k
    if not len(plain["label"]):
        assert all(full[k].shape == (0,) and full[k].dtype == (np.int64 if k == "euler_number" else np.float64) for k in S.shape_keys(lbl.ndim))


def test_with_an_image_the_shape_columns_come_last():
    lbl, img = M.case("2d_u8_rgb")
    t = measure(lbl, img, shape=True)
    assert list(t) == M.case_keys("2d_u8_rgb") + S.shape_keys(2)
    assert all(np.array_equal(t[k], M.host("2d_u8_rgb")[k]) for k in M.host("2d_u8_rgb"))
    assert all(np.array_equal(t[k], S.host("small_2d")[k]) for k in S.shape_keys(2))


def test_argument_errors(monkeypatch):
    from stardist_amd import label_ops
    monkeypatch.setattr(label_ops, "_measure_raw_host", lambda *a, **k: pytest.fail("something ran"))
    monkeypatch.setattr(label_ops, "_measure_raw_device", lambda *a, **k: pytest.fail("something ran"))
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.int32), shape=(2 ** 21, 2 ** 21), strides=(0, 0))     # 2^42 pixels x 2^42
    for dev in (None, "cuda"):
        with pytest.raises(ValueError, match="2\\^63"):
            measure(big, shape=True, device=dev)
        with pytest.raises(ValueError, match="2D or 3D"):
            measure(np.zeros(7, np.int32), shape=True, device=dev)
        with pytest.raises(ValueError, match="shape"):
            measure(np.zeros((4, 5), np.int32), np.zeros((4, 6)), shape=True, device=dev)
    with pytest.raises(TypeError):
        measure(np.zeros((4, 5), np.int32), None, True)                     # keyword only


def test_float_labels_are_refused():
    with pytest.raises(ValueError, match="integer"):
        measure(np.zeros((4, 5), np.float32), shape=True)


@pytest.mark.parametrize("name", ("small_2d", "small_3d", "patterns3x3", "patterns4x4", "blobs2d", "blobs3d", "empty_2d", "empty_3d", "huge_ids"))
def test_host_tensors_against_numpy(name):
    """as_tensors=True on host tensors: == on every column that is + - * / sqrt of the integer tables; atan2 and pow may differ by the
    two libraries' rounding, at most 1e-14 of max(|a|, |b|, 1) -- 45 ulp, above the 6 and 16 ulp a device library is allowed plus 1"""
    import torch
    lbl = S.case(name)
    want = S.host(name)
    got = measure(torch.from_numpy(lbl.copy()), shape=True, as_tensors=True)
    assert list(got) == list(want)
    for k in want:
        assert isinstance(got[k], torch.Tensor) and got[k].device.type == "cpu" and got[k].dim() == 1
        a, b = got[k].numpy(), want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if k == "orientation" or (k == "equivalent_diameter" and lbl.ndim == 3):
            assert (np.abs(a - b) <= 1e-14 * np.maximum(np.maximum(np.abs(a), np.abs(b)), 1)).all(), k
        else:
            assert np.array_equal(a, b), k
