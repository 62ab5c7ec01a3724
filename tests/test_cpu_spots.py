"""CPU: stardist_amd.spots on host input -- gaussian_filter against scipy bit for bit, its weight table against scipy's impulse response,
peak_local_max against a loop over the definition (tests/_spots_cases.py) and against scikit-image 0.18.3
(tests/golden/peaks_reference.npz, written by tests/golden/make_peaks_golden.py), measure_labels(spots=) against a loop -- and the
per-element rules of the device pass (csrc/spots.h through tests/host/spots_check.cpp) against the host route, as a stand-alone program
built plain and under the address and undefined-behaviour sanitizers.  All comparisons are exact."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import _label_contacts_cases as LC
import _spots_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "spots_check.cpp")
GAUSS = C.gauss_cases()
PEAKS = C.peak_cases()


def U():
    from stardist_amd import utils
    return utils


def same_floats(got, want):
    """bit for bit, but for the payload and sign of a NaN"""
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(np.where(nan, 0, got.view(np.uint32)), np.where(nan, 0, want.view(np.uint32)))


def test_the_names_are_public():
    import stardist_amd
    from stardist_amd import spots, utils
    for name in ("gaussian_filter", "difference_of_gaussians", "peak_local_max", "detect_spots"):
        assert getattr(utils, name) is getattr(spots, name) and not hasattr(stardist_amd, name)


# ----------------------------------------------------------------------------- gaussian_filter

@pytest.mark.parametrize("case", GAUSS, ids=[c[0] for c in GAUSS])
def test_gaussian_equals_scipy(case):
    import scipy.ndimage as ndi
    _, img, sigma, truncate = case
    keep = img.copy()
    got = U().gaussian_filter(img, sigma, truncate=truncate)
    assert same_floats(got, ndi.gaussian_filter(img, sigma, output=np.float32, mode="reflect", truncate=truncate))
    assert np.array_equal(img, keep) and got.flags["C_CONTIGUOUS"]


@pytest.mark.parametrize("name", ("inf_nan", "denormals", "huge"))
def test_gaussian_special_floats_equal_scipy(name):
    import scipy.ndimage as ndi
    img = C.special_float_images()[name]
    with np.errstate(all="ignore"):
        want = ndi.gaussian_filter(img, (1.0, 2.5), output=np.float32)
    assert same_floats(U().gaussian_filter(img, (1.0, 2.5)), want)


@pytest.mark.parametrize("sigma", (0.5, 1, 1.3, 2.5, 7))
def test_weight_table_is_scipys_impulse_response(sigma):
    import scipy.ndimage as ndi
    from stardist_amd.spots import gaussian_weights
    r = int(4.0 * sigma + 0.5)
    impulse = np.zeros(8 * r + 1)
    impulse[4 * r] = 1.0
    w = gaussian_weights(float(sigma), r)
    assert w.dtype == np.float64 and w.shape == (2 * r + 1,)
    assert np.array_equal(ndi.gaussian_filter(impulse, sigma, mode="reflect")[3 * r:5 * r + 1], w)


def test_difference_of_gaussians_is_one_subtraction():
    img = C.noise((40, 50), np.uint16, 1)
    low, high = U().gaussian_filter(img, (1.0, 2.0)), U().gaussian_filter(img, (1.6 * 1.0, 1.6 * 2.0))
    assert same_floats(U().difference_of_gaussians(img, (1.0, 2.0)), low - high)
    assert same_floats(U().difference_of_gaussians(img, (1.0, 2.0), 3.0), low - U().gaussian_filter(img, 3.0))
    assert np.abs(low - high).max() > 100


def test_inputs_of_other_kinds_and_bad_arguments(monkeypatch):
    import torch
    from stardist_amd import spots
    monkeypatch.setattr(spots, "_gaussian_device", lambda *a, **k: pytest.fail("device path taken"))
    monkeypatch.setattr(spots, "_peaks_device", lambda *a, **k: pytest.fail("device path taken"))
    img = C.noise((20, 30), np.float32, 2)
    want = U().gaussian_filter(img, 1.5)
    got = U().gaussian_filter(torch.from_numpy(img), 1.5)                    # a host tensor: the host code, a tensor back
    assert isinstance(got, torch.Tensor) and same_floats(got.numpy(), want)
    assert same_floats(U().gaussian_filter(np.asfortranarray(img), 1.5), want)
    peaks = U().peak_local_max(torch.from_numpy(img), 2, as_tensors=True)
    assert isinstance(peaks, torch.Tensor) and peaks.dtype == torch.int64 and np.array_equal(peaks.numpy(), U().peak_local_max(img, 2))
    for fn in (lambda a, **k: U().gaussian_filter(a, 1.0, **k), lambda a, **k: U().difference_of_gaussians(a, 1.0, **k),
               lambda a, **k: U().peak_local_max(a, **k), lambda a, **k: U().detect_spots(a, 1.0, **k)):
        for dev in (None, "cuda"):
            for dtype in (np.float64, np.int32, np.int8, bool, np.float16):
                with pytest.raises(TypeError, match="uint8, uint16 or float32"):
                    fn(np.zeros((4, 5), dtype), device=dev)
            for shape in ((5,), (2, 3, 4, 5)):
                with pytest.raises(ValueError, match="2D or 3D"):
                    fn(np.zeros(shape, np.float32), device=dev)
            with pytest.raises(ValueError, match="2\\^32 - 1 pixels"):
                fn(np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), (2 ** 16, 2 ** 16), (0, 0)), device=dev)
    for dev in (None, "cuda"):
        for bad in (-1.0, (1.0, 2.0, 3.0), np.nan, np.inf, "a"):
            with pytest.raises(ValueError, match="sigma"):
                U().gaussian_filter(img, bad, device=dev)
        for bad in (0, -1, np.inf, np.nan, "4"):
            with pytest.raises(ValueError, match="truncate"):
                U().gaussian_filter(img, 1.0, truncate=bad, device=dev)
        for kw in (dict(min_distance=-1), dict(min_distance=1.5), dict(min_distance=(1, 2, 3)), dict(exclude_border=-1), dict(exclude_border=(1, -2)),
                   dict(exclude_border=(1,)), dict(threshold_abs=np.nan), dict(threshold_abs="1"), dict(threshold_rel=np.nan), dict(num_peaks=-1),
                   dict(num_peaks=1.5), dict(num_peaks_per_label=-2), dict(labels=np.zeros((20, 30), np.float32)), dict(labels=np.zeros((20, 31), int)),
                   dict(labels=np.full((20, 30), -1)), dict(labels=np.full((20, 30), 2 ** 31))):
            with pytest.raises(ValueError, match="peak_local_max"):
                U().peak_local_max(img, device=dev, **kw)


# ----------------------------------------------------------------------------- peak_local_max

def same_table(got, want):
    return list(got) == ["coords", "values", "labels"] and all(
        isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got.values(), want))


@pytest.mark.parametrize("name", sorted(PEAKS))
def test_peaks_equal_the_definition(name):
    img, kw = PEAKS[name]
    keep = img.copy()
    want = C.brute_peaks(img, **kw)
    assert same_table(U().peak_local_max(img, return_table=True, **kw), want)
    coords = U().peak_local_max(img, **kw)
    assert coords.dtype == np.int64 and np.array_equal(coords, want[0]) and np.array_equal(img, keep, equal_nan=True)


def test_peak_cases_are_what_they_say():
    run = lambda name: U().peak_local_max(PEAKS[name][0], **PEAKS[name][1]).tolist()
    assert run("constant") == [] and run("constant_low_threshold") == [[0, 0]]
    assert run("ramp") == [] and run("ramp_no_border") == [[17, 66]] and run("all_nan") == [] and run("border_half") == []
    assert run("value_equals_threshold") == [[5, 5]] and run("signed_zeros") == [[4, 10], [7, 63]]
    assert run("labels_touching") == [[10, 31], [10, 30]] and run("num_peaks_0") == [] and run("labels_per_label_0") == []
    assert run("abs_and_rel_abs_wins") == [[5, 5], [10, 70]] and run("abs_and_rel_rel_wins") == [[5, 5], [10, 70]]
    assert run("rel_equals_value") == [[5, 5]] and run("inf")[:2] == [[5, 5], [15, 64]] and run("inf_rel") == []
    for d in (1, 2, 5):
        for where in ("inside", "x_edge", "y_edge", "corner", "anti", "z_edge", "zy"):
            assert len(run("pair_d%d_gap%d_%s" % (d, d, where))) == 1 and len(run("pair_d%d_gap%d_%s" % (d, d + 1, where))) == 2
    t = U().peak_local_max(PEAKS["labels_sparse_ids"][0], return_table=True, **PEAKS["labels_sparse_ids"][1])
    assert set(t["labels"].tolist()) == {1, 5, 12, 70000, 2 ** 31 - 1} and t["labels"].dtype == np.int32
    t = U().peak_local_max(PEAKS["labels_per_label"][0], return_table=True, **PEAKS["labels_per_label"][1])
    assert np.bincount(np.unique(t["labels"], return_inverse=True)[1]).max() == 2 and (np.diff(t["values"]) < 0).all()
    assert 5 not in U().peak_local_max(PEAKS["labels_below_threshold"][0], return_table=True, **PEAKS["labels_below_threshold"][1])["labels"]


def test_peaks_equal_scikit_image_where_it_is_well_defined():
    g = np.load(os.path.join(ROOT, "tests", "golden", "peaks_reference.npz"))
    assert str(g["skimage_version"]) == "0.18.3"
    cases = json.loads(str(g["cases"]))
    assert len(cases) >= 3 * 3 * 5 + 1 + 4
    for i, c in enumerate(cases):
        kw = {k: tuple(v) if isinstance(v, list) else v for k, v in c["keywords"].items()}
        got = U().peak_local_max(g[c["image"]], labels=None if c["labels"] is None else g[c["labels"]], **kw)
        want = g["coords_%d" % i]
        if c["compare"] == "order":
            assert got.shape == want.shape and np.array_equal(got, want), (i, c)
        else:
            assert sorted(map(tuple, got)) == sorted(map(tuple, want)), (i, c)


def test_detect_spots_is_the_composition():
    img, lab = C.scene((96, 120), np.uint16, seed=2, spots=25)
    kw = dict(min_distance=2, threshold_rel=0.2)
    want = U().peak_local_max(U().difference_of_gaussians(img, 1.5, 1.5 * 1.6), return_table=True, **kw)
    assert len(want["coords"]) > 10 and want["values"].dtype == np.float32
    assert same_table(U().detect_spots(img, 1.5, return_table=True, **kw), list(want.values()))
    ratio = U().detect_spots(img, (1.0, 2.0), sigma_ratio=2.0, labels=lab, **kw)
    assert np.array_equal(ratio, U().peak_local_max(U().difference_of_gaussians(img, (1.0, 2.0), (2.0, 4.0)), labels=lab, **kw))


# ----------------------------------------------------------------------------- measure_labels(spots=)

@pytest.mark.parametrize("name", ("blobs_2d", "blobs_3d", "huge_ids", "all_background"))
def test_measure_labels_spot_count(name):
    import torch
    lab = LC.SMALL[name]
    rng = np.random.RandomState(9)
    coords = np.stack([rng.randint(0, n, 300) for n in lab.shape], axis=1)
    coords = np.concatenate([coords, coords[:40], np.argwhere(lab == 0)[:7]])          # duplicates count twice, background for nobody
    before = U().measure_labels(lab, neighbors=1)
    t = U().measure_labels(lab, neighbors=1, spots=coords)
    assert list(t) == list(before) + ["spot_count"] and t["spot_count"].dtype == np.int64
    assert all(np.array_equal(t[k], before[k]) and t[k].dtype == before[k].dtype for k in before)
    want = [sum(1 for c in coords if lab[tuple(c)] == i) for i in t["label"]]
    assert t["spot_count"].tolist() == want and (name == "all_background" or max(want) > 1)
    assert t["spot_count"].sum() == (lab[tuple(coords.T)] > 0).sum()
    for other in (coords.astype(np.int32), coords.tolist(), torch.from_numpy(coords)):
        assert U().measure_labels(lab, spots=other)["spot_count"].tolist() == want
    m = U().measure_labels(torch.from_numpy(lab.copy()), spots=coords, as_tensors=True)
    assert isinstance(m["spot_count"], torch.Tensor) and m["spot_count"].tolist() == want
    assert U().measure_labels(lab, spots=np.zeros((0, lab.ndim), np.int64))["spot_count"].tolist() == [0] * len(want)
    assert "spot_count" not in U().measure_labels(lab) and list(U().measure_labels(lab, neighbors=1)) == list(before)
    for bad in (coords[:, :1], coords.astype(np.float64), coords.reshape(-1)):
        with pytest.raises(ValueError, match="spots"):
            U().measure_labels(lab, spots=bad)
    for axis in range(lab.ndim):
        for value in (-1, lab.shape[axis]):
            outside = coords.copy()
            outside[3, axis] = value
            with pytest.raises(ValueError, match="outside the image"):
                U().measure_labels(lab, spots=outside)


# ----------------------------------------------------------------------------- the device pass's rules on the host

_CODE = {"uint8": 0, "uint16": 1, "float32": 2}


def records():
    """[bytes] as spots_check.cpp reads them: every Gaussian case and every peak case with the host route's result"""
    from stardist_amd import spots
    recs = []
    for _, img, sigma, truncate in GAUSS + [("", a, (1.0, 2.5), 4.0) for a in C.special_float_images().values()]:
        nd = img.ndim
        plan = spots._gaussian_plan(spots._sigmas(sigma, nd, "test"), truncate)
        radius = [-1, -1, -1]
        for ax, r, _ in plan:
            radius[ax + 3 - nd] = r
        head = struct.pack("<2i3q3i", 0, _CODE[img.dtype.name], *((1,) * (3 - nd) + img.shape), *radius)
        want = U().gaussian_filter(img, sigma, truncate=truncate)
        recs.append(head + b"".join(w.tobytes() for _, _, w in plan) + np.ascontiguousarray(img).tobytes() + want.tobytes())
    for name in sorted(PEAKS):
        img, kw = PEAKS[name]
        nd, lab = img.ndim, kw.get("labels")
        d, b, t_abs, t_rel, num_peaks, per_label = spots._peak_args(img.shape, kw.get("min_distance", 1), kw.get("threshold_abs"),
                                                                    kw.get("threshold_rel"), kw.get("exclude_border", True),
                                                                    kw.get("num_peaks"), kw.get("num_peaks_per_label"))
        pad = (0,) * (3 - nd)
        coords = U().peak_local_max(img, **kw)
        index = np.ravel_multi_index(tuple(coords.T), img.shape).astype(np.int64) if len(coords) else np.zeros(0, np.int64)
        head = struct.pack("<2i3q6i6q2d", 1, _CODE[img.dtype.name], *((1,) * (3 - nd) + img.shape), *(pad + d), int(lab is not None),
                           int(t_abs is not None), int(t_rel is not None), *(pad + b), -1 if per_label is None else per_label,
                           -1 if num_peaks is None else num_peaks, len(index), t_abs or 0.0, t_rel or 0.0)
        recs.append(head + np.ascontiguousarray(img).tobytes() + (b"" if lab is None else np.ascontiguousarray(lab, np.int32).tobytes())
                    + index.tobytes())
    return recs


@pytest.fixture(scope="module")
def records_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("spots") / "records.bin")
    recs = records()
    with open(path, "wb") as f:
        f.write(b"".join(recs))
    return path, len(recs)


def test_harness_equals_host_route(records_file, tmp_path):
    path, n = records_file
    exe = str(tmp_path / "spots_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", SRC, "-o", exe], check=True)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert n > 150 and "%d records, 0 bad" % n in r.stdout
    assert int(r.stdout.split(",")[-1].split()[0]) > 100000                 # and it went over the pixels


def test_stand_alone_sanitizer_build_passes_every_case(records_file, tmp_path):
    path, n = records_file
    exe = str(tmp_path / "spots_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC,
                    "-o", exe], check=True)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d records, 0 bad" % n in r.stdout


def test_harness_notices_a_wrong_result(records_file, tmp_path):
    path, n = records_file
    exe, broken = str(tmp_path / "spots_check"), str(tmp_path / "broken.bin")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", SRC, "-o", exe], check=True)
    data = bytearray(open(path, "rb").read())
    first = len(records()[0])
    data[first - 4] ^= 1                                                    # the last float of the first Gaussian record, one ulp off
    data[-8] ^= 1                                                           # the last index of the last peak record
    open(broken, "wb").write(bytes(data))
    r = subprocess.run([exe, broken], capture_output=True, text=True)
    assert r.returncode == 1 and "%d records, 2 bad" % n in r.stdout
