"""CPU: stardist_amd.utils.point_neighbors and measure_labels(nearest=, within=, spacing=) on host input -- against the O(n m) numpy
statement of the definition (tests/_point_neighbors_cases.py), on the cases without ties also against scipy's cKDTree itself -- and the
per-query rules of the device pass (csrc/point_neighbors.h through tests/host/point_neighbors_check.cpp: the grid, the ring walk, the
bound that ends it) against the host route, as a stand-alone program built plain and under the address and undefined-behaviour
sanitizers, with automatic and explicit cell sizes.  All comparisons are exact."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _label_contacts_cases as LC
import _point_neighbors_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "point_neighbors_check.cpp")


def U():
    from stardist_amd import utils
    return utils


def run(name, k, radius, count_only, **more):
    c = C.CASES[name]
    return U().point_neighbors(c["points"], k, radius, queries=c["queries"], spacing=c["spacing"], count_only=count_only, **more)


def assert_same(got, want, names=None):
    names = names or [n for n in want if n != "d2"]
    assert list(got) == names
    for n in names:
        assert isinstance(got[n], np.ndarray) and got[n].dtype == want[n].dtype and got[n].shape == want[n].shape, n
        assert got[n].tobytes() == want[n].tobytes(), n                     # bit for bit: -1 / inf pads, distances


def test_the_name_is_public():
    import stardist_amd
    from stardist_amd import label_ops, utils
    assert utils.point_neighbors is label_ops.point_neighbors and not hasattr(stardist_amd, "point_neighbors")


@pytest.mark.parametrize("call", C.calls(), ids=C.call_id)
def test_host_equals_brute_force(call):
    got = run(*call)
    want = C.expected(*call)
    assert_same(got, want)
    assert all(v.dtype in (np.int64, np.float64) for v in got.values())


def test_cases_are_what_they_say():
    t = run("two_2d", 3, None, False)
    assert t["indices"].tolist() == [[1, -1, -1], [0, -1, -1]] and t["distances"][0].tolist() == [np.sqrt(5.0), np.inf, np.inf]
    assert run("one_3d", 1, None, False)["indices"].tolist() == [[-1]] and run("empty_2d", 2, 1.0, False)["indices"].shape == (0, 2)
    assert run("empty_3d", None, 1.0, False)["offsets"].tolist() == [0]
    # every rank of a lattice is a tie, resolved by the index; radii equal to a distance include it
    t = run("lattice_2d", 8, None, False)
    assert t["indices"][41].tolist() == [1, 40, 42, 81, 0, 2, 80, 82] and t["distances"][41].tolist() == [1.0] * 4 + [np.sqrt(2.0)] * 4
    assert run("lattice_2d", None, 1, True)["counts"][41] == 4 and run("lattice_2d", None, float(np.sqrt(np.float64(2))), True)["counts"][41] == 8
    assert run("lattice_2d", None, 5, True)["counts"][20 * 40 + 20] == 80     # (3, 4) and (5, 0) lie on the circle
    # only the own index is left out: the four copies of a point come first, at distance 0
    t = run("five_fold", 8, None, False)
    assert (t["distances"][:, :4] == 0).all() and (t["distances"][:, 4] > 0).all()
    assert (run("five_fold", None, 0, True)["counts"] == 4).all() and (run("identical", None, 0, True)["counts"] == 499).all()
    assert run("identical", 8, None, False)["indices"][3].tolist() == [0, 1, 2, 4, 5, 6, 7, 8]
    assert not run("random_2d", None, 1e-9, True)["counts"].any() and (run("all_within", None, 2.0, True)["counts"] == 699).all()
    # one ulp decides, and the radius test is on d2
    t = run("one_ulp", 2, None, False)
    assert t["indices"][0].tolist() == [1, 2] and t["distances"][0, 0] < t["distances"][0, 1]
    assert np.diff(run("one_ulp", None, 0.7, False)["offsets"]).tolist() == [1, 1, 0]
    # queries that are the points: no index is left out, the point itself comes first
    t = run("queries_are_the_points", 3, None, False)
    assert (t["indices"][:, 0] == np.arange(1200)).all() and (t["distances"][:, 0] == 0).all()
    assert (run("queries_are_the_points", None, 0, True)["counts"] == 1).all()
    assert run("no_queries", 3, None, False)["indices"].shape == (0, 3) and run("no_queries", None, 5.0, False)["offsets"].tolist() == [0]
    # the spacing is applied: the unscaled answer is another
    c = C.CASES["random_3d_spacing"]
    plain = U().point_neighbors(c["points"], 8)
    assert (plain["indices"] != run("random_3d_spacing", 8, None, False)["indices"]).mean() > 0.3


@pytest.mark.parametrize("name", C.TIE_FREE)
def test_host_equals_ckdtree_where_nothing_ties(name):
    from scipy.spatial import cKDTree
    c = C.CASES[name]
    P = C.scaled(c["points"], c["spacing"])
    Q = P if c["queries"] is None else C.scaled(c["queries"], c["spacing"])
    own = c["queries"] is None
    tree = cKDTree(P)
    for k, radius, count_only in c["calls"]:
        got = run(name, k, radius, count_only)
        if k is not None and radius is None:
            d, i = tree.query(Q, k=k + own)
            d, i = d.reshape(len(Q), -1)[:, own:own + k], i.reshape(len(Q), -1)[:, own:own + k]
            w = d.shape[1]
            assert np.array_equal(got["indices"][:, :w], np.where(np.isfinite(d), i, -1)) and np.array_equal(got["distances"][:, :w], d)
        elif k is None:
            lists = tree.query_ball_point(Q, radius)
            lists = [sorted(j for j in l if not (own and j == i)) for i, l in enumerate(lists)]
            if count_only:
                assert got["counts"].tolist() == [len(l) for l in lists]
            else:
                assert got["indices"].tolist() == [j for l in lists for j in l] and np.diff(got["offsets"]).tolist() == [len(l) for l in lists]


@pytest.mark.parametrize("name", C.LATTICES)
def test_sorted_distances_equal_ckdtree_on_lattices(name):
    from scipy.spatial import cKDTree
    c = C.CASES[name]
    P = C.scaled(c["points"], c["spacing"])
    for k in (3, 8):
        d = cKDTree(P).query(P, k=k + 1)[0][:, 1:]
        assert np.array_equal(U().point_neighbors(c["points"], k, spacing=c["spacing"])["distances"], d)


def test_inputs_of_other_kinds_and_as_tensors(monkeypatch):
    import torch
    from stardist_amd import label_ops
    monkeypatch.setattr(label_ops, "_point_neighbors_device", lambda *a, **k: pytest.fail("device path taken"))
    c = C.CASES["lattice_2d"]
    want = C.expected("lattice_2d", 8, None, False)
    for pts in (c["points"].tolist(), c["points"].astype(np.int32), c["points"].astype(np.float32), torch.from_numpy(c["points"])):
        assert_same(U().point_neighbors(pts, 8), want)
    got = U().point_neighbors(torch.from_numpy(c["points"]), radius=1, as_tensors=True)
    want = C.expected("lattice_2d", None, 1, False)
    assert list(got) == ["offsets", "indices", "distances"]
    assert all(isinstance(v, torch.Tensor) and v.device.type == "cpu" and v.numpy().tobytes() == want[n].tobytes() for n, v in got.items())
    got = U().point_neighbors(c["points"], radius=1, count_only=True, as_tensors=True)
    assert got["counts"].dtype == torch.int64 and got["counts"].tolist() == C.expected("lattice_2d", None, 1, True)["counts"].tolist()
    f32 = np.random.RandomState(3).rand(200, 3).astype(np.float32)          # float32 is widened exactly
    assert_same(U().point_neighbors(f32, 4), U().point_neighbors(f32.astype(np.float64), 4), ["indices", "distances"])


@pytest.mark.parametrize("dev", (None, "cuda"))
def test_bad_arguments_raise_before_anything_runs(dev, monkeypatch):
    from stardist_amd import label_ops
    monkeypatch.setattr(label_ops, "_point_neighbors_device", lambda *a, **k: pytest.fail("device path taken"))
    monkeypatch.setattr(label_ops.N, "require_device", lambda: pytest.fail("the device was asked for"))
    for points, kw in C.ERRORS:
        with pytest.raises(ValueError, match="point_neighbors"):
            U().point_neighbors(points, device=dev, **kw)


def test_device_route_gets_scaled_points_and_results_come_back(monkeypatch):
    import torch
    from stardist_amd import label_ops
    seen = []

    def fake(P, Q, mode, k, r2, cell_size=0.0, cell=None):
        seen.append((mode, k, r2, None if Q is None else tuple(Q.shape)))
        s = C.d2_matrix(P.numpy(), None if Q is None else Q.numpy())
        b = C.brute(s, k, None if r2 is None else np.sqrt(r2), mode == 1)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        return t(b["counts"]) if mode == 1 else (t(b["indices"]), t(b["d2"])) if mode == 0 else (t(b["offsets"]), t(b["indices"]), t(b["d2"]))
    monkeypatch.setattr(label_ops, "_point_neighbors_device", fake)
    monkeypatch.setattr(label_ops.N, "require_device", lambda: None)
    monkeypatch.setattr(label_ops.R, "to_device_tensor", lambda x, device=None: torch.as_tensor(np.ascontiguousarray(x)))
    c = C.CASES["spots_and_nuclei"]
    for k, radius, count_only in ((2, None, False), (None, 4.0, False), (None, 4.0, True), (2, 4.0, False)):
        got = U().point_neighbors(c["points"], k, radius, queries=c["queries"], spacing=c["spacing"], count_only=count_only, device="cuda")
        assert_same(got, C.expected("spots_and_nuclei", k, radius, count_only))
    assert seen == [(0, 2, None, (900, 3)), (2, None, 16.0, (900, 3)), (1, None, 16.0, (900, 3)), (0, 2, 16.0, (900, 3))]
    got = U().point_neighbors(c["points"], 2, spacing=c["spacing"], device="cuda", as_tensors=True)
    assert seen[-1] == (0, 2, None, None) and all(isinstance(v, torch.Tensor) for v in got.values())
    n = len(seen)
    U().point_neighbors(c["points"], 2)                                      # no device=: the host code
    assert len(seen) == n


# ----------------------------------------------------------------------------- measure_labels(nearest=, within=, spacing=)

# the columns of a call without the new keywords, as they were before the keywords existed
PLAIN_2D = ["label", "area", "bbox-0", "bbox-1", "bbox-2", "bbox-3", "centroid-0", "centroid-1"]
PLAIN_3D = ["label", "area", "bbox-0", "bbox-1", "bbox-2", "bbox-3", "bbox-4", "bbox-5", "centroid-0", "centroid-1", "centroid-2"]
WITH_NEIGHBORS = ["neighbors", "contact_objects", "contact_background"]


def test_measure_labels_without_the_keywords_is_what_it_was():
    assert list(U().measure_labels(LC.SMALL["blobs_2d"])) == PLAIN_2D
    assert list(U().measure_labels(LC.SMALL["blobs_3d"])) == PLAIN_3D
    assert list(U().measure_labels(LC.SMALL["blobs_2d"], neighbors=1)) == PLAIN_2D + WITH_NEIGHBORS
    img = np.random.RandomState(0).randint(0, 200, LC.SMALL["blobs_2d"].shape).astype(np.uint8)
    assert list(U().measure_labels(LC.SMALL["blobs_2d"], img, percentiles=(50,), hull=True, neighbors=2)) == PLAIN_2D + [
        "sum_intensity", "mean_intensity", "min_intensity", "max_intensity", "std_intensity", "p50_intensity", "convex_area", "solidity",
        "feret_diameter_max"] + WITH_NEIGHBORS


@pytest.mark.parametrize("name", ("blobs_2d", "blobs_3d", "noise_2d", "noise_3d", "one_label", "all_background", "huge_ids"))
def test_measure_labels_nearest_and_within(name):
    a = LC.SMALL[name]
    nd = a.ndim
    before = U().measure_labels(a, neighbors=1)
    spacing = (2.0, 0.7, 0.7)[3 - nd:]
    for sp in (1, spacing):
        t = U().measure_labels(a, neighbors=1, nearest=3, within=6.5, spacing=sp)
        names = ["nearest_label-0", "nearest_distance-0", "nearest_label-1", "nearest_distance-1", "nearest_label-2", "nearest_distance-2",
                 "neighbors_within"]
        assert list(t) == list(before) + names                              # after all existing columns, the neighbors ones included
        for key in before:
            assert t[key].dtype == before[key].dtype and np.array_equal(t[key], before[key])
        cent = np.stack([t["centroid-%d" % d] for d in range(nd)], axis=1)
        near = U().point_neighbors(cent, 3, spacing=sp)
        for j in range(3):
            lab = np.where(near["indices"][:, j] >= 0, t["label"][np.maximum(near["indices"][:, j], 0)] if len(cent) else 0, 0)
            assert t["nearest_label-%d" % j].dtype == np.int64 and np.array_equal(t["nearest_label-%d" % j], lab)
            assert t["nearest_distance-%d" % j].dtype == np.float64
            assert t["nearest_distance-%d" % j].tobytes() == np.ascontiguousarray(near["distances"][:, j]).tobytes()
        counts = U().point_neighbors(cent, radius=6.5, spacing=sp, count_only=True)["counts"]
        assert t["neighbors_within"].dtype == np.int64 and np.array_equal(t["neighbors_within"], counts)
    one = U().measure_labels(a, nearest=1)
    assert list(one) == [k for k in before if k not in WITH_NEIGHBORS] + ["nearest_label-0", "nearest_distance-0"]
    assert list(U().measure_labels(a, within=3))[-1] == "neighbors_within"


def test_measure_labels_nearest_is_not_trivial_and_checks_its_arguments():
    import torch
    a = LC.SMALL["blobs_2d"]
    t = U().measure_labels(a, nearest=2, within=12.0)
    assert len(t["label"]) > 5 and (t["nearest_label-0"] > 0).all() and (t["nearest_label-0"] != t["label"]).all()
    assert (t["nearest_distance-0"] <= t["nearest_distance-1"]).all() and t["neighbors_within"].max() > 0
    scaled = U().measure_labels(a, nearest=2, spacing=(5.0, 0.2))
    assert (scaled["nearest_label-0"] != t["nearest_label-0"]).any()        # the spacing is applied
    assert np.array_equal(scaled["centroid-0"], t["centroid-0"])            # and to the new columns only
    m = U().measure_labels(torch.from_numpy(a.copy()), nearest=2, within=12.0, as_tensors=True)
    assert list(m) == list(t) and all(isinstance(m[k], torch.Tensor) and m[k].numpy().tobytes() == t[k].tobytes() for k in t)
    one = U().measure_labels(LC.SMALL["one_label"], nearest=2, within=3)
    assert one["nearest_label-0"].tolist() == [0] and one["nearest_distance-1"].tolist() == [np.inf] and one["neighbors_within"].tolist() == [0]
    for bad in (0, 65, 1.0, True, "1"):
        with pytest.raises(ValueError, match="nearest"):
            U().measure_labels(a, nearest=bad)
    for bad in (-1, np.inf, np.nan, "3"):
        with pytest.raises(ValueError, match="within"):
            U().measure_labels(a, within=bad)
    for bad in (2.0, (1, 1)):
        with pytest.raises(ValueError, match="spacing"):
            U().measure_labels(a, spacing=bad)
    for bad in (0, (1, 2, 3), np.inf):
        with pytest.raises(ValueError, match="spacing"):
            U().measure_labels(a, nearest=1, spacing=bad)


# ----------------------------------------------------------------------------- the device pass's rules on the host

def records():
    """[(head, arrays)] as point_neighbors_check.cpp reads them: every case and call, with the host route's squared distances, for the
    automatic cell size and the case's own"""
    from stardist_amd.label_ops import _nearest_host, _within_host
    recs = []
    for name, c in C.CASES.items():
        P = np.ascontiguousarray(C.scaled(c["points"], c["spacing"]))
        own = c["queries"] is None
        Q = P if own else np.ascontiguousarray(C.scaled(c["queries"], c["spacing"]))
        for k, radius, count_only in c["calls"]:
            r2 = None if radius is None else float(np.float64(radius) * np.float64(radius))
            if k is not None:
                mode, total, out = 0, 0, list(_nearest_host(P, Q, own, k, r2))
            elif count_only:
                mode, total, out = 1, 0, [_within_host(P, Q, own, float(radius), r2, True)[0]]
            else:
                counts, idx, d2 = _within_host(P, Q, own, float(radius), r2, False)
                mode, total, out = 2, len(idx), [np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), idx, d2]
            for cell in (0.0,) + c["cell_sizes"]:
                head = struct.pack("<5i3q2d", P.shape[1], mode, k or 0, int(r2 is not None), int(own), len(P), len(Q), total, r2 or 0.0, cell)
                recs.append((head, [P] + ([] if own else [Q]) + out))
    return recs


@pytest.fixture(scope="module")
def records_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("point_neighbors") / "records.bin")
    recs = records()
    with open(path, "wb") as f:
        for head, arrays in recs:
            f.write(head)
            for a in arrays:
                assert a.dtype in (np.int64, np.float64)
                f.write(np.ascontiguousarray(a).tobytes())
    return path, len(recs)


def test_harness_equals_host_route(records_file, tmp_path):
    path, n = records_file
    exe = str(tmp_path / "point_neighbors_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", SRC, "-o", exe], check=True)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert n > 150 and "%d records, 0 bad" % n in r.stdout
    assert int(r.stdout.split(",")[-1].split()[0]) > 10000                  # and the searches walked rings


def test_stand_alone_sanitizer_build_passes_every_case(records_file, tmp_path):
    path, n = records_file
    exe = str(tmp_path / "point_neighbors_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC,
                    "-o", exe], check=True)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d records, 0 bad" % n in r.stdout


def test_harness_notices_a_wrong_distance(records_file, tmp_path):
    path, n = records_file
    exe, broken = str(tmp_path / "point_neighbors_check"), str(tmp_path / "broken.bin")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", SRC, "-o", exe], check=True)
    data = bytearray(open(path, "rb").read())
    data[-8] ^= 1                                                           # the last d2 of the last record, one ulp off
    open(broken, "wb").write(bytes(data))
    r = subprocess.run([exe, broken], capture_output=True, text=True)
    assert r.returncode == 1 and "%d records, 1 bad" % n in r.stdout


def test_ring_bound_is_below_what_a_cell_distance_guarantees():
    """the bound of csrc/point_neighbors.h in exact arithmetic: for R cells, ((R - 2^-20) h)^2 (1 - 2^-50) rounded three times stays below
    ((R - 2^-29) h)^2 (1 - 2^-52)^2, the least computed d2 of a pair more than R cells apart"""
    from fractions import Fraction as F
    for h in (0.65, 1.0, 3.7e-5, 2.0 ** -499 * 1.3, 1.9 * 2.0 ** 478):
        for R in (1, 2, 3, 1000, 2 ** 21 - 1, 2 ** 21):
            e = np.float64(R - 2.0 ** -20) * np.float64(h)
            lb = (e * e) * np.float64(1.0 - 2.0 ** -50)
            assert (R - 2.0 ** -20) == F(R) - F(1, 2 ** 20)                 # exact in float64
            least = ((F(R) - F(1, 2 ** 29)) * F(float(h))) ** 2 * (1 - F(1, 2 ** 52)) ** 2
            assert 0 < F(float(lb)) < least
