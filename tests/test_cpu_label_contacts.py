"""CPU: stardist_amd.utils.label_contacts and measure_labels(neighbors=) on host input -- against a brute-force statement of the
definition (tests/_label_contacts_cases.py: loops over pixels and offsets), exhaustively over all 3^9 3 x 3 windows and all 3^8
2 x 2 x 2 windows of three values, the pairs against the edge sets of scikit-image 0.18.3's future.graph.RAG
(tests/golden/label_contacts_reference.npz) -- and the per-pixel and per-wave rules of the device pass (csrc/label_contacts.h through
tests/host/label_contacts_check.cpp: tiles with their halo, forward offsets, runs of equal keys among 64 lanes) against the host route,
as a stand-alone program built plain and under the address and undefined-behaviour sanitizers.  All comparisons are exact."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _label_contacts_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "label_contacts_check.cpp")
NEIGHBOR_NAMES = ("neighbors", "contact_objects", "contact_background")


def U():
    from stardist_amd import utils
    return utils


def connectivities(a):
    return range(1, a.ndim + 1)


def test_the_name_is_public():
    import stardist_amd
    from stardist_amd import label_ops, utils
    assert utils.label_contacts is label_ops.label_contacts and not hasattr(stardist_amd, "label_contacts")


def test_forward_offsets_are_half_of_scipy_s_structure():
    from scipy.ndimage import generate_binary_structure
    from stardist_amd.label_ops import _forward_offsets
    for nd, sizes in ((2, (2, 4)), (3, (3, 9, 13))):
        for c, n in zip(range(1, nd + 1), sizes):
            offs = _forward_offsets(nd, c)
            assert offs == C.forward_offsets(nd, c) and len(offs) == n == (generate_binary_structure(nd, c).sum() - 1) // 2
            both = set(offs) | {tuple(-v for v in o) for o in offs}
            assert both == {tuple(int(v) - 1 for v in p) for p in np.argwhere(generate_binary_structure(nd, c))} - {(0,) * nd}


@pytest.mark.parametrize("name", sorted(C.SMALL))
def test_host_equals_brute_force(name):
    a = C.SMALL[name]
    for c in connectivities(a):
        for background in (False, True):
            got = U().label_contacts(a, c, background=background)
            assert list(got) == ["label_a", "label_b", "contacts"]
            assert all(isinstance(v, np.ndarray) and v.dtype == np.int64 and v.ndim == 1 for v in got.values())
            assert C.as_lists(got) == C.brute(a, c, background), (c, background)


def test_cases_are_what_they_say():
    t = U().label_contacts(C.SMALL["two_halves"], 1)
    assert C.as_lists(t) == ([1], [2], [4])
    assert C.as_lists(U().label_contacts(C.SMALL["two_halves"], 2)) == ([1], [2], [4 + 2 * 3])
    for name in ("diagonal_only", "anti_diagonal_only"):                    # objects that touch at a corner only
        assert C.as_lists(U().label_contacts(C.SMALL[name], 1)) == ([], [], [])
        assert C.as_lists(U().label_contacts(C.SMALL[name], 2)) == ([1], [2], [1])
        assert C.as_lists(U().label_contacts(C.SMALL[name], 1, background=True)) == ([0, 0], [1, 2], [2, 2])
    for name in ("one_label", "all_background", "one_pixel"):               # the image edge is no contact
        assert C.as_lists(U().label_contacts(C.SMALL[name], 2, background=True)) == ([], [], [])
    assert C.as_lists(U().label_contacts(C.SMALL["one_row"], 2)) == ([2], [3], [1])
    assert C.as_lists(U().label_contacts(C.SMALL["wide_ids"], 1)) == ([1, 1, 2 ** 30], [2 ** 30, 2 ** 31 - 1, 2 ** 31 - 1], [2, 2, 1])
    assert C.as_lists(U().label_contacts(C.SMALL["huge_ids"], 1)) == ([3, 3], [10 ** 12, 10 ** 15], [3, 2])
    assert C.as_lists(U().label_contacts(C.SMALL["ring"], 2)) == ([1], [2], [8 + 4 * 3])
    assert C.as_lists(U().label_contacts(C.SMALL["far_corner_diagonals"], 2)) == ([1], [2], [1])
    assert C.as_lists(U().label_contacts(C.SMALL["bool_mask"], 1, background=True))[:2] == ([0], [1])
    assert C.as_lists(U().label_contacts(C.balls(), 1))[:2] == ([1, 2, 3, 4], [2, 3, 4, 5])


@pytest.mark.parametrize("nd", (2, 3))
def test_host_equals_brute_force_around_the_tile_extents(nd):
    for shape in C.tile_shapes(nd):
        for kind in C.KINDS:
            a = C.tiled(kind, shape)
            for c in connectivities(a):
                assert C.as_lists(U().label_contacts(a, c, background=True)) == C.brute(a, c, True), (kind, shape, c)
                assert C.as_lists(U().label_contacts(a, c)) == C.brute(a, c, False), (kind, shape, c)


@pytest.mark.parametrize("which", ("windows_2d", "windows_3d", "balls"))
def test_host_equals_brute_force_on_all_small_windows(which):
    a = getattr(C, which)()
    if which == "windows_2d":                                               # every window is there, at its place
        assert a.shape == (729, 243) and [a[3 * 5 + k // 3, 3 * 7 + k % 3] for k in range(9)] == [((5 * 81 + 7) // 3 ** k) % 3 for k in range(9)]
    if which == "windows_3d":
        assert a.shape == (2, 162, 162) and len({a[:, 2 * i:2 * i + 2, 2 * j:2 * j + 2].tobytes() for i in range(81) for j in range(81)}) == 3 ** 8
    for c in connectivities(a):
        for background in (False, True):
            assert C.as_lists(U().label_contacts(a, c, background=background)) == C.brute(a, c, background)


@pytest.mark.parametrize("name", C.GOLDEN)
def test_pairs_equal_scikit_image_s_rag_edges(name):
    golden = np.load(os.path.join(ROOT, "tests", "golden", "label_contacts_reference.npz"))
    a = C.SMALL[name]
    assert np.array_equal(golden["%s/img" % name], a) and golden["%s/img" % name].dtype == a.dtype
    for c in connectivities(a):
        t = U().label_contacts(a, c, background=True)
        assert np.array_equal(np.stack([t["label_a"], t["label_b"]], axis=1), golden["%s/c%d" % (name, c)]), c


def test_golden_file_is_not_trivial():
    golden = np.load(os.path.join(ROOT, "tests", "golden", "label_contacts_reference.npz"))
    edges = [golden[k] for k in golden.files if "/c" in k]
    assert len(C.GOLDEN) >= 12 and len(edges) == sum(C.SMALL[n].ndim for n in C.GOLDEN) and sum(len(e) for e in edges) > 150
    assert len(golden["diagonal_only/c1"]) == 2 and len(golden["diagonal_only/c2"]) == 3
    for c in (1, 2):                                                        # and the counts RAG does not have are there for every edge
        t = U().label_contacts(C.SMALL["diagonal_only"], c, background=True)
        assert len(t["contacts"]) == len(golden["diagonal_only/c%d" % c]) and (t["contacts"] > 0).all()


@pytest.mark.parametrize("name", ("blobs_2d", "blobs_3d", "noise_3d", "one_row", "all_background", "huge_ids", "bool_mask"))
def test_symmetric_and_offsets(name):
    a = C.SMALL[name]
    for c in connectivities(a):
        for background in (False, True):
            plain = C.as_lists(U().label_contacts(a, c, background=background))
            s = U().label_contacts(a, c, background=background, symmetric=True)
            assert list(s) == ["label_a", "label_b", "contacts", "offsets"] and all(v.dtype == np.int64 for v in s.values())
            rows = sorted([(x, y, n) for x, y, n in zip(*plain)] + [(y, x, n) for x, y, n in zip(*plain)])
            assert list(zip(*C.as_lists(s))) == rows
            present = [int(v) for v in np.unique(a) if v > 0]
            off = s["offsets"].tolist()
            assert len(off) == len(present) + 1 and off[-1] == len(rows) and off[0] == sum(1 for r in rows if r[0] == 0)
            for i, l in enumerate(present):                                 # the slice of a label: its rows and no others
                assert [r for r in rows if r[0] == l] == rows[off[i]:off[i + 1]]


@pytest.mark.parametrize("name", ("blobs_2d", "blobs_3d", "noise_2d", "noise_3d", "one_label", "all_background", "huge_ids", "ring"))
def test_measure_labels_neighbor_columns(name):
    a = C.SMALL[name]
    before = U().measure_labels(a)
    for c in connectivities(a):
        t = U().measure_labels(a, neighbors=c)
        assert list(t) == list(before) + list(NEIGHBOR_NAMES)               # after all existing columns
        for k in before:                                                    # and those are what they were, column by column
            assert t[k].dtype == before[k].dtype and np.array_equal(t[k], before[k])
        want = C.brute_neighbors(a, c)
        assert t["label"].tolist() == sorted(want)
        for j, k in enumerate(NEIGHBOR_NAMES):
            assert t[k].dtype == np.int64 and t[k].tolist() == [want[l][j] for l in sorted(want)], (c, k)


def test_measure_labels_neighbors_with_the_other_keywords():
    a = C.SMALL["blobs_2d"]
    img = np.random.RandomState(0).randint(0, 200, a.shape).astype(np.uint8)
    before = U().measure_labels(a, img, shape=True, percentiles=(50,))
    t = U().measure_labels(a, img, shape=True, percentiles=(50,), neighbors=2)
    assert list(t) == list(before) + list(NEIGHBOR_NAMES)
    assert all(np.array_equal(t[k], before[k], equal_nan=t[k].dtype.kind == "f") for k in before)
    want = C.brute_neighbors(a, 2)
    assert t["neighbors"].tolist() == [want[l][0] for l in sorted(want)]
    for bad in (0, 3, 1.0, True, "1"):
        with pytest.raises(ValueError, match="neighbors"):
            U().measure_labels(a, neighbors=bad)
    with pytest.raises(ValueError, match="Negative"):
        U().measure_labels(np.array([[1, -1]], np.int32), neighbors=1)
    assert list(U().measure_labels(np.array([[1, -1]], np.int32))["label"]) == [1]     # without the keyword: as before


def test_as_tensors_arguments_errors_and_routing(monkeypatch):
    import torch
    from stardist_amd import label_ops
    monkeypatch.setattr(label_ops, "_label_contacts_device", lambda *a, **k: pytest.fail("device path taken"))
    a = C.SMALL["blobs_2d"]
    want = U().label_contacts(a, 2, background=True, symmetric=True)
    # a host tensor, a list: the host code, numpy columns; as_tensors: tensors where the labels are
    for x in (torch.from_numpy(a.copy()), a.tolist()):
        got = U().label_contacts(x, 2, background=True, symmetric=True)
        assert all(isinstance(got[k], np.ndarray) and np.array_equal(got[k], want[k]) for k in want)
    got = U().label_contacts(torch.from_numpy(a.copy()), 2, background=True, symmetric=True, as_tensors=True)
    assert list(got) == list(want)
    assert all(isinstance(got[k], torch.Tensor) and got[k].dtype == torch.int64 and got[k].device.type == "cpu" and
               np.array_equal(got[k].numpy(), want[k]) for k in want)
    m = U().measure_labels(torch.from_numpy(a.copy()), neighbors=1, as_tensors=True)
    ref = U().measure_labels(a, neighbors=1)
    assert list(m) == list(ref) and all(isinstance(m[k], torch.Tensor) and np.array_equal(m[k].numpy(), ref[k]) for k in ref)
    for bad in (0, 3, -1, 1.5, "1", True, None):
        with pytest.raises(ValueError, match="connectivity"):
            U().label_contacts(a, bad)
    for dev in (None, "cuda"):
        with pytest.raises(ValueError, match="connectivity"):
            U().label_contacts(a, 3, device=dev)
        with pytest.raises(ValueError, match="2D or 3D"):
            U().label_contacts(np.zeros(5, np.int32), device=dev)
        with pytest.raises(ValueError, match="2D or 3D"):
            U().label_contacts(np.zeros((2, 2, 2, 2), np.int32), device=dev)
        with pytest.raises(ValueError, match="bool or integer"):
            U().label_contacts(np.zeros((3, 3), np.float32), device=dev)
    with pytest.raises(ValueError, match="Negative"):
        U().label_contacts(np.array([[1, -2]], np.int32))
    empty = U().label_contacts(np.zeros((0, 4), np.int32), symmetric=True)
    assert [len(v) for v in empty.values()] == [0, 0, 0, 1] and empty["offsets"].tolist() == [0]


def test_device_route_gets_its_arguments_and_results_come_back_like_measure_labels(monkeypatch):
    import torch
    from stardist_amd import label_ops
    seen = []

    def fake(lbl, connectivity, background, device=None, runs=None):
        seen.append((type(lbl), connectivity, background, device))
        return tuple(torch.as_tensor(np.asarray(v, np.int64)) for v in C.brute(np.asarray(lbl), connectivity, background))
    monkeypatch.setattr(label_ops, "_label_contacts_device", fake)
    a = C.SMALL["blobs_2d"]
    want = U().label_contacts(a, 2, background=True, symmetric=True)        # the host route computed its own
    assert not seen
    monkeypatch.setattr(label_ops, "_labels_present", lambda lbl, on_device, device: torch.as_tensor(np.unique(lbl)[1:].astype(np.int64)))
    got = U().label_contacts(a, 2, background=True, symmetric=True, device="cuda")
    assert seen == [(np.ndarray, 2, True, "cuda")]
    assert all(isinstance(got[k], np.ndarray) and got[k].dtype == np.int64 and np.array_equal(got[k], want[k]) for k in want)
    got = U().label_contacts(a, 1, device="cuda", as_tensors=True)          # the derived columns by torch operations: the same values
    assert seen[-1] == (np.ndarray, 1, False, "cuda") and all(isinstance(v, torch.Tensor) for v in got.values())
    assert C.as_lists({k: v.numpy() for k, v in got.items()}) == C.brute(a, 1, False)
    got = U().label_contacts(a, 2, background=True, symmetric=True, device="cuda", as_tensors=True)
    assert all(np.array_equal(got[k].numpy(), want[k]) for k in want)
    n = len(seen)
    U().label_contacts(a.astype(np.float32).astype(np.int64), 1)            # no device=: the host code
    assert len(seen) == n


def test_neighbor_columns_are_the_same_operations_on_tensors():
    import torch
    from stardist_amd.label_ops import _label_contacts_host, _neighbor_columns
    for name in ("blobs_2d", "noise_3d", "all_background"):
        a = C.SMALL[name]
        label = np.array(sorted(C.brute_neighbors(a, 1)), np.int64)
        table = _label_contacts_host(a, 1, True)
        on_arrays = _neighbor_columns(label, *table)
        on_tensors = _neighbor_columns(torch.from_numpy(label), *[torch.from_numpy(np.ascontiguousarray(v)) for v in table])
        assert all(np.array_equal(x, y.numpy()) for x, y in zip(on_arrays, on_tensors))


# ----------------------------------------------------------------------------- the device pass's rules on the host

def zyx(shape):
    return ((1,) + tuple(shape)) if len(shape) == 2 else tuple(shape)


def records():
    """[(head, tail, arrays)]: the cases as label_contacts_check.cpp reads them, with the host route's tables"""
    images = [a for name, a in sorted(C.SMALL.items()) if name != "huge_ids"]
    images = [a.astype(np.uint8) if a.dtype == np.bool_ else a for a in images]
    for nd in (2, 3):
        images += [C.tiled(kind, shape) for shape in C.tile_shapes(nd) for kind in C.KINDS]
    images += [C.windows_2d(), C.windows_3d(), C.balls(), C.balls()[5:6], stripes()]
    recs = []
    for a in images:
        for c in connectivities(a):
            for background in (0, 1):
                t = U().label_contacts(a, c, background=bool(background))
                recs.append(((a.ndim,) + zyx(a.shape) + (c, background), (len(t["contacts"]), 0),
                             [a.astype(np.int32), (t["label_a"] << 32) | t["label_b"], t["contacts"]]))
    return recs


def stripes():
    """horizontal stripes over three tiles along x: the runs of a wave are combined"""
    return np.repeat(np.arange(1, 8, dtype=np.int32)[:, None], 3 * C.TX + 5, axis=1)


@pytest.fixture(scope="module")
def records_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("label_contacts") / "records.bin")
    recs = records()
    with open(path, "wb") as f:
        for head, tail, arrays in recs:
            f.write(struct.pack("<6i2q", *[int(v) for v in head + tail]))
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
    return path, len(recs)


def test_harness_equals_host_route(records_file, tmp_path):
    path, n = records_file
    exe = str(tmp_path / "label_contacts_check")
    subprocess.run(["g++", "-O2", "-std=c++17", SRC, "-o", exe], check=True)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert n > 400 and "%d records, 0 bad" % n in r.stdout
    assert int(r.stdout.split(",")[-1].split()[0]) > 100                    # and many of them had lanes to combine


def test_stand_alone_sanitizer_build_passes_every_case(records_file, tmp_path):
    path, n = records_file
    exe = str(tmp_path / "label_contacts_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe], check=True)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d records, 0 bad" % n in r.stdout


def test_harness_notices_a_wrong_count(records_file, tmp_path):
    path, n = records_file
    exe, broken = str(tmp_path / "label_contacts_check"), str(tmp_path / "broken.bin")
    subprocess.run(["g++", "-O2", "-std=c++17", SRC, "-o", exe], check=True)
    data = bytearray(open(path, "rb").read())
    data[-8] ^= 1                                                           # the last count of the last record, off by one
    open(broken, "wb").write(bytes(data))
    r = subprocess.run([exe, broken], capture_output=True, text=True)
    assert r.returncode == 1 and "%d records, 1 bad" % n in r.stdout
