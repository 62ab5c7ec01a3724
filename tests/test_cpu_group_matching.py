"""CPU: the host half of the device group_matching_labels (stardist_amd.matching_sparse).  With sparse_overlap standing in for the stack
overlap kernel and lookup_tables for the relabel kernel, the composition of raw-pair matchings (group_tables_from_overlaps) equals the
host group_matching_labels -- and, where the reference sources are at hand, the reference's own function -- array for array, on every
scene of tests/_group_cases.py with iou / iot / iop and thresh 1e-10, 0.3, 0.5, 0.7; matched_pairs_from_overlap returns the pairs that
matching(report_matches=True) marks in matched_tps; the device entry raises the host function's errors before it touches a device."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest

import _group_cases as G

REF = "/root/reference/stardist"
SCENES = G.scenes()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_composition_equals_host_function(name):
    from stardist_amd import matching as M
    ys = SCENES[name]
    before = [np.array(y, copy=True) for y in ys]
    for crit in G.CRITERIA:
        for thr in G.THRESHS:
            h = M.group_matching_labels(ys, thresh=thr, criterion=crit)
            c = G.compose(ys, thr, crit)
            assert c.dtype == h.dtype == np.int32 and c.shape == h.shape
            assert np.array_equal(c, h), (name, crit, thr, int(np.count_nonzero(c != h)))
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(before, ys))


def test_scenes_cover_what_they_claim():
    """splits, merges, gaps, large ids and both input kinds are really in the scenes"""
    from stardist_amd import matching as M
    g = M.group_matching_labels(SCENES["split_merge"])
    assert len(np.unique(g[1][24:52, 39:72])) == 3 and len(np.unique(g[0][25:50, 40:70])) == 1       # background + two parts of one object
    assert len(set(np.unique(g[1][24:52, 39:93])) - {0}) == 3 and len(set(np.unique(g[2][26:49, 41:90])) - {0}) == 1
    bg = SCENES["background"]
    assert bg[2].max() == 0 and bg[-1].max() == 0
    gb = M.group_matching_labels(bg)
    assert gb[3].min() == 0 and np.unique(gb[3])[1] > gb[:2].max()                                   # everything after the gap is new
    assert SCENES["big_ids"].dtype == np.int64 and SCENES["big_ids"].max() > 2 ** 31 - 1 - 200
    assert SCENES["volumes"][0].ndim == 3
    assert isinstance(SCENES["moving0"], np.ndarray) and isinstance(SCENES["moving1"], list)
    assert SCENES["moving_uint16"][0].dtype == np.uint16 and SCENES["moving_int64"].dtype == np.int64
    assert not M.label_are_sequential(SCENES["moving1"][1])


@pytest.mark.parametrize("name", sorted(SCENES))
def test_matched_pairs_equal_the_dense_true_positives(name):
    from stardist_amd import matching as M
    from stardist_amd import matching_sparse as S
    ys = SCENES[name]
    for a, b in zip(ys[:-1], ys[1:]):
        a, b = np.asarray(a), np.asarray(b)
        if a.max() == 0 and b.max() == 0:
            continue
        lst = S.sparse_overlap(a, b)
        for crit in G.CRITERIA:
            for thr in G.THRESHS:
                r = M.matching(a, b, thresh=thr, criterion=crit, report_matches=True)
                dense = {r.matched_pairs[i] for i in r.matched_tps}
                mt, mp = S.matched_pairs_from_overlap(*lst, thr, crit)
                assert len(mt) == len(mp) == r.tp
                assert set(zip(mt.tolist(), mp.tolist())) == dense, (name, crit, thr)
    with pytest.raises(ValueError, match="thresh > 0"):
        S.matched_pairs_from_overlap(*S.sparse_overlap(np.asarray(ys[0]), np.asarray(ys[1])), 0, "iou")
    with pytest.raises(ValueError, match="not supported"):
        S.matched_pairs_from_overlap(*S.sparse_overlap(np.asarray(ys[0]), np.asarray(ys[1])), 0.5, "dice")


def test_tables_have_the_documented_form():
    from stardist_amd import matching_sparse as S
    ys = SCENES["moving1"]
    lists = [S.sparse_overlap(a, b) for a, b in zip(ys[:-1], ys[1:])]
    tables = S.group_tables_from_overlaps(lists, int(ys[0].max()), 0.3, "iou")
    assert len(tables) == len(ys)
    assert np.array_equal(tables[0][0], tables[0][1])                                                # frame 0 keeps its ids
    seen = set(tables[0][1].tolist())
    for y, (ids, new) in zip(ys, tables):
        assert np.array_equal(ids, np.unique(y[y > 0])) and len(set(new.tolist())) == len(new) and new.min() > 0
        fresh = sorted(set(new.tolist()) - seen)
        assert fresh == list(range(max(seen) + 1, max(seen) + 1 + len(fresh)))                     # consecutive free ids
        seen |= set(new.tolist())
    with pytest.raises(ValueError, match="2\\*\\*31"):
        S.group_tables_from_overlaps(lists, 2 ** 31 - 2, 0.3, "iou")


def _ref_matching(monkeypatch):
    stubs = {"numba": types.ModuleType("numba"), "skimage": types.ModuleType("skimage"), "skimage.measure": types.ModuleType("skimage.measure"),
             "csbdeep": types.ModuleType("csbdeep"), "csbdeep.utils": types.ModuleType("csbdeep.utils")}
    stubs["numba"].jit = lambda *a, **k: (lambda f: f)

    def regionprops(y):                                                # the two attributes the reference reads: .label, .slice (ascending labels)
        from scipy.ndimage import find_objects
        return [types.SimpleNamespace(label=i, slice=sl) for i, sl in enumerate(find_objects(y), 1) if sl is not None]

    def _raise(e):
        raise e
    stubs["skimage.measure"].regionprops = regionprops
    stubs["csbdeep.utils"]._raise = _raise
    for k, v in stubs.items():
        monkeypatch.setitem(sys.modules, k, v)
    spec = importlib.util.spec_from_file_location("_ref_matching_group", os.path.join(REF, "matching.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference sources (build container only)")
def test_composition_equals_the_reference_function(monkeypatch):
    """the reference's own group_matching_labels, loaded from source (numba's jit stood in for by the identity, regionprops by find_objects)"""
    ref = _ref_matching(monkeypatch)
    for name, ys in sorted(SCENES.items()):
        for crit in G.CRITERIA:
            for thr in G.THRESHS:
                r = ref.group_matching_labels(ys, thresh=thr, criterion=crit)
                c = G.compose(ys, thr, crit)
                assert r.dtype == c.dtype and np.array_equal(r, c), (name, crit, thr)


def test_lattice_stack_first_frames_equal_host():
    """a small cut of the timing scene: the composition equals the host function on the first two frames"""
    from stardist_amd import matching as M
    ys = G.lattice_stack(frames=3, size=512)
    assert np.array_equal(G.compose(ys, 1e-10, "iou")[:2], M.group_matching_labels(ys[:2]))


def error_cases(y, neg, device_free):
    """inputs the host function refuses.  A negative label in frames of one shape is found by the overlap kernel (the frames' minima), so
    those cases need a device: tests/test_gpu_group_matching.py runs the full list."""
    cases = [[y], np.stack([y]), [y, y.astype(np.float32)], np.stack([y, y]).astype(np.float64), [y, y[:10]], [neg, y[:10]],
             [y[:10], y.astype(np.float32)], np.arange(5), -np.arange(5), [y, [[1, 2], [3, 4]]]]
    return cases if device_free else cases + [[y, neg], np.stack([neg, y]), [y, y, neg.astype(np.int64)]]


def test_errors_equal_the_host_function():
    """same exception type and message as the host function, raised before any device work (the host box has no device)"""
    from stardist_amd import matching as M
    from stardist_amd import matching_sparse as S
    y = G.discs((40, 50), 10, 3)
    neg = y.copy()
    neg[0, 0] = -1
    for ys in error_cases(y, neg, device_free=True):
        with pytest.raises(ValueError) as host:
            M.group_matching_labels(ys)
        with pytest.raises(ValueError) as dev:
            M.group_matching_labels(ys, device="cuda:0")
        assert str(dev.value) == str(host.value), (str(dev.value), str(host.value))
        with pytest.raises(ValueError) as direct:
            S.group_matching_labels_device(ys, device="cuda:0")
        assert str(direct.value) == str(host.value)
    with pytest.raises(ValueError, match="HIP device"):
        M.group_matching_labels([y, y], device="cpu")
