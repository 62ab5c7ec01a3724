"""CPU: the sparse finishing of the device matching (stardist_amd.matching_sparse.matching_from_overlap) against the host matching
(stardist_amd.matching.matching, pinned to the reference by test_cpu_vs_reference_source.py), fed by the numpy statement of the overlap
list the kernel sd_label_overlap_device returns (sparse_overlap).  Integer fields equal, float fields bit-identical for thresh > 0 and
within 1e-6 relative for thresh <= 0, report_matches identical, matching_dataset identical."""
import numpy as np
import pytest

from stardist_amd import matching as M
from stardist_amd import matching_sparse as S

THRESHS = (0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0)


def _discs(rng, shape, n, rmin=2, rmax=9):
    y = np.zeros(shape, np.int32)
    grids = np.ogrid[tuple(slice(0, s) for s in shape)]
    for i in range(1, n + 1):
        c = [rng.randint(0, s) for s in shape]
        r = rng.randint(rmin, rmax)
        y[sum((g - ci) ** 2 for g, ci in zip(grids, c)) < r * r] = i
    return y


def _perturb(rng, y):
    """a prediction of y: shifted, a few pixels dropped, some objects removed, some ids shuffled, a few extra objects"""
    ax = rng.randint(0, y.ndim)
    p = np.roll(y, rng.randint(-3, 4), axis=ax)
    p = np.where(rng.rand(*p.shape) < 0.03, 0, p)
    ids = np.unique(p)[1:]
    if len(ids):
        drop = rng.choice(ids, size=rng.randint(0, max(1, len(ids) // 4) + 1), replace=True)
        p[np.isin(p, drop)] = 0
        perm = np.zeros(ids.max() + 1, np.int64)
        perm[ids] = rng.permutation(ids)
        p = perm[p].astype(np.int32)
    extra = _discs(rng, y.shape, rng.randint(0, 4))
    return np.where((p == 0) & (extra > 0), extra + 1000, p).astype(np.int32)


def _scenes(seed, count, shape=(80, 96)):
    rng = np.random.RandomState(seed)
    for k in range(count):
        y = _discs(rng, shape, rng.randint(0, 30))
        kind = k % 4
        if kind == 0:
            p = _perturb(rng, y)
        elif kind == 1:
            p = _discs(rng, shape, rng.randint(0, 30))             # unrelated objects, n_true != n_pred
        elif kind == 2:
            p = np.roll(y, (rng.randint(-4, 5), rng.randint(-4, 5)), axis=(0, 1))
        else:
            p = M._shuffle_labels(_perturb(rng, y))
        yield y, p


def _compare(h, d, exact):
    assert h._fields == d._fields
    for key in h._fields:
        u, v = getattr(h, key), getattr(d, key)
        if exact or isinstance(u, (str, int)) or key in ("tp", "fp", "fn", "n_true", "n_pred"):
            assert type(u) == type(v) and (u == v), (key, h.thresh, u, v)
        else:
            assert np.isclose(float(u), float(v), rtol=1e-6, atol=0), (key, h.thresh, u, v)


def _sparse_matching(y_true, y_pred, thresh, criterion="iou", report_matches=False):
    t, p, c = S.sparse_overlap(y_true, y_pred)
    return S.matching_from_overlap(t, p, c, y_true.size, thresh=thresh, criterion=criterion, report_matches=report_matches)


def test_sparse_overlap_is_the_dense_table():
    rng = np.random.RandomState(0)
    for _ in range(20):
        y = _discs(rng, (40, 50), rng.randint(0, 12))
        p = _perturb(rng, y)
        yt, _, bt = M.relabel_sequential(y)
        yp, _, bp = M.relabel_sequential(p)
        dense = M.label_overlap(yt, yp)
        t, q, c = S.sparse_overlap(y, p)
        assert np.all(np.diff(t * (1 << 32) + q) > 0)                  # ascending by (t, p), unique
        assert not np.any((t == 0) & (q == 0)) and np.all(c > 0)
        i, j = np.nonzero(dense)
        keep = (i > 0) | (j > 0)
        assert np.array_equal(bt[i[keep]], t) and np.array_equal(bp[j[keep]], q) and np.array_equal(dense[i, j][keep], c)


@pytest.mark.parametrize("criterion", ["iou", "iot", "iop"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sparse_matching_equals_host(criterion, seed):
    for y, p in _scenes(seed * 10 + len(criterion), 40):
        h = M.matching(y, p, thresh=THRESHS, criterion=criterion)
        d = _sparse_matching(y, p, THRESHS, criterion)
        for a, b in zip(h, d):
            _compare(a, b, exact=a.thresh > 0)
        # a scalar threshold and None (= 0)
        _compare(M.matching(y, p, thresh=0.5, criterion=criterion), _sparse_matching(y, p, 0.5, criterion), exact=True)
        _compare(M.matching(y, p, thresh=None, criterion=criterion), _sparse_matching(y, p, None, criterion), exact=False)


@pytest.mark.parametrize("criterion", ["iou", "iot", "iop"])
def test_sparse_report_matches_equals_host(criterion):
    for y, p in _scenes(77, 24):
        for thr in (0.1, 0.5, 0.7):
            h = M.matching(y, p, thresh=thr, criterion=criterion, report_matches=True)
            d = _sparse_matching(y, p, thr, criterion, report_matches=True)
            assert h == d and h._fields == d._fields
            assert [type(x) for x in h.matched_scores] == [type(x) for x in d.matched_scores]


def test_3d_uint16_and_non_sequential_ids():
    rng = np.random.RandomState(4)
    for _ in range(12):
        y = _discs(rng, (12, 30, 34), rng.randint(1, 15))
        p = _perturb(rng, y)
        ids = rng.choice(60000, size=y.max() + 1, replace=False).astype(np.uint16)
        ids[0] = 0
        yu = ids[y]                                                     # uint16 ground truth, non-sequential ids
        h = M.matching(yu, p, thresh=THRESHS)
        d = _sparse_matching(yu, p, THRESHS)
        for a, b in zip(h, d):
            _compare(a, b, exact=a.thresh > 0)
        assert M.matching(yu, p, thresh=0.3, report_matches=True) == _sparse_matching(yu, p, 0.3, report_matches=True)


def _huge(rng, k):
    """k distinct ascending ids in [2**30, 2**31 - 1)"""
    ids = np.unique(rng.randint(2 ** 30, 2 ** 31 - 1, size=4 * k + 8, dtype=np.int64))
    return np.sort(rng.permutation(ids)[:k])


def test_huge_ids():
    """ids up to 2**31 - 1 (the host path's dense relabelling map would not fit): the sparse result equals the host's on the
    sequentially relabelled images, matched pairs mapped back to the original ids"""
    rng = np.random.RandomState(5)
    for _ in range(10):
        y = _discs(rng, (60, 60), rng.randint(1, 20))
        p = _perturb(rng, y)
        ids_t = np.r_[0, _huge(rng, y.max())]
        ids_t[-1] = 2 ** 31 - 1
        ids_p = np.r_[0, _huge(rng, p.max())]
        yh, ph = ids_t[y], ids_p[p]
        seq = lambda a: np.unique(a, return_inverse=True)[1].reshape(a.shape).astype(np.int32)      # 0 stays first: sequential ids
        h = M.matching(seq(yh), seq(ph), thresh=THRESHS)
        d = _sparse_matching(yh, ph, THRESHS)
        for a, b in zip(h, d):
            _compare(a, b, exact=a.thresh > 0)
        hr = M.matching(y, p, thresh=0.5, report_matches=True)
        dr = _sparse_matching(yh, ph, 0.5, report_matches=True)
        assert dr.matched_pairs == tuple((int(ids_t[a]), int(ids_p[b])) for a, b in hr.matched_pairs)
        assert dr.matched_scores == hr.matched_scores and dr.matched_tps == hr.matched_tps


def test_empty_and_single_object_images():
    z = np.zeros((20, 30), np.int32)
    one = z.copy()
    one[5:9, 6:12] = 7
    other = z.copy()
    other[6:10, 8:13] = 3
    for y, p in [(z, z), (one, z), (z, one), (one, one), (one, other), (other, one)]:
        for crit in ("iou", "iot", "iop"):
            h = M.matching(y, p, thresh=THRESHS, criterion=crit)
            d = _sparse_matching(y, p, THRESHS, crit)
            for a, b in zip(h, d):
                _compare(a, b, exact=a.thresh > 0)
            assert M.matching(y, p, thresh=0.5, criterion=crit, report_matches=True) == \
                _sparse_matching(y, p, 0.5, crit, report_matches=True)


@pytest.mark.parametrize("by_image", [False, True])
def test_matching_dataset_through_the_sparse_finisher(by_image, monkeypatch):
    scenes = list(_scenes(9, 12))
    Y, P = [s[0] for s in scenes], [s[1] for s in scenes]
    host = M.matching_dataset(Y, P, thresh=(0.3, 0.5, 0.7), by_image=by_image, show_progress=False)

    def sparse(y_true, y_pred, thresh=0.5, criterion="iou", report_matches=False, device=None):
        return _sparse_matching(y_true, y_pred, thresh, criterion, report_matches)
    monkeypatch.setattr(M, "matching", sparse)
    dev = M.matching_dataset(Y, P, thresh=(0.3, 0.5, 0.7), by_image=by_image, show_progress=False)
    for a, b in zip(host, dev):
        _compare(a, b, exact=True)


def test_dense_limit_of_report_matches(monkeypatch):
    rng = np.random.RandomState(3)
    y = _discs(rng, (50, 50), 10)
    monkeypatch.setattr(S, "DENSE_LIMIT", 4)
    with pytest.raises(ValueError, match="report_matches=True needs the dense"):
        _sparse_matching(y, y, 0.5, report_matches=True)
    assert _sparse_matching(y, y, 0.5).tp == len(np.unique(y)) - 1
