"""Proof of the scenes of tests/_nms_graph_cases.py (no GPU): the compiled reference returns the constructed keep flags, it suppresses across
sampled designed edges and not across sampled designed non-edges when given the two candidates alone, and the generators keep their own
invariants -- so whatever tests/test_gpu_nms_graph.py finds different on these scenes is the scheduler's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nms_graph_cases as C  # noqa: E402


def _ref_keep(refmods, sc, sel=None):
    sel = slice(None) if sel is None else np.asarray(sel)
    d, p = np.ascontiguousarray(sc.dist[sel]), np.ascontiguousarray(sc.points[sel])
    if sc.dim == 2:
        return refmods.stardist2d().c_non_max_suppression_inds(d, p, 1, 1, 0, sc.thr)
    V, F = sc.rays()
    refmods.set_threads(1)                       # (the reference's 3D result is only defined for one thread: oracle/ref.py)
    return refmods.stardist3d().c_non_max_suppression_inds(d, p, V, F, np.ascontiguousarray(sc.scores[sel]), 1, 1, 0, sc.thr)


def _boxes(sc):
    """conservative bounding boxes: every vertex lies within the largest ray of its centre; 2D vertices are truncated to integers
    (stardist2d.cpp:447-471; all coordinates are positive here, so that is floor)"""
    r = sc.dist.max(1, keepdims=True).astype(np.float64)
    lo, hi = sc.points - r, sc.points + r
    return (np.floor(lo), np.floor(hi)) if sc.dim == 2 else (lo, hi)


def _pairs_within(sc, reach):
    """all pairs i < j of ordinary candidates with centres closer than `reach` (chunked all-pairs)"""
    p = sc.points.astype(np.float64)
    out = []
    for a in range(0, sc.n, 512):
        d = np.linalg.norm(p[a:a + 512, None, :] - p[None, :, :], axis=2)
        i, j = np.nonzero(d < reach)
        i += a
        m = i < j
        out.append(np.stack([i[m], j[m]], 1))
    out = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    if sc.big is not None:
        out = out[(out != sc.big).all(1)]
    return out


@pytest.mark.parametrize("key", C.SCENES_2D + C.SCENES_3D)
def test_generator_invariants(key):
    sc = C.scene(key)
    n = sc.n
    assert sc.dist.shape == (n, sc.n_rays) and sc.points.shape == (n, sc.dim) and sc.keep.shape == (n,)
    assert sc.dist.dtype == np.float32 and sc.points.dtype == np.float32 and sc.scores.dtype == np.float32
    assert np.all(np.diff(sc.scores) < 0), "scores distinct and best first"
    assert (sc.points - sc.dist.max(1, keepdims=True) > 1).all(), "every vertex has positive coordinates"
    assert np.any(sc.points != np.round(sc.points), 1).all() or n < 3, "non-integer centres"
    e = sc.edges
    assert (e[:, 0] < e[:, 1]).all() and len(np.unique(e[:, 0] * n + e[:, 1])) == len(e)
    assert np.array_equal(sc.keep, C.greedy(n, e)) and (n == 0 or sc.keep[0])
    # the designed distances
    p = sc.points.astype(np.float64)
    ordinary = e if sc.big is None else e[(e != sc.big).all(1)]
    if len(ordinary):
        de = np.linalg.norm(p[ordinary[:, 0]] - p[ordinary[:, 1]], axis=1)
        assert sc.edge_dist[0] <= de.min() and de.max() <= sc.edge_dist[1], (de.min(), de.max(), sc.edge_dist)
    if sc.non_edge_min is not None:
        near = _pairs_within(sc, sc.non_edge_min)
        is_edge = np.isin(near[:, 0] * n + near[:, 1], e[:, 0] * n + e[:, 1])
        assert is_edge.all(), "designed non-neighbours closer than %g: %s" % (sc.non_edge_min, near[~is_edge][:5])
    # the claimed disjoint bounding boxes
    lo, hi = _boxes(sc)
    for lab in sc.labelings:
        idx = np.flatnonzero(lab >= 0)
        for a in range(0, len(idx), 512):
            ia = idx[a:a + 512]
            apart = ((hi[ia, None, :] < lo[None, idx, :]) | (hi[None, idx, :] < lo[ia, None, :])).any(2)
            bad = ~apart & (lab[ia, None] != lab[None, idx])
            assert not bad.any(), (key, ia[np.nonzero(bad)[0][:5]], idx[np.nonzero(bad)[1][:5]])
    if getattr(sc, "depth", None):
        assert np.array_equal(sc.keep, np.arange(n) % 2 == 0), "a monotone chain keeps every other candidate"


def test_round_count_of_a_monotone_chain():
    """the regime bounds the GPU test places on stats[2], from the host loop of sd_nms2d"""
    assert [C.rounds_2d_monotone(n) for n in (1, 2, 5, 6, 7, 12, 13, 64, 600, 3000)] == [1, 2, 3, 4, 4, 7, 7, 29, 252, 1252]
    assert [C.rounds_2d_monotone(n) for n in (1023, 1024, 1025)] == [428, 429, 429]
    for n in list(C.CHAIN_N_2D) + list(range(1, 200)):
        t = min(n // 6, 65536)
        assert C.rounds_2d_monotone(n) >= (n - t) // 2
        if t >= 5:                               # ceil((n + 1 - t) / 2) + 1 <= (n + 4 - t) / 2 < n / 2
            assert C.rounds_2d_monotone(n) < (n + 1) // 2


@pytest.mark.parametrize("key", C.SCENES_2D + [k for k in C.SCENES_3D if C.scene(k).n <= C.REF_MAX_3D])
def test_reference_returns_the_constructed_flags(refmods, key):
    sc = C.scene(key)
    ref = np.asarray(_ref_keep(refmods, sc), bool)
    diff = np.flatnonzero(ref != sc.keep)
    assert len(diff) == 0, (key, diff[:10], int(ref.sum()), int(sc.keep.sum()))


def _sample(rng, rows, k):
    return rows if len(rows) <= k else rows[rng.choice(len(rows), k, replace=False)]


@pytest.mark.parametrize("key", C.SCENES_2D + C.SCENES_3D)
def test_sampled_pairs_alone(refmods, key):
    """the margins, for the polygons / polyhedra of this ray count: the reference, given two candidates alone, suppresses the second across
    a designed edge and keeps it across a designed non-edge -- sampled among the NEAREST non-edges (centres closer than three radii), which are the ones that could be mistaken"""
    sc = C.scene(key)
    n = sc.n
    rng = np.random.RandomState(n + sc.n_rays)
    k = 24 if sc.dim == 2 else 8
    for i, j in _sample(rng, sc.edges, k):
        assert np.asarray(_ref_keep(refmods, sc, [i, j])).tolist() == [True, False], (key, "edge", i, j)
    rmax = float(np.sort(sc.dist.max(1))[-2]) if (sc.big is not None and n > 1) else float(sc.dist.max()) if n else 0.0
    near = _pairs_within(sc, 3.0 * rmax)
    if sc.big is not None:
        outer = np.flatnonzero(sc.labelings[-1] > 0)
        near = np.concatenate([near, np.stack([np.minimum(outer, sc.big), np.maximum(outer, sc.big)], 1)])
    near = near[~np.isin(near[:, 0] * n + near[:, 1], sc.edges[:, 0] * n + sc.edges[:, 1])]
    for i, j in _sample(rng, near, k):
        assert np.asarray(_ref_keep(refmods, sc, [i, j])).tolist() == [True, True], (key, "non-edge", i, j)
