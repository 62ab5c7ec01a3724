"""Proof of the scenes of tests/_nms_graph_cases.py (no GPU): the compiled reference returns the constructed keep flags, it suppresses across
sampled designed edges and not across sampled designed non-edges when given the two candidates alone, and the generators keep their own
invariants -- so whatever tests/test_gpu_nms_graph.py finds different on these scenes is the scheduler's.  At the end the large hubs of
tests/test_gpu_nms_slot_limits.py: their slot totals by the numpy mirror, their invariants, the reference at a reduced size."""
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


# ---- the slot-limit scenes (tests/test_gpu_nms_slot_limits.py): tens of thousands of candidates, so the pair searches go through a k-d tree
def _mirror_total(key):
    import _nms2d_np as M
    sc = C.scene(key)
    return M.slot_capacities(sc.dist, sc.points, sc.thr)["total"]


def test_slot_capacity_mirror_on_the_small_hub():
    """the figure the scene list was sized from: hub radius 200, m = 2000"""
    assert _mirror_total(C.HUBS_2D[0]) == 4194674


@pytest.mark.parametrize("key", C.SLOT_LIMIT_2D)
def test_slot_limit_scene_lies_on_its_side_of_the_limit(key):
    """the mirrored slot total (float32 cell arithmetic of cell_of / cell_window, reach, cell size and origin of build_grid) is the recorded
    one and keeps the margins to 2^31 - 1, 2^31, 2^32 that the scene was sized for"""
    t = _mirror_total(key)
    assert t == C.SLOT_TOTALS[key], (key, t)
    if key == C.BELOW_2D:
        assert t <= C.SLOT_LIMIT - 5 * 10 ** 6
        f, a, kw = C._FACTORIES[key]                     # the largest m in steps of 100 that keeps the margin
        nxt = C.hub(2, a[1] + 100, True, hub_radius=kw["hub_radius"])
        import _nms2d_np as M
        assert M.slot_capacities(nxt.dist, nxt.points, nxt.thr)["total"] > C.SLOT_LIMIT - 5 * 10 ** 6
    elif key in C.BAND_2D:
        assert 2 ** 31 + 5 * 10 ** 6 <= t <= 2 ** 32 - 10 ** 9
    else:
        assert key == C.WRAP_2D and 10 ** 8 <= t - 2 ** 32 <= 2 ** 31 - 10 ** 8


@pytest.mark.parametrize("key", C.SLOT_LIMIT_2D)
def test_slot_limit_scene_invariants(key):
    """test_generator_invariants for the large hubs: the small candidates keep their distance (non_edge_min) and the claimed bounding boxes
    are disjoint (labelings) -- pairs found by scipy's cKDTree"""
    from scipy.spatial import cKDTree
    sc = C.scene(key)
    n = sc.n
    assert sc.dist.shape == (n, sc.n_rays) and sc.points.shape == (n, 2) and sc.keep.shape == (n,)
    assert sc.dist.dtype == np.float32 and sc.points.dtype == np.float32
    assert np.all(np.diff(sc.scores) < 0)
    assert (sc.points - sc.dist.max(1, keepdims=True) > 1).all(), "every vertex has positive coordinates"
    assert np.any(sc.points != np.round(sc.points), 1).all()
    e = sc.edges
    assert len(e) == sc.m and (e[:, 0] < e[:, 1]).all() and (e == sc.big).any(1).all(), "every edge joins the hub and a small candidate"
    assert np.array_equal(sc.keep, C.greedy(n, e)) and sc.keep[0]
    assert int(sc.keep.sum()) == (n - sc.m if sc.big == 0 else n - 1)
    p = sc.points.astype(np.float64)
    small = np.flatnonzero(np.arange(n) != sc.big)
    assert len(cKDTree(p[small]).query_pairs(sc.non_edge_min)) == 0, "small candidates closer than %g" % sc.non_edge_min
    lo, hi = _boxes(sc)
    lab_small, lab_hub = sc.labelings
    assert lab_small[sc.big] == -1 and len(np.unique(lab_small[small])) == n - 1        # every pair of small candidates is claimed
    reach = float((hi - lo)[small].max()) + 1.0                                            # boxes further apart than this (Chebyshev) cannot meet
    near = small[cKDTree(p[small]).query_pairs(reach, p=np.inf, output_type="ndarray")]
    apart = ((hi[near[:, 0]] < lo[near[:, 1]]) | (hi[near[:, 1]] < lo[near[:, 0]])).any(1)
    assert len(near) > n and apart.all(), near[~apart][:5]
    outer = np.flatnonzero(lab_hub > 0)
    assert lab_hub[sc.big] == 0 and len(outer) == sc.m // 10
    assert ((hi[outer] < lo[sc.big]) | (hi[sc.big] < lo[outer])).any(1).all(), "an outer candidate's box meets the hub's"


@pytest.mark.parametrize("hub_radius,m,hub_first", [(1000.0, 20000, True), (1000.0, 5000, False), (1300.0, 20000, True)])
def test_reference_on_the_large_hubs_at_reduced_m(refmods, hub_radius, m, hub_first):
    """The reference's time grows with n^2 (every candidate's radius search covers the scene): 9.4, 11.2, 254 and 19.7 s on 8 threads for
    the four full scenes, where it returned the constructed flags when the scenes were sized.  Beyond C.REF_MAX_2D candidates it is not run in
    the suite; here the same hubs with fewer small candidates (the first m of the same lattice: the scene's innermost part)."""
    sc = C.hub(2, m, hub_first, hub_radius=hub_radius)
    assert sc.n <= C.REF_MAX_2D
    refmods.set_threads(8)
    ref = np.asarray(_ref_keep(refmods, sc), bool)
    diff = np.flatnonzero(ref != sc.keep)
    assert len(diff) == 0, (diff[:10], int(ref.sum()), int(sc.keep.sum()))


@pytest.mark.parametrize("key", C.SLOT_LIMIT_2D)
def test_slot_limit_scene_margins_at_the_rim(refmods, key):
    """the pairs of the full scenes that could be mistaken, given to the reference alone: the hub with the inner small candidates furthest
    from its centre (suppressed, or suppressing it) and with the outer ones nearest to it (both kept)"""
    sc = C.scene(key)
    p = sc.points.astype(np.float64)
    d = np.linalg.norm(p - p[sc.big], axis=1)
    inner = np.setdiff1d(np.unique(sc.edges), [sc.big])
    outer = np.flatnonzero(sc.labelings[1] > 0)
    for j in inner[np.argsort(d[inner])[-12:]]:
        pair = sorted([sc.big, int(j)])
        assert np.asarray(_ref_keep(refmods, sc, pair)).tolist() == [True, False], (key, "edge", pair)
    for j in outer[np.argsort(d[outer])[:12]]:
        pair = sorted([sc.big, int(j)])
        assert np.asarray(_ref_keep(refmods, sc, pair)).tolist() == [True, True], (key, "non-edge", pair)


def test_clique_without_an_edge_list():
    """the cliques of the capacity tests: same candidates and flags as the listed form"""
    a, b = C.clique(2, 300), C.clique(2, 300, list_edges=False)
    assert b.edges is None and np.array_equal(a.dist, b.dist) and np.array_equal(a.points, b.points) and np.array_equal(a.keep, b.keep)
    big = C.clique(2, 93000, list_edges=False)
    assert big.n == 93000 and int(big.keep.sum()) == 1 and big.keep[0]
    assert np.ptp(big.points, 0).max() < 1.0 and big.n * (big.n - 1) // 2 >= 2 ** 32
