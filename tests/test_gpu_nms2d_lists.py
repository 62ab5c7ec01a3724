"""The neighbour lists of the 2D NMS hold the better-scored neighbours only, a new survivor finds its pairs by walking its own cell window
(csrc/nms2d.hip: k_neighbours, k_round_emit, walk_window), and a round does not sweep a pair whose j a decided pair of the same round has
suppressed (k_pair_bucket_*).  Everything is compared exactly:

  keep flags   with the compiled reference's.  The reference runs once per scene, with the kd-tree and the bounding boxes on: with a
               threshold >= 0 its flags do not depend on either switch (a pair one of them leaves out has disjoint polygons, overlap 0).
  stats[3]     the number of ordered neighbour relations = 2 x the unordered pairs that pass `may_interact`, counted brute force by numpy
               (tests/_nms2d_np.py) -- whichever form built the lists, single pass into slots or count / scan / fill.
  stats[0, 2]  pairs evaluated and rounds: equal between the two list forms.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nms_graph_cases as C  # noqa: E402
import _nms2d_np as P  # noqa: E402

pytestmark = pytest.mark.gpu

FLAGS = [(1, 1), (0, 0), (1, 0), (0, 1)]


def _uniform():
    from oracle import synth
    d, p, s = synth.s2d_uniform(192, 192, prob_thresh=0.85)
    return d, p, np.float32(0.4)


def _graph(key):
    sc = C.scene(key)
    return sc.dist, sc.points, sc.thr


SCENES = {
    "hub": lambda: _graph(C.HUBS_2D[1]),
    "clique": lambda: _graph([k for k in C.OTHERS_2D if k.startswith("clique")][0]),
    "forest": lambda: _graph([k for k in C.OTHERS_2D if k.startswith("forest")][0]),
    "chain64": lambda: _graph([k for k in C.CHAINS_2D if C.is_monotone_chain(k) and C.scene(k).n == 64 and "serpentine" not in k][0]),
    "uniform192": _uniform,
}
_DATA, _REF, _PAIRS = {}, {}, {}


def _data(name):
    if name not in _DATA:
        _DATA[name] = SCENES[name]()
    return _DATA[name]


def _ref(refmods, name):
    if name not in _REF:
        d, p, thr = _data(name)
        refmods.set_threads(8)
        _REF[name] = np.asarray(refmods.stardist2d().c_non_max_suppression_inds(d, p, 1, 1, 0, thr), bool)
    return _REF[name]


def _pairs(name, flags):
    d, p, thr = _data(name)
    key = (name,) if thr >= 0 else (name, flags)          # (with a threshold >= 0 the predicate does not read the switches)
    if key not in _PAIRS:
        _PAIRS[key] = P.neighbour_pairs(d, p, flags[0], flags[1], thr)
    return _PAIRS[key]


def _run(d, p, thr, flags, single):
    from stardist_amd.lib import _native as N, stardist2d as sd2
    with N.option("nms2d_neighbours_single_pass", single):
        keep, stats = sd2.c_non_max_suppression_inds(d, p, flags[0], flags[1], 0, thr, return_stats=True)
    return np.asarray(keep, bool), [int(v) for v in stats]


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", list(SCENES))
def test_lists_of_better_scored_neighbours(refmods, name, flags):
    d, p, thr = _data(name)
    ref = _ref(refmods, name)
    want = 2 * _pairs(name, flags)
    got = {}
    for single in (0, 1):
        keep, stats = _run(d, p, thr, flags, single)
        print("%-10s flags=%s single_pass=%d n=%d kept=%d pairs=%d rounds=%d neighbour relations=%d (numpy %d) skipped=%d"
              % (name, flags, single, len(d), int(keep.sum()), stats[0], stats[2], stats[3], want, stats[11]))
        assert np.array_equal(keep, ref), (name, flags, single, np.flatnonzero(keep != ref)[:10])
        assert stats[3] == want, (name, flags, single, stats[3], want)
        got[single] = stats
    assert got[0][0] == got[1][0] and got[0][2] == got[1][2], (name, flags, got[0][:4], got[1][:4])


@pytest.mark.parametrize("single", [0, 1])
def test_pair_whose_j_is_already_suppressed_is_not_swept(refmods, single):
    """the triples scene (tests/_nms2d_np.py): B suppresses j by a pair the area enclosure decides; (A, j) is a pair of the same round, and
    for some of the 200 distances the enclosure leaves it undecided (stats[0] - stats[9] >= 1) -- those are not swept (stats[11] >= 1)"""
    d, p, kinds = P.triples_scene()
    refmods.set_threads(8)
    ref = np.asarray(refmods.stardist2d().c_non_max_suppression_inds(d, p, 1, 1, 0, P.TRIPLES_THR), bool)
    keep, stats = _run(d, p, P.TRIPLES_THR, (1, 1), single)
    print("triples: kept=%d pairs=%d decided=%d rounds=%d skipped=%d" % (int(keep.sum()), stats[0], stats[9], stats[2], stats[11]))
    assert np.array_equal(keep, ref), np.flatnonzero(keep != ref)[:10]
    assert stats[0] - stats[9] >= 1, stats[:12]
    assert stats[11] >= 1, stats[:12]
