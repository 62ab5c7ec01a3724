"""The triples scene of tests/test_gpu_nms2d_lists.py (tests/_nms2d_np.py) against the compiled reference alone: every B and every A is
kept, no j is.  And the scene's premise, from the numpy statement of the neighbour predicate: no A lists a B."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nms2d_np as P  # noqa: E402


def test_reference_keeps_every_a_and_b_and_no_j(refmods):
    d, p, kinds = P.triples_scene()
    refmods.set_threads(8)
    for flags in ((1, 1), (0, 0)):
        keep = np.asarray(refmods.stardist2d().c_non_max_suppression_inds(d, p, flags[0], flags[1], 0, P.TRIPLES_THR), bool)
        assert keep[kinds == "B"].all() and keep[kinds == "A"].all(), (flags, np.flatnonzero(~keep & (kinds != "j"))[:10])
        assert not keep[kinds == "j"].any(), (flags, np.flatnonzero(keep & (kinds == "j"))[:10])


def test_triples_neighbour_relations():
    """each triple has exactly the relations (B, j) and (A, j): 400 unordered pairs, none between an A and a B, none across triples"""
    d, p, kinds = P.triples_scene()
    assert P.neighbour_pairs(d, p, 1, 1, P.TRIPLES_THR) == 2 * P.TRIPLES
    ab = kinds != "j"
    assert P.neighbour_pairs(d[ab], p[ab], 1, 1, P.TRIPLES_THR) == 0
