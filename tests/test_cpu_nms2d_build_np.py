"""The numpy statement of the 2D NMS's build step (tests/_nms2d_np.py) against the compiled reference.  The reference exposes its polygon
area only through its Clipper call (stardist2d.cpp:152-165: the area of every output path by :128-138), so a polygon is intersected with
itself: the output is the polygon again -- possibly starting at another vertex and without collinear vertices -- and the float the
reference returns for it must equal `path_area` of THAT path, in its order; its bounding box must be the polygon's.  Regime (a) takes the
exact integer sum, regime (c) (sum |term| >= 2^24) the serial float accumulation, where the order of the additions decides the bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nms2d_np as P  # noqa: E402


@pytest.mark.parametrize("R", [5, 8, 32])
@pytest.mark.parametrize("regime", ["a", "c"])
def test_path_area_and_bbox_against_the_reference(refmods, regime, R):
    dist, pts = P.build_case(regime, 64, R)
    b = P.build(dist, pts)
    if regime == "a":
        assert (b["sum_abs"] < (1 << 24)).all()
    else:
        assert (b["sum_abs"] >= (1 << 24)).all()
    checked = 0
    for i in range(len(dist)):
        X, Y = b["X"][i], b["Y"][i]
        paths = refmods.clipper_paths(X, Y, X, Y)
        if len(paths) != 1:                 # (a self-touching integer polygon: Clipper splits it; not what this test is about)
            continue
        path = paths[0]
        area, sum_abs = P.path_area(path[None, :, 0], path[None, :, 1])
        ref_area = np.float32(refmods.clipper_area(X, Y, X, Y))
        assert area[0] == ref_area, (regime, R, i, float(area[0]), float(ref_area))
        if regime == "c":
            assert sum_abs[0] >= (1 << 24)
        assert [path[:, 0].min(), path[:, 0].max(), path[:, 1].min(), path[:, 1].max()] == list(b["bbox"][i]), (regime, R, i)
        # the same polygon in its own order: the same set of edges, so the exact sums agree; the float sums may differ in regime (c)
        if regime == "a" and len(path) == R:
            assert b["area"][i] == ref_area, (R, i)
        checked += 1
    assert checked >= 48, (regime, R, checked)
