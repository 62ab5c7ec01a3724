"""The build step of the 2D NMS (csrc/nms2d.hip: k_build32 for up to 32 rays -- one thread per candidate, rows staged through LDS -- and
k_build above), through its probe sd_nms2d_build_device, against the numpy float32 / int64 statement of stardist2d.cpp:454-471 and
:128-148 in tests/_nms2d_np.py (proven against the compiled reference in tests/test_cpu_nms2d_build_np.py).  Every output is compared for
equality: integer vertices, bounding boxes, radii, areas and the five extremes the grid set-up reads back."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nms2d_np as P  # noqa: E402

pytestmark = pytest.mark.gpu

NS = (1, 7, 64, 65, 1000)          # one lane, a partial wave, exactly one wave, one candidate in a second workgroup, many workgroups
RS = (3, 5, 8, 31, 32)             # (odd R: rows do not start on 16-byte boundaries)


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("regime", P.REGIMES)
def test_build_equals_numpy_statement(regime, R):
    from stardist_amd.lib import stardist2d as sd2
    for n in NS:
        dist, pts = P.build_case(regime, n, R)
        want = P.build(dist, pts)
        # the regime must reach the area path it was made for
        if regime == "a":
            assert (want["sum_abs"] < (1 << 24)).all(), (n, R, int(want["sum_abs"].max()))
        if regime == "c":
            assert (want["sum_abs"] >= (1 << 24)).all(), (n, R, int(want["sum_abs"].min()))
        if regime == "b" and n >= 64:
            assert (want["X"] < 0).any() and (want["X"] > 0).any() and (want["Y"] < 0).any() and (want["Y"] > 0).any()
        if regime == "d":
            assert (want["area"] == 0).all()
        vx, vy, bbox, radius, area, gstats = sd2.nms2d_build(dist, pts)
        tag = (regime, R, n)
        assert np.array_equal(vx, want["X"]), (tag, np.argwhere(vx != want["X"])[:5])
        assert np.array_equal(vy, want["Y"]), (tag, np.argwhere(vy != want["Y"])[:5])
        assert np.array_equal(bbox, want["bbox"]), (tag, np.argwhere(bbox != want["bbox"])[:5])
        assert radius.dtype == np.float32 and np.array_equal(radius, want["radius"]), tag
        assert area.dtype == np.float32 and np.array_equal(area, want["area"]), (tag, np.flatnonzero(area != want["area"])[:5])
        assert np.array_equal(gstats, want["gstats"]), (tag, gstats, want["gstats"])


def test_build_above_32_rays_unchanged_kernel():
    """k_build (more than 32 rays) behind the same host function"""
    from stardist_amd.lib import stardist2d as sd2
    for regime in ("a", "c"):
        dist, pts = P.build_case(regime, 130, 64)
        want = P.build(dist, pts)
        vx, vy, bbox, radius, area, gstats = sd2.nms2d_build(dist, pts)
        assert np.array_equal(vx, want["X"]) and np.array_equal(vy, want["Y"]) and np.array_equal(bbox, want["bbox"])
        assert np.array_equal(radius, want["radius"]) and np.array_equal(area, want["area"]) and np.array_equal(gstats, want["gstats"])
