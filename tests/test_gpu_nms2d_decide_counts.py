"""GPU: the 2D NMS around its decide kernel (k_pairs_decide, csrc/nms2d.hip): on the recorded scenes the keep flags are the compiled
reference's, and the number of pairs, of pairs decided by the area enclosure, of undecided pairs deferred to the tail batch and of pairs
skipped are those of the build of commit 2d2206f (tests/golden/area_enclosure_golden.json).  The last scene reaches the tail batch with
deferred undecided pairs."""
import numpy as np
import pytest

import _area_golden

pytestmark = pytest.mark.gpu
REC = _area_golden.recorded()


def test_the_tail_scene_defers_undecided_pairs():
    assert REC["nms"][-1]["scene"] == REC["tail_scene"] and REC["nms"][-1]["stats"]["deferred_undecided"] > 0
    assert [r["scene"] for r in REC["nms"]] == _area_golden.generator().nms_scenes(REC["tail_scene"])


@pytest.mark.parametrize("k", range(len(REC["nms"])))
def test_keep_flags_and_decide_counts(refmods, k):
    gen = _area_golden.generator()
    rec = REC["nms"][k]
    sc = rec["scene"]
    d, p, keep, st = gen.run_scene(sc)
    assert len(d) == rec["n_candidates"]
    ref_keep = refmods.stardist2d().c_non_max_suppression_inds(d, p, 1, 1, 0, np.float32(sc["thr"]))
    assert np.array_equal(keep, ref_keep), np.flatnonzero(keep != ref_keep)[:10]
    got = {"pairs": st[0], "decided": st[9], "deferred_undecided": st[10], "skipped": st[11]}
    print(sc, got)
    assert got == rec["stats"]
    if k == len(REC["nms"]) - 1:
        assert st[10] > 0
