"""The neighbour lists of the NMS (csrc/nms_rounds.h: build_neighbour_lists, shared by 2D and 3D) at and past their 32-bit limits.

The single-pass lists give every candidate a slot as large as the population of the cells its list is built from; one large candidate
among many small ones puts the whole set into a handful of cells, and the slot total becomes about n^2.  The hubs of
tests/_nms_graph_cases.py (SLOT_LIMIT_2D; keep flags known by construction, proven against the compiled reference in
tests/test_cpu_nms_graph_cases.py) place that total, computed exactly by the numpy mirror tests/_nms2d_np.py: slot_capacities,

  below2d  just below 2^31 - 1: the slots, 8.6 GB of them;
  band2d   in [2^31, 2^32): the fall-back to the two-pass lists, reached by size alone;
  wrap2d   past 2^32, where a sum in the counts' own 32 bits returns a plausible total: T - 2^32.

In front of them the exclusive sum itself (sd_exclusive_sum_i32_i64_device, the one scan behind every total) against numpy's int64 cumsum,
and behind them the two "exceed the capacity of one call" errors on cliques whose list entries pass 2^31 and 2^32.  The order of the
file is the order of risk: the scan indexes nothing with its result; below2d and band2d were within the range checks before the sum
was 64-bit; wrap2d and the cliques rely on it.

stats[12] (slot total) and stats[13] (form: 1 slots, 0 two passes) of sd_nms2d_device prove the regime.  3D: sd_nms3d_device uses all 16
entries of its statistics, so the regime cannot be observed there; the builder and the scan are the ones tested here.

Every test frees the workspace at its end (sd_release_workspace): the arena only grows, and these calls grow it to gigabytes.
Sizes, totals, forms and times of one run on an MI355X: profiles/nms_graph_tests.txt."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nms2d_np as M  # noqa: E402
import _nms_graph_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

SINGLE = "nms2d_neighbours_single_pass"
OPTS = [None, (SINGLE, 0), (SINGLE, 1)]
_MIRROR = {}


def _id(o):
    return "default" if o is None else "%s=%d" % o


@pytest.fixture
def workspace():
    from stardist_amd.lib import _native as N
    yield
    N.lib().sd_release_workspace()


# ---- the scan
def _scan_counts(name):
    rng = np.random.RandomState(7)
    if name == "flat":                                   # 5 000 counts of 2^20: 5.2 10^9, past 2^32
        return np.full(5000, 1 << 20, np.int32)
    if name == "random":                                 # counts up to 2^31 - 1: every partial sum but the first few is past 2^32
        return rng.randint(0, 2 ** 31, 5000, dtype=np.int64).astype(np.int32)
    if name == "one":
        return np.array([2 ** 31 - 1], np.int32)
    assert name == "blocks"                              # many workgroups of the scan: the carry between them is 64-bit as well
    return rng.randint(0, 2 ** 31, 300003, dtype=np.int64).astype(np.int32)


@pytest.mark.parametrize("name", ["flat", "random", "one", "blocks"])
def test_exclusive_sum_of_int_counts_is_64_bit(workspace, name):
    """d_out[k] = sum of d_in[0 .. k) exactly, in int64: the last start of "flat" is 4 999 * 2^20 = 5 241 831 424 > 2^32.  (hipcub's
    ExclusiveSum over the same ints sums in 32 bits whatever the output type: its accumulator is the input's value type.)"""
    import torch
    from stardist_amd.lib import _native as N
    counts = _scan_counts(name)
    want = np.concatenate([[0], np.cumsum(counts.astype(np.int64))[:-1]])
    if name != "one":
        assert want[-1] > 2 ** 32
    d_in = torch.from_numpy(counts).to("cuda:0")
    d_out = torch.full((len(counts),), -1, dtype=torch.int64, device="cuda:0")
    N.dcall(d_in, "sd_exclusive_sum_i32_i64_device", N.tptr(d_in), len(counts), N.tptr(d_out))
    got = d_out.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (name, bad[:5], got[bad[:5]], want[bad[:5]])


# ---- the mirror, on the small scenes: grids of many cells, windows that cover a part of them
@pytest.mark.parametrize("key", ["chain2d(3000)", "chain2d(600,layout=serpentine)", "ladder2d(600)", "clique2d(300)", "forest2d(6000)"] + C.HUBS_2D)
@pytest.mark.parametrize("mode", ["bbox", "radius"])
def test_slot_total_equals_the_mirror(workspace, key, mode):
    """stats[12] = the sum of tests/_nms2d_np.py: slot_capacities, exactly, in either form of the lists; mode "radius": threshold -1 and the
    k-d tree alone, the window of a centre +- 2 reach instead of a bounding box grown by the reach"""
    from stardist_amd.lib import _native as N, stardist2d as sd2
    sc = C.scene(key)
    kd, bbox, thr = (1, 1, sc.thr) if mode == "bbox" else (1, 0, np.float32(-1))
    want = M.slot_capacities(sc.dist, sc.points, thr, use_bbox=bbox)["total"]
    for single in (1, 0):
        with N.option(SINGLE, single):
            keep, stats = sd2.c_non_max_suppression_inds(sc.dist, sc.points, kd, bbox, 0, thr, return_stats=True)
        assert int(stats[12]) == want and int(stats[13]) == single, (key, mode, single, stats[12:14], want)
        if mode == "bbox":
            assert np.array_equal(keep, sc.keep)


# ---- the hubs
def _mirror(key):
    if key not in _MIRROR:
        sc = C.scene(key)
        _MIRROR[key] = M.slot_capacities(sc.dist, sc.points, sc.thr)["total"]
    return _MIRROR[key]


def _run(key, opt):
    from stardist_amd.lib import _native as N, stardist2d as sd2
    sc = C.scene(key)
    t0 = time.time()
    if opt is None:
        keep, stats = sd2.c_non_max_suppression_inds(sc.dist, sc.points, 1, 1, 0, sc.thr, return_stats=True)
    else:
        with N.option(opt[0], opt[1]):
            keep, stats = sd2.c_non_max_suppression_inds(sc.dist, sc.points, 1, 1, 0, sc.thr, return_stats=True)
    dt = time.time() - t0
    print("%-42s %-34s n=%6d kept=%6d rounds=%3d neighbour entries=%7d slot total=%11d form=%s %.3f s"
          % (key, _id(opt), sc.n, int(keep.sum()), int(stats[2]), int(stats[3]), int(stats[12]), "slots" if stats[13] else "two passes", dt))
    return np.asarray(keep, bool), stats


def _check(refmods, key, opt, slots):
    sc = C.scene(key)
    keep, stats = _run(key, opt)
    diff = np.flatnonzero(keep != sc.keep)
    assert len(diff) == 0, "%s: %d flags differ from the constructed ones, first %s (kept %d, expected %d)" % (key, len(diff), diff[:10], int(keep.sum()), int(sc.keep.sum()))
    if sc.n <= C.REF_MAX_2D:
        refmods.set_threads(8)
        ref = np.asarray(refmods.stardist2d().c_non_max_suppression_inds(sc.dist, sc.points, 1, 1, 0, sc.thr), bool)
        assert np.array_equal(keep, ref), (key, np.flatnonzero(keep != ref)[:10])
    assert int(stats[12]) == _mirror(key) == C.SLOT_TOTALS[key], (key, int(stats[12]), _mirror(key), C.SLOT_TOTALS[key])
    assert int(stats[13]) == int(slots), (key, opt, stats[12:14])
    # the hub and each of the m small candidates inside it list each other, and nothing else does (the small ones have pairwise
    # disjoint bounding boxes, the outer ones lie outside the hub's: labelings, proven in the CPU test): 2 m ordered relations
    assert int(stats[3]) == 2 * sc.m, (key, int(stats[3]), sc.m)


@pytest.mark.parametrize("opt", OPTS, ids=_id)
def test_below2d_takes_the_slots(refmods, workspace, opt):
    """slot total 8.7 10^6 below 2^31 - 1: the slots, unless the two-pass form is asked for"""
    assert C.SLOT_LIMIT - 2 * 10 ** 7 < C.SLOT_TOTALS[C.BELOW_2D] <= C.SLOT_LIMIT - 5 * 10 ** 6
    _check(refmods, C.BELOW_2D, opt, slots=opt != (SINGLE, 0))


@pytest.mark.parametrize("opt", OPTS, ids=_id)
@pytest.mark.parametrize("key", C.BAND_2D)
def test_band2d_falls_back_to_two_passes(refmods, workspace, key, opt):
    """slot total in [2^31, 2^32): two passes whatever the option says"""
    assert 2 ** 31 + 5 * 10 ** 6 <= C.SLOT_TOTALS[key] <= 2 ** 32 - 10 ** 9
    _check(refmods, key, opt, slots=False)


@pytest.mark.parametrize("opt", OPTS, ids=_id)
def test_wrap2d_falls_back_to_two_passes(refmods, workspace, opt):
    """slot total T = 2^32 + 5.0 10^8: two passes.  (Summed in 32 bits T came back as 501 664 188, inside every range check.)"""
    assert 10 ** 8 <= C.SLOT_TOTALS[C.WRAP_2D] - 2 ** 32 <= 2 ** 31 - 10 ** 8
    _check(refmods, C.WRAP_2D, opt, slots=False)


# ---- more list entries than one call holds
@pytest.mark.parametrize("k", [66000, 93000])
def test_capacity_errors_name_the_true_count(workspace, k):
    """k near-coincident candidates: every pair passes the neighbour predicate, so the lists would hold k (k - 1) / 2 entries -- 2.18 10^9
    in [2^31, 2^32) and 4.32 10^9 past 2^32.  sd_nms2d_device (slot totals k (k - 1) > 2^32: the counting pass of the two-pass form) and
    sd_nms2d_old_device without max_bbox_search (every j > i whose bounding box meets i's) refuse the call and name the true count.
    Only the counting passes run."""
    from oracle import port
    from stardist_amd.lib import _native as N, stardist2d as sd2
    sc = C.clique(2, k, list_edges=False)
    pairs = k * (k - 1) // 2
    assert pairs >= (2 ** 31 if k == 66000 else 2 ** 32)
    t0 = time.time()
    with pytest.raises(N.NativeError) as e:
        sd2.c_non_max_suppression_inds(sc.dist, sc.points, 1, 1, 0, sc.thr)
    t1 = time.time()
    msg = str(e.value)
    assert "sd_nms2d: %d neighbour entries for %d candidates exceed the capacity of one call" % (pairs, k) in msg, msg
    polys = np.ascontiguousarray(port.dist_to_coord(sc.dist, np.floor(sc.points).astype(np.int64)).astype(np.int32))
    t2 = time.time()
    with pytest.raises(N.NativeError) as e:
        sd2.c_non_max_suppression_inds_old(polys, np.empty((0, 0), np.int32), sc.thr, np.int32(0), np.int32(1), np.int32(1), np.int32(0))
    msg = str(e.value)
    print("clique of %d: %d pairs; sd_nms2d refused in %.3f s, sd_nms2d_old in %.3f s" % (k, pairs, t1 - t0, time.time() - t2))
    assert "sd_nms2d_old: %d candidate pairs exceed the capacity of one call" % pairs in msg, msg
