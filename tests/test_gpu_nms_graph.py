"""The greedy schedulers of the 2D and 3D NMS (csrc/nms2d.hip, csrc/nms3d.hip: parallel rounds, persistent waits, deferred pairs, the
speculative tail batch and its device-side replay) on scenes whose suppression graph is known by construction (tests/_nms_graph_cases.py,
proven against the compiled reference in tests/test_cpu_nms_graph_cases.py): dependency chains as deep as the scene, one candidate with
thousands of neighbours, cliques, ladders, and thousands of short chains in one tail batch.  The margins of every pair are wide, so a
difference can only come from the scheduler.  Keep flags are compared exactly -- no exempt candidate, no tolerance -- with the constructed
flags and with the compiled reference's; the returned statistics prove that each scene reached the regime it was built for.

Sizes, rounds, neighbour entries and times of one run on an MI355X: profiles/nms_graph_tests.txt."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nms_graph_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

_REF = {}
_DEFAULT = {}


def _ref(refmods, key):
    """the compiled reference's flags (default flags: kd-tree and bounding boxes on), once per process; None for the 3D scenes the CPU test
    does not take either"""
    if key not in _REF:
        sc = C.scene(key)
        if sc.dim == 2:
            refmods.set_threads(8)
            _REF[key] = np.asarray(refmods.stardist2d().c_non_max_suppression_inds(sc.dist, sc.points, 1, 1, 0, sc.thr), bool)
        elif sc.n <= C.REF_MAX_3D:
            V, F = sc.rays()
            refmods.set_threads(1)
            _REF[key] = np.asarray(refmods.stardist3d().c_non_max_suppression_inds(sc.dist, sc.points, V, F, sc.scores, 1, 1, 0, sc.thr), bool)
        else:
            _REF[key] = None
    return _REF[key]


def _run(key, opt=None, flags=(1, 1)):
    """keep flags (numpy bool), stats, seconds of one call with one option changed"""
    import torch
    from stardist_amd.lib import _native as N, stardist2d as sd2, stardist3d as sd3
    sc = C.scene(key)

    def call():
        if sc.dim == 2:
            return sd2.c_non_max_suppression_inds(sc.dist, sc.points, flags[0], flags[1], 0, sc.thr, return_stats=True)
        dev = torch.device("cuda:0")
        V, F = sc.rays()
        t = [torch.from_numpy(a).to(dev) for a in (sc.dist, sc.points, V, F, sc.scores)]
        keep, stats = sd3.c_non_max_suppression_inds(t[0], t[1], t[2], t[3], t[4], 1, 1, 0, sc.thr, return_stats=True)
        return keep.cpu().numpy(), stats
    t0 = time.time()
    if opt is None:
        keep, stats = call()
    else:
        with N.option(opt[0], opt[1]):
            keep, stats = call()
    dt = time.time() - t0
    rounds, nbr = (int(stats[2]), int(stats[3])) if sc.dim == 2 else (int(stats[4]), int(stats[5]))
    print("%-46s %-34s flags=%s n=%5d kept=%5d rounds=%5d neighbour entries=%8d %.3f s"
          % (key, "default" if opt is None else "%s=%d" % opt, flags, sc.n, int(keep.sum()), rounds, nbr, dt))
    return np.asarray(keep, bool), stats, dt


def _default_run(key):
    if key not in _DEFAULT:
        _DEFAULT[key] = _run(key)
    return _DEFAULT[key]


def _check(refmods, key, keep):
    sc = C.scene(key)
    diff = np.flatnonzero(keep != sc.keep)
    assert len(diff) == 0, "%s: %d flags differ from the constructed ones, first %s (kept %d, expected %d)" % (key, len(diff), diff[:10], int(keep.sum()), int(sc.keep.sum()))
    ref = _ref(refmods, key)
    if ref is not None:
        assert np.array_equal(keep, ref), (key, np.flatnonzero(keep != ref)[:10])


OPTS_2D = [None, ("nms2d_strict", 1), ("nms2d_area_bounds", 0), ("nms2d_defer_undecided", 0), ("nms2d_defer_undecided", 1),
           ("nms2d_neighbours_single_pass", 0), ("nms2d_neighbours_single_pass", 1)]
OPTS_3D = [None, ("nms3d_tail_batch", 0), ("nms3d_neighbours_single_pass", 0), ("nms3d_neighbours_single_pass", 1),
           ("nms3d_defer_exact", 0), ("nms3d_defer_exact", 1)]


def _id(o):
    return "default" if o is None else "%s=%d" % o


@pytest.mark.parametrize("opt", OPTS_2D, ids=_id)
@pytest.mark.parametrize("key", C.SCENES_2D)
def test_nms2d_flags_exact(refmods, key, opt):
    keep, stats, dt = _default_run(key) if opt is None else _run(key, opt)
    _check(refmods, key, keep)


@pytest.mark.parametrize("flags", [(1, 1), (0, 0)])
@pytest.mark.parametrize("key", C.CHAINS_2D + C.HUBS_2D)
def test_nms2d_flags_exact_kdtree_bbox(refmods, key, flags):
    """use_kdtree / use_bbox both on and both off (all pairs pass the reference's filters; the designed non-neighbours still overlap below
    the threshold, so the flags are the same)"""
    keep, stats, dt = _run(key, None, flags)
    _check(refmods, key, keep)


@pytest.mark.parametrize("opt", OPTS_3D, ids=_id)
@pytest.mark.parametrize("key", C.SCENES_3D)
def test_nms3d_flags_exact(refmods, key, opt):
    keep, stats, dt = _default_run(key) if opt is None else _run(key, opt)
    _check(refmods, key, keep)
    if opt == ("nms3d_tail_batch", 0) and C.is_monotone_chain(key):
        # plain rounds only: a round promotes the head of the chain and suppresses the next candidate, so N // 2 rounds at least
        # (observed: (N + 2) // 2 -- 2, 21, 201, 261, 1601: the undecided count of a round is read before its suppressions)
        assert stats[4] >= C.scene(key).n // 2, stats[:6]


@pytest.mark.parametrize("key", C.CHAINS_3D)
def test_nms3d_flags_exact_without_volume_bounds(refmods, key):
    keep, stats, dt = _run(key, ("nms3d_volume_bounds", 0))
    _check(refmods, key, keep)


# ---- evidence that each scene reached its regime (default options)
@pytest.mark.parametrize("n", C.CHAIN_N_2D)
def test_nms2d_monotone_chain_rounds(refmods, n):
    """A chain decides at most one survivor and one suppressed candidate per round, and the tail batch starts (never in round 1) once
    at most tailT = min(N // 6, 65536) candidates are undecided: stats[2] >= (N - tailT) // 2.  The host loop gives the exact count
    (tests/_nms_graph_cases.py: rounds_2d_monotone): round r promotes one candidate and suppresses the next, but the undecided count it
    reads back was taken before that suppression, so N - (2 r - 1) candidates go on; ceil((N + 1 - tailT) / 2) rounds + the tail batch,
    (N + 2) // 2 rounds where no tail batch starts.  No more than that.  With tailT >= 5 (N >= 30) the count is below (N + 1) // 2:
    ceil((N + 1 - tailT) / 2) + 1 <= (N + 4 - tailT) / 2 < N / 2.  With the flags that means the replay resolved a chain of N // 6
    candidates -- 10 at N = 64, 100 at N = 600, 500 at N = 3000: past the 10 fixed k_tail_step launches, k_tail_resolve did the rest.
    Below N = 30 the tail batch holds at most 4 candidates and saves at most one round, so that upper bound cannot hold there (N = 1: one
    round; N = 2: two, (N + 1) // 2 = 1); the exact count is asserted instead.
    Observed on an MI355X for N = 1, 2, 5, 6, 7, 12, 13, 64, 600, 3000: 1, 2, 3, 4, 4, 7, 7, 29, 252, 1252 rounds -- the exact counts;
    the largest takes 0.12 s."""
    key = [k for k in C.CHAINS_2D if C.is_monotone_chain(k) and C.scene(k).n == n and C.scene(k).n_rays == 32 and "serpentine" not in k][0]
    keep, stats, dt = _default_run(key)
    _check(refmods, key, keep)
    rounds = int(stats[2])
    assert rounds >= (n - min(n // 6, 65536)) // 2, (n, rounds)
    assert rounds <= C.rounds_2d_monotone(n), (n, rounds)
    if n // 6 >= 5:
        assert rounds < (n + 1) // 2, (n, rounds)


@pytest.mark.parametrize("n_rays", [8, 64])
def test_nms2d_monotone_chain_forced_into_the_tail_replay(refmods, n_rays):
    """The monotone chain of 600 with 8 and with 64 rays does NOT take 250 rounds (observed: 4 and 3; trace in profiles/nms_graph_tests.txt).
    8 rays: the area enclosure leaves the octagon pairs undecided (edges 7.7 long: its band is wider than the margin), and from round 2 on a
    round defers its few undecided pairs to the tail batch (nms2d_defer_undecided = 2, k_defer_undecided).  64 rays: no enclosure; 64-gons
    with vertices truncated to integers have collinear edges, the pair needs the general path, which a normal round defers (k_defer).
    Either way candidate 1 resp. 3 is pending, everything behind it waits, the round without progress forces the tail batch (`forceTail`)
    -- and the whole chain, 597 resp. 599 candidates, is resolved by the replay.  The chain is deep somewhere: whatever the host rounds did
    not decide (at most two candidates each), the replay did; that remainder must be far past the 10 fixed k_tail_step launches."""
    key = [k for k in C.CHAINS_2D if C.is_monotone_chain(k) and C.scene(k).n_rays == n_rays][0]
    keep, stats, dt = _default_run(key)
    _check(refmods, key, keep)
    n, rounds = C.scene(key).n, int(stats[2])
    assert rounds >= (n - n // 6) // 2 or n - 2 * rounds > 100, (n, rounds)


def test_nms3d_monotone_chain_of_400_goes_to_the_tail_replay(refmods):
    """tailT = max(N // 32, 512): the 399 candidates still listed after round 1 all go to the tail batch in round 2 (stats[4] <= 3; observed 2),
    whose replay decides one candidate per k_tail3_mark / k_tail3_promote sweep in the worst case: 398 sweeps, 50 passes of the
    `while (left)` loop (its guard allows N / 8 + 4 = 54).  N = 520 and 3200 reach the tail batch with 511 candidates (observed 6 and 1346
    rounds = the N - (2 r - 1) <= 512 of the host loop): 64 passes."""
    key = [k for k in C.CHAINS_3D if C.is_monotone_chain(k) and C.scene(k).n == 400 and C.scene(k).n_rays == 96 and "serpentine" not in k][0]
    keep, stats, dt = _default_run(key)
    _check(refmods, key, keep)
    assert 2 <= stats[4] <= 3, stats[:6]


@pytest.mark.parametrize("key", C.HUBS_2D + C.HUBS_3D)
def test_hub_neighbour_entries_and_rounds(refmods, key):
    """every small candidate inside the hub lists the hub and the hub lists each of them: at least 2 M neighbour entries (observed: 2D
    4000 = 2 M exactly, the bounding boxes of the small ones are disjoint; 3D 7656, the balls' neighbour predicate is a distance); with the hub last it waits for M better-scored neighbours and is decided in a later round
    than they are: at least 2 rounds (observed: 2D 2, 3D 4)"""
    sc = C.scene(key)
    keep, stats, dt = _default_run(key)
    _check(refmods, key, keep)
    rounds, nbr = (int(stats[2]), int(stats[3])) if sc.dim == 2 else (int(stats[4]), int(stats[5]))
    assert nbr >= 2 * sc.m, (key, nbr)
    if sc.big != 0:
        assert rounds >= 2, (key, rounds)


@pytest.mark.parametrize("key", C.HUBS_2D + [k for k in C.OTHERS_2D if k.startswith("forest")])
def test_nms2d_repeatable_in_one_process(refmods, key):
    a = _run(key)[0]
    b = _run(key)[0]
    assert np.array_equal(a, b), np.flatnonzero(a != b)[:10]
    _check(refmods, key, a)


# ---- the legacy NMS: one workgroup replays the greedy order
@pytest.mark.parametrize("max_bbox_search", [0, 1])
@pytest.mark.parametrize("n", [64, 600])
def test_nms2d_old_on_deep_chains(refmods, n, max_bbox_search):
    """c_non_max_suppression_inds_old on the monotone chains: integer polygons around the pixels of the centres and the pixel -> candidate
    mapping, as test_nms2d_old_equals_reference_old_and_new builds them; the reference's old function and the constructed flags"""
    from oracle import port
    from stardist_amd.lib import stardist2d as sd2
    key = [k for k in C.CHAINS_2D if C.is_monotone_chain(k) and C.scene(k).n == n and C.scene(k).n_rays == 32 and "serpentine" not in k][0]
    sc = C.scene(key)
    pix = np.floor(sc.points).astype(np.int64)
    polys = np.ascontiguousarray(port.dist_to_coord(sc.dist, pix).astype(np.int32))
    if max_bbox_search:
        mapping = -np.ones(tuple(pix.max(0) + 16), np.int32)
        mapping[pix[:, 0], pix[:, 1]] = np.arange(n)
    else:
        mapping = np.empty((0, 0), np.int32)
    refmods.set_threads(8)
    args = (polys, mapping, sc.thr, np.int32(max_bbox_search), np.int32(1), np.int32(1), np.int32(0))
    ref_old = np.asarray(refmods.stardist2d().c_non_max_suppression_inds_old(*args), bool)
    t0 = time.time()
    mine = sd2.c_non_max_suppression_inds_old(*args)
    print("old NMS, chain of %d, max_bbox_search=%d: %.3f s" % (n, max_bbox_search, time.time() - t0))
    assert np.array_equal(ref_old, sc.keep), np.flatnonzero(ref_old != sc.keep)[:10]
    assert mine.dtype == bool and np.array_equal(mine, sc.keep), np.flatnonzero(mine != sc.keep)[:10]
