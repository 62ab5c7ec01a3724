"""CPU: the cases and references of the exact rasteriser tests (_raster_cases.py), checked without a GPU.

  * the constants come from the launch code and are what the cases assume (caps, ray and LDS limits);
  * every case reaches the regime it is named for, by a host model of the kernels' clip and loop arithmetic (clip2d, clip3d, lds3d): window
    faces straddled, shapes culled, stack depths, a final painter from beyond the block cap, the LDS byte count on its side of the opt-in;
  * the 2D reference (oracle.port) reproduces the committed scikit-image goldens, whole and through windows as crops;
  * the repeat-based expectation of the polygon-loop case == a plain polygons_to_label_coord run on a reduced instance;
  * compose3d (the reference's label rule on per-polyhedron masks) == the compiled reference on the all-at-once, zero-buffer cases."""
import numpy as np
import pytest

import _raster_cases as RC

K = RC.source_constants()


def test_constants_are_the_ones_the_cases_assume():
    assert K["cap2d"] > 10 ** 6 and K["rays2d"] == 3750 and K["cap3d"] == 8192 and K["hull_rays"] == 800
    assert K["optin3d"] == 64 * 1024 and K["limit3d"] > 2 * K["optin3d"]
    assert set(RC.RAYS2D) >= {RC.THREADS - 1, RC.THREADS, RC.THREADS + 1, 3, 5, 300} and K["rays2d"] > 14 * RC.THREADS
    assert 2 * 8 * K["rays2d"] <= 60000 < 2 * 8 * (K["rays2d"] + 1)


def _faces_cut(lo, hi, live, window):
    """per window face (low, high of every axis): how many live shapes it cuts"""
    out = []
    for a, (w0, wn) in enumerate(zip(*window)):
        s_lo, s_hi = RC.straddles(lo[:, a], hi[:, a], w0, wn)
        out += [int((s_lo & live).sum()), int((s_hi & live).sum())]
    return out


def test_windows2d_regimes():
    coord, labels = RC.windows2d_scene()
    H, W = RC.SHAPE2
    want = RC.windows2d_want()
    assert len(coord) == 150 and coord.shape[2] == 32 and sorted(labels.tolist()) == list(range(150))
    _, culled, ext = RC.clip2d(coord, RC.SHAPE2)
    lo, hi = ext[:, 0::2], ext[:, 1::2]                                                   # float extremes per axis
    assert min(_faces_cut(lo, hi, ~culled, ((0, 0), RC.SHAPE2))) >= 3                        # cut by every image border
    for a, n in enumerate(RC.SHAPE2):                                                     # wholly outside, beyond every border
        assert (hi[:, a] < 0).sum() >= 5 and (lo[:, a] > n).sum() >= 5
    assert ((lo < 0).all(1) & (hi[:, 0] > H) & (hi[:, 1] > W)).sum() >= 3                    # larger than the image
    assert want.any() and (want == 0).any()
    for name, win in RC.WINDOWS2D:
        _, cw, _ = RC.clip2d(coord, RC.SHAPE2, win)
        assert cw.any(), name
        if name == "empty":
            assert not RC.crop(want, win).any() and (~cw).any()                             # boxes reach it, no polygon does
            continue
        assert min(_faces_cut(lo, hi, ~cw, win)) >= 1, (name, _faces_cut(lo, hi, ~cw, win))
        if "pixel" not in name:
            assert RC.crop(want, win).any(), name
    assert RC.crop(want, dict(RC.WINDOWS2D)["pixel"]).item() > 0
    for o, s in RC.BAD_WINDOWS2D:
        assert o[0] < 0 or o[1] < 0 or o[0] + s[0] > H or o[1] + s[1] > W


@pytest.mark.parametrize("name", ("stars32", "stars8_small", "stars64_big", "stars5_int"))
def test_reference2d_reproduces_the_skimage_goldens_through_windows(name):
    coord, labels, shape, gold = RC.golden2d(name)
    got = RC.want2d(coord, labels, shape)
    assert np.array_equal(got, gold), RC.describe(got, gold)
    for win in RC.golden_windows(shape):
        assert np.array_equal(RC.crop(got, win), RC.crop(gold, win)) and RC.crop(gold, win).shape == win[1]


def test_stack2d_regimes():
    from oracle import port
    coord, labs = RC.stack2d()
    masks = RC.stack2d_masks()
    cover = np.zeros(RC.SHAPE2, np.int64)
    for rr, cc in masks:
        cover[rr, cc] += 1
    assert len(coord) == 400 and cover.max() >= RC.STACK2_DEPTH and (RC.crop(cover, RC.STACK2) >= 20).all()
    for name in ("perm", "neg_last"):                                                      # the shared masks paint what the plain loop paints
        assert np.array_equal(RC.paint2d(masks, labs[name]), port.polygons_to_label_coord(coord, RC.SHAPE2, labels=labs[name]))
    assert sorted(labs["perm"].tolist()) == list(range(400)) and len(np.unique(labs["dup"])) == 7
    mid, last = labs["neg_mid"], labs["neg_last"]
    assert (mid == -1).sum() > 30 and mid[-1] != -1 and (mid[150:260] == -1).any() and last[-1] == -1 and last[0] == -1
    img = RC.paint2d(masks, mid)
    assert ((img == 0) & (cover > 0)).any()                                                 # erased and left so ...
    erasers = np.zeros(RC.SHAPE2, bool)
    for (rr, cc), l in zip(masks, mid):
        if l == -1:
            erasers[rr, cc] = True
    assert ((img > 0) & erasers).any()                                                      # ... and erased, then painted again
    rr, cc = masks[-1]
    assert len(rr) > 20 and not RC.paint2d(masks, last)[rr, cc].any()                       # the last painter erases
    # the order matters: reversed painting gives another image
    assert not np.array_equal(RC.paint2d(masks[::-1], labs["perm"][::-1]), RC.paint2d(masks, labs["perm"]))


def test_rays2d_cases():
    for R in RC.RAYS2D + (K["rays2d"],):
        coord, labels = RC.rays2d_case(R)
        want = RC.rays2d_want(R)
        assert coord.shape[1:] == (2, R) and set(np.unique(want).tolist()) >= set((labels[-2:] + 1).tolist())
        _, culled, ext = RC.clip2d(coord, RC.SHAPE2)
        assert not culled.all() and ((ext[:, 0] < 0) | (ext[:, 2] < 0) | (ext[:, 1] > 63) | (ext[:, 3] > 79)).any()


def test_loop2d_expectation_equals_plain_painting_on_a_reduced_instance():
    from oracle import port
    base, assign = RC.loop2d(3000, 300, seed=5, tail=(300, 40))
    coord = base[assign]
    want = port.polygons_to_label_coord(coord, RC.SHAPE2, labels=np.arange(len(coord)))
    got = RC.loop2d_want(base, assign)
    assert np.array_equal(got, want), RC.describe(got, want)
    assert (RC.loop2d_last(assign, 300) >= 0).sum() == len(np.unique(assign)) and got.max() > 2900


def test_loop2d_reaches_beyond_the_block_cap():
    base, assign, want = RC.loop2d_case()
    cap = K["cap2d"]
    assert len(assign) == cap + RC.LOOP2_EXTRA and len(base) == RC.LOOP2_BASE and len(np.unique(base.reshape(len(base), -1), axis=0)) == len(base)
    beyond = want > cap                                                                     # label = painter's index + 1
    assert beyond.sum() > 500 and ((want > 0) & ~beyond).sum() > 500
    one_pass = RC.loop2d_want(base, assign[:cap])                                           # what a single pass of the grid paints
    assert (one_pass != want).sum() == beyond.sum()
    _, culled, _ = RC.clip2d(base, RC.SHAPE2)
    assert culled.any() and not culled[assign[cap:]].all()


# ---- 3D ------------------------------------------------------------------------------------------------------------------------------------
def test_windows3d_regimes(refmods):
    d, p, labels, below = RC.windows3d_scene()
    V, F = RC.rays("golden32")
    S = RC.SHAPE3
    assert len(d) == 50 and d.shape[1] == 32 and sorted(labels.tolist()) == list(range(1, 51)) and below.sum() == 4
    _, culled, raw, unsafe = RC.clip3d(d, p, V, S)
    lo, hi = raw[:, 0::2], raw[:, 1::2]
    assert not unsafe.any()
    assert min(_faces_cut(lo, hi, ~culled, ((0, 0, 0), S))) >= 2                              # clipped by every face of the volume
    assert (hi[below] < 0).any(1).all() and culled[below].all() and not (hi[~below] < 0).any()
    assert (lo > np.asarray(S) - 1).any(1).sum() >= 6                                         # wholly beyond the upper faces
    assert ((lo < 0).all(1) & (hi > np.asarray(S) - 1).all(1)).sum() >= 3                     # boxes larger than the volume
    for mode in (0, 1):
        want = RC.windows3d_want(refmods, mode)
        assert want.dtype == np.int32 and want.shape == S
        for name, win in RC.WINDOWS3D:
            _, cw, _, _ = RC.clip3d(d, p, V, S, win)
            assert cw.sum() > below.sum(), name
            if name == "empty":
                assert not RC.crop(want, win).any() and (~cw).any()
                continue
            assert min(_faces_cut(lo, hi, ~cw, win)) >= 1, (name, _faces_cut(lo, hi, ~cw, win))
            if name not in ("voxel", "line-y"):
                assert RC.crop(want, win).any(), (name, mode)
    for o, s in RC.BAD_WINDOWS3D:
        assert any(o[a] < 0 or o[a] + s[a] > S[a] for a in range(3))


def test_far3d_takes_the_unsafe_path(refmods):
    d, p, labels = RC.far3d_scene()
    V, F = RC.rays("golden32")
    _, _, raw, unsafe = RC.clip3d(d, p, V, RC.FAR_SHAPE)
    beyond = p[:, 0] >= RC.UNSAFE
    assert beyond.sum() == 12 and unsafe[beyond].all()
    assert (unsafe & ~beyond).sum() == 3 and (~unsafe).sum() == 3                             # vertices beyond 8192 only; wholly below it
    want = RC.far3d_want(refmods)
    assert want.shape == RC.FAR_SHAPE == (8300, 24, 24)
    for (name, win), who in zip(RC.FAR_WINDOWS, (beyond, ~beyond)):
        assert win[1] == (40, 24, 24) and set(np.unique(RC.crop(want, win)).tolist()) >= set(labels[who].tolist()), name
        _, cw, _, _ = RC.clip3d(d, p, V, RC.FAR_SHAPE, win)
        assert cw.any() and not cw[who].any()
    assert dict(RC.FAR_WINDOWS)["far"] == ((8240, 0, 0), (40, 24, 24))


@pytest.mark.parametrize("mode", (0, 1))
def test_compose3d_equals_the_compiled_reference(refmods, mode):
    d, p, labs = RC.labels3d_scene()
    V, F = RC.rays("golden32")
    masks = RC.labels3d_masks(refmods, mode)
    cover = np.sum(masks, 0)
    assert len(masks) == 60 and cover.max() >= RC.STACK3_DEPTH and (cover >= 2).mean() > 0.2 and (cover == 1).any() and (cover == 2).any()
    zero = np.zeros(RC.SHAPE3L, np.int32)
    for name in ("perm", "dup", "neg"):
        for ov in RC.OVERLAPS:
            o = RC.overlap_value(ov, labs[name])
            want = RC.ref3d(refmods, d, p, V, F, labs[name], mode, RC.SHAPE3L, overlap=o)
            got = RC.compose3d(masks, labs[name], o, zero)
            assert np.array_equal(got, want), (name, ov, RC.describe(got, want))
    assert (labs["neg"] < 0).sum() > 10 and len(np.unique(labs["dup"])) == 5 and sorted(labs["perm"].tolist()) == list(range(1, 61))


def test_labels3d_degenerate_cases_differ_from_the_plain_ones(refmods):
    """what the compiled reference cannot be asked: the composition on a pre-filled buffer and with zero labels really takes another turn"""
    _, _, labs = RC.labels3d_scene()
    masks = RC.labels3d_masks(refmods, 0)
    zero, pre = np.zeros(RC.SHAPE3L, np.int32), RC.prefill3d()
    plain = RC.compose3d(masks, labs["perm"], None, zero)
    on_pre = RC.compose3d(masks, labs["perm"], None, pre)
    painted = np.any(masks, 0)
    assert (pre != 0).mean() > 0.5 and (pre < 0).any() and ((pre == 0) & painted).any() and ((pre != 0) & painted).any()
    assert np.array_equal(on_pre[pre != 0], pre[pre != 0]) and np.array_equal(on_pre[pre == 0], plain[pre == 0])
    with_ov = RC.compose3d(masks, labs["perm"], 77, pre)
    assert (with_ov[(pre != 0) & painted] == 77).all() and np.array_equal(with_ov[~painted], pre[~painted])
    for name in ("zero_first", "zero_mid", "zero_last"):
        lab = labs[name]
        z = np.flatnonzero(lab == 0)
        assert len(z) >= 1
        got = RC.compose3d(masks, lab, None, zero)
        sub = RC.compose3d(masks, np.where(lab == 0, 12345, lab), None, zero)
        if name != "zero_last":
            assert ((sub == 12345) & (got != 0)).any()                                        # a zero label leaves the voxel open for a later polyhedron
        assert ((sub == 12345) & (got == 0)).any()
    assert {"zero_first": 0, "zero_last": 59}.items() <= {k: int(np.flatnonzero(labs[k] == 0)[0]) for k in ("zero_first", "zero_last")}.items()
    ov0 = RC.compose3d(masks, labs["perm"], 0, zero)
    assert ((ov0 == 0) & painted).any() and not np.array_equal(ov0 != 0, plain != 0)


def test_rays3d_lds_sides():
    seen = set()
    for R, mode in RC.RAYS3D:
        V, F = RC.rays("golden%d" % R)
        assert len(V) == R and R > RC.THREADS and 3 * len(F) > RC.THREADS
        lds = RC.lds3d(R, len(F), mode)
        seen.add((R, mode, lds > K["optin3d"]))
        assert lds <= K["limit3d"]
    assert seen == {(257, 0, False), (257, 1, False), (300, 0, False), (300, 1, False), (300, 2, False), (420, 0, True), (420, 2, True), (672, 1, True)}
    assert RC.lds3d(420, len(RC.rays("golden420")[1]), 1) <= K["optin3d"]                     # at 420 rays it is the hull's share that passes 64 KiB
    assert RC.lds3d(400, len(RC.rays("golden400")[1]), 0) <= K["optin3d"] < RC.lds3d(401, len(RC.rays("golden401")[1]), 0)
    assert RC.lds3d(657, len(RC.rays("golden657")[1]), 1) <= K["optin3d"] < RC.lds3d(658, len(RC.rays("golden658")[1]), 1)
    R = K["hull_rays"] + 1
    assert RC.lds3d(R, len(RC.rays("golden%d" % R)[1]), 0) <= K["limit3d"]                    # 801 rays fit the LDS: it is the hull limit that raises
    assert RC.lds3d(RC.OVER_LIMIT_RAYS, len(RC.rays("golden%d" % RC.OVER_LIMIT_RAYS)[1]), 1) > K["limit3d"]
    for R, _ in RC.RAYS3D:
        d, p, lab = RC.rays3d_case(R)
        _, culled, raw, unsafe = RC.clip3d(d, p, RC.rays("golden%d" % R)[0], RC.SHAPE3R)
        assert 6 <= len(d) <= 10 and not culled.any() and not unsafe.any() and ((raw[:, 0::2] < 0) | (raw[:, 1::2] > 39)).any()


@pytest.mark.parametrize("mode", (0, 1))
def test_loop3d_reaches_beyond_the_block_cap(refmods, mode):
    d, p, lab = RC.loop3d_case()
    cap = K["cap3d"]
    assert len(d) == cap + RC.LOOP3_EXTRA and d.shape[1] == 6 and d.min() >= 1.5 and d.max() <= 3 and np.array_equal(lab, np.arange(1, len(d) + 1))
    want = RC.loop3d_want(refmods, mode)
    beyond = want > cap                                                                       # label = painter's index + 1: the FIRST painter comes from beyond the cap
    assert beyond.sum() > 500 and ((want > 0) & ~beyond).sum() > 500
    one_pass = RC.ref3d(refmods, d[:cap], p[:cap], *RC.rays("octo1"), lab[:cap], mode, RC.SHAPE3R)
    assert np.array_equal(one_pass != want, beyond)
