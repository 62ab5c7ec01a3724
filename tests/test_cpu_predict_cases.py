"""CPU: the preconditions of the exact prediction tests (test_gpu_predict_exact.py) on the cases, data and references of _predict_cases.py --
the integer family is exact (float32 == float64 up to the features and for the distances, integer logits, small activations, a dozen
probability values on both sides of 0.5), the cases reach what they are for (padding, cut tiles, more tile shapes than the graph cache
holds, destination regions that partition the image), tiled == untiled holds with `==` on the CPU model for the integer and the shift
networks, and the comparison CAN fail: with the tile overlap shortened below the measured reach the shift network of that axis differs.

The CPU model's heads are torch's sigmoid / softmax; P.scalar_heads makes them functions of the value alone (see there)."""
import numpy as np
import pytest
import torch

import _predict_cases as P

NAMES = [c.name for c in P.CASES]
AXIS_SIGN_2D = [(0, 1), (0, -1), (1, 1), (1, -1)]
AXIS_SIGN_3D = [(0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1)]          # on slabs (P.slab): cheap enough for both directions
# a boundary pixel of a strided convolution's tile is one its extreme tap never reads (measure_reach gives 0 there): the ResNet's negative
# control runs in the direction in which the first pixel beyond a read region is read
NEGATIVE_3D = [(0, 1), (1, 1), (2, 1)]


@pytest.fixture(autouse=True)
def _threads():
    with P.cpu_threads():
        yield


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and u.dtype == v.dtype
        if not np.array_equal(u, v):
            bad = np.argwhere(u != v)
            pytest.fail("%s: output %d differs at %d of %d elements, first %s: %r vs %r" % (
                what, k, len(bad), u.size, tuple(bad[0]), u[tuple(bad[0])], v[tuple(bad[0])]))


_REF = {}


def _ref(name):
    """(model, image, reference, untiled prediction) of the integer family, once per case"""
    if name not in _REF:
        case = P.BY_NAME[name]
        m = P.integer_model(case)
        img = P.integer_image(case)
        with P.scalar_heads():
            pred = m.predict(img, axes=case.axes)
        _REF[name] = (m, img, P.reference(m, img, case.axes), pred)
    return _REF[name]


@pytest.mark.parametrize("name", NAMES)
def test_integer_family_is_exact(name):
    case = P.BY_NAME[name]
    m, img, ref, pred = _ref(name)
    f32, f64 = ref["f32"], ref["f64"]
    for k in ("features", "logit", "dist", "class_logit"):
        if f64[k] is not None:
            assert torch.equal(f32[k].double(), f64[k]), k
    assert f64["peak"] <= 2048 and f32["peak"] == f64["peak"]
    lg = f64["logit"]
    assert bool((lg == lg.round()).all()) and bool((f64["dist"] == f64["dist"].round()).all())
    # the prediction of the CPU model: the crop of the pad, the clamp
    shape = P.spatial_shape(case)
    grid = m.config.grid
    assert pred[0].shape == tuple(-(-s // g) for s, g in zip(shape, grid)) == ref["logit"].shape
    assert np.array_equal(pred[1].astype(np.float64), ref["dist"])
    assert float(pred[1].min()) == float(np.float32(1e-3)) and float(pred[1].max()) >= 2
    assert np.abs(pred[0].astype(np.float64) - ref["prob"]).max() <= 1e-7
    if case.cfg.get("n_classes"):
        assert np.abs(pred[2].astype(np.float64) - ref["prob_class"]).max() <= 1e-7
    # a dozen probabilities, on both sides of 0.5
    vals = np.unique(pred[0])
    assert int(((vals > 0) & (vals < 1)).sum()) >= 6
    assert (ref["logit"] > 0).mean() >= 0.01 and (ref["logit"] < 0).mean() >= 0.01
    # equal logits, equal probability bits (the function of the value alone the GPU tests ask of the head kernel)
    for v in np.unique(ref["logit"]):
        assert len(np.unique(pred[0][ref["logit"] == v])) == 1


@pytest.mark.parametrize("name", NAMES)
def test_cases_reach_what_they_are_for(name):
    case = P.BY_NAME[name]
    m = P.make_model(case)
    padded, blocks, tiles = P.plan(m, case)
    shape, n_tiles = P.spatial_shape(case), P.tiles_spatial(case)
    nd = len(shape)
    assert all(p % b == 0 and 0 <= p - s < b for p, s, b in zip(padded, shape, blocks))
    if name == "padded2d":
        assert all(p > s for p, s in zip(padded, shape))
    else:
        assert padded == shape
    if name == "many2d":
        assert len(set(P.tile_shapes(tiles))) >= 10 > 8 and len(tiles) <= 24
        assert any(n > p // b for n, p, b in zip(n_tiles, padded, blocks))                     # _tile_slices clamps n to the blocks
        want = tuple(min(n, p // b) for n, p, b in zip(n_tiles, padded, blocks))
    else:
        want = n_tiles
    assert len(tiles) == int(np.prod(want))
    # destination regions tile the padded image exactly once; the source region of a tile is its destination
    cover = np.zeros(padded, np.int32)
    for tile, src, dst in tiles:
        cover[dst] += 1
        for t, s, d in zip(tile, src, dst):
            assert t.start + s.start == d.start and t.start + s.stop == d.stop and t.start <= d.start and d.stop <= t.stop
    assert int(cover.min()) == 1 == int(cover.max())
    # every multi-tile axis has the full overlap cut off on either side: by ONE tile where the axis has three or more (with two tiles
    # each is cut on one side), and tiles that touch the image's edges.  (many2d is about tile SHAPES: its image is smaller than two overlaps)
    overlap = m._axes_tile_overlap(m.config.axes.replace("C", ""))
    for d in range(nd):
        if want[d] == 1 or name == "many2d":
            continue
        spans = sorted(set((t[0][d].start, t[0][d].stop, t[2][d].start, t[2][d].stop) for t in tiles))
        ovb = -(-overlap[d] // blocks[d]) * blocks[d]
        full_lo = [s for s in spans if s[0] > 0 and s[2] - s[0] == ovb]
        full_hi = [s for s in spans if s[1] < padded[d] and s[1] - s[3] == ovb]
        assert full_lo and full_hi, (name, d, spans)
        if want[d] >= 3:
            assert set(full_lo) & set(full_hi), (name, d, spans)
        assert any(s[0] == 0 for s in spans) and any(s[1] == padded[d] for s in spans)


@pytest.mark.parametrize("name", NAMES)
def test_tiled_equals_untiled_integer(name):
    case = P.BY_NAME[name]
    m, img, ref, pred = _ref(name)
    with P.scalar_heads():
        tiled = m.predict(img, axes=case.axes, n_tiles=case.n_tiles)
    _same(tiled, pred, "%s tiled %s" % (name, case.n_tiles))


def _shift_params():
    out = []
    for c in P.CASES:
        for axis, sign in (AXIS_SIGN_2D if c.nd == 2 else AXIS_SIGN_3D):
            out.append(pytest.param(c.name, axis, sign, id="%s-axis%d%s" % (c.name, axis, "+" if sign > 0 else "-")))
    return out


def _negative_params():
    out = []
    for c in P.CASES:
        for axis, sign in (AXIS_SIGN_2D if c.nd == 2 else NEGATIVE_3D):
            out.append(pytest.param(c.name, axis, sign, id="%s-axis%d%s" % (c.name, axis, "+" if sign > 0 else "-")))
    return out


_SHIFT = {}


def _shift(name, axis, sign):
    """(model, reach per position in a block) of a shift network, once"""
    key = (name, axis, sign)
    if key not in _SHIFT:
        m = P.shift_model(P.BY_NAME[name], axis, sign)
        _SHIFT[key] = (m, P.measure_reach(m, axis, sign))
    return _SHIFT[key]


@pytest.mark.parametrize("name,axis,sign", _shift_params())
def test_tiled_equals_untiled_shift_and_reach_within_bound(name, axis, sign):
    case = P.BY_NAME[name]
    m, reaches = _shift(name, axis, sign)
    bound = m._receptive_field_radius()[axis]
    assert 0 < max(reaches) <= bound, (reaches, bound)
    if case.nd == 3:
        case = P.slab(case, axis)
    if P.tiles_spatial(case)[axis] == 1:
        return
    img = P.shift_image(m, case, axis, sign, max(reaches))
    padded, _, tiles = P.plan(m, case)
    cut = any((t[0][axis].stop < padded[axis]) if sign > 0 else (t[0][axis].start > 0) for t in tiles)
    assert bool((img > 0).any()) == cut
    if not cut:                                                     # (a side no tile is cut on has nothing to probe)
        return
    with P.scalar_heads():
        whole = m.predict(img, axes=case.axes)
        tiled = m.predict(img, axes=case.axes, n_tiles=case.n_tiles)
    assert float(whole[1].max()) >= 1                               # the impulses arrive at the distance head
    _same(tiled, whole, "%s shift axis %d sign %d" % (case.name, axis, sign))


@pytest.mark.parametrize("name,axis,sign", _negative_params())
def test_negative_control_a_short_overlap_is_seen(name, axis, sign):
    """the overlap of one axis patched to the largest multiple of div_by below the reach measured at a tile edge: the shift network of that
    axis must differ between tiled and untiled"""
    case = P.BY_NAME[name]
    if case.nd == 3:
        case = P.slab(case, axis)
    if P.tiles_spatial(case)[axis] == 1:
        return
    m0, reaches = _shift(name, axis, sign)
    reach = P.boundary_reach(reaches, sign)
    assert reach > 0
    m = P.shift_model(case, axis, sign)
    block = m._axes_div_by(m.config.axes.replace("C", ""))[axis]
    short = (reach - 1) // block * block
    assert short < reach <= m._receptive_field_radius()[axis]
    P.shortened_overlap(m, axis, short)
    assert m._axes_tile_overlap(m.config.axes)[axis] == short
    img = P.shift_image(m, case, axis, sign, max(reaches))
    with P.scalar_heads():
        whole = m.predict(img, axes=case.axes)
        tiled = m.predict(img, axes=case.axes, n_tiles=case.n_tiles)
    assert not np.array_equal(whole[1], tiled[1]), "a tile overlap of %d against a reach of %d went unnoticed" % (short, reach)
    # ... and it is the overlap: the same image, the model's own overlap
    del m._axes_tile_overlap
    with P.scalar_heads():
        _same(m.predict(img, axes=case.axes, n_tiles=case.n_tiles), whole, "%s with its own overlap" % case.name)


def test_sparse_statement_by_hand():
    """P.sparse_numpy on a grid worked out by hand: 4 x 6 grid cells of a padded 8 x 12 image with grid (2, 2), of which 7 x 9 pixels are
    image (the dense prediction keeps 4 x 5 cells: one padded column cropped, the cells of column 4 start at x = 8 < 9)"""
    prob = np.full((4, 5), 0.25, np.float32)
    prob[0, 0] = prob[1, 1] = prob[2, 4] = prob[3, 2] = prob[1, 3] = 0.75
    prob[2, 2] = 0.5                                                # not above a threshold of 0.5
    dist = np.tile(np.arange(20, dtype=np.float32).reshape(4, 5, 1) - 5, (1, 1, 3))
    cls = np.arange(40, dtype=np.float32).reshape(4, 5, 2)
    p, d, c, pts = P.sparse_numpy(prob, dist, cls, (2, 2), (8, 12), (7, 9), 0.5, 0)
    assert pts.tolist() == [[0, 0], [2, 2], [2, 6], [4, 8], [6, 4]] and p.tolist() == [0.75] * 5
    assert d[:, 0].tolist() == [np.float32(1e-3), 1.0, 3.0, 9.0, 12.0] and c[:, 0].tolist() == [0.0, 12.0, 16.0, 28.0, 34.0]
    # a border of one cell of the PADDED grid (4 x 6): row 0 and row 3 go, column 0 goes, column 4 stays (the padded grid's last is 5)
    assert P.sparse_numpy(prob, dist, cls, (2, 2), (8, 12), (7, 9), 0.5, 1)[3].tolist() == [[2, 2], [2, 6], [4, 8]]
    assert P.sparse_numpy(prob, dist, cls, (2, 2), (8, 12), (7, 9), 0.5, 2)[3].tolist() == []
    # points of the pad go: an image of 7 x 8 pixels ends before x = 8
    assert P.sparse_numpy(prob, dist, cls, (2, 2), (8, 12), (7, 8), 0.5, 0)[3].tolist() == [[0, 0], [2, 2], [2, 6], [6, 4]]
