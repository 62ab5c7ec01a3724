"""GPU: the prediction driver around the network (stardist_amd/models/base.py), exactly.  With the integer weights and inputs of
_predict_cases.py every activation, distance and probability logit is a small integer -- the same float32 in any summation order, kernel form
and tile position (test_cpu_predict_cases.py holds the preconditions) -- so the comparisons are `==`:

  1  untiled predict == the CPU evaluation of the module graph (distances: the clamp and the crop of the pad included); the probabilities within
     2e-6 of the float64 sigmoid / softmax of the integer logits (the bound test_gpu_heads.py holds the head kernels to), and a function of
     the logit alone
  2  tiled == untiled bit for bit, for the integer family and for the shift networks on images built from the tile plan
  3  predict_sparse, untiled and tiled, == the numpy statement (P.sparse_numpy) of the GPU's own dense prediction
  4  the HIP-graph cache: more tile shapes in one call than it holds, replays, interleaved images == a model that never captures
  5  the lazy-features knobs take effect after a capture, and change no bit
  6  predict_instances through the presorted sparse path == through the dense path, with a dozen score values among thousands of candidates

Buffers the package allocates are poisoned (nan_empty).  The default conv mode throughout; plain2d also on the exact-f32 kernels and
without split16 activations."""
import contextlib

import numpy as np
import pytest
import torch

import _predict_cases as P
from _exact import nan_empty

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = [c.name for c in P.CASES]
VARIANTS = NAMES + ["plain2d-hand", "plain2d-nosplit"]
SHIFTS_3D = [(0, 1), (1, -1), (2, 1)]                                 # one direction per axis
SHIFTS_2D = [(0, 1), (0, -1), (1, 1), (1, -1)]


@contextlib.contextmanager
def _variant(v):
    from stardist_amd.models import unet as U
    with contextlib.ExitStack() as st:
        if v.endswith("-hand"):
            st.enter_context(U.force_conv_mode("hand"))
        if v.endswith("-nosplit"):
            st.enter_context(U.force_split16(False))
        yield


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and u.dtype == v.dtype, (what, k, u.shape, v.shape)
        if not np.array_equal(u, v):
            bad = np.argwhere(~(u == v))
            pytest.fail("%s: output %d differs at %d of %d elements (%d NaN), first %s: %r vs %r" % (
                what, k, len(bad), u.size, int(np.isnan(u).sum()), tuple(bad[0]), u[tuple(bad[0])], v[tuple(bad[0])]))


_CPU, _GPU = {}, {}


def _cpu(name):
    """(CPU model, image, reference) of the integer family, once per case (the float32 evaluation: equal to the float64 one, asserted
    for every case by test_cpu_predict_cases.py; sigmoid and softmax of its integer logits in float64)"""
    if name not in _CPU:
        case = P.BY_NAME[name]
        m = P.integer_model(case)
        img = P.integer_image(case)
        _CPU[name] = (m, img, P.reference(m, img, case.axes, double=False))
    return _CPU[name]


def _gpu(variant):
    """(GPU model, its untiled dense prediction) once per case and variant"""
    if variant not in _GPU:
        name = variant.split("-")[0]
        case = P.BY_NAME[name]
        m, img, _ = _cpu(name)
        g = P.like(m, DEV)
        with _variant(variant), nan_empty():
            pred = g.predict(img, axes=case.axes)
        _GPU[variant] = (g, pred)
    return _GPU[variant]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_untiled_equals_the_reference(variant):
    name = variant.split("-")[0]
    _, _, ref = _cpu(name)
    _, pred = _gpu(variant)
    prob, dist = pred[0], pred[1]
    assert prob.shape == ref["logit"].shape and prob.dtype == np.float32 and dist.dtype == np.float32
    _same((dist.astype(np.float64),), (ref["dist"],), "%s distances" % variant)
    err = float(np.abs(prob.astype(np.float64) - ref["prob"]).max())
    print("%s: probability within %.3g of the float64 sigmoid" % (variant, err))
    assert err <= 2e-6
    for v in np.unique(ref["logit"]):
        bits = np.unique(prob[ref["logit"] == v].view(np.uint32))
        assert len(bits) == 1, "logit %g gives %d different probabilities" % (v, len(bits))
    if ref["prob_class"] is not None:
        err = float(np.abs(pred[2].astype(np.float64) - ref["prob_class"]).max())
        print("%s: class probabilities within %.3g of the float64 softmax" % (variant, err))
        assert pred[2].shape == ref["prob_class"].shape and err <= 2e-6
    else:
        assert len(pred) == 2
    if variant != name:
        _same(pred, _gpu(name)[1], "%s against the default kernels" % variant)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_tiled_equals_untiled_integer(variant):
    name = variant.split("-")[0]
    case = P.BY_NAME[name]
    _, img, _ = _cpu(name)
    g, pred = _gpu(variant)
    with _variant(variant), nan_empty():
        tiled = g.predict(img, axes=case.axes, n_tiles=case.n_tiles)
    _same(tiled, pred, "%s tiled %s" % (variant, case.n_tiles))


def _shift_params():
    return [pytest.param(c.name, axis, sign, id="%s-axis%d%s" % (c.name, axis, "+" if sign > 0 else "-"))
            for c in P.CASES for axis, sign in (SHIFTS_2D if c.nd == 2 else SHIFTS_3D)]


@pytest.mark.parametrize("name,axis,sign", _shift_params())
def test_tiled_equals_untiled_shift(name, axis, sign):
    case = P.BY_NAME[name]
    m = P.shift_model(case, axis, sign)
    # impulses out to the analytic receptive field (never less than the measured reach: test_cpu_predict_cases.py)
    img = P.shift_image(m, case, axis, sign, m._receptive_field_radius()[axis])
    padded, _, tiles = P.plan(m, case)
    if not (img > 0).any():                                           # no tile is cut on the side this network looks towards
        assert not any((t[0][axis].stop < padded[axis]) if sign > 0 else (t[0][axis].start > 0) for t in tiles)
        return
    g = P.like(m, DEV)
    with nan_empty():
        whole = g.predict(img, axes=case.axes)
        tiled = g.predict(img, axes=case.axes, n_tiles=case.n_tiles)
    assert float(whole[1].max()) >= 1 and float(whole[1].max()) == round(float(whole[1].max()))
    _same(tiled, whole, "%s shift axis %d sign %d" % (name, axis, sign))


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def _value_threshold(prob):
    """one of the probability values of `prob` with pixels at it and above it: the strict `>` must leave the pixels AT it out"""
    vals, counts = np.unique(prob, return_counts=True)
    k = int(np.argmin(np.abs(vals - 0.7310586)))                      # sigmoid(1)
    assert counts[k] > 10 and counts[k + 1:].sum() > 10
    return float(vals[k])


def _check_sparse(got, want, case, grid, tiled, what):
    if tiled:                                                         # candidates come tile by tile, as in the reference
        got = P.c_order(got)
    pts = got[-1]
    assert pts.dtype == np.int64 and pts.shape == want[3].shape, (what, pts.shape, want[3].shape)
    assert np.array_equal(pts, want[3]), what
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
    if want[2] is not None:
        assert len(got) == 4 and np.array_equal(got[2], want[2]), what
    else:
        assert len(got) == 3
    assert bool((pts < np.asarray(P.spatial_shape(case))).all()) and bool((pts % np.asarray(grid) == 0).all()), what


@pytest.mark.parametrize("name", NAMES)
def test_sparse_equals_the_statement_of_the_dense_prediction(name):
    case = P.BY_NAME[name]
    _, img, ref = _cpu(name)
    g, pred = _gpu(name)
    grid = tuple(g.config.grid)
    shape = P.spatial_shape(case)
    thr_v = _value_threshold(pred[0])
    pc = pred[2] if len(pred) == 3 else None
    default = type(g.net).lazy_features_min_bytes
    try:
        for lazy_min in (default, 0):
            g.net.lazy_features_min_bytes = lazy_min
            for thr, b in ((thr_v, 0), (thr_v, 2), (thr_v, 5), (0.5, 2)):
                want = P.sparse_numpy(pred[0], pred[1], pc, grid, ref["padded"], shape, thr, b)
                assert len(want[0]) > 100 and (thr != thr_v or not (want[0] == np.float32(thr_v)).any())
                for n_tiles in (None, case.n_tiles):
                    with nan_empty():
                        got = g.predict_sparse(img, axes=case.axes, prob_thresh=thr, n_tiles=n_tiles, b=b)
                    assert g._head_mode == ("sparse_lazy" if lazy_min == 0 else "sparse")
                    _check_sparse(got, want, case, grid, n_tiles is not None, "%s lazy_min %d thr %g b %d tiles %s" % (name, lazy_min, thr, b, n_tiles))
    finally:
        g.net.__dict__.pop("lazy_features_min_bytes", None)
    if name == "padded2d":                                            # the border is relative to the PADDED image: candidates in the last rows
        last = P.sparse_numpy(pred[0], pred[1], pc, grid, ref["padded"], shape, 0.5, 2)[3]
        assert int(last[:, 0].max()) == shape[0] - 1 and int(last[:, 1].max()) == shape[1] - 1


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def _predict_watching_the_cache(model, img, **kw):
    """model.predict, looking at the graph cache after every tile"""
    r, sizes = None, []
    for r in model._predict_generator(img, **kw):
        sizes.append(len(model.__dict__.get("_graphs", {})))
    assert max(sizes) <= 8, sizes
    return tuple(t.cpu().numpy() for t in r), sizes


def test_graph_cache_with_more_tile_shapes_than_entries():
    case = P.MANY
    m, img, _ = _cpu(case.name)
    _, pred = _gpu(case.name)
    padded, _, tiles = P.plan(m, case)
    n_shapes = len(set(P.tile_shapes(tiles)))
    assert n_shapes >= 10
    g = P.like(m, DEV)
    assert "_graphs" not in g.__dict__
    with nan_empty():
        first, sizes = _predict_watching_the_cache(g, img, axes=case.axes, n_tiles=case.n_tiles)
        assert sizes[-1] == 8 and len(sizes) == len(tiles) + 1                     # captured, filled, evicted
        _same(first, pred, "tiled with evictions against untiled")
        again, _ = _predict_watching_the_cache(g, img, axes=case.axes, n_tiles=case.n_tiles)
        _same(again, first, "the same call again")
        # three images of two shapes, interleaved: replays of graphs captured for another image, re-captures of evicted shapes
        eager = P.like(m, DEV)
        eager.use_hip_graph = False
        other = P.integer_image(case, salt=2)
        small = P.integer_image(case, salt=3)[:80, :104]
        imgs = dict(a=img, b=other, c=small)
        want = {k: eager.predict(v, axes=case.axes, n_tiles=case.n_tiles) for k, v in imgs.items()}
        assert "_graphs" not in eager.__dict__
        _same(want["a"], pred, "eager tiled against untiled")
        assert not np.array_equal(want["a"][1], want["b"][1])
        for k in "acbca":
            got, _ = _predict_watching_the_cache(g, imgs[k], axes=case.axes, n_tiles=case.n_tiles)
            _same(got, want[k], "image %s through the graph cache against the eager model" % k)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiled", [False, True])
def test_lazy_features_knob_is_followed_after_a_capture(tiled):
    """net.lazy_features_min_bytes changed between predict_sparse calls on one shape, the graph cache left alone: the head mode follows
    and no bit changes (the graphs are keyed by what StarDistNet._lazy_ok reads)"""
    case = P.BY_NAME["plain2d"]
    m, img, _ = _cpu(case.name)
    g = P.like(m, DEV)
    n_tiles = case.n_tiles if tiled else None
    results, modes = [], []
    for lazy_min in (4 << 30, 0, 4 << 30, 0):
        g.net.lazy_features_min_bytes = lazy_min
        with nan_empty():
            results.append(g.predict_sparse(img, axes=case.axes, prob_thresh=0.5, n_tiles=n_tiles))
        modes.append(g._head_mode)
    assert modes == ["sparse", "sparse_lazy", "sparse", "sparse_lazy"], modes
    assert len(results[0][0]) > 1000
    for r in results[1:]:
        _same(r, results[0], "predict_sparse after the knob changed")


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_instances_under_ties_sparse_equals_dense():
    case = P.BY_NAME["plain2d"]
    _, img, _ = _cpu(case.name)
    g, pred = _gpu(case.name)
    calls = []
    own = g._select_sorted
    g._select_sorted = lambda *a, **k: calls.append(1) or own(*a, **k)
    try:
        labels_s, res_s = g.predict_instances(img, axes=case.axes, sparse=True)
        assert calls == [1]                                           # the presorted path
        labels_d, res_d = g.predict_instances(img, axes=case.axes, sparse=False)
        assert calls == [1]
    finally:
        del g._select_sorted
    n_cand = int((pred[0][2:-2, 2:-2] > 0.5).sum())
    assert n_cand > 3000 and len(np.unique(pred[0][pred[0] > 0.5])) <= 16          # thousands of candidates, a dozen scores
    assert len(res_s["prob"]) > 50
    assert np.array_equal(labels_s, labels_d)
    assert sorted(res_s) == sorted(res_d)
    for k in res_s:
        assert np.array_equal(np.asarray(res_s[k]), np.asarray(res_d[k])), k
