"""CPU: the host side of training a multi-class model (train(..., classes=...) of stardist_amd/training.py, training3d.py).
  * utils.mask_to_categorical against the reference's function, executed from its sources.
  * utils.nearest_zoom_table: the per-axis gather reproduces scipy.ndimage.zoom(..., 1 / grid, order=0) of whole arrays, the rows that
    scipy reads from outside the array included.
  * the numpy composition of prob_class (tests/_class_cases.compose, what sd_class_targets_device is held to on the GPU) against the class
    output of the reference's StarDistData2D.__getitem__, executed from its sources on a seeded batch.
  * training.reference_class_loss in float64 against the reference's weighted_categorical_crossentropy on numpy.
  * the classes argument, validation pairs / triples and the scope check.
  * seeded TrainData2D / TrainData3D with classes draw the patches of the single-class generator."""
import os
import types
from collections import defaultdict

import numpy as np
import pytest
import torch

from _class_cases import SHAPES2D, SHAPES3D, compose, gather, scene
from test_cpu_reference_build import ref_methods
from test_cpu_training import _NpK, _Rolling, _csbdeep_choice, _images
from test_cpu_vs_reference_source import REF, _raise, ref_functions

needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference sources (build container only)")


# ---- mask_to_categorical
def _ref_mask_to_categorical():
    from stardist_amd.matching import _check_label_array
    ns = ref_functions("utils.py", {"mask_to_categorical", "_invert_dict"}, dict(np=np, defaultdict=defaultdict, _check_label_array=_check_label_array))
    return ns["mask_to_categorical"]


@needs_ref
def test_mask_to_categorical_equals_reference():
    from stardist_amd.utils import mask_to_categorical
    ref = _ref_mask_to_categorical()
    rng = np.random.RandomState(0)
    y = rng.randint(0, 7, (20, 17)).astype(np.int32)
    y3 = rng.randint(0, 5, (4, 9, 8)).astype(np.uint16)
    cases = [
        (y, 3, {1: 1, 2: 2, 3: 3, 4: 1, 5: 2, 6: 3}),
        (y, 3, {1: 1, 2: None, 3: 0, 4: 1, 5: None, 6: 3, 99: 2}),          # ignored objects, class 0, a label not in the image
        (y, 2, 2), (y, 2, 0), (y, 2, None), (y, 1, np.int64(1)),
        (y3, 4, {1: 4, 2: None, 3: 0, 4: 2}), (y3, 1, 1),
        (np.zeros((5, 6), np.int32), 2, {}),
    ]
    for lab, n, cls in cases:
        want, wd = ref(lab, n, cls, return_cls_dict=True)
        got, gd = mask_to_categorical(lab, n, cls, return_cls_dict=True)
        assert got.dtype == want.dtype == np.float32 and got.shape == lab.shape + (n + 1,) and np.array_equal(got, want)
        assert dict(gd) == dict(wd)
        assert np.array_equal(mask_to_categorical(lab, n, cls), want)
    assert (mask_to_categorical(y, 3, cases[1][2])[y == 2] == [0, -1, -1, -1]).all()
    assert (mask_to_categorical(y, 3, cases[1][2])[y == 3] == 0).all()


@needs_ref
@pytest.mark.parametrize("n, cls, word", [
    (3, {1: 1, 2: 2}, "all gt labels should be present"),                     # labels 3 ... 6 missing
    (3, {1: 1, 2: 2, 3: 3, 4: 4, 5: 1, 6: 1}, "Wrong class id"),
    (3, {1: 1, 2: 2, 3: 3, 4: -1, 5: 1, 6: 1}, "Wrong class id"),
    (3, {1: 1, 2: 2, 3: 3, 4: 1.5, 5: 1, 6: 1}, "Wrong class id"),
    (2, 3, "Wrong class id"),
    (2, "auto", "classes should be dict"),
    (0, 1, "n_classes"),
    (2.0, 1, "n_classes"),
])
def test_mask_to_categorical_errors_equal_reference(n, cls, word):
    from stardist_amd.utils import mask_to_categorical
    ref = _ref_mask_to_categorical()
    y = np.arange(7 * 6).reshape(7, 6).astype(np.int32) % 7
    msgs = []
    for fn in (ref, mask_to_categorical):
        with pytest.raises(ValueError, match=word) as e:
            fn(y, n, cls)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]
    for fn in (ref, mask_to_categorical):
        with pytest.raises(ValueError, match="non-negative integers"):
            fn(y.astype(np.float32), 2, 1)


# ---- the nearest zoom as per-axis gather tables
def test_gather_tables_equal_scipy_zoom():
    from scipy.ndimage import zoom
    from stardist_amd.utils import nearest_zoom_table
    rng = np.random.RandomState(1)
    outside = 0
    for shape, grid in SHAPES2D + SHAPES3D:
        a = rng.randint(-1, 2, (2,) + shape + (3,)).astype(np.float32)
        want = zoom(a, (1,) + tuple(1 / g for g in grid) + (1,), order=0)
        got = np.stack([gather(s, grid) for s in a])
        assert got.shape == want.shape == (2,) + tuple(s // g for s, g in zip(shape, grid)) + (3,)
        assert np.array_equal(got, want), (shape, grid)
        tabs = [nearest_zoom_table(n, g) for n, g in zip(shape, grid)]
        assert all(t.dtype == np.int32 and t.min() >= -1 and t.max() < n for t, n in zip(tabs, shape))
        outside += sum(int((t < 0).sum()) for t in tabs)
    # the lengths named for it do read outside the array with this scipy: the zero rows were compared above
    assert outside > 0
    for n, g in [(48, 2), (32, 2), (56, 2)]:
        t = nearest_zoom_table(n, g)
        assert (t < 0).any() and np.array_equal(zoom(np.arange(1.0, n + 1), 1 / g, order=0) - 1, t)
    # and the zoom is not [::g]
    assert not np.array_equal(nearest_zoom_table(40, 4), np.arange(0, 40, 4))
    assert np.array_equal(nearest_zoom_table(24, 1), np.arange(24))
    assert nearest_zoom_table(48, 2) is nearest_zoom_table(48, 2)


# ---- the whole target against the reference's generator
def _reference_generator(X, Y, classes, n_classes, n_rays, patch_size, grid, batch_size, foreground_prob=0.0):
    """StarDistData2D.__getitem__ executed from the reference's sources on an object that holds what __init__ would have set.  edt_prob
    and star_dist (native code there) are stood in for by zeros: the class output does not depend on them."""
    from scipy.ndimage import maximum_filter, zoom
    ns = ref_functions("sample_patches.py", {"sample_patches", "get_valid_inds"}, dict(np=np, _raise=_raise, choice=_csbdeep_choice))
    on_grid = tuple(slice(0, None, g) for g in grid)
    mns = dict(np=np, zoom=zoom, sample_patches=ns["sample_patches"], mask_to_categorical=_ref_mask_to_categorical(), _gen_rtype=tuple,
               edt_prob=lambda lbl: np.zeros(lbl.shape, np.float32),
               star_dist=lambda lbl, n, mode=None, grid=None: np.zeros(lbl[on_grid].shape + (n,), np.float32))
    bns = dict(np=np)
    base = ref_methods("models/base.py", "StarDistDataBase", {"get_valid_inds"}, bns)
    bns["get_valid_inds"] = ns["get_valid_inds"]          # the method's global of that name is the module function (base.py:27)
    getitem = ref_methods("models/model2d.py", "StarDistData2D", {"__getitem__"}, mns)["__getitem__"]
    roll = _Rolling(len(X), batch_size)
    obj = types.SimpleNamespace(X=X, Y=Y, patch_size=patch_size, foreground_prob=foreground_prob, maxfilter_patch_size=patch_size,
                                sample_ind_cache=True, _ind_cache_fg={}, _ind_cache_all={}, lock=__import__("threading").Lock(),
                                max_filter=lambda y, p: maximum_filter(y, p, mode="constant"), batch=roll.batch, n_channel=None,
                                channels_as_tuple=lambda x: (x,), b=(slice(None), slice(None)), augmenter=lambda *a: a,
                                ss_grid=(slice(None),) + on_grid, grid=tuple(grid), shape_completion=False, n_rays=n_rays, sd_mode="cpp",
                                n_classes=n_classes, classes=classes)
    obj.get_valid_inds = lambda k, foreground_prob=None: base["get_valid_inds"](obj, k, foreground_prob)
    return lambda i: getitem(obj, i), roll


def _class_images(n=4, seed=0):
    X, Y = _images(n, seed)
    classes = []
    for i, y in enumerate(Y):
        y[5:15, 40:52] = -1                                # an unlabelled region
        ids = [int(v) for v in np.unique(y) if v > 0]
        classes.append({k: (None if k == 2 else (0 if k == 3 else 1 + k % 3)) for k in ids} if i != 1 else 2)
    classes[2] = None
    return X, Y, classes


@needs_ref
@pytest.mark.parametrize("patch_size, grid", [((48, 40), (2, 2)), ((48, 40), (1, 4)), ((32, 56), (2, 2))])
def test_composition_equals_reference_generator(patch_size, grid):
    from stardist_amd.training import TrainData2D
    X, Y, classes = _class_images()
    np.random.seed(5)
    ref, _ = _reference_generator(X, Y, classes, 3, 8, patch_size, grid, batch_size=3)
    want = [ref(i) for i in range(4)]
    np.random.seed(5)
    d = TrainData2D(X, Y, batch_size=3, n_rays=8, length=4, patch_size=patch_size, grid=grid, n_classes=3, classes=classes)
    seen = set()
    for i, ((xw,), (_, _, pcw)) in enumerate(want):
        Xg, Yg = d.sample(i)
        tables, idx = d.batch_classes(i)
        assert np.array_equal(np.stack(Xg)[..., None], xw)
        got = compose(Yg, [classes[k] for k in idx], 3, grid)
        assert got.dtype == pcw.dtype and np.array_equal(got, pcw), i
        seen |= set(np.unique(got).tolist())
    assert seen == {-1.0, 0.0, 1.0}


# ---- the loss
@needs_ref
@pytest.mark.parametrize("C, weights", [(2, (1.0, 1.0)), (4, (0.5, 1.0, 2.0, 4.0)), (7, (1.0, 0.3, 2.0, 1.5, 0.7, 3.0, 0.1))])
def test_class_loss_equals_reference_formula(C, weights):
    from stardist_amd.training import reference_class_loss

    class K(_NpK):
        sum = staticmethod(lambda x, axis=None, keepdims=False: np.sum(x, axis=axis, keepdims=keepdims))
        clip = staticmethod(np.clip)
        log = staticmethod(np.log)
    ns = ref_functions("models/base.py", {"weighted_categorical_crossentropy"}, dict(np=np, K=K, backend_channels_last=lambda: True))
    for seed, nd in [(0, 2), (1, 3), (2, 2)]:
        rng = np.random.RandomState(seed)
        shape = (2, 9, 11) if nd == 2 else (2, 3, 5, 7)
        z = rng.randn(*shape, C) * 3
        z[0, 0] = 0.0
        z[0, 0, ..., 0] = 40.0                             # saturated: the other channels' probabilities are clipped from below
        z[1, 1, ..., C - 1] = -40.0
        t = np.zeros(shape + (C,))
        lab = rng.randint(0, C, shape)
        np.put_along_axis(t, lab[..., None], 1.0, -1)
        t[rng.rand(*shape) < 0.15] = -1                    # a fully masked pixel
        part = rng.rand(*shape) < 0.15                     # an ignored object: every channel but the background's
        t[part, 1:] = -1
        t[part, 0] = 0
        t[rng.rand(*shape) < 0.1] = 0                      # a class-0 object: all zero
        e = np.exp(z - z.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
        want = np.mean(ns["weighted_categorical_crossentropy"](weights, ndim=nd)(t.copy(), p.copy()))
        got = float(reference_class_loss(torch.from_numpy(z), torch.from_numpy(t), weights))
        got_p = float(reference_class_loss(torch.from_numpy(p), torch.from_numpy(t), weights, from_logits=False))
        assert want > 0
        assert abs(got - want) <= 1e-13 * abs(want), (got, want)
        assert abs(got_p - want) <= 1e-13 * abs(want), (got_p, want)


# ---- the classes argument, validation data, scope
def _model(n_classes, nd=2):
    from stardist_amd.models import Config2D, Config3D, StarDist2D, StarDist3D
    if nd == 2:
        return StarDist2D(Config2D(n_rays=8, n_classes=n_classes), basedir=None, device="cpu")
    return StarDist3D(Config3D(n_rays=8, n_classes=n_classes, backbone="unet", unet_n_depth=1), basedir=None, device="cpu")


@needs_ref
@pytest.mark.parametrize("nd", [2, 3])
def test_parse_classes_arg_equals_reference(nd):
    ref = ref_methods("models/base.py", "StarDistBase", {"_parse_classes_arg"}, dict(np=np, _raise=_raise))["_parse_classes_arg"]
    args = ["auto", "other", [1, 2, 3], ({1: 1}, None, 2), np.array([1, 2, 1]), [1, 2], (), 1, None, {1: 2}]
    for n_classes in (None, 1, 3):
        m = _model(n_classes, nd)
        stand_in = types.SimpleNamespace(config=types.SimpleNamespace(n_classes=n_classes))
        for a in args:
            try:
                want = ref(stand_in, a, 3)
            except ValueError as e:
                with pytest.raises(ValueError) as g:
                    m._parse_classes_arg(a, 3)
                assert str(g.value) == str(e), (n_classes, a)
            else:
                got = m._parse_classes_arg(a, 3)
                assert type(got) is type(want) and (got is want or np.array_equal(got, want)), (n_classes, a)
    assert _model(1)._parse_classes_arg("auto", 3) == (1, 1, 1) and _model(None)._parse_classes_arg("auto", 3) is None


def test_scope_with_classes():
    from stardist_amd.models import Config2D, Config3D
    from stardist_amd.training import check_trainable
    from stardist_amd.training3d import check_trainable3d
    check_trainable(Config2D(n_rays=8, n_classes=2), classes=[{1: 1}, 2])
    check_trainable(Config2D(n_rays=8, n_classes=2), [None])
    check_trainable(Config2D(n_rays=8, n_classes=1))
    check_trainable(Config2D(n_rays=8, n_classes=1), "auto")
    check_trainable3d(Config3D(n_rays=8, n_classes=2), classes=(1,))
    check_trainable3d(Config3D(n_rays=8, n_classes=3, backbone="resnet"), classes=(1,))
    check_trainable3d(Config3D(n_rays=8, n_classes=1))
    for check, cfg in [(check_trainable, Config2D(n_rays=8, n_classes=2)), (check_trainable3d, Config3D(n_rays=8, n_classes=2))]:
        for args in [(), ("auto",)]:
            with pytest.raises(NotImplementedError, match="n_classes") as e:
                check(cfg, *args)
            assert "using classes = 'auto' for n_classes > 1 not supported" in str(e.value)
    # every other setting stays out of scope for a multi-class model too
    with pytest.raises(NotImplementedError, match="train_dist_loss"):
        check_trainable(Config2D(n_rays=8, n_classes=2, train_dist_loss="iou"), classes=[1])
    with pytest.raises(NotImplementedError, match="n_channel_in"):
        check_trainable3d(Config3D(n_rays=8, n_classes=2, n_channel_in=2), classes=[1])


def test_train_hands_classes_to_the_check():
    """on a host without a device the scope check comes first: with classes given it passes, and train stops at the device"""
    X = [np.zeros((64, 64), np.float32)]
    Y = [np.zeros((64, 64), np.int32)]
    m = _model(2)
    with pytest.raises(NotImplementedError, match="n_classes"):
        m.train(X, Y, validation_data=(X, Y), epochs=1, steps_per_epoch=1)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.train(X, Y, validation_data=(X, Y, [1]), classes=[{1: 2}], epochs=1, steps_per_epoch=1)
    with pytest.raises(RuntimeError, match="HIP device"):
        _model(1).train(X, Y, validation_data=(X, Y), epochs=1, steps_per_epoch=1)


def test_validation_pair_or_triple(monkeypatch):
    from stardist_amd import training
    monkeypatch.setattr(training.N, "require_device", lambda: None)
    X = [np.zeros((64, 64), np.float32)] * 2

    def begin(n_classes, vd):
        m = _model(n_classes)
        monkeypatch.setattr(m, "device", types.SimpleNamespace(type="cuda"), raising=False)
        return training.begin_training(m, vd, None, 1, 1)[2]
    assert begin(2, (X, X)) == (X, X, "auto")
    assert begin(2, [X, X]) == (X, X, "auto")
    assert begin(2, (X, X, [1, 2])) == (X, X, [1, 2])
    assert begin(None, (X, X)) == (X, X)
    for n_classes, vd in [(2, (X,)), (2, (X, X, X, X)), (2, X[0]), (None, (X, X, [1, 2])), (None, (X,))]:
        with pytest.raises(ValueError):
            begin(n_classes, vd)


# ---- the data classes
def test_class_tables_and_wrong_class_ids():
    from stardist_amd.training import CODE_IGNORE, CODE_MISSING, ClassTables
    t = ClassTables([{1: 1, 2: None, 3: 0, 2 ** 30 + 5: 2}, 2, None, {1: 1, 5: 2}, {0: 1, 4: 2}], 2)
    keys, codes = t._host
    (o0, n0, f0, d0), (o1, n1, f1, d1), (o2, n2, f2, d2), (o3, n3, f3, d3), (o4, n4, f4, d4) = t.meta.tolist()
    assert f0 == 1 and keys[o0:o0 + n0].tolist() == [0, 1, 2, 3, 2 ** 30 + 5] and codes[o0:o0 + n0].tolist() == [0, 1, CODE_IGNORE, 0, 2]
    assert d0 == d3 == CODE_MISSING
    assert (f1, d1, codes[o1:o1 + n1].tolist()) == (0, 2, [0]) and (f2, d2, codes[o2:o2 + n2].tolist()) == (0, CODE_IGNORE, [0])
    assert f3 == 0 and codes[o3:o3 + n3].tolist() == [0, 1, CODE_MISSING, CODE_MISSING, CODE_MISSING, 2]
    assert codes[o4:o4 + n4].tolist() == [1, CODE_MISSING, CODE_MISSING, CODE_MISSING, 2]      # a dict may name label 0, as in the reference
    for bad in ([{1: 3}], [{1: -1}], [{1: 1.0}], [3], ["auto"], [[1]]):
        with pytest.raises(ValueError):
            ClassTables(bad, 2)
    with pytest.raises(ValueError, match="n_classes"):
        ClassTables([1], 0)


@pytest.mark.parametrize("nd", [2, 3])
def test_seeded_patches_do_not_depend_on_classes(nd):
    from stardist_amd.rays3d import Rays_GoldenSpiral
    from stardist_amd.training import TrainData2D
    from stardist_amd.training3d import TrainData3D
    rng = np.random.RandomState(3)
    shape, ps, grid = ((70, 64), (48, 40), (2, 2)) if nd == 2 else ((12, 40, 36), (8, 24, 20), (1, 2, 2))
    X = [rng.rand(*shape).astype(np.float32) for _ in range(3)]
    Y = [scene(shape, 2, 10 + i, B=1)[0][0] for i in range(3)]
    classes = [scene(shape, 2, 10 + i, B=1)[1][0] for i in range(3)]

    def make(**kw):
        common = dict(batch_size=2, length=6, patch_size=ps, grid=grid, foreground_prob=0.5, **kw)
        return TrainData2D(X, Y, n_rays=8, **common) if nd == 2 else TrainData3D(X, Y, rays=Rays_GoldenSpiral(8), **common)
    np.random.seed(11)
    a = make()
    pa = [a.sample(i) for i in range(5)]
    state_a = np.random.get_state()[1].copy()
    np.random.seed(11)
    b = make(n_classes=2, classes=classes)
    pb = []
    for i in range(5):
        pb.append(b.sample(i))
        tables, idx = b.batch_classes(i)
        assert tables is b.class_tables and np.array_equal(idx, b.batch(i)) and len(idx) == 2
    assert np.array_equal(state_a, np.random.get_state()[1])
    assert a.batch_classes(0) is None
    for (xa, ya), (xb, yb) in zip(pa, pb):
        assert all(np.array_equal(u, v) for u, v in zip(xa + ya, xb + yb))
    with pytest.raises(ValueError, match="same length"):
        make(n_classes=2, classes=classes[:2])
    with pytest.warns(UserWarning, match="Ignoring classes"):
        make(classes=classes)
