"""GPU: training a multi-class model (csrc/train_classes.hip; train(..., classes=...) of stardist_amd/training.py, training3d.py).
  * sd_class_targets_device equals the numpy composition of the reference's prob_class (tests/_class_cases.compose, proven against the
    reference's generator and scipy in test_cpu_training_classes.py) with ==, at shapes where scipy's zoom reads past the patch.
  * sd_class_loss_device against float64 autograd of training.reference_class_loss; repeatable bit for bit, with and without a gradient.
  * one step of a small 2D U-Net and a small 3D ResNet with a class head against float64 autograd of StarDistNet; no library
    convolution / GEMM in the step; two seeded steps give the same bits.
  * StarDist2D.train with classes end to end: the class loss falls below that of the best constant prediction, the history, a reloaded
    model predicts classes.  A single-class train keeps today's history keys."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _class_cases import BIG_ID, SHAPES2D, SHAPES3D, compose, scene
from _training_cases import DEV, balls as _balls, discs as _discs, randomise as _randomise

pytestmark = pytest.mark.gpu


# ---- targets
@pytest.mark.parametrize("shape, grid", SHAPES2D + SHAPES3D, ids=lambda v: "x".join(str(i) for i in v))
def test_class_targets_equal_the_composition(shape, grid):
    from stardist_amd.training import ClassTables, _upload_labels, class_targets_device
    n_classes = 3
    Y, classes = scene(shape, n_classes, seed=len(shape) * 100 + shape[-1])
    assert any((y < 0).any() for y in Y) and any((y == BIG_ID).any() for y in Y)
    want = compose(Y, classes, n_classes, grid)
    assert set(np.unique(want).tolist()) == {-1.0, 0.0, 1.0} and all((want[..., c] == 1).any() for c in range(n_classes + 1))
    tables = ClassTables(classes, n_classes)
    assert sorted(tables.meta[:, 2].tolist()) == [0, 1]                  # a dense and a sorted table
    lab, neg, d_lab, _ = _upload_labels(Y, grid, DEV)
    got = [class_targets_device(d_lab, neg, grid, tables, [0, 1]) for _ in range(2)]
    assert got[0].dtype == torch.float32 and tuple(got[0].shape) == want.shape
    assert np.array_equal(got[0].cpu().numpy(), want)
    assert torch.equal(got[0], got[1])
    tables.check()                                                      # every label is in its dict
    # the samples in the other order, through the other table of each
    swapped = class_targets_device(d_lab.flip(0).contiguous(), neg[::-1], grid, tables, [1, 0])
    assert np.array_equal(swapped.cpu().numpy(), want[::-1])


@pytest.mark.parametrize("nd", [2, 3])
def test_targets_functions_with_classes(nd):
    """targets_device / targets_device3d with classes: the other two targets are those of the call without, prob_class the composition;
    integer and None classes"""
    from stardist_amd.rays3d import Rays_GoldenSpiral
    from stardist_amd.training import ClassTables, targets_device
    from stardist_amd.training3d import targets_device3d
    shape, grid = SHAPES2D[0] if nd == 2 else SHAPES3D[0]
    Y, classes = scene(shape, 2, seed=7)
    classes = [classes[0], 2, None]
    Y = [Y[0], np.maximum(Y[1], 0) % 1000, Y[1]]
    tables = ClassTables(classes, 2)
    if nd == 2:
        fn = lambda *cls: targets_device(Y, 8, grid, DEV, *cls)
    else:
        rays = Rays_GoldenSpiral(8)
        fn = lambda *cls: targets_device3d(Y, rays, grid, None, DEV, *cls)
    p0, d0 = fn()
    p1, d1, pc = fn((tables, np.array([0, 1, 2])))
    assert torch.equal(p0, p1) and torch.equal(d0, d1)
    assert np.array_equal(pc.cpu().numpy(), compose(Y, classes, 2, grid))
    tables.check()


def test_missing_label_raises_the_reference_error():
    from stardist_amd.training import ClassTables, _upload_labels, class_targets_device
    shape, grid = SHAPES2D[0]
    Y, classes = scene(shape, 2, seed=3)
    for drop in (5, BIG_ID):                               # from the dense table of sample 0 / the sorted table of sample 1
        b = 0 if drop == 5 else 1
        cls = [dict(c) for c in classes]
        del cls[b][drop]
        # the label sits on one pixel that the zoom does not sample (row 1 of grid 2): the whole patch is checked, as in the reference
        Yd = [np.where(y == drop, 0, y) for y in Y]
        Yd[b][1, 1] = drop
        tables = ClassTables(cls, 2)
        _, neg, d_lab, _ = _upload_labels(Yd, grid, DEV)
        class_targets_device(d_lab, neg, grid, tables, [0, 1])
        with pytest.raises(ValueError, match="all gt labels should be present in class dict provided"):
            tables.check()
        tables.check()                                     # the flag was cleared
        class_targets_device(d_lab, neg, grid, ClassTables(classes, 2), [0, 1])


# ---- loss
def _loss_case(n_pix_shape, C, seed):
    rng = np.random.RandomState(seed)
    z = rng.randn(*n_pix_shape, C) * 3
    z[0, 0, :4] = 0.0
    z[0, 0, :4, 0] = 40.0                                  # logits 40 apart: p / S leaves [eps, 1 - eps], the clip branch
    z[0, 1, :4, C - 1] = -40.0
    t = np.zeros(n_pix_shape + (C,))
    np.put_along_axis(t, rng.randint(0, C, n_pix_shape)[..., None], 1.0, -1)
    t[rng.rand(*n_pix_shape) < 0.15] = -1                  # fully masked pixels (negative labels)
    part = rng.rand(*n_pix_shape) < 0.15                   # masked in the object channels only (an ignored object)
    t[part, 1:] = -1
    t[part, 0] = 0
    t[rng.rand(*n_pix_shape) < 0.1] = 0                    # all-zero pixels (class 0, or outside the zoom)
    t[0, 0, :2] = 0
    t[0, 0, 0, 1] = 1                                      # the clipped channels carry a target
    t[0, 1, 0] = 0
    t[0, 1, 0, C - 1] = 1
    return torch.from_numpy(z).float(), torch.from_numpy(t).float()


@pytest.mark.parametrize("shape", [(2, 50, 47), (1, 17, 241)], ids=["4700", "4097"])      # two blocks of partial sums, the second ragged
@pytest.mark.parametrize("n_classes", [1, 3, 6, 9])
def test_class_loss_and_gradient(shape, n_classes):
    from stardist_amd.lib import _native as N
    from stardist_amd.training import _p, reference_class_loss
    C = n_classes + 1
    weights = (0.5, 1.0, 2.0, 4.0, 0.25, 3.0, 1.5, 0.75, 1.25, 2.5)[:C]
    w_class = 0.7
    z, t = _loss_case(shape, C, seed=n_classes)
    n_pix = int(np.prod(shape))
    dz, dt = z.to(DEV).contiguous(), t.to(DEV).contiguous()
    dw = torch.tensor(weights, dtype=torch.float64, device=DEV)

    def call(grad):
        losses = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
        g = torch.full_like(dz, float("nan")) if grad else None
        N.dcall(dz, "sd_class_loss_device", _p(dz), _p(dt), _p(dw), n_pix, C, w_class, _p(losses), _p(g))
        return losses, g
    (l0, g0), (l1, g1), (l2, _) = call(True), call(True), call(False)
    z64 = z.double().requires_grad_(True)
    ref = reference_class_loss(z64, t.double(), weights)
    (w_class * ref).backward()
    print("class loss", float(l0[0]), "reference", float(ref), "gradient error",
          float((g0.double().cpu() - z64.grad).norm() / z64.grad.norm()))
    assert abs(float(l0[0]) - float(ref)) <= 1e-6 * abs(float(ref))
    assert abs(float(l0[1]) - w_class * float(ref)) <= 1e-6 * abs(w_class * float(ref))
    assert float((g0.double().cpu() - z64.grad).norm() / z64.grad.norm()) <= 1e-6
    # the clip branch: no gradient where p / S leaves [eps, 1 - eps], in the reference and here
    for px in [(0, 0, 0), (0, 0, 1), (0, 1, 0)]:
        assert float(z64.grad[px].abs().max()) == 0.0 and float(g0[px].abs().max()) == 0.0
    assert bool(torch.isfinite(g0).all())
    assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(l0, l2)


# ---- one step of a network with a class head
def _model2d():
    from stardist_amd.models import Config2D, StarDist2D
    cfg = Config2D(n_rays=8, grid=(2, 2), n_classes=3, unet_n_depth=1, train_patch_size=(48, 40), train_batch_size=2,
                   train_class_weights=(0.5, 1, 2, 4), train_loss_weights=(1, 0.2, 0.6))
    return StarDist2D(cfg, basedir=None, device=DEV, seed=0)


def _model3d():
    from stardist_amd.models import Config3D, StarDist3D
    cfg = Config3D(backbone="resnet", n_rays=8, grid=(1, 2, 2), n_classes=2, resnet_n_blocks=2, resnet_n_filter_base=32,
                   resnet_n_conv_per_block=2, net_conv_after_resnet=32, train_patch_size=(8, 24, 20), train_batch_size=2,
                   train_class_weights=(0.5, 1, 2))
    return StarDist3D(cfg, basedir=None, device=DEV, seed=0)


def _step_inputs(model, seed=0):
    """x, prob_true, dist_true_mask, prob_class_true of a batch of 2 for the model, and the loss function"""
    from stardist_amd.training import ClassTables, targets_device, train_loss
    from stardist_amd.training3d import targets_device3d, train_loss3d
    c = model.config
    shape, K = tuple(c.train_patch_size), c.n_classes
    gen = _discs if len(shape) == 2 else _balls
    xs, ys = zip(*[gen(shape, 6, seed * 10 + b, 3, 7) for b in range(2)])
    classes = [{k: (None if k == 2 else (0 if k == 3 else 1 + k % K)) for k in range(1, 7)} for _ in ys]
    ys = [y.copy() for y in ys]
    ys[0][:3, ..., :4] = -1
    x = torch.from_numpy(np.stack(xs)[..., None]).to(DEV)
    cls = (ClassTables(classes, K), [0, 1])
    if len(shape) == 2:
        return (x,) + targets_device(ys, c.n_rays, c.grid, DEV, cls), train_loss
    from stardist_amd.rays3d import rays_from_json
    return (x,) + targets_device3d(ys, rays_from_json(c.rays_json), c.grid, c.anisotropy, DEV, cls), train_loss3d


def _native_step(model, batch, loss_fn):
    x, pt, dtm, pc = batch
    params = list(model.net.parameters())
    for p in params:
        p.requires_grad_(True)
        p.grad = None
    loss, losses = loss_fn(model.net, model.config, x, pt, dtm, prob_class_true=pc)
    loss.backward()
    grads = [p.grad.detach().clone() for p in params]
    for p in params:
        p.grad = None
    return loss.detach().clone(), losses.clone(), grads


@pytest.mark.parametrize("make", [_model2d, _model3d], ids=["unet2d", "resnet3d"])
def test_network_gradient_with_class_head(make):
    from stardist_amd.training import reference_class_loss, reference_losses
    model = make()
    _randomise(model.net, 5)
    batch, loss_fn = _step_inputs(model)
    x, pt, dtm, pc = batch
    assert set(np.unique(pc.cpu().numpy()).tolist()) == {-1.0, 0.0, 1.0}
    loss, losses, got = _native_step(model, batch, loss_fn)
    _, losses2, got2 = _native_step(model, batch, loss_fn)
    assert torch.equal(losses, losses2) and all(torch.equal(a, b) for a, b in zip(got, got2))
    c = model.config
    nd = x.ndim - 2
    to_first, to_last = (0, nd + 1) + tuple(range(1, nd + 1)), (0,) + tuple(range(2, nd + 2)) + (1,)
    net64 = copy.deepcopy(model.net).cpu().double().to(memory_format=torch.contiguous_format)
    prob, dist, prob_class = net64(x.permute(*to_first).double().cpu())
    ref = reference_losses(prob[:, 0], dist.permute(*to_last), pt.double().cpu(), dtm.double().cpu(), dist_loss=c.train_dist_loss,
                           loss_weights=c.train_loss_weights[:2], background_reg=c.train_background_reg)
    ref_cls = reference_class_loss(prob_class.permute(*to_last), pc.double().cpu(), c.train_class_weights, from_logits=False)
    total = ref[2] + c.train_loss_weights[2] * ref_cls
    total.backward()
    assert tuple(losses.shape) == (4,) and float(loss) == float(losses[2])
    # (the bounds of the existing network-gradient tests: 1e-5 on the 2D loss, 1e-4 on the 3D ResNet's, 1e-4 on every gradient)
    tol = 1e-5 if nd == 2 else 1e-4
    print("class loss", float(losses[3]), float(ref_cls), "total", float(losses[2]), float(total))
    assert abs(float(losses[3]) - float(ref_cls)) <= tol * abs(float(ref_cls)), (float(losses[3]), float(ref_cls))
    assert abs(float(losses[2]) - float(total)) <= tol * abs(float(total)), (float(losses[2]), float(total))
    names = [n for n, _ in net64.named_parameters()]
    assert any(n.startswith("features_class") for n in names) and any(n.startswith("prob_class") for n in names)
    for (name, p64), g in zip(net64.named_parameters(), got):
        want = p64.grad
        rel = float((g.double().cpu() - want).norm() / want.norm().clamp_min(1e-300))
        print(name, rel)
        assert float(want.norm()) > 0 and rel <= 1e-4, (name, rel)


@pytest.mark.parametrize("make", [_model2d, _model3d], ids=["unet2d", "resnet3d"])
def test_no_library_convolution_with_class_head(monkeypatch, make):
    model = make()
    batch, loss_fn = _step_inputs(model)

    def boom(*a, **k):
        raise AssertionError("library convolution / GEMM called")
    for mod, name in [(F, "conv2d"), (torch, "conv2d"), (F, "conv3d"), (torch, "conv3d"), (torch, "matmul"), (torch, "mm"), (F, "linear"),
                      (torch, "softmax"), (F, "softmax")]:
        monkeypatch.setattr(mod, name, boom)
    _, losses, grads = _native_step(model, batch, loss_fn)
    assert bool(torch.isfinite(losses).all()) and all(bool(torch.isfinite(g).all()) for g in grads)
    with torch.no_grad():                                  # validation: the same losses without gradient buffers
        x, pt, dtm, pc = batch
        _, l0 = loss_fn(model.net, model.config, x, pt, dtm, prob_class_true=pc)
    assert torch.equal(l0, losses)
    with pytest.raises(ValueError, match="prob_class_true"):
        loss_fn(model.net, model.config, x, pt, dtm)


# ---- end to end
def _two_radii(S, seed, ignore=False):
    """discs of radius 3 (class 1) and 7 (class 2) on a grid of cells, a noisy image of them, and the dict label id -> class id"""
    rng = np.random.RandomState(seed)
    y = np.zeros((S, S), np.int32)
    cls = {}
    yy, xx = np.mgrid[:S, :S]
    k = 0
    for cy in range(10, S - 8, 20):
        for cx in range(10, S - 8, 20):
            k += 1
            big = rng.rand() < 0.5
            r = 7 if big else 3
            y[(yy - cy - rng.randint(-2, 3)) ** 2 + (xx - cx - rng.randint(-2, 3)) ** 2 < r * r] = k
            cls[k] = 2 if big else 1
    if ignore:
        cls[1] = None
    x = (y > 0).astype(np.float32) + 0.05 * rng.randn(S, S).astype(np.float32)
    return x, y, cls


E2E_EPOCHS, E2E_STEPS = 4, 30


def test_train_with_classes_end_to_end(tmp_path):
    from stardist_amd.models import Config2D, StarDist2D
    X, Y, C = (list(v) for v in zip(*[_two_radii(128, s, ignore=(s == 0)) for s in range(6)]))
    Xv, Yv, Cv = (list(v) for v in zip(*[_two_radii(64, 100 + s) for s in range(4)]))
    weights, lw, grid = (1.0, 2.0, 1.0), (1, 0.2, 1.5), (2, 2)
    cfg = Config2D(n_rays=8, grid=grid, n_classes=2, unet_n_depth=2, train_patch_size=(64, 64), train_batch_size=4,
                   train_learning_rate=1e-3, train_class_weights=weights, train_loss_weights=lw, train_reduce_lr=None)
    model = StarDist2D(cfg, name="classes", basedir=str(tmp_path), device=DEV, seed=0)
    hist = model.train(X, Y, validation_data=(Xv, Yv, Cv), classes=C, seed=0, epochs=E2E_EPOCHS, steps_per_epoch=E2E_STEPS)
    from stardist_amd.training import HISTORY_KEYS, HISTORY_KEYS_MULTICLASS
    assert tuple(hist) == HISTORY_KEYS_MULTICLASS and set(HISTORY_KEYS_MULTICLASS) == set(HISTORY_KEYS) | {"prob_class_loss", "val_prob_class_loss"}
    assert all(len(v) == E2E_EPOCHS for v in hist.values())
    for pre in ("", "val_"):
        for tot, p, d, c in zip(*(hist[pre + k] for k in ("loss", "prob_loss", "dist_loss", "prob_class_loss"))):
            assert abs(tot - (lw[0] * p + lw[1] * d + lw[2] * c)) <= 1e-12 * abs(tot)
    # the best constant prediction: the weighted cross entropy of the class frequencies of the validation targets (the validation
    # patches are the whole 64 x 64 images)
    t = compose(Yv, Cv, 2, grid).reshape(-1, 3).astype(np.float64)
    A = (np.asarray(weights) * np.where(t >= 0, t, 0)).sum(0)
    constant = float(-(A * np.log(A / A.sum())).sum() / len(t))
    v = hist["val_prob_class_loss"]
    print("val_prob_class_loss per epoch:", v, "best constant:", constant)
    assert v[-1] < v[0] and v[-1] < constant
    for f in ("weights_best.npz", "weights_last.npz"):
        assert os.path.exists(os.path.join(str(tmp_path), "classes", f))
    loaded = StarDist2D(None, name="classes", basedir=str(tmp_path), device=DEV)
    n = 0
    for x in Xv:
        _, res = loaded.predict_instances(x)
        cid, cp = np.asarray(res["class_id"]), np.asarray(res["class_prob"])
        n += len(cid)
        assert len(cid) == len(res["prob"]) and cp.shape == (len(cid), 3)
        assert ((cid >= 1) & (cid <= 2)).all(), cid
        assert np.allclose(cp.sum(-1), 1, atol=1e-5)
    print("instances with a class:", n)
    assert n > 0


def test_missing_training_label_surfaces_in_train():
    from stardist_amd.models import Config2D, StarDist2D
    X, Y, C = (list(v) for v in zip(*[_two_radii(64, s) for s in range(2)]))
    cfg = Config2D(n_rays=8, grid=(2, 2), n_classes=2, unet_n_depth=1, train_patch_size=(64, 64), train_batch_size=2)
    bad = [dict(C[0]), dict(C[1])]
    del bad[1][2]
    with pytest.raises(ValueError, match="all gt labels should be present in class dict provided"):
        StarDist2D(cfg, basedir=None, device=DEV, seed=0).train(X, Y, validation_data=(X, Y, C), classes=bad, epochs=1, steps_per_epoch=1)
    with pytest.raises(ValueError, match="all gt labels should be present in class dict provided"):
        StarDist2D(cfg, basedir=None, device=DEV, seed=0).train(X, Y, validation_data=(X, Y, bad), classes=C, epochs=1, steps_per_epoch=1)


def test_single_class_history_keys_unchanged():
    from stardist_amd.models import Config2D, StarDist2D
    from stardist_amd.training import HISTORY_KEYS
    X, Y, _ = (list(v) for v in zip(*[_two_radii(64, s) for s in range(2)]))
    cfg = Config2D(n_rays=8, grid=(2, 2), unet_n_depth=1, train_patch_size=(64, 64), train_batch_size=2)
    hist = StarDist2D(cfg, basedir=None, device=DEV, seed=0).train(X, Y, validation_data=(X, Y), epochs=1, steps_per_epoch=2)
    assert tuple(hist) == HISTORY_KEYS and len(HISTORY_KEYS) == 15
    assert all(len(v) == 1 and np.isfinite(v[0]) for v in hist.values())
