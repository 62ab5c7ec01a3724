"""GPU: StarDist2D.train on the library's own kernels (csrc/train2d.hip, stardist_amd/training.py), against float64 CPU autograd.
  * weight / bias gradients (sd_conv_wgrad_ndhwc_device) of 1 -> 32, 32 -> 32, 64 -> 64, the up-level form (64 up + 32) -> 32 and the
    1x1 heads 128 -> 33: error <= 1e-5 of sum |terms|, bit-identical over two calls;
  * data gradients with the ReLU mask and the up-sampling / concatenation adjoint: same bound;
  * the max-pool adjoint: equal to torch's CPU max-pool backward;
  * losses and their gradients (sd_stardist_loss2d_device): 1e-6 relative;
  * one step of the 2D_demo topology: every parameter's gradient within 1e-4 (norm-wise) of float64 autograd of StarDistNet;
  * the targets equal stardist_targets(); no library convolution / GEMM in a step; two seeded runs give the same bits;
  * the reference's test_model scenarios (train, save, reload, predict) and convergence on synthetic discs.
The shapes here are small: each kernel's work partition is a single iteration.  test_gpu_training_scale.py checks the same kernels at
training shapes (several tiles per weight-gradient chunk, ragged chunks, grid-stride loops past 2^24 elements), exactly on ternary
data, and one step of the 2D_demo topology at B = 8."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _training_cases import DEV, cat64, discs as _discs, f32 as _f32, randomise as _randomise

pytestmark = pytest.mark.gpu


def _conv_case(c0, c1, co, up, k=3, B=2, H=24, W=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    s0 = torch.randn((B, H >> up, W >> up, c0), generator=g, dtype=torch.float64)
    s1 = torch.randn((B, H, W, c1), generator=g, dtype=torch.float64) if c1 else None
    w = torch.randn((co, c0 + c1, k, k), generator=g, dtype=torch.float64) * 0.2
    b = torch.randn((co,), generator=g, dtype=torch.float64) * 0.1
    gy = torch.randn((B, H, W, co), generator=g, dtype=torch.float64)
    return s0, s1, w, b, gy


def _wgrad(g, s0, s1, co, up, k):
    from stardist_amd.lib import _native as N
    from stardist_amd.training import _p
    B, H, W = (int(v) for v in g.shape[:3])
    c0, c1 = int(s0.shape[3]), (int(s1.shape[3]) if s1 is not None else 0)
    dw = torch.empty((co, c0 + c1, k, k), dtype=torch.float32, device=DEV)
    db = torch.empty((co,), dtype=torch.float32, device=DEV)
    N.dcall(g, "sd_conv_wgrad_ndhwc_device", _p(g), co, _p(s0), c0, 3 if up else 0, _p(s1), c1, 0, B, H, W, k, _p(dw), _p(db))
    return dw, db


def _cat64(s0, s1, up):
    return cat64(s0, s1, 3 if up else 0)


CASES = [(1, 0, 32, 0, 3), (32, 0, 32, 0, 3), (64, 0, 64, 0, 3), (64, 32, 32, 1, 3), (128, 0, 33, 0, 1)]


@pytest.mark.parametrize("c0, c1, co, up, k", CASES)
def test_weight_gradient(c0, c1, co, up, k):
    s0, s1, w, b, gy = _conv_case(c0, c1, co, up, k)
    x = _cat64(s0, s1, up)
    gx = gy.permute(0, 3, 1, 2)
    # float64: dW = sum g * in (conv2d's weight gradient), and the sum of |terms| for the bound
    want = torch.nn.grad.conv2d_weight(x, w.shape, gx, padding=k // 2)
    scale = torch.nn.grad.conv2d_weight(x.abs(), w.shape, gx.abs(), padding=k // 2)
    dw, db = _wgrad(_f32(gy), _f32(s0), _f32(s1), co, up, k)
    err = (dw.double().cpu() - want).abs() / scale.clamp_min(1e-300)
    assert float(err.max()) <= 1e-5, float(err.max())
    want_b = gy.sum((0, 1, 2))
    assert float(((db.double().cpu() - want_b).abs() / gy.abs().sum((0, 1, 2))).max()) <= 1e-5
    dw2, db2 = _wgrad(_f32(gy), _f32(s0), _f32(s1), co, up, k)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("c0, c1, co, up, k", [c for c in CASES if c[0] != 1 and c[4] == 3])      # (the heads': test_network_gradient)
def test_data_gradient(c0, c1, co, up, k):
    from stardist_amd.training import Conv3, HeadsLoss  # noqa: F401
    s0, s1, w, b, gy = _conv_case(c0, c1, co, up, k)
    # float64 reference: relu(conv(cat(up(s0), s1))) backward
    a0 = s0.clone().requires_grad_(True)
    a1 = s1.clone().requires_grad_(True) if s1 is not None else None
    y = torch.relu(F.conv2d(_cat64(a0, a1, up), w, b, padding=1))
    gx = gy.permute(0, 3, 1, 2)
    y.backward(gx)
    # sum of |terms| of d(in): the same expression on absolute values, with the ReLU mask of the reference output
    mask = (y.detach() > 0).double()
    xa = _cat64(s0, s1, up).abs().requires_grad_(True)
    F.conv2d(xa, w.abs(), None, padding=1).backward(gx.abs() * mask)
    sc = xa.grad
    sc0 = sc[:, :c0]
    if up:
        sc0 = F.avg_pool2d(sc0, 2) * 4
    t0, t1 = _f32(s0).requires_grad_(True), (_f32(s1).requires_grad_(True) if s1 is not None else None)
    out = Conv3.apply(t0, t1, _f32(w), _f32(b), None, 3 if up else 0, True)
    out.backward(_f32(gy))
    e0 = (t0.grad.double().cpu() - a0.grad).abs() / sc0.permute(0, 2, 3, 1).clamp_min(1e-300)
    assert float(e0.max()) <= 1e-5, float(e0.max())
    if s1 is not None:
        e1 = (t1.grad.double().cpu() - a1.grad).abs() / sc[:, c0:].permute(0, 2, 3, 1).clamp_min(1e-300)
        assert float(e1.max()) <= 1e-5, float(e1.max())
    g0 = t0.grad.clone()
    t0.grad = None
    Conv3.apply(t0, t1, _f32(w), _f32(b), None, 3 if up else 0, True).backward(_f32(gy))
    assert torch.equal(g0, t0.grad)


def test_maxpool_adjoint():
    from stardist_amd.training import MaxPool
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-3, 4, (2, 22, 34, 32), generator=g).float()        # many ties: the first maximum in scan order takes the gradient
    go = torch.randn((2, 11, 17, 32), generator=g)
    xc = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(xc, (2, 2)).backward(go.permute(0, 3, 1, 2))
    t = x.to(DEV).requires_grad_(True)
    out = MaxPool.apply(t, 2, 2)
    assert torch.equal(out.cpu(), F.max_pool2d(x.permute(0, 3, 1, 2), (2, 2)).permute(0, 2, 3, 1))
    out.backward(go.to(DEV))
    assert torch.equal(t.grad.cpu(), xc.grad.permute(0, 2, 3, 1))
    # a pool of (2, 1) (grid stages) and an odd extent
    x2 = torch.randint(-3, 4, (1, 9, 8, 4), generator=g).float()
    go2 = torch.randn((1, 4, 8, 4), generator=g)
    xc2 = x2.permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(xc2, (2, 1)).backward(go2.permute(0, 3, 1, 2))
    t2 = x2.to(DEV).requires_grad_(True)
    MaxPool.apply(t2, 2, 1).backward(go2.to(DEV))
    assert torch.equal(t2.grad.cpu(), xc2.grad.permute(0, 2, 3, 1))


@pytest.mark.parametrize("dist_loss, reg", [("mae", 1e-4), ("mse", 0.0), ("mae", 0.5)])
def test_loss_and_gradients(dist_loss, reg):
    from stardist_amd.lib import _native as N
    from stardist_amd.training import _p, reference_losses
    rng = np.random.RandomState(3)
    B, h, w, R = 2, 20, 24, 16
    z = rng.randn(B, h, w) * 4
    z[0, 0, :2] = [30.0, -30.0]                         # clipped probabilities
    prob = torch.sigmoid(torch.from_numpy(z).float())
    dist = torch.from_numpy(rng.randn(B, h, w, R) * 3).float()
    pt = torch.from_numpy(rng.rand(B, h, w)).float()
    pt[torch.from_numpy(rng.rand(B, h, w) < 0.2)] = -1
    dtm = torch.from_numpy(np.concatenate([np.abs(rng.randn(B, h, w, R)) * 4, (rng.rand(B, h, w, 1) > 0.4) * rng.rand(B, h, w, 1)], -1)).float()
    wts = (1.0, 0.2)
    losses = torch.empty(3, dtype=torch.float64, device=DEV)
    gz = torch.empty((B, h, w), device=DEV)
    gd = torch.empty((B, h, w, R), device=DEV)
    dp, dd, dpt, ddtm = (t.to(DEV).contiguous() for t in (prob, dist, pt, dtm))
    N.dcall(dp, "sd_stardist_loss2d_device", _p(dp), _p(dd), _p(dpt), _p(ddtm), B * h * w, R, int(dist_loss == "mse"), wts[0], wts[1], reg,
            _p(losses), _p(gz), _p(gd))
    # float64 reference from the same float32 inputs; the prob gradient is taken w.r.t. the logit through the float64 sigmoid
    zl = torch.logit(prob.double()).requires_grad_(True)
    d64 = dist.double().requires_grad_(True)
    ref = reference_losses(torch.sigmoid(zl), d64, pt.double(), dtm.double(), dist_loss=dist_loss, loss_weights=wts, background_reg=reg)
    ref[2].backward()
    got = losses.cpu()
    for i in range(3):
        assert abs(float(got[i]) - float(ref[i])) <= 1e-6 * abs(float(ref[i])), (i, float(got[i]), float(ref[i]))
    assert float((gz.double().cpu() - zl.grad).norm() / zl.grad.norm()) <= 1e-6
    assert float((gd.double().cpu() - d64.grad).norm() / d64.grad.norm()) <= 1e-6


@pytest.mark.parametrize("dtype", [np.int32, np.uint16, np.int64])
def test_targets_equal_stardist_targets(dtype):
    from stardist_amd.targets import stardist_targets
    from stardist_amd.training import targets_device
    Y = [_discs((96, 80), 12, s)[1] for s in range(3)]
    if dtype != np.uint16:
        Y[1][:5, :7] = -1
    Y = [y.astype(dtype) for y in Y]
    for grid in [(1, 1), (2, 2), (2, 4)]:
        p, d = targets_device(Y, 17, grid, DEV)
        wp, wd = stardist_targets(Y, n_rays=17, grid=grid)
        assert np.array_equal(p.cpu().numpy(), wp[..., 0]) and np.array_equal(d.cpu().numpy(), wd)


def test_pipeline_targets_of_uint16_labels():
    """what a training step sees (TrainData2D.batch_device) for uint16 label images: the sampled patches and their stardist_targets()"""
    from stardist_amd.targets import stardist_targets
    from stardist_amd.training import TrainData2D
    xs, ys = zip(*[_discs((160, 144), 20, 50 + s) for s in range(3)])
    ys = [y.astype(np.uint16) for y in ys]
    kw = dict(batch_size=2, n_rays=32, length=4, patch_size=(64, 96), grid=(2, 2), foreground_prob=0.9)
    np.random.seed(3)
    d = TrainData2D(list(xs), ys, **kw)
    got = [d.batch_device(i, DEV) for i in range(3)]
    np.random.seed(3)
    d2 = TrainData2D(list(xs), ys, **kw)
    for i, (x, p, dtm) in enumerate(got):
        X, Y = d2.sample(i)
        assert all(y.dtype == np.uint16 for y in Y)
        wp, wd = stardist_targets(Y, n_rays=32, grid=(2, 2))
        assert np.array_equal(x.cpu().numpy()[..., 0], np.stack(X))
        assert np.array_equal(p.cpu().numpy(), wp[..., 0]) and np.array_equal(dtm.cpu().numpy(), wd)
        assert float(wd[..., :32].max()) > 0


def test_losses_without_gradients():
    """validation: the loss call without gradient buffers gives the losses of the full call, bit for bit"""
    from stardist_amd.training import train_loss
    model = _demo_model()
    x, pt, dtm = _demo_batch(model)
    with torch.no_grad():
        _, l0 = train_loss(model.net, model.config, x, pt, dtm)
    params = list(model.net.parameters())
    for p in params:
        p.requires_grad_(True)
    _, l1 = train_loss(model.net, model.config, x, pt, dtm)
    assert torch.equal(l0, l1)


def _demo_model(**kw):
    from stardist_amd.models import Config2D, StarDist2D
    cfg = Config2D(n_rays=32, grid=(2, 2), train_patch_size=(128, 128), train_batch_size=2, **kw)
    return StarDist2D(cfg, basedir=None, device=DEV, seed=0)


def _demo_batch(model, seed=0, B=2, S=128):
    from stardist_amd.training import targets_device
    xs, ys = zip(*[_discs((S, S), 14, seed * 10 + b) for b in range(B)])
    x = torch.from_numpy(np.stack(xs)[..., None]).to(DEV)
    pt, dtm = targets_device(ys, model.config.n_rays, model.config.grid, DEV)
    return x, pt, dtm


def test_network_gradient():
    from stardist_amd.training import reference_losses, train_loss
    model = _demo_model()
    _randomise(model.net, 5)
    x, pt, dtm = _demo_batch(model)
    net = model.net
    params = list(net.parameters())
    for p in params:
        p.requires_grad_(True)
        p.grad = None
    loss, losses = train_loss(net, model.config, x, pt, dtm)
    loss.backward()
    got = [p.grad.detach().double().cpu() for p in params]
    for p in params:
        p.grad = None
    net64 = copy.deepcopy(net).cpu().double().to(memory_format=torch.contiguous_format)
    prob, dist = net64(x.permute(0, 3, 1, 2).double().cpu())
    c = model.config
    ref = reference_losses(prob[:, 0], dist.permute(0, 2, 3, 1), pt.double().cpu(), dtm.double().cpu(), dist_loss=c.train_dist_loss,
                           loss_weights=c.train_loss_weights, background_reg=c.train_background_reg)
    ref[2].backward()
    assert abs(float(losses[2]) - float(ref[2])) <= 1e-5 * abs(float(ref[2]))
    for (name, p64), g in zip(net64.named_parameters(), got):
        want = p64.grad
        rel = float((g - want).norm() / want.norm().clamp_min(1e-300))
        assert rel <= 1e-4, (name, rel)


def test_no_library_convolution(monkeypatch):
    from stardist_amd.training import train_loss
    model = _demo_model()
    x, pt, dtm = _demo_batch(model)

    def boom(*a, **k):
        raise AssertionError("library convolution / GEMM called")
    for mod, name in [(F, "conv2d"), (torch, "conv2d"), (torch, "matmul"), (torch, "mm"), (F, "linear")]:
        monkeypatch.setattr(mod, name, boom)
    params = list(model.net.parameters())
    for p in params:
        p.requires_grad_(True)
    loss, _ = train_loss(model.net, model.config, x, pt, dtm)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)


def _train_set(n, S, seed):
    xs, ys = zip(*[_discs((S, S), max(4, S * S // 1600), seed + i) for i in range(n)])
    return list(xs), list(ys)


def test_training_is_deterministic():
    X, Y = _train_set(4, 160, 100)
    Xv, Yv = _train_set(2, 160, 200)
    res = []
    for _ in range(2):
        m = _demo_model()
        h = m.train(X, Y, validation_data=(Xv, Yv), seed=0, epochs=2, steps_per_epoch=5)
        res.append((h, [p.detach().cpu().clone() for p in m.net.parameters()]))
    assert res[0][0] == res[1][0]
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))
    assert len(res[0][0]["loss"]) == 2 and all(np.isfinite(v) for v in res[0][0]["val_loss"])


def _circles(S=160, n=2, seed=0):
    """the reference's test data, restated: circles of random radii in an S x S image (tests/utils.py circle_image style)"""
    rng = np.random.RandomState(seed)
    X, Y = [], []
    for i in range(n):
        yy, xx = np.mgrid[:S, :S]
        lbl = np.zeros((S, S), np.uint16)
        for k, (cy, cx) in enumerate([(S // 4, S // 4), (S // 2, 3 * S // 4), (3 * S // 4, S // 3)]):
            r = rng.randint(10, 25)
            lbl[(yy - cy - rng.randint(-5, 6)) ** 2 + (xx - cx - rng.randint(-5, 6)) ** 2 < r * r] = k + 1
        X.append((lbl > 0).astype(np.float32) + 0.05 * rng.randn(S, S).astype(np.float32))
        Y.append(lbl)
    return X, Y


@pytest.mark.parametrize("n_rays, grid", [(17, (1, 1)), (32, (2, 4))])
def test_model_train_save_load_predict(tmp_path, n_rays, grid):
    from stardist_amd.models import Config2D, StarDist2D
    X, Y = _circles()
    cfg = Config2D(n_rays=n_rays, grid=grid, train_patch_size=(128, 128), train_batch_size=2, train_epochs=2, train_steps_per_epoch=1)
    model = StarDist2D(cfg, name="stardist", basedir=str(tmp_path), device=DEV)
    hist = model.train(X, Y, validation_data=(X[:1], Y[:1]), epochs=2, steps_per_epoch=1)
    assert len(hist["val_loss"]) == 2
    for f in ("weights_best.npz", "weights_last.npz"):
        assert os.path.exists(os.path.join(str(tmp_path), "stardist", f))
    assert model.net.training is False and "_graphs" not in model.__dict__
    img = X[0]
    lbl, res = model.predict_instances(img)
    loaded = StarDist2D(None, name="stardist", basedir=str(tmp_path), device=DEV)
    lbl2, res2 = loaded.predict_instances(img)
    to_np = lambda t: t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    p1, d1 = model.predict(img)
    p2, d2 = loaded.predict(img)
    assert np.array_equal(to_np(p1), to_np(p2)) and np.array_equal(to_np(d1), to_np(d2))
    assert np.array_equal(lbl, lbl2) and np.array_equal(res["points"], res2["points"])


def test_convergence_on_discs():
    from stardist_amd.matching import matching
    from stardist_amd.models import Config2D, StarDist2D
    X, Y = _train_set(8, 256, 1000)
    Xv, Yv = _train_set(2, 256, 2000)
    cfg = Config2D(n_rays=32, grid=(2, 2), train_patch_size=(128, 128), train_batch_size=4, train_learning_rate=3e-4,
                   train_reduce_lr=None)
    model = StarDist2D(cfg, basedir=None, device=DEV, seed=0)
    hist = model.train(X, Y, validation_data=(Xv, Yv), seed=0, epochs=10, steps_per_epoch=100)
    print("val_loss per epoch:", [round(v, 4) for v in hist["val_loss"]])
    f1 = []
    for x, y in zip(*_train_set(3, 256, 3000)):
        lbl, _ = model.predict_instances(x)
        f1.append(matching(y, lbl, thresh=0.5).f1)
    print("f1 on held-out images:", f1)
    assert min(f1) >= 0.9, (f1, hist["val_loss"])
