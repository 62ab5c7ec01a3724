"""GPU: StarDist3D.train on the library's own kernels (csrc/train3d.hip, stardist_amd/training3d.py), against float64 CPU autograd.
  * weight / bias gradients of 3x3x3 layers (one or two sources, up masks 4 / 7 / 6, c_in = 1) and of general layers (7x7x7 with
    c_in = 1, strided 3x3x3 and 1x1x1 at (1, 2, 2) / (2, 2, 2), TensorFlow 'same' padding, odd and even extents): error <= 1e-5 of
    sum |terms|, bit-identical over two calls;
  * data gradients of the stride-1 3x3x3 layer (two sources, up-sampling) and of strided layers: same bound;
  * the 3D max-pool (ties) and up-sampling / concatenation adjoints: equal to torch's CPU results;
  * targets equal stardist_targets() bit for bit; the loss kernel on 3D-shaped inputs equals reference_losses;
  * one step of a small U-Net and a small ResNet: every parameter's gradient within 1e-4 (norm-wise) of float64 autograd of StarDistNet;
  * no library convolution / GEMM in a step; two seeded runs give the same bits;
  * the reference's test_model3D scenarios in scope (train, predict with and without tiles, save, reload), test_foreground_warning,
    and convergence on synthetic anisotropic balls.
The shapes here are small: each kernel's work partition is a single iteration.  test_gpu_training_scale.py checks the same kernels at
the 3D_demo's training shape (ragged voxel-row chunks, k_dgrad3 and the adjoints past 2^24 elements), exactly on ternary data, and
one step of the 3D_demo configuration."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _training_cases import DEV, balls as _balls, cat64 as _cat64, f32 as _f32, randomise as _randomise, up_nearest as _up3

pytestmark = pytest.mark.gpu


def _half(shape, up):
    D, H, W = shape
    return (D >> ((up >> 2) & 1), H >> ((up >> 1) & 1), W >> (up & 1))


def _conv3_case(c0, c1, co, up, B=2, shape=(6, 8, 10), seed=0):
    g = torch.Generator().manual_seed(seed)
    s0 = torch.randn((B,) + _half(shape, up) + (c0,), generator=g, dtype=torch.float64)
    s1 = torch.randn((B,) + shape + (c1,), generator=g, dtype=torch.float64) if c1 else None
    w = torch.randn((co, c0 + c1, 3, 3, 3), generator=g, dtype=torch.float64) * 0.2
    b = torch.randn((co,), generator=g, dtype=torch.float64) * 0.1
    gy = torch.randn((B,) + shape + (co,), generator=g, dtype=torch.float64)
    return s0, s1, w, b, gy


CONV3 = [(32, 0, 32, 0), (1, 0, 32, 0), (64, 32, 32, 4), (32, 32, 64, 7), (64, 32, 32, 6)]


@pytest.mark.parametrize("c0, c1, co, up", CONV3)
def test_conv3_weight_gradient(c0, c1, co, up):
    from stardist_amd.lib import _native as N
    from stardist_amd.training import _p
    s0, s1, w, b, gy = _conv3_case(c0, c1, co, up)
    x = _cat64(s0, s1, up)
    gx = gy.permute(0, 4, 1, 2, 3)
    want = torch.nn.grad.conv3d_weight(x, w.shape, gx, padding=1)
    scale = torch.nn.grad.conv3d_weight(x.abs(), w.shape, gx.abs(), padding=1)
    B, D, H, W = (int(v) for v in gy.shape[:4])
    t0, t1, tg = _f32(s0), _f32(s1), _f32(gy)
    outs = []
    for _ in range(2):
        dw = torch.empty(tuple(w.shape), dtype=torch.float32, device=DEV)
        db = torch.empty((co,), dtype=torch.float32, device=DEV)
        N.dcall(tg, "sd_conv3_wgrad_ndhwc_device", _p(tg), co, _p(t0), c0, up, _p(t1), c1, 0, B, D, H, W, _p(dw), _p(db))
        outs.append((dw, db))
    dw, db = outs[0]
    err = (dw.double().cpu() - want).abs() / scale.clamp_min(1e-300)
    assert float(err.max()) <= 1e-5, float(err.max())
    want_b = gy.sum((0, 1, 2, 3))
    assert float(((db.double().cpu() - want_b).abs() / gy.abs().sum((0, 1, 2, 3))).max()) <= 1e-5
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _tf_pads(shape, k3, s3):
    from stardist_amd.models.unet import tf_same_pad_before
    p = tuple(tf_same_pad_before(n, k, s) for n, k, s in zip(shape, k3, s3))
    O = tuple(-(-n // s) for n, s in zip(shape, s3))
    total = tuple(max((o - 1) * s + k - n, 0) for o, s, k, n in zip(O, s3, k3, shape))
    return p, O, total


def _convg64(x, w, b, k3, s3):
    """float64 reference of a TensorFlow-'same' convolution: x (B, C, D, H, W)"""
    p, O, total = _tf_pads(tuple(x.shape[2:]), k3, s3)
    pads = []
    for d in reversed(range(3)):
        pads += [p[d], total[d] - p[d]]
    return F.conv3d(F.pad(x, pads), w, b, stride=s3)


GENERAL = [((7, 7, 7), (1, 1, 1), 1, 32, (6, 9, 11)), ((7, 7, 7), (1, 1, 1), 1, 32, (8, 10, 12)),
           ((3, 3, 3), (1, 2, 2), 32, 64, (5, 9, 11)), ((3, 3, 3), (1, 2, 2), 32, 64, (6, 8, 10)),
           ((3, 3, 3), (2, 2, 2), 32, 64, (7, 9, 10)), ((3, 3, 3), (2, 2, 2), 64, 64, (6, 8, 12)),
           ((1, 1, 1), (1, 2, 2), 32, 64, (5, 9, 11)), ((1, 1, 1), (2, 2, 2), 32, 64, (6, 8, 10))]


def _general_case(k3, ci, co, shape, seed=1, B=2):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B,) + shape + (ci,), generator=g, dtype=torch.float64)
    w = torch.randn((co, ci) + k3, generator=g, dtype=torch.float64) * 0.1
    b = torch.randn((co,), generator=g, dtype=torch.float64) * 0.1
    return x, w, b


@pytest.mark.parametrize("k3, s3, ci, co, shape", GENERAL)
def test_general_weight_gradient(k3, s3, ci, co, shape):
    from stardist_amd.lib import _native as N
    from stardist_amd.training import _p
    x, w, b = _general_case(k3, ci, co, shape)
    p3, O3, _ = _tf_pads(shape, k3, s3)
    g = torch.Generator().manual_seed(9)
    gy = torch.randn((x.shape[0],) + O3 + (co,), generator=g, dtype=torch.float64)
    xc = x.permute(0, 4, 1, 2, 3)
    w64 = w.clone().requires_grad_(True)
    _convg64(xc, w64, None, k3, s3).backward(gy.permute(0, 4, 1, 2, 3))
    wa = w.abs().requires_grad_(True)
    _convg64(xc.abs(), wa, None, k3, s3).backward(gy.abs().permute(0, 4, 1, 2, 3))
    B = int(x.shape[0])
    tx, tg = _f32(x), _f32(gy)
    outs = []
    for _ in range(2):
        dw = torch.empty(tuple(w.shape), dtype=torch.float32, device=DEV)
        db = torch.empty((co,), dtype=torch.float32, device=DEV)
        N.dcall(tg, "sd_convg_wgrad_ndhwc_device", _p(tg), co, _p(tx), ci, B, *shape, *k3, *s3, *p3, *O3, _p(dw), _p(db))
        outs.append((dw, db))
    err = (outs[0][0].double().cpu() - w64.grad).abs() / wa.grad.clamp_min(1e-300)
    assert float(err.max()) <= 1e-5, float(err.max())
    want_b = gy.sum((0, 1, 2, 3))
    assert float(((outs[0][1].double().cpu() - want_b).abs() / gy.abs().sum((0, 1, 2, 3))).max()) <= 1e-5
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("c0, c1, co, up", [c for c in CONV3 if c[0] != 1])
def test_conv3_data_gradient(c0, c1, co, up):
    from stardist_amd.training import Conv3
    s0, s1, w, b, gy = _conv3_case(c0, c1, co, up)
    a0 = s0.clone().requires_grad_(True)
    a1 = s1.clone().requires_grad_(True) if s1 is not None else None
    y = torch.relu(F.conv3d(_cat64(a0, a1, up), w, b, padding=1))
    gx = gy.permute(0, 4, 1, 2, 3)
    y.backward(gx)
    mask = (y.detach() > 0).double()
    xa = _cat64(s0, s1, up).abs().requires_grad_(True)
    F.conv3d(xa, w.abs(), None, padding=1).backward(gx.abs() * mask)
    sc = xa.grad
    sc0 = sc[:, :c0]
    if up:
        k = tuple(2 if up & bit else 1 for bit in (4, 2, 1))
        sc0 = F.avg_pool3d(sc0, k) * (k[0] * k[1] * k[2])
    t0, t1 = _f32(s0).requires_grad_(True), (_f32(s1).requires_grad_(True) if s1 is not None else None)
    Conv3.apply(t0, t1, _f32(w), _f32(b), None, up, True).backward(_f32(gy))
    e0 = (t0.grad.double().cpu() - a0.grad).abs() / sc0.permute(0, 2, 3, 4, 1).clamp_min(1e-300)
    assert float(e0.max()) <= 1e-5, float(e0.max())
    if s1 is not None:
        e1 = (t1.grad.double().cpu() - a1.grad).abs() / sc[:, c0:].permute(0, 2, 3, 4, 1).clamp_min(1e-300)
        assert float(e1.max()) <= 1e-5, float(e1.max())
    g0 = t0.grad.clone()
    t0.grad = None
    Conv3.apply(t0, t1, _f32(w), _f32(b), None, up, True).backward(_f32(gy))
    assert torch.equal(g0, t0.grad)


@pytest.mark.parametrize("k3, s3, ci, co, shape", [c for c in GENERAL if c[2] != 1])
@pytest.mark.parametrize("relu", [False, True])
def test_strided_data_gradient(k3, s3, ci, co, shape, relu):
    from stardist_amd.training3d import ConvG
    x, w, b = _general_case(k3, ci, co, shape)
    p3, O3, _ = _tf_pads(shape, k3, s3)
    g = torch.Generator().manual_seed(11)
    gy = torch.randn((x.shape[0],) + O3 + (co,), generator=g, dtype=torch.float64)
    xc = x.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    y = _convg64(xc, w, b, k3, s3)
    y = torch.relu(y) if relu else y
    y.backward(gy.permute(0, 4, 1, 2, 3))
    mask = (y.detach() > 0).double() if relu else 1.0
    xa = x.permute(0, 4, 1, 2, 3).abs().requires_grad_(True)
    _convg64(xa, w.abs(), None, k3, s3).backward(gy.abs().permute(0, 4, 1, 2, 3) * mask)
    tx = _f32(x).requires_grad_(True)
    out = ConvG.apply(tx, _f32(w), _f32(b), k3, s3, p3, O3, relu)
    assert tuple(out.shape[1:4]) == O3
    yf = y.detach().permute(0, 2, 3, 4, 1)
    assert float((out.detach().double().cpu() - yf).abs().max()) <= 1e-4 * float(yf.abs().max())
    out.backward(_f32(gy))
    err = (tx.grad.double().cpu() - xc.grad.permute(0, 2, 3, 4, 1)).abs() / xa.grad.permute(0, 2, 3, 4, 1).clamp_min(1e-300)
    assert float(err.max()) <= 1e-5, float(err.max())
    g0 = tx.grad.clone()
    tx.grad = None
    ConvG.apply(tx, _f32(w), _f32(b), k3, s3, p3, O3, relu).backward(_f32(gy))
    assert torch.equal(g0, tx.grad)


@pytest.mark.parametrize("pool, shape", [((2, 2, 2), (8, 10, 12)), ((2, 2, 2), (9, 11, 7)), ((1, 2, 2), (5, 10, 9))])
def test_maxpool3d_adjoint(pool, shape):
    from stardist_amd.training import MaxPool
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-2, 3, (2,) + shape + (32,), generator=g).float()        # many ties: the first maximum in scan order takes the gradient
    O = tuple(s // p for s, p in zip(shape, pool))
    go = torch.randn((2,) + O + (32,), generator=g)
    xc = x.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    ref = F.max_pool3d(xc, pool)
    ref.backward(go.permute(0, 4, 1, 2, 3))
    t = x.to(DEV).requires_grad_(True)
    out = MaxPool.apply(t, *pool)
    assert torch.equal(out.detach().cpu(), ref.detach().permute(0, 2, 3, 4, 1))
    out.backward(go.to(DEV))
    assert torch.equal(t.grad.cpu(), xc.grad.permute(0, 2, 3, 4, 1))


@pytest.mark.parametrize("up", [4, 7, 6, 3])
def test_upcat3d_adjoint(up):
    from stardist_amd.lib import _native as N
    from stardist_amd.training import _p
    g = torch.Generator().manual_seed(2)
    B, shape, c0, c1 = 2, (6, 8, 10), 32, 64
    gcat = torch.randint(-50, 50, (B,) + shape + (c0 + c1,), generator=g).float()     # integers: every sum is exact
    d0 = torch.empty((B,) + _half(shape, up) + (c0,), device=DEV)
    d1 = torch.empty((B,) + shape + (c1,), device=DEV)
    tg = gcat.to(DEV)
    N.dcall(tg, "sd_upcat3d_adjoint_ndhwc_device", _p(tg), c0, up, c1, B, *shape, _p(d0), _p(d1))
    # autograd of [up(s0) | s1]
    s0 = torch.zeros((B, c0) + _half(shape, up), dtype=torch.float64, requires_grad=True)
    s1 = torch.zeros((B, c1) + shape, dtype=torch.float64, requires_grad=True)
    torch.cat([_up3(s0, up), s1], 1).backward(gcat.double().permute(0, 4, 1, 2, 3))
    assert torch.equal(d0.double().cpu(), s0.grad.permute(0, 2, 3, 4, 1))
    assert torch.equal(d1.double().cpu(), s1.grad.permute(0, 2, 3, 4, 1))


# ---- targets and losses
@pytest.mark.parametrize("dtype", [np.int32, np.uint16, np.int64])
def test_targets_equal_stardist_targets(dtype):
    from stardist_amd.rays3d import Rays_GoldenSpiral
    from stardist_amd.targets import stardist_targets
    from stardist_amd.training3d import targets_device3d
    Y = [_balls((20, 36, 40), 14, s)[1] for s in range(3)]
    if dtype != np.uint16:
        Y[1][:3, :5, :7] = -1
    Y = [y.astype(dtype) for y in Y]
    for aniso in (None, (2.0, 1.0, 1.0)):
        rays = Rays_GoldenSpiral(32, anisotropy=aniso)
        for grid in [(1, 1, 1), (1, 2, 2), (2, 2, 2)]:
            p, d = targets_device3d(Y, rays, grid, aniso, DEV)
            wp, wd = stardist_targets(Y, grid=grid, rays=rays, anisotropy=aniso)
            assert np.array_equal(p.cpu().numpy(), wp[..., 0]) and np.array_equal(d.cpu().numpy(), wd)


def test_pipeline_targets():
    """what a training step sees (TrainData3D.batch_device): the sampled patches and their stardist_targets()"""
    from stardist_amd.rays3d import Rays_GoldenSpiral
    from stardist_amd.targets import stardist_targets
    from stardist_amd.training3d import TrainData3D
    xs, ys = zip(*[_balls((24, 48, 40), 20, 50 + s) for s in range(3)])
    rays = Rays_GoldenSpiral(24, anisotropy=(2, 1, 1))
    kw = dict(batch_size=2, rays=rays, length=4, patch_size=(16, 32, 24), grid=(1, 2, 2), anisotropy=(2, 1, 1), foreground_prob=0.9)
    np.random.seed(3)
    d = TrainData3D(list(xs), list(ys), **kw)
    got = [d.batch_device(i, DEV) for i in range(3)]
    np.random.seed(3)
    d2 = TrainData3D(list(xs), list(ys), **kw)
    for i, (x, p, dtm) in enumerate(got):
        X, Y = d2.sample(i)
        wp, wd = stardist_targets(Y, grid=(1, 2, 2), rays=rays, anisotropy=(2, 1, 1))
        assert np.array_equal(x.cpu().numpy()[..., 0], np.stack(X))
        assert np.array_equal(p.cpu().numpy(), wp[..., 0]) and np.array_equal(dtm.cpu().numpy(), wd)


@pytest.mark.parametrize("dist_loss, reg", [("mae", 1e-4), ("mse", 0.0)])
def test_loss_on_3d_inputs(dist_loss, reg):
    from stardist_amd.lib import _native as N
    from stardist_amd.training import _p, reference_losses
    rng = np.random.RandomState(4)
    B, d, h, w, R = 2, 6, 10, 12, 24
    z = rng.randn(B, d, h, w) * 4
    prob = torch.sigmoid(torch.from_numpy(z).float())
    dist = torch.from_numpy(rng.randn(B, d, h, w, R) * 3).float()
    pt = torch.from_numpy(rng.rand(B, d, h, w)).float()
    pt[torch.from_numpy(rng.rand(B, d, h, w) < 0.2)] = -1
    dtm = torch.from_numpy(np.concatenate([np.abs(rng.randn(B, d, h, w, R)) * 4, (rng.rand(B, d, h, w, 1) > 0.4) * rng.rand(B, d, h, w, 1)],
                                          -1)).float()
    wts = (4.0, 1.0)
    losses = torch.empty(3, dtype=torch.float64, device=DEV)
    gz = torch.empty((B, d, h, w), device=DEV)
    gd = torch.empty((B, d, h, w, R), device=DEV)
    dp, dd, dpt, ddtm = (t.to(DEV).contiguous() for t in (prob, dist, pt, dtm))
    N.dcall(dp, "sd_stardist_loss2d_device", _p(dp), _p(dd), _p(dpt), _p(ddtm), B * d * h * w, R, int(dist_loss == "mse"), wts[0], wts[1],
            reg, _p(losses), _p(gz), _p(gd))
    zl = torch.logit(prob.double()).requires_grad_(True)
    d64 = dist.double().requires_grad_(True)
    ref = reference_losses(torch.sigmoid(zl), d64, pt.double(), dtm.double(), dist_loss=dist_loss, loss_weights=wts, background_reg=reg)
    ref[2].backward()
    got = losses.cpu()
    for i in range(3):
        r = float(ref[i].detach())
        assert abs(float(got[i]) - r) <= 1e-6 * abs(r), (i, float(got[i]), r)
    assert float((gz.double().cpu() - zl.grad).norm() / zl.grad.norm()) <= 1e-6
    assert float((gd.double().cpu() - d64.grad).norm() / d64.grad.norm()) <= 1e-6


# ---- the network
def _small_model(backbone, **kw):
    from stardist_amd.models import Config3D, StarDist3D
    if backbone == "unet":
        base = dict(grid=(1, 2, 2), n_rays=16, unet_n_depth=2, unet_n_filter_base=32, net_conv_after_unet=32)
    else:
        base = dict(grid=(1, 2, 4), n_rays=16, resnet_n_blocks=2, resnet_n_filter_base=32, resnet_n_conv_per_block=3, net_conv_after_resnet=64)
    base.update(kw)
    return StarDist3D(Config3D(backbone=backbone, **base), basedir=None, device=DEV, seed=0)


def _batch(model, shape, seed=0, B=2):
    from stardist_amd.rays3d import rays_from_json
    from stardist_amd.training3d import targets_device3d
    xs, ys = zip(*[_balls(shape, 10, seed * 10 + b) for b in range(B)])
    x = torch.from_numpy(np.stack(xs)[..., None]).to(DEV)
    c = model.config
    pt, dtm = targets_device3d(ys, rays_from_json(c.rays_json), c.grid, c.anisotropy, DEV)
    return x, pt, dtm


SHAPES = {"unet": (8, 32, 24), "resnet": (6, 18, 20)}          # the ResNet's: odd extents after the first stride


@pytest.mark.parametrize("backbone", ["unet", "resnet"])
def test_network_gradient(backbone):
    from stardist_amd.training import reference_losses
    from stardist_amd.training3d import train_loss3d
    model = _small_model(backbone)
    _randomise(model.net, 5)
    x, pt, dtm = _batch(model, SHAPES[backbone])
    net = model.net
    params = list(net.parameters())
    for p in params:
        p.requires_grad_(True)
        p.grad = None
    loss, losses = train_loss3d(net, model.config, x, pt, dtm)
    loss.backward()
    got = [p.grad.detach().double().cpu() for p in params]
    for p in params:
        p.grad = None
    net64 = copy.deepcopy(net).cpu().double().to(memory_format=torch.contiguous_format)
    prob, dist = net64(x.permute(0, 4, 1, 2, 3).double().cpu())[:2]
    c = model.config
    assert tuple(prob.shape[2:]) == tuple(pt.shape[1:])
    ref = reference_losses(prob[:, 0], dist.permute(0, 2, 3, 4, 1), pt.double().cpu(), dtm.double().cpu(), dist_loss=c.train_dist_loss,
                           loss_weights=c.train_loss_weights, background_reg=c.train_background_reg)
    ref[2].backward()
    # (the float32 probability after the sigmoid carries a relative error of up to 6e-8 / (1 - p) into the cross entropy of confident
    # background voxels: the random ResNet's logits reach ~10, hence the looser bound on the loss than on the gradients below)
    assert abs(float(losses[2]) - float(ref[2])) <= 1e-4 * abs(float(ref[2]))
    for (name, p64), g in zip(net64.named_parameters(), got):
        want = p64.grad
        rel = float((g - want).norm() / want.norm().clamp_min(1e-300))
        assert rel <= 1e-4, (name, rel)


@pytest.mark.parametrize("backbone", ["unet", "resnet"])
def test_no_library_convolution(monkeypatch, backbone):
    from stardist_amd.training3d import train_loss3d
    model = _small_model(backbone)
    x, pt, dtm = _batch(model, SHAPES[backbone])

    def boom(*a, **k):
        raise AssertionError("library convolution / GEMM called")
    for mod, name in [(F, "conv3d"), (torch, "conv3d"), (torch, "matmul"), (torch, "mm"), (F, "linear")]:
        monkeypatch.setattr(mod, name, boom)
    params = list(model.net.parameters())
    for p in params:
        p.requires_grad_(True)
    loss, _ = train_loss3d(model.net, model.config, x, pt, dtm)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)


def test_losses_without_gradients():
    """validation: the loss call without gradient buffers gives the losses of the full call, bit for bit"""
    from stardist_amd.training3d import train_loss3d
    model = _small_model("resnet")
    x, pt, dtm = _batch(model, SHAPES["resnet"])
    with torch.no_grad():
        _, l0 = train_loss3d(model.net, model.config, x, pt, dtm)
    for p in model.net.parameters():
        p.requires_grad_(True)
    _, l1 = train_loss3d(model.net, model.config, x, pt, dtm)
    assert torch.equal(l0, l1)


def test_training_is_deterministic():
    X, Y = zip(*[_balls((24, 40, 40), 12, 100 + i) for i in range(3)])
    Xv, Yv = zip(*[_balls((24, 40, 40), 12, 200 + i) for i in range(2)])
    res = []
    for _ in range(2):
        m = _small_model("resnet", grid=(1, 2, 2), train_patch_size=(16, 32, 32), train_batch_size=2, anisotropy=(2, 1, 1))
        h = m.train(list(X), list(Y), validation_data=(list(Xv), list(Yv)), seed=0, epochs=2, steps_per_epoch=3)
        res.append((h, [p.detach().cpu().clone() for p in m.net.parameters()]))
    assert res[0][0] == res[1][0]
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))
    assert len(res[0][0]["loss"]) == 2 and all(np.isfinite(v) for v in res[0][0]["val_loss"])


# ---- the reference's test_model3D, in scope
def _circle_image(shape, radius=None):
    """tests/utils.py circle_image, restated: a centred ball of radius min(shape) // 4"""
    radius = min(shape) // 4 if radius is None else radius
    Xs = np.meshgrid(*tuple(np.arange(s) - s // 2 for s in shape), indexing="ij")
    return (np.sqrt(sum(X ** 2 for X in Xs)) < radius).astype(np.uint16)


@pytest.mark.parametrize("n_rays, grid, backbone", [(73, (2, 2, 2), "resnet"), (33, (1, 2, 4), "resnet"), (7, (2, 1, 1), "unet")])
def test_model_train_save_load_predict(tmp_path, n_rays, grid, backbone):
    from stardist_amd.models import Config3D, StarDist3D
    img = _circle_image((64, 80, 96))
    imgs = np.repeat(img[np.newaxis], 3, axis=0)
    rng = np.random.RandomState(0)
    X = imgs + .6 * rng.uniform(0, 1, imgs.shape)
    Y = imgs.astype(int)
    conf = Config3D(backbone=backbone, rays=n_rays, grid=grid, n_channel_in=1, use_gpu=False, train_epochs=1, train_steps_per_epoch=1,
                    train_batch_size=2, train_loss_weights=(4, 1), train_patch_size=(48, 64, 32))
    model = StarDist3D(conf, name="stardist", basedir=str(tmp_path), device=DEV)
    hist = model.train(X, Y, validation_data=(X[:2], Y[:2]), workers=1)
    assert len(hist["val_loss"]) == 1 and np.isfinite(hist["loss"][0])
    for f in ("weights_best.npz", "weights_last.npz"):
        assert os.path.exists(os.path.join(str(tmp_path), "stardist", f))
    assert model.net.training is False and "_graphs" not in model.__dict__
    to_np = lambda t: t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    p1, d1 = (to_np(t) for t in model.predict(X[0]))
    pt, dt = (to_np(t) for t in model.predict(X[0], n_tiles=(1, 2, 3)))
    assert p1.shape == pt.shape and d1.shape == dt.shape and d1.shape[-1] == n_rays
    loaded = StarDist3D(None, name="stardist", basedir=str(tmp_path), device=DEV)
    p2, d2 = (to_np(t) for t in loaded.predict(X[0]))
    assert np.array_equal(p1, p2) and np.array_equal(d1, d2)


def test_foreground_warning():
    from stardist_amd.models import Config3D, StarDist3D
    conf = Config3D(n_rays=32, train_patch_size=(16, 32, 16), train_foreground_only=1, train_steps_per_epoch=1, train_epochs=1,
                    train_batch_size=2)
    X, Y = np.ones((2, 32, 48, 16), np.float32), np.ones((2, 32, 48, 16), np.uint16)
    with pytest.warns(UserWarning):
        StarDist3D(conf, None, None, device=DEV).train(X, Y, validation_data=(X[-1:], Y[-1:]))


# ---- convergence
def _ball_set(n, seed, shape=(32, 64, 64)):
    """well-separated anisotropic balls (half the radius along z, anisotropy (2, 1, 1)) on a jittered lattice"""
    rng = np.random.RandomState(seed)
    Xs, Ys = [], []
    for _ in range(n):
        y = np.zeros(shape, np.int32)
        k = 0
        zz, yy, xx = np.ogrid[:shape[0], :shape[1], :shape[2]]
        for cz in range(8, shape[0], 16):
            for cy in range(10, shape[1], 21):
                for cx in range(10, shape[2], 21):
                    r = rng.uniform(5, 8)
                    c = (cz + rng.randint(-2, 3), cy + rng.randint(-3, 4), cx + rng.randint(-3, 4))
                    k += 1
                    y[(2 * (zz - c[0]) / r) ** 2 + ((yy - c[1]) / r) ** 2 + ((xx - c[2]) / r) ** 2 < 1] = k
        Xs.append((y > 0).astype(np.float32) * rng.uniform(0.7, 1.0) + 0.1 * rng.randn(*shape).astype(np.float32))
        Ys.append(y)
    return Xs, Ys


CONVERGE = {
    "unet": dict(backbone="unet", n_rays=32, grid=(1, 2, 2), anisotropy=(2, 1, 1), train_patch_size=(16, 48, 48)),
    "resnet": dict(backbone="resnet", n_rays=96, grid=(1, 2, 2), anisotropy=(2, 1, 1), train_patch_size=(16, 48, 48)),   # the 3D_demo topology
}
CONVERGE_STEPS = (4, 100)            # epochs, steps per epoch


def converge_f1(backbone, seed):
    """train on _ball_set from `seed`, return (F1 at IoU 0.5 of predict_instances on three held-out volumes, history)"""
    from stardist_amd.matching import matching
    from stardist_amd.models import Config3D, StarDist3D
    X, Y = _ball_set(6, 1000 + seed)
    Xv, Yv = _ball_set(2, 2000 + seed)
    cfg = Config3D(train_batch_size=2, train_learning_rate=3e-4, train_reduce_lr=None, **CONVERGE[backbone])
    model = StarDist3D(cfg, basedir=None, device=DEV, seed=seed)
    hist = model.train(X, Y, validation_data=(Xv, Yv), seed=seed, epochs=CONVERGE_STEPS[0], steps_per_epoch=CONVERGE_STEPS[1])
    f1 = []
    for x, y in zip(*_ball_set(3, 3000 + seed)):
        lbl, _ = model.predict_instances(x)
        f1.append(matching(y, lbl, thresh=0.5).f1)
    return f1, hist


@pytest.mark.parametrize("backbone", ["unet", "resnet"])
def test_convergence_on_balls(backbone):
    # measured on an MI355X for seeds 0, 1, 2: F1 1.0 on all three held-out volumes, both backbones; validation loss after 400 steps
    # 0.187-0.224 (U-Net), 0.204-0.210 (ResNet)
    f1, hist = converge_f1(backbone, 0)
    print("val_loss per epoch:", [round(v, 4) for v in hist["val_loss"]])
    print("f1 on held-out volumes:", f1)
    assert min(f1) >= 0.8, (f1, hist["val_loss"])
