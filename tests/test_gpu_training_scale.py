"""GPU: the training kernels (csrc/train2d.hip, csrc/train3d.hip) at the shapes real training runs, where their work partitions take
more than one iteration: several 8 x 32 tiles per weight-gradient chunk and a ragged last chunk (2D), ragged voxel-row chunks (3D), the
2^24-float workspace cap, and the second pass of every grid-stride loop (launches are capped at 2^24 threads).  The smaller tests of
test_gpu_training.py, test_gpu_training3d.py and test_gpu_training_metrics.py reach none of these; test_cpu_training_partition.py checks,
on the partition formulas (_train_partition.py), that the case lists below still do.

  * exact comparisons: the linear kernels on ternary data (inputs, output gradients, weights and biases in {-1, 0, 1}).  Every product
    is exact and every partial sum an integer below 2^24, so f32 holds it exactly in any order, and the kernels' result must EQUAL the
    exact one.  The CPU references sum in f32 over slabs of fewer than 2^24 terms (exact for the same reason) and add the slabs in
    float64.  Covered: weight / bias gradients (sd_conv_wgrad_ndhwc_device, sd_conv3_wgrad_ndhwc_device, sd_convg_wgrad_ndhwc_device),
    data gradients through training.Conv3 (3x3 and 3x3x3 kernels) and training3d.ConvG (with their ReLU masks, the many y == 0 ties of
    integer data included), the max-pool, up-sampling / concatenation and ReLU adjoints.  Output buffers start as NaN (the kernels'
    own, and those the autograd functions allocate), so an element no thread writes fails.
  * one random-float case per weight-gradient family, with the bounds of the smaller tests (1e-5 of sum |terms|);
  * the losses and metrics (sd_stardist_loss2d_device, sd_stardist_loss2d_metrics_device) past 2^24 gradient elements, against
    reference_losses / reference_metrics in float64 (1e-6 relative), an empty distance mask (norm = eps) and an all-foreground one;
  * every entry point twice, bit-identical; the weight gradients with a larger unrelated call in between (stale workspace partials);
  * one train_loss step of the 2D_demo topology at B = 8, 272 x 272 and one of the 3D_demo configuration at its training shape, against
    float64 autograd of StarDistNet (every parameter within 1e-4 norm-wise; the loss within 1e-5, 1e-4 in 3D as in
    test_gpu_training3d.py), with a prob head scaled down (see _randomise)."""
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _exact import nan_empty as _nan_empty
from _training_cases import DEV, discs as _discs, randomise

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the cases (plain tuples, importable without a GPU: test_cpu_training_partition.py checks their regimes) ---------------------
# 2D weight gradient: (B, H, W, c0, c1, c_out, up, k); up: src0 at half resolution (the up level's first convolution)
WGRAD2D = [
    (8, 256, 256, 32, 0, 32, 0, 3),          # 2 tiles per chunk, the 2^24 cap binds
    (3, 264, 200, 64, 0, 64, 0, 3),          # 693 tiles in pairs: a ragged last chunk of one tile
    (4, 64, 64, 128, 0, 256, 0, 3),
    (4, 64, 64, 256, 0, 128, 0, 3),
    (8, 256, 256, 64, 32, 32, 1, 3),         # the up level: (64 up + 32) -> 32
    (8, 256, 256, 128, 0, 33, 0, 1),         # the heads: 8 tiles per chunk
    (4, 60, 20, 1, 0, 32, 0, 3),             # W < 32
    (4, 6, 300, 1, 0, 32, 0, 3),             # H < 8
    (6, 200, 136, 1, 0, 32, 0, 3),           # sizes not multiples of the tile
]
# 3D weight gradient: (entry, B, (D, H, W), c_in, c_out, kernel, stride); 'conv3': sd_conv3_wgrad_ndhwc_device (3x3x3, stride 1),
# 'convg': sd_convg_wgrad_ndhwc_device with TensorFlow 'same' padding
WGRAD3 = [
    ("convg", 2, (48, 96, 96), 1, 32, (7, 7, 7), (1, 1, 1)),       # the 3D_demo stem: 659 chunks of 14 rows, the last of 4
    ("conv3", 2, (48, 96, 96), 32, 32, (3, 3, 3), (1, 1, 1)),
    ("convg", 2, (48, 96, 96), 32, 64, (3, 3, 3), (1, 2, 2)),      # a strided first block convolution
    ("convg", 2, (48, 96, 96), 32, 64, (1, 1, 1), (1, 2, 2)),      # its projection
    ("conv3", 2, (48, 48, 48), 64, 64, (3, 3, 3), (1, 1, 1)),      # 63 rows per chunk, the last of 9
    ("convg", 2, (47, 50, 46), 32, 64, (3, 3, 3), (2, 2, 2)),      # odd extents
]
# data gradients: Conv3 on images (B, H, W, c0, c1, c_out, up); 3D ConvG (B, (D, H, W), c_in, c_out, kernel, stride);
# Conv3 on volumes (B, (D, H, W), c0, c1, c_out, up)
DGRAD2D = [(8, 256, 256, 64, 32, 32, 1)]
DGRAD3G = [(2, (48, 96, 96), 32, 64, (3, 3, 3), (1, 2, 2))]
DGRAD3 = [(1, (48, 96, 96), 64, 32, 32, 7)]
# adjoints: element counts above 2^24 and not multiples of 256
RELU_N = [(1 << 24) + 4099]
MAXPOOL2D = [((8, 257, 255, 33), (2, 2)), ((4, 515, 255, 33), (2, 1))]                  # (B, H, W, C), pool
MAXPOOL3D = [((2, 47, 97, 95, 20), (1, 2, 2)), ((2, 49, 97, 95, 19), (2, 2, 2))]        # (B, D, H, W, C), pool
UPCAT2D = [((8, 254, 258), 33, 31, 3)]                                                   # (B, H, W), c0, c1, up
UPCAT3D = [((1, 48, 94, 98), 63, 33, 7), ((1, 48, 94, 98), 63, 33, 6)]                  # (B, D, H, W), c0, c1, up
# losses: (n_rays, batch shape, dist_loss, background_reg, distance mask: 'mixed' / 'empty' / 'full')
LOSSES = [
    (96, (2, 47, 48, 48), "mae", 1e-4, "mixed"),
    (1, (8, 1025, 1030), "mse", 0.0, "mixed"),
    (33, (8, 255, 250), "mae", 0.5, "mixed"),
    (96, (2, 47, 48, 48), "mae", 1e-4, "empty"),
    (96, (2, 47, 48, 48), "mse", 1e-4, "full"),
]


def _tf_same(shape, k3, s3):
    """TensorFlow 'same': (padding before, output extent)"""
    O3 = tuple(-(-n // s) for n, s in zip(shape, s3))
    p3 = tuple(max((o - 1) * s + k - n, 0) // 2 for o, s, k, n in zip(O3, s3, k3, shape))
    return p3, O3


def wgrad3_geometry(case):
    """(B, (D, H, W), c_in, c_out, kernel, stride, padding, output extent) of a WGRAD3 case"""
    entry, B, shape, ci, co, k3, s3 = case
    p3, O3 = _tf_same(shape, k3, s3)
    return B, shape, ci, co, k3, s3, p3, O3


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def _tern(shape, seed):
    """ternary float32 CPU tensor: values in {-1, 0, 1}"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1, 2, shape, generator=g).float()


def _nan(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _p(t):
    from stardist_amd.training import _p as p
    return p(t)


def _call(name, anchor, *args):
    from stardist_amd.lib import _native as N
    N.dcall(anchor, name, *args)


def _up_nd(t, up, axes):
    """nearest up-sampling by 2 of a channels-last CPU tensor along the axes whose bit is set in up; axes: [(dim, bit)]"""
    for dim, bit in axes:
        if up & bit:
            t = t.repeat_interleave(2, dim=dim)
    return t


UP2D = [(1, 2), (2, 1)]                  # bit 2: y (dim 1), bit 1: x (dim 2) of (B, H, W, C)
UP3D = [(1, 4), (2, 2), (3, 1)]          # (B, D, H, W, C)


def _pad_for(x, k3, s3, p3, O3):
    """x (B, D, H, W, C) zero-padded so that every window of the output extent O3 lies inside"""
    pads = []
    for n, k, s, p, o in reversed(list(zip(x.shape[1:4], k3, s3, p3, O3))):
        pads += [p, max((o - 1) * s + k - n - p, 0)]
    return F.pad(x, [0, 0] + pads)


def _slabs(n_rows, per_row, limit=1 << 23):
    """row ranges of at most `limit` // per_row rows (at least one)"""
    step = max(1, limit // max(per_row, 1))
    return [(r, min(n_rows, r + step)) for r in range(0, n_rows, step)]


def _im2col(xp, z0, z1, k3, s3, O3):
    """(rows of the output planes z0..z1, C * taps) of the padded input xp (D', H', W', C) of one sample: column c * taps + tap"""
    kz, ky, kx = k3
    sz, sy, sx = s3
    sl = xp[z0 * sz:(z1 - 1) * sz + kz]
    u = sl.unfold(0, kz, sz).unfold(1, ky, sy).unfold(2, kx, sx)        # (z1 - z0, Ho', Wo', C, kz, ky, kx)
    u = u[:, :O3[1], :O3[2]]
    return u.reshape(-1, u.shape[3] * kz * ky * kx)


def ref_wgrad(g, x, k3, s3, p3):
    """exact weight / bias gradients of ternary data: g (B, Do, Ho, Wo, co), x (B, D, H, W, ci) float32 CPU -> dW (co, ci, *k3),
    db (co,) float64"""
    B, Do, Ho, Wo, co = g.shape
    ci = x.shape[4]
    taps = k3[0] * k3[1] * k3[2]
    O3 = (Do, Ho, Wo)
    dw = torch.zeros((co, ci * taps), dtype=torch.float64)
    for b in range(B):
        xp = _pad_for(x[b:b + 1], k3, s3, p3, O3)[0]
        for z0, z1 in _slabs(Do, Ho * Wo * ci * taps):
            cols = _im2col(xp, z0, z1, k3, s3, O3)
            gs = g[b, z0:z1].reshape(-1, co)
            assert gs.shape[0] < (1 << 24)
            dw += (gs.t() @ cols).double()
    db = g.reshape(-1, co).double().sum(0)
    return dw.reshape((co, ci) + tuple(k3)), db


def ref_forward(x, w, b, k3, s3, p3, O3, relu):
    """exact act(conv(x) + b) of ternary data: x (B, D, H, W, ci), w (co, ci, *k3) float32 CPU -> (B, *O3, co) float32"""
    B, ci, co = x.shape[0], x.shape[4], w.shape[0]
    wm = w.reshape(co, -1).t().contiguous()
    out = torch.empty((B,) + tuple(O3) + (co,))
    for bb in range(B):
        xp = _pad_for(x[bb:bb + 1], k3, s3, p3, O3)[0]
        for z0, z1 in _slabs(O3[0], O3[1] * O3[2] * ci * k3[0] * k3[1] * k3[2]):
            out[bb, z0:z1] = (_im2col(xp, z0, z1, k3, s3, O3) @ wm + b).reshape(z1 - z0, O3[1], O3[2], co)
    return torch.relu(out) if relu else out


def ref_dgrad(g, w, shape, k3, s3, p3):
    """exact data gradient of ternary data: g (B, Do, Ho, Wo, co), w (co, ci, *k3) float32 CPU -> (B, *shape, ci) float32"""
    B, Do, Ho, Wo, co = g.shape
    ci = w.shape[1]
    ext = tuple(max((o - 1) * s + k, n + p) for o, s, k, n, p in zip((Do, Ho, Wo), s3, k3, shape, p3))
    gin = torch.zeros((B,) + ext + (ci,))
    g2 = g.reshape(-1, co)
    for dz in range(k3[0]):
        for dy in range(k3[1]):
            for dx in range(k3[2]):
                c = (g2 @ w[:, :, dz, dy, dx]).reshape(B, Do, Ho, Wo, ci)
                gin[:, dz:dz + (Do - 1) * s3[0] + 1:s3[0], dy:dy + (Ho - 1) * s3[1] + 1:s3[1], dx:dx + (Wo - 1) * s3[2] + 1:s3[2]] += c
    return gin[:, p3[0]:p3[0] + shape[0], p3[1]:p3[1] + shape[1], p3[2]:p3[2] + shape[2]].contiguous()


def ref_upcat_adjoint(gcat, c0, up, axes):
    """(g0, g1) of [UpSampling(src0) | src1] from gcat (B, ..., c0 + c1): the sum over each up-sampling window, the last channels"""
    g0 = gcat[..., :c0]
    for dim, bit in axes:
        if up & bit:
            s = list(g0.shape)
            g0 = g0.reshape(s[:dim] + [s[dim] // 2, 2] + s[dim + 1:]).sum(dim + 1)
    return g0.contiguous(), gcat[..., c0:].contiguous()


def _same(got, want, what):
    got = got.cpu().double()
    want = want.double()
    bad = ~(got == want)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        pytest.fail("%s: %d of %d elements differ (first at flat %d: %r, want %r)" % (what, int(bad.sum()), bad.numel(), i,
                                                                                         float(got.flatten()[i]), float(want.flatten()[i])))


# a larger call of each weight-gradient entry with a different partition, made between the two calls of a case: the workspace then
# holds stale partials of another shape
_spoil_args = {}


def _spoil(entry):
    if entry not in _spoil_args:
        if entry == "2d":
            B, H, W, ci, co = 4, 64, 64, 256, 256
            g, x = _tern((B, H, W, co), 91).to(DEV), _tern((B, H, W, ci), 92).to(DEV)
            dw, db = _nan((co, ci, 3, 3)), _nan((co,))
            args = ("sd_conv_wgrad_ndhwc_device", g, _p(g), co, _p(x), ci, 0, None, 0, 0, B, H, W, 3, _p(dw), _p(db))
        elif entry == "conv3":
            B, S, ci, co = 2, (24, 40, 36), 96, 128
            g, x = _tern((B,) + S + (co,), 93).to(DEV), _tern((B,) + S + (ci,), 94).to(DEV)
            dw, db = _nan((co, ci, 3, 3, 3)), _nan((co,))
            args = ("sd_conv3_wgrad_ndhwc_device", g, _p(g), co, _p(x), ci, 0, None, 0, 0, B, *S, _p(dw), _p(db))
        else:
            B, S, ci, co = 2, (20, 36, 40), 128, 128
            g, x = _tern((B,) + S + (co,), 95).to(DEV), _tern((B,) + S + (ci,), 96).to(DEV)
            dw, db = _nan((co, ci, 3, 3, 3)), _nan((co,))
            args = ("sd_convg_wgrad_ndhwc_device", g, _p(g), co, _p(x), ci, B, *S, 3, 3, 3, 1, 1, 1, 1, 1, 1, *S, _p(dw), _p(db))
        _spoil_args[entry] = (args, (g, x, dw, db))
    args, _ = _spoil_args[entry]
    _call(*args)


# ---- weight gradients ----------------------------------------------------------------------------------------------------------
def _wgrad2d(tg, t0, t1, co, up, k):
    B, H, W = (int(v) for v in tg.shape[:3])
    c0, c1 = int(t0.shape[3]), (int(t1.shape[3]) if t1 is not None else 0)
    dw, db = _nan((co, c0 + c1, k, k)), _nan((co,))
    _call("sd_conv_wgrad_ndhwc_device", tg, _p(tg), co, _p(t0), c0, 3 if up else 0, _p(t1), c1, 0, B, H, W, k, _p(dw), _p(db))
    return dw, db


def _cat2d(s0, s1, up):
    x = _up_nd(s0, 3 if up else 0, UP2D)
    return torch.cat([x, s1], -1) if s1 is not None else x


@pytest.mark.parametrize("case", WGRAD2D, ids=str)
def test_wgrad2d_exact(case):
    B, H, W, c0, c1, co, up, k = case
    s0 = _tern((B, H >> up, W >> up, c0), 1)
    s1 = _tern((B, H, W, c1), 2) if c1 else None
    g = _tern((B, H, W, co), 3)
    tg, t0, t1 = g.to(DEV), s0.to(DEV), (s1.to(DEV) if s1 is not None else None)
    dw, db = _wgrad2d(tg, t0, t1, co, up, k)
    _spoil("2d")
    dw2, db2 = _wgrad2d(tg, t0, t1, co, up, k)
    x = _cat2d(s0, s1, up)
    want, want_b = ref_wgrad(g[:, None], x[:, None], (1, k, k), (1, 1, 1), (0, k // 2, k // 2))
    _same(dw, want[:, :, 0], "dW")
    _same(db, want_b, "db")
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


def _wgrad3(entry, tg, tx, tx1, B, shape, ci, co, k3, s3, p3, O3, up=0, c1=0):
    dw, db = _nan((co, ci + c1) + tuple(k3)), _nan((co,))
    if entry == "conv3":
        _call("sd_conv3_wgrad_ndhwc_device", tg, _p(tg), co, _p(tx), ci, up, _p(tx1), c1, 0, B, *shape, _p(dw), _p(db))
    else:
        _call("sd_convg_wgrad_ndhwc_device", tg, _p(tg), co, _p(tx), ci, B, *shape, *k3, *s3, *p3, *O3, _p(dw), _p(db))
    return dw, db


@pytest.mark.parametrize("case", WGRAD3, ids=str)
def test_wgrad3_exact(case):
    entry = case[0]
    B, shape, ci, co, k3, s3, p3, O3 = wgrad3_geometry(case)
    x = _tern((B,) + shape + (ci,), 4)
    g = _tern((B,) + O3 + (co,), 5)
    tg, tx = g.to(DEV), x.to(DEV)
    dw, db = _wgrad3(entry, tg, tx, None, B, shape, ci, co, k3, s3, p3, O3)
    _spoil(entry)
    dw2, db2 = _wgrad3(entry, tg, tx, None, B, shape, ci, co, k3, s3, p3, O3)
    want, want_b = ref_wgrad(g, x, k3, s3, p3)
    _same(dw, want, "dW")
    _same(db, want_b, "db")
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


def _float_bound_check(got, g, x, k3, s3, p3):
    """random floats: error <= 1e-5 of sum |terms| (float64 reference)"""
    want, _ = ref_wgrad(g.double(), x.double(), k3, s3, p3)
    scale, _ = ref_wgrad(g.double().abs(), x.double().abs(), k3, s3, p3)
    err = (got.double().cpu() - want).abs() / scale.clamp_min(1e-300)
    assert float(err.max()) <= 1e-5, float(err.max())


def test_wgrad2d_random_floats():
    B, H, W, c0, c1, co, up, k = WGRAD2D[1]
    gen = torch.Generator().manual_seed(6)
    s0 = torch.randn((B, H, W, c0), generator=gen)
    g = torch.randn((B, H, W, co), generator=gen)
    dw, _ = _wgrad2d(g.to(DEV), s0.to(DEV), None, co, 0, k)
    _float_bound_check(dw[:, :, None], g[:, None], s0[:, None], (1, k, k), (1, 1, 1), (0, 1, 1))


@pytest.mark.parametrize("case", [WGRAD3[0], WGRAD3[4]], ids=str)
def test_wgrad3_random_floats(case):
    entry = case[0]
    B, shape, ci, co, k3, s3, p3, O3 = wgrad3_geometry(case)
    gen = torch.Generator().manual_seed(7)
    x = torch.randn((B,) + shape + (ci,), generator=gen)
    g = torch.randn((B,) + O3 + (co,), generator=gen)
    dw, _ = _wgrad3(entry, g.to(DEV), x.to(DEV), None, B, shape, ci, co, k3, s3, p3, O3)
    _float_bound_check(dw, g, x, k3, s3, p3)


# ---- data gradients ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DGRAD2D, ids=str)
def test_conv3x3_backward_exact(case):
    from stardist_amd.training import Conv3
    B, H, W, c0, c1, co, up = case
    s0, s1 = _tern((B, H >> up, W >> up, c0), 11), _tern((B, H, W, c1), 12)
    w, b = _tern((co, c0 + c1, 3, 3), 13), _tern((co,), 14)
    gy = _tern((B, H, W, co), 15)
    x = _cat2d(s0, s1, up)
    y = ref_forward(x[:, None], w[:, :, None], b, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, H, W), True)[:, 0]
    assert 0.1 < float((y == 0).double().mean()) < 0.9                      # ReLU ties and zeros
    g = gy * (y > 0)
    want_w, want_b = ref_wgrad(g[:, None], x[:, None], (1, 3, 3), (1, 1, 1), (0, 1, 1))
    dcat = ref_dgrad(g[:, None], w[:, :, None], (1, H, W), (1, 3, 3), (1, 1, 1), (0, 1, 1))[:, 0]
    want0, want1 = ref_upcat_adjoint(dcat, c0, 3 if up else 0, UP2D)
    tw, tb, tgy = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True), gy.to(DEV)
    grads = []
    for _ in range(2):
        t0, t1 = s0.to(DEV).requires_grad_(True), s1.to(DEV).requires_grad_(True)
        tw.grad = tb.grad = None
        with _nan_empty():
            out = Conv3.apply(t0, t1, tw, tb, None, 3 if up else 0, True)
            out.backward(tgy)
        grads.append([t0.grad, t1.grad, tw.grad, tb.grad])
    _same(out.detach(), y, "forward")
    for got, want, what in zip(grads[0], (want0, want1, want_w[:, :, 0], want_b), ("d src0", "d src1", "dW", "db")):
        _same(got, want, what)
    assert all(torch.equal(a, c) for a, c in zip(*grads))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", DGRAD3G, ids=str)
def test_convg_backward_exact(case, relu):
    from stardist_amd.training3d import ConvG
    B, shape, ci, co, k3, s3 = case
    p3, O3 = _tf_same(shape, k3, s3)
    x = _tern((B,) + shape + (ci,), 21)
    w, b = _tern((co, ci) + k3, 22), _tern((co,), 23)
    gy = _tern((B,) + O3 + (co,), 24)
    y = ref_forward(x, w, b, k3, s3, p3, O3, relu)
    g = gy * (y > 0) if relu else gy
    want_w, want_b = ref_wgrad(g, x, k3, s3, p3)
    want_x = ref_dgrad(g, w, shape, k3, s3, p3)
    tw, tb, tgy = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True), gy.to(DEV)
    grads = []
    for _ in range(2):
        tx = x.to(DEV).requires_grad_(True)
        tw.grad = tb.grad = None
        with _nan_empty():
            out = ConvG.apply(tx, tw, tb, k3, s3, p3, O3, relu)
            out.backward(tgy)
        grads.append([tx.grad, tw.grad, tb.grad])
    _same(out.detach(), y, "forward")
    for got, want, what in zip(grads[0], (want_x, want_w, want_b), ("dx", "dW", "db")):
        _same(got, want, what)
    assert all(torch.equal(a, c) for a, c in zip(*grads))


@pytest.mark.parametrize("case", DGRAD3, ids=str)
def test_conv3x3x3_backward_exact(case):
    from stardist_amd.training import Conv3
    B, shape, c0, c1, co, up = case
    half = tuple(n >> ((up >> bit) & 1) for n, bit in zip(shape, (2, 1, 0)))
    s0, s1 = _tern((B,) + half + (c0,), 31), _tern((B,) + shape + (c1,), 32)
    w, b = _tern((co, c0 + c1, 3, 3, 3), 33), _tern((co,), 34)
    gy = _tern((B,) + shape + (co,), 35)
    x = torch.cat([_up_nd(s0, up, UP3D), s1], -1)
    k3, s3, p3 = (3, 3, 3), (1, 1, 1), (1, 1, 1)
    y = ref_forward(x, w, b, k3, s3, p3, shape, True)
    g = gy * (y > 0)
    want_w, want_b = ref_wgrad(g, x, k3, s3, p3)
    want0, want1 = ref_upcat_adjoint(ref_dgrad(g, w, shape, k3, s3, p3), c0, up, UP3D)
    del x
    tw, tb, tgy = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True), gy.to(DEV)
    grads = []
    for _ in range(2):
        t0, t1 = s0.to(DEV).requires_grad_(True), s1.to(DEV).requires_grad_(True)
        tw.grad = tb.grad = None
        with _nan_empty():
            out = Conv3.apply(t0, t1, tw, tb, None, up, True)
            out.backward(tgy)
        grads.append([t0.grad, t1.grad, tw.grad, tb.grad])
    _same(out.detach(), y, "forward")
    for got, want, what in zip(grads[0], (want0, want1, want_w, want_b), ("d src0", "d src1", "dW", "db")):
        _same(got, want, what)
    assert all(torch.equal(a, c) for a, c in zip(*grads))


# ---- adjoints ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", RELU_N)
def test_relu_mask_adjoint(n):
    dy, y = _tern((n,), 41), _tern((n,), 42)
    tdy, ty = dy.to(DEV), y.to(DEV)
    outs = []
    for _ in range(2):
        out = _nan((n,))
        _call("sd_relu_mask_device", tdy, _p(tdy), _p(ty), n, _p(out))
        outs.append(out)
    _same(outs[0], torch.where(y > 0, dy, torch.zeros(())), "relu adjoint")
    assert torch.equal(outs[0], outs[1])


def _maxpool_case(shape, pool, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, shape, generator=gen).float()            # ties: the first maximum in scan order takes the gradient
    O = tuple(s // p for s, p in zip(shape[1:-1], pool))
    go = torch.randn((shape[0],) + O + (shape[-1],), generator=gen)
    return x, go


@pytest.mark.parametrize("shape, pool", MAXPOOL2D, ids=str)
def test_maxpool2d_adjoint(shape, pool):
    x, go = _maxpool_case(shape, pool, 43)
    B, H, W, C = shape
    tx, tgo = x.to(DEV), go.to(DEV)
    outs = []
    for _ in range(2):
        gin = _nan(shape)
        _call("sd_maxpool_adjoint_ndhwc_device", tx, _p(tx), _p(tgo), C, B, H, W, pool[0], pool[1], _p(gin))
        outs.append(gin)
    xc = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(xc, pool).backward(go.permute(0, 3, 1, 2))
    _same(outs[0], xc.grad.permute(0, 2, 3, 1), "max-pool adjoint")
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("shape, pool", MAXPOOL3D, ids=str)
def test_maxpool3d_adjoint(shape, pool):
    x, go = _maxpool_case(shape, pool, 44)
    B, D, H, W, C = shape
    tx, tgo = x.to(DEV), go.to(DEV)
    outs = []
    for _ in range(2):
        gin = _nan(shape)
        _call("sd_maxpool3d_adjoint_ndhwc_device", tx, _p(tx), _p(tgo), C, B, D, H, W, *pool, _p(gin))
        outs.append(gin)
    xc = x.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    F.max_pool3d(xc, pool).backward(go.permute(0, 4, 1, 2, 3))
    _same(outs[0], xc.grad.permute(0, 2, 3, 4, 1), "max-pool adjoint")
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("shape, c0, c1, up", UPCAT2D, ids=str)
def test_upcat2d_adjoint(shape, c0, c1, up):
    B, H, W = shape
    gcat = _tern(shape + (c0 + c1,), 45)
    tg = gcat.to(DEV)
    outs = []
    for _ in range(2):
        d0, d1 = _nan((B, H >> ((up >> 1) & 1), W >> (up & 1), c0)), _nan((B, H, W, c1))
        _call("sd_upcat_adjoint_ndhwc_device", tg, _p(tg), c0, up, c1, B, H, W, _p(d0), _p(d1))
        outs.append((d0, d1))
    want0, want1 = ref_upcat_adjoint(gcat, c0, up, UP2D)
    _same(outs[0][0], want0, "d src0")
    _same(outs[0][1], want1, "d src1")
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("shape, c0, c1, up", UPCAT3D, ids=str)
def test_upcat3d_adjoint(shape, c0, c1, up):
    B, D, H, W = shape
    gcat = _tern(shape + (c0 + c1,), 46)
    tg = gcat.to(DEV)
    outs = []
    for _ in range(2):
        d0 = _nan((B, D >> ((up >> 2) & 1), H >> ((up >> 1) & 1), W >> (up & 1), c0))
        d1 = _nan((B, D, H, W, c1))
        _call("sd_upcat3d_adjoint_ndhwc_device", tg, _p(tg), c0, up, c1, B, D, H, W, _p(d0), _p(d1))
        outs.append((d0, d1))
    want0, want1 = ref_upcat_adjoint(gcat, c0, up, UP3D)
    _same(outs[0][0], want0, "d src0")
    _same(outs[0][1], want1, "d src1")
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- losses --------------------------------------------------------------------------------------------------------------------
def _loss_inputs(R, bshape, mask_kind, seed):
    rng = np.random.RandomState(seed)
    z = rng.randn(*bshape) * 4
    z.flat[:2] = [30.0, -30.0]                          # clipped probabilities
    prob = torch.sigmoid(torch.from_numpy(z).float())
    dist = torch.from_numpy(rng.randn(*bshape, R) * 3).float()
    pt = torch.from_numpy(rng.rand(*bshape)).float()
    pt[torch.from_numpy(rng.rand(*bshape) < 0.2)] = -1
    if mask_kind == "mixed":
        m = (rng.rand(*bshape, 1) > 0.4) * rng.rand(*bshape, 1)
    elif mask_kind == "empty":
        m = np.zeros(bshape + (1,))
    else:
        m = 0.05 + 0.95 * rng.rand(*bshape, 1)
    dtm = torch.from_numpy(np.concatenate([np.abs(rng.randn(*bshape, R)) * 4, m], -1)).float()
    return prob, dist, pt, dtm


@pytest.mark.parametrize("metrics", [False, True])
@pytest.mark.parametrize("R, bshape, dist_loss, reg, mask_kind", LOSSES, ids=str)
def test_losses_at_scale(R, bshape, dist_loss, reg, mask_kind, metrics):
    from stardist_amd.training import reference_losses, reference_metrics
    prob, dist, pt, dtm = _loss_inputs(R, bshape, mask_kind, 47)
    n_pix = int(np.prod(bshape))
    wts = (1.0, 0.2)
    dp, dd, dpt, ddtm = (t.to(DEV).contiguous() for t in (prob, dist, pt, dtm))
    outs = []
    for _ in range(2):
        losses = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
        met = torch.full((4,), float("nan"), dtype=torch.float64, device=DEV)
        gz, gd = _nan(bshape), _nan(bshape + (R,))
        args = (_p(dp), _p(dd), _p(dpt), _p(ddtm), n_pix, R, int(dist_loss == "mse"), wts[0], wts[1], reg, _p(losses), _p(gz), _p(gd))
        if metrics:
            _call("sd_stardist_loss2d_metrics_device", dp, *args, _p(met))
        else:
            _call("sd_stardist_loss2d_device", dp, *args)
        outs.append((losses, met, gz, gd))
    losses, met, gz, gd = outs[0]
    assert torch.equal(losses, outs[1][0]) and torch.equal(gz, outs[1][2]) and torch.equal(gd, outs[1][3])
    zl = torch.logit(prob.double()).requires_grad_(True)
    d64 = dist.double().requires_grad_(True)
    ref = reference_losses(torch.sigmoid(zl), d64, pt.double(), dtm.double(), dist_loss=dist_loss, loss_weights=wts, background_reg=reg)
    ref[2].backward()
    got = losses.cpu()
    for i in range(3):
        r = float(ref[i].detach())
        assert abs(float(got[i]) - r) <= 1e-6 * abs(r), (i, float(got[i]), r)
    assert float((gz.double().cpu() - zl.grad).norm() / zl.grad.norm()) <= 1e-6
    if float(d64.grad.norm()) > 0:
        assert float((gd.double().cpu() - d64.grad).norm() / d64.grad.norm()) <= 1e-6
    else:
        assert not bool(gd.any())
    if metrics:
        assert torch.equal(met, outs[1][1])
        with torch.no_grad():
            want = reference_metrics(prob.double(), dist.double(), pt.double(), dtm.double())
        for i, w in enumerate(want):
            assert abs(float(met[i]) - float(w)) <= 1e-6 * abs(float(w)), (i, float(met[i]), float(w))


# ---- one step of the demo configurations ---------------------------------------------------------------------------------------
def _randomise(net, seed):
    """the smaller tests' perturbation of the initial weights, and a prob head scaled down: at these shapes the initial networks' logits
    reach saturated probabilities, where the float32 sigmoid of the training step (as in Keras) alone moves every parameter's gradient
    by ~1 % from the float64 one (torch's float32 CPU autograd of the same network shows the same); the step is compared away from it"""
    randomise(net, seed)
    with torch.no_grad():
        net.prob.weight.mul_(0.1)
        net.prob.bias.zero_()


def _check_step(net, loss_fn, config, x, pt, dtm, loss_tol):
    from stardist_amd.training import reference_losses
    params = list(net.parameters())
    for p in params:
        p.requires_grad_(True)
        p.grad = None
    loss, losses = loss_fn(net, config, x, pt, dtm)
    loss.backward()
    got = [p.grad.detach().double().cpu() for p in params]
    for p in params:
        p.grad = None
    net64 = copy.deepcopy(net).cpu().double().to(memory_format=torch.contiguous_format)
    nd = x.dim() - 2
    prob, dist = net64(x.permute(0, nd + 1, *range(1, nd + 1)).double().cpu())[:2]
    c = config
    ref = reference_losses(prob[:, 0], dist.permute(0, *range(2, nd + 2), 1), pt.double().cpu(), dtm.double().cpu(),
                           dist_loss=c.train_dist_loss, loss_weights=c.train_loss_weights, background_reg=c.train_background_reg)
    ref[2].backward()
    assert abs(float(losses[2]) - float(ref[2].detach())) <= loss_tol * abs(float(ref[2].detach()))
    rels = {name: float((g - p64.grad).norm() / p64.grad.norm().clamp_min(1e-300)) for (name, p64), g in zip(net64.named_parameters(), got)}
    worst = max(rels, key=rels.get)
    assert rels[worst] <= 1e-4, (worst, rels[worst])


STEP2D = (8, 272)                     # B, patch: level 1 past 2 tiles per chunk, its ReLU tensor past 2^24 elements


def test_network_step_2d_demo():
    from stardist_amd.models import Config2D, StarDist2D
    from stardist_amd.training import targets_device, train_loss
    B, S = STEP2D
    cfg = Config2D(n_rays=32, grid=(2, 2), train_patch_size=(S, S), train_batch_size=B)
    model = StarDist2D(cfg, basedir=None, device=DEV, seed=0)
    _randomise(model.net, 5)
    xs, ys = zip(*[_discs((S, S), 40, 70 + b) for b in range(B)])
    x = torch.from_numpy(np.stack(xs)[..., None]).to(DEV)
    pt, dtm = targets_device(ys, cfg.n_rays, cfg.grid, DEV)
    _check_step(model.net, train_loss, cfg, x, pt, dtm, 1e-5)


def test_network_step_3d_demo():
    from stardist_amd.models import Config3D, StarDist3D
    from stardist_amd.rays3d import rays_from_json
    from stardist_amd.training3d import targets_device3d, train_loss3d
    with open(os.path.join(ROOT, "tests", "golden", "pretrained", "StarDist3D", "3D_demo", "config.json")) as fh:
        conf = json.load(fh)
    keys = ("n_rays", "grid", "anisotropy", "backbone", "resnet_n_blocks", "resnet_kernel_size", "resnet_n_filter_base",
            "resnet_n_conv_per_block", "resnet_activation", "resnet_batch_norm", "net_conv_after_resnet", "train_patch_size",
            "train_background_reg", "train_dist_loss", "train_loss_weights", "train_batch_size")
    cfg = Config3D(**{k: (tuple(conf[k]) if isinstance(conf[k], list) else conf[k]) for k in keys})
    model = StarDist3D(cfg, basedir=None, device=DEV, seed=0)
    _randomise(model.net, 5)
    B, shape = cfg.train_batch_size, tuple(cfg.train_patch_size)
    xs, ys = zip(*[_discs(shape, 60, 80 + b, rmin=4, rmax=9) for b in range(B)])
    x = torch.from_numpy(np.stack(xs)[..., None]).to(DEV)
    pt, dtm = targets_device3d(ys, rays_from_json(cfg.rays_json), cfg.grid, cfg.anisotropy, DEV)
    # the loss bound of test_gpu_training3d.test_network_gradient (float32 sigmoid of confident background voxels)
    _check_step(model.net, train_loss3d, cfg, x, pt, dtm, 1e-4)
