"""GPU: the Keras metrics of StarDist2D/3D.train (sd_stardist_loss2d_metrics_device, training.fit).
  * the kernel's four values (kld, relevant_mae, relevant_mse, dist_iou_metric) against the float64 restatement
    training.reference_metrics: 1e-6 relative, for 1, 8 and 32 rays, pixel counts that are not a multiple of the kernel's block,
    ignored pixels and clipped probabilities; two calls give the same bits;
  * with the metrics on, the losses and both gradients are those of sd_stardist_loss2d_device bit for bit (with gradients and without);
  * StarDist2D.train: the validation metrics of the history equal reference_metrics of the trained network in float64 over the
    validation batches (a short last batch), combined by Keras' rules; the keys and the History object;
  * StarDist3D.train: the same keys, all finite, two seeded runs give the same history.
test_gpu_training_scale.py checks the metrics and losses past 2^24 gradient elements, with empty and all-foreground distance masks."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

KEYS = ["loss", "prob_loss", "dist_loss", "prob_kld", "dist_relevant_mae", "dist_relevant_mse", "dist_dist_iou_metric",
        "val_loss", "val_prob_loss", "val_dist_loss", "val_prob_kld", "val_dist_relevant_mae", "val_dist_relevant_mse",
        "val_dist_dist_iou_metric", "lr"]


def _inputs(B, h, w, R, seed):
    rng = np.random.RandomState(seed)
    z = rng.randn(B, h, w) * 4
    z[0, 0, :2] = [30.0, -30.0]                         # clipped probabilities
    prob = torch.sigmoid(torch.from_numpy(z).float())
    prob[0, 1, :3] = torch.tensor([0.0, 1.0, 1e-9])
    dist = torch.from_numpy(rng.randn(B, h, w, R) * 3).float()           # negative distances included
    pt = torch.from_numpy(rng.rand(B, h, w)).float()
    pt[0, 2, :3] = torch.tensor([0.0, 1.0, 1e-9])
    pt[torch.from_numpy(rng.rand(B, h, w) < 0.2)] = -1  # ignored pixels
    dtm = torch.from_numpy(np.concatenate([np.abs(rng.randn(B, h, w, R)) * 4, (rng.rand(B, h, w, 1) > 0.4) * rng.rand(B, h, w, 1)], -1)).float()
    return prob, dist, pt, dtm


def _call(name, prob, dist, pt, dtm, mse, reg, grads, metrics=True):
    from stardist_amd.lib import _native as N
    from stardist_amd.training import _p
    B, h, w, R = (int(v) for v in dist.shape)
    dp, dd, dpt, ddtm = (t.to(DEV).contiguous() for t in (prob, dist, pt, dtm))
    losses = torch.empty(3, dtype=torch.float64, device=DEV)
    gz = torch.empty((B, h, w), device=DEV) if grads else None
    gd = torch.empty((B, h, w, R), device=DEV) if grads else None
    args = [_p(dp), _p(dd), _p(dpt), _p(ddtm), B * h * w, R, int(mse), 1.0, 0.2, reg, _p(losses), _p(gz), _p(gd)]
    met = torch.empty(4, dtype=torch.float64, device=DEV) if metrics else None
    if name == "sd_stardist_loss2d_metrics_device":
        args.append(_p(met))
    N.dcall(dp, name, *args)
    return losses, gz, gd, met


# pixel counts 6519, 8192 (two full blocks of the kernel), 6771 and 35
@pytest.mark.parametrize("R, shape", [(1, (3, 41, 53)), (8, (2, 64, 64)), (32, (3, 37, 61)), (32, (1, 5, 7))])
def test_metrics_kernel_equals_reference(R, shape):
    from stardist_amd.training import reference_metrics
    prob, dist, pt, dtm = _inputs(*shape, R, seed=R)
    want = reference_metrics(prob.double(), dist.double(), pt.double(), dtm.double())
    for mse in (0, 1):
        _, _, _, met = _call("sd_stardist_loss2d_metrics_device", prob, dist, pt, dtm, mse, 1e-4, grads=bool(mse))
        got = met.cpu()
        for i in range(4):
            assert abs(float(got[i]) - float(want[i])) <= 1e-6 * abs(float(want[i])), (i, float(got[i]), float(want[i]))
        _, _, _, met2 = _call("sd_stardist_loss2d_metrics_device", prob, dist, pt, dtm, mse, 1e-4, grads=bool(mse))
        assert torch.equal(met, met2)


@pytest.mark.parametrize("mse, reg", [(0, 1e-4), (1, 0.0), (0, 0.5)])
def test_losses_and_gradients_unchanged(mse, reg):
    prob, dist, pt, dtm = _inputs(2, 45, 71, 16, seed=11)
    for grads in (True, False):
        l0, gz0, gd0, _ = _call("sd_stardist_loss2d_device", prob, dist, pt, dtm, mse, reg, grads)
        l1, gz1, gd1, _ = _call("sd_stardist_loss2d_metrics_device", prob, dist, pt, dtm, mse, reg, grads)
        assert torch.equal(l0, l1)
        if grads:
            assert torch.equal(gz0, gz1) and torch.equal(gd0, gd1)


def test_metrics_entry_rejects_missing_output():
    from stardist_amd.lib import _native as N
    prob, dist, pt, dtm = _inputs(1, 8, 8, 4, seed=0)
    with pytest.raises(N.NativeError, match="d_metrics"):
        _call("sd_stardist_loss2d_metrics_device", prob, dist, pt, dtm, 0, 0.0, grads=False, metrics=False)


def test_train_loss_with_metrics_keeps_losses_and_gradients():
    from test_gpu_training import _demo_batch, _demo_model
    from stardist_amd.training import train_loss
    model = _demo_model()
    x, pt, dtm = _demo_batch(model)
    params = list(model.net.parameters())
    for p in params:
        p.requires_grad_(True)
    res = []
    for met in (None, torch.empty(4, dtype=torch.float64, device=DEV)):
        for p in params:
            p.grad = None
        loss, losses = train_loss(model.net, model.config, x, pt, dtm, metrics_out=met)
        loss.backward()
        res.append((loss.detach(), losses, [p.grad.clone() for p in params], met))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert all(torch.equal(a, b) for a, b in zip(res[0][2], res[1][2]))
    assert bool(torch.isfinite(res[1][3]).all())


def _discs(S, seed):
    from test_gpu_training import _discs as discs
    return discs((S, S), max(4, S * S // 900), seed)


def test_train2d_validation_metrics_equal_reference():
    from stardist_amd.models import Config2D, StarDist2D
    from stardist_amd.training import TrainData2D, reference_metrics, targets_device
    X, Y = zip(*[_discs(96, 300 + i) for i in range(4)])
    Xv, Yv = zip(*[_discs(96, 400 + i) for i in range(5)])
    cfg = Config2D(n_rays=32, grid=(2, 2), train_patch_size=(64, 64), train_batch_size=2)
    model = StarDist2D(cfg, basedir=None, device=DEV, seed=0)
    hist = model.train(list(X), list(Y), validation_data=(list(Xv), list(Yv)), seed=3, epochs=1, steps_per_epoch=2)
    assert list(hist.keys()) == KEYS
    assert hist.history is hist and hist.epoch == [0]
    assert hist.params == {"verbose": 1, "epochs": 1, "steps": 2}
    assert all(len(v) == 1 and np.isfinite(v[0]) for v in hist.values())
    # the validation patches as train() draws them: np.random.seed(seed), then one sample of all five images
    np.random.seed(3)
    dv = TrainData2D(list(Xv), list(Yv), batch_size=5, n_rays=32, length=1, patch_size=cfg.train_patch_size, grid=cfg.grid,
                     foreground_prob=cfg.train_foreground_only, sample_ind_cache=cfg.train_sample_cache)
    xs, ys = dv.sample(0)
    net64 = copy.deepcopy(model.net).cpu().double().to(memory_format=torch.contiguous_format)
    vals, pix = [], []
    with torch.no_grad():
        for i in range(0, 5, 2):
            x = torch.from_numpy(np.stack(xs[i:i + 2])[:, None]).double()
            pt, dtm = targets_device(ys[i:i + 2], 32, cfg.grid, DEV)
            prob, dist = net64(x)
            vals.append([float(v) for v in reference_metrics(prob[:, 0], dist.permute(0, 2, 3, 1), pt.double().cpu(), dtm.double().cpu())])
            pix.append(pt.numel())
    assert pix[-1] * 2 == pix[0]                        # the last batch holds one image
    vals = np.array(vals)
    want = [vals[:, 0].mean()] + list((vals[:, 1:] * np.array(pix)[:, None]).sum(0) / sum(pix))
    for k, w in zip(["val_prob_kld", "val_dist_relevant_mae", "val_dist_relevant_mse", "val_dist_dist_iou_metric"], want):
        assert abs(hist[k][0] - w) <= 1e-5 * abs(w), (k, hist[k][0], w)


def test_train3d_history_metrics():
    from test_gpu_training3d import _balls, _small_model
    X, Y = zip(*[_balls((24, 40, 40), 12, 500 + i) for i in range(3)])
    Xv, Yv = zip(*[_balls((24, 40, 40), 12, 600 + i) for i in range(3)])
    hs = []
    for _ in range(2):
        m = _small_model("unet", train_patch_size=(16, 32, 32), train_batch_size=2)
        hs.append(m.train(list(X), list(Y), validation_data=(list(Xv), list(Yv)), seed=1, epochs=2, steps_per_epoch=2))
    h = hs[0]
    assert list(h.keys()) == KEYS and h.history is h and h.epoch == [0, 1]
    assert all(len(v) == 2 and all(np.isfinite(x) for x in v) for v in h.values())
    assert 0 <= h["val_dist_dist_iou_metric"][-1] <= 1 and h["val_prob_kld"][-1] >= 0
    assert hs[0] == hs[1]
