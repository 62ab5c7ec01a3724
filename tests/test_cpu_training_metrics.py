"""CPU: the Keras metrics StarDist2D/3D.train report (stardist_amd/training.py).
  * training.reference_metrics (the formulas sd_stardist_loss2d_metrics_device evaluates) equals a numpy evaluation of the reference's
    kld, masked_metric_mae, masked_metric_mse and masked_metric_iou (stardist/models/base.py, executed from its sources) with
    ignored pixels, clipped probabilities, negative distances and an all-zero mask channel;
  * keras_epoch_metrics follows Keras' Mean rules: kld counts once per batch, the distance metrics once per pixel, which differ when
    the last batch is short;
  * the History object and its keys."""
import numpy as np
import pytest
import torch

from test_cpu_training import _batch, _NpK, needs_ref
from test_cpu_vs_reference_source import ref_functions


class _NpK2(_NpK):
    """_NpK plus the backend functions the metrics call"""
    clip = staticmethod(lambda x, lo, hi: np.clip(x, lo, hi))
    maximum = staticmethod(np.maximum)
    minimum = staticmethod(np.minimum)
    expand_dims = staticmethod(lambda x, axis=-1: np.expand_dims(x, axis))


def _ref_metric_fns():
    ns = ref_functions("models/base.py", {"generic_masked_loss", "masked_loss", "kld", "masked_metric_mae", "masked_metric_mse",
                                          "masked_metric_iou"}, dict(np=np, K=_NpK2(), backend_channels_last=lambda: True))

    def metrics(prob, dist, pt, dtm):
        """the values Keras reports for one batch: kld is a scalar, the others the mean of their per-pixel maps"""
        R = dist.shape[-1]
        dist_true, dist_mask = dtm[..., :R], dtm[..., R:]
        out = [float(ns["kld"](pt, prob))]
        for name in ("masked_metric_mae", "masked_metric_mse", "masked_metric_iou"):
            v = ns[name](dist_mask)(dist_true, dist)
            assert v.shape == dist.shape[:-1], (name, v.shape)
            out.append(float(np.mean(v)))
        return out
    return metrics


def _cases():
    for seed in range(3):
        prob, dist, pt, dtm = _batch(seed, R=(1, 8, 32)[seed])
        pt[0, 1, :3] = [0.0, 1.0, 1e-9]                 # clipped targets
        yield prob, dist, pt, dtm
    prob, dist, pt, dtm = _batch(7, B=1, h=5, w=9, R=4)
    dtm[..., -1] = 0                                    # no pixel with a distance target: every masked metric is 0
    yield prob, dist, pt, dtm


@needs_ref
def test_reference_metrics_equal_reference_formulas():
    from stardist_amd.training import reference_metrics
    want_fn = _ref_metric_fns()
    for k, (prob, dist, pt, dtm) in enumerate(_cases()):
        assert (dist < 0).any() and (pt < 0).any()
        want = want_fn(prob, dist, pt, dtm)
        got = [float(v) for v in reference_metrics(*(torch.from_numpy(a) for a in (prob, dist, pt, dtm)))]
        for i, (g, w) in enumerate(zip(got, want)):
            assert abs(g - w) <= 1e-12 * abs(w), (k, i, g, w)
        if k == 3:
            assert got[1:] == [0.0, 0.0, 0.0]
        else:
            assert all(v > 0 for v in got)


def test_epoch_metrics_follow_keras_mean_rules():
    """five images in batches of 2, 2 and 1: Keras' Mean over one scalar per batch (kld) and over the per-pixel values (the rest)"""
    from stardist_amd.training import keras_epoch_metrics
    rng = np.random.RandomState(0)
    hw = 6 * 7
    sizes = [2, 2, 1]
    per_pixel = [rng.rand(n * hw, 4) * (1 + 3 * i) for i, n in enumerate(sizes)]        # the per-pixel values of each batch
    values = np.stack([pp.mean(0) for pp in per_pixel])                                 # what one call reports per batch
    got = keras_epoch_metrics(torch.from_numpy(values), [n * hw for n in sizes]).numpy()
    once_per_batch = values.mean(0)
    per_pixel_mean = np.concatenate(per_pixel).mean(0)
    assert abs(got[0] - once_per_batch[0]) <= 1e-14 * once_per_batch[0]
    assert np.all(np.abs(got[1:] - per_pixel_mean[1:]) <= 1e-14 * per_pixel_mean[1:])
    # the short last batch makes the two rules differ
    assert np.all(np.abs(once_per_batch - per_pixel_mean) > 1e-3 * per_pixel_mean)
    # equal batches (the training steps): both rules give the mean over steps
    eq = keras_epoch_metrics(torch.from_numpy(values), [hw] * 3).numpy()
    assert np.allclose(eq, once_per_batch, rtol=1e-14, atol=0)
    with pytest.raises(ValueError):
        keras_epoch_metrics(torch.from_numpy(values), [hw] * 2)


def test_history_object():
    from stardist_amd.training import History
    h = History(epochs=3, steps=10)
    assert list(h) == ["loss", "prob_loss", "dist_loss", "prob_kld", "dist_relevant_mae", "dist_relevant_mse", "dist_dist_iou_metric",
                       "val_loss", "val_prob_loss", "val_dist_loss", "val_prob_kld", "val_dist_relevant_mae", "val_dist_relevant_mse",
                       "val_dist_dist_iou_metric", "lr"]
    assert isinstance(h, dict) and h.history is h
    assert h.epoch == [] and h.params == {"verbose": 1, "epochs": 3, "steps": 10}
    h["val_loss"].append(1.5)
    assert h.history["val_loss"] == [1.5]
