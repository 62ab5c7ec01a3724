"""CPU: the host side of StarDist2D.train (stardist_amd/training.py).
  * patch sampling: the reference's sample_patches / get_valid_inds (stardist/sample_patches.py) and StarDistDataBase.get_valid_inds
    (stardist/models/base.py), executed from its sources at run time, draw the same patches as TrainData2D.sample after the same
    np.random.seed; csbdeep (absent) is stood in for by its published `choice` and RollingSequence.batch.
  * losses: the float64 restatement (training.reference_losses, the formulas sd_stardist_loss2d_device evaluates) equals a numpy
    evaluation of the reference's generic_masked_loss / masked_loss_* (base.py:34-60, executed from its sources) and of prob_loss
    (base.py:315-318, restated with Keras' binary_crossentropy), with ignored pixels (prob = -1) and background regularisation.
  * scope: train raises NotImplementedError naming each configuration outside it."""
import os
import random
import types

import numpy as np
import pytest
import torch

from test_cpu_reference_build import ref_methods
from test_cpu_vs_reference_source import REF, _raise, ref_functions

needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference sources (build container only)")


# ---- csbdeep names, restated (csbdeep.utils.choice, csbdeep.internals.train.RollingSequence.batch)
def _csbdeep_choice(population, k=1, replace=True):
    state = random.getstate()
    try:
        random.seed(np.random.randint(np.iinfo(int).min, np.iinfo(int).max))
        return random.choices(population, k=k) if replace else random.sample(population, k=k)
    finally:
        random.setstate(state)


class _Rolling(object):
    def __init__(self, data_size, batch_size):
        self.data_size, self.batch_size, self.index_map = data_size, batch_size, {}

    def _index(self, loop):
        return self.index_map.setdefault(loop, np.random.permutation(self.data_size)) if loop not in self.index_map else self.index_map[loop]

    def batch(self, i):
        pos = i * self.batch_size
        loop, pos_loop = pos // self.data_size, pos % self.data_size
        sl = slice(pos_loop, pos_loop + self.batch_size)
        index = self._index(loop)
        _loop = loop
        while sl.stop > len(index):
            _loop += 1
            index = np.concatenate((index, self._index(_loop)))
        return index[sl]


def _images(n=3, seed=0):
    rng = np.random.RandomState(seed)
    Y, X = [], []
    for i in range(n):
        H, W = 90 + 7 * i, 100 - 5 * i
        y = np.zeros((H, W), np.int32)
        for k in range(1, 8):
            cy, cx, r = rng.randint(0, H), rng.randint(0, W), rng.randint(3, 9)
            yy, xx = np.ogrid[:H, :W]
            y[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = k
        if i == 0:
            y[:, :30] = 0                   # a region without foreground near the border
        Y.append(y)
        X.append(rng.rand(H, W).astype(np.float32))
    return X, Y


def _reference_sampler(X, Y, patch_size, batch_size, foreground_prob):
    from scipy.ndimage import maximum_filter
    ns = ref_functions("sample_patches.py", {"sample_patches", "get_valid_inds"}, dict(np=np, _raise=_raise, choice=_csbdeep_choice))
    mns = dict(np=np)
    meth = ref_methods("models/base.py", "StarDistDataBase", {"get_valid_inds"}, mns)
    mns["get_valid_inds"] = ns["get_valid_inds"]          # the method's global of that name is the module function (base.py:27)
    obj = types.SimpleNamespace(Y=Y, patch_size=patch_size, foreground_prob=foreground_prob, maxfilter_patch_size=patch_size,
                                sample_ind_cache=True, _ind_cache_fg={}, _ind_cache_all={}, lock=__import__("threading").Lock(),
                                max_filter=lambda y, p: maximum_filter(y, p, mode="constant"))
    obj.get_valid_inds = lambda k, foreground_prob=None: meth["get_valid_inds"](obj, k, foreground_prob)
    roll = _Rolling(len(X), batch_size)

    def sample(i):                                      # StarDistData2D.__getitem__, the patch part (model2d.py:51-58)
        idx = roll.batch(i)
        arrays = [ns["sample_patches"]((Y[k], X[k]), patch_size=patch_size, n_samples=1, valid_inds=obj.get_valid_inds(k)) for k in idx]
        return list(zip(*[(x[0], y[0]) for y, x in arrays]))
    return sample


@needs_ref
@pytest.mark.parametrize("foreground_prob", [0.0, 0.9, 1.0])
def test_patches_equal_reference(foreground_prob):
    from stardist_amd.training import TrainData2D
    X, Y = _images()
    ps, bs = (48, 64), 2
    for seed in (0, 7):
        np.random.seed(seed)
        ref = _reference_sampler(X, Y, ps, bs, foreground_prob)
        want = [ref(i) for i in range(5)]
        np.random.seed(seed)
        d = TrainData2D(X, Y, batch_size=bs, n_rays=8, length=5, patch_size=ps, grid=(1, 1), foreground_prob=foreground_prob)
        got = [d.sample(i) for i in range(5)]
        for (xw, yw), (xg, yg) in zip(want, got):
            assert len(xw) == len(xg) == bs
            for a, b in zip(xw + yw, xg + yg):
                assert a.dtype == b.dtype and np.array_equal(a, b)


@needs_ref
def test_valid_inds_equal_reference():
    from scipy.ndimage import maximum_filter
    from stardist_amd.training import get_valid_inds
    ns = ref_functions("sample_patches.py", {"get_valid_inds"}, dict(np=np, _raise=_raise))
    _, Y = _images()
    for y in Y:
        for ps in [(16, 16), (33, 20), (y.shape[0], 8)]:
            for filt in (None, lambda a, p: maximum_filter(a, p, mode="constant") > 0):
                w, g = ns["get_valid_inds"](y, ps, patch_filter=filt), get_valid_inds(y, ps, patch_filter=filt)
                assert len(w) == len(g) and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(w, g))


# ---- losses
class _NpK(object):
    """the Keras backend functions base.py's losses call, on numpy float64"""
    floatx = staticmethod(lambda: "float64")
    epsilon = staticmethod(lambda: 1e-7)
    cast = staticmethod(lambda x, dt: np.asarray(x, np.float64))
    mean = staticmethod(lambda x, axis=None: np.mean(x, axis=axis))
    abs = staticmethod(np.abs)
    square = staticmethod(np.square)

    @staticmethod
    def binary_crossentropy(target, output):            # tf.keras.backend.binary_crossentropy, from_logits=False
        eps = 1e-7
        output = np.clip(output, eps, 1 - eps)
        return -(target * np.log(output + eps) + (1 - target) * np.log(1 - output + eps))


def _batch(seed, B=2, h=12, w=10, R=8, neg=True):
    rng = np.random.RandomState(seed)
    prob = rng.rand(B, h, w)
    prob[0, 0, :3] = [0.0, 1.0, 1e-9]                  # clipped values
    pt = rng.rand(B, h, w)
    if neg:
        pt[rng.rand(B, h, w) < 0.2] = -1
    dist = rng.randn(B, h, w, R) * 3
    dtm = np.concatenate([np.abs(rng.randn(B, h, w, R)) * 4, (rng.rand(B, h, w, 1) > 0.4) * rng.rand(B, h, w, 1)], -1)
    return prob, dist, pt, dtm


@needs_ref
@pytest.mark.parametrize("dist_loss", ["mae", "mse"])
@pytest.mark.parametrize("reg", [0.0, 1e-4, 0.3])
def test_losses_equal_reference_formulas(dist_loss, reg):
    from stardist_amd.training import reference_losses
    K = _NpK()
    ns = ref_functions("models/base.py", {"generic_masked_loss", "masked_loss", "masked_loss_mae", "masked_loss_mse"}, dict(np=np, K=K))
    for seed in range(3):
        prob, dist, pt, dtm = _batch(seed)
        w = (1.0, 0.2)
        # prob_loss (base.py:315-318): mean of the cross entropy over the pixels with y_true >= 0
        mask = pt >= 0
        want_p = K.mean(K.binary_crossentropy(pt[mask], prob[mask]), axis=-1)
        # dist_loss (base.py:322-324) + Keras' mean over the per-pixel map
        R = dist.shape[-1]
        dist_true, dist_mask = dtm[..., :R], dtm[..., R:]
        masked = ns["masked_loss_%s" % dist_loss](dist_mask, reg_weight=reg)
        want_d = np.mean(masked(dist_true, dist))
        got = reference_losses(*(torch.from_numpy(a) for a in (prob, dist, pt, dtm)), dist_loss=dist_loss, loss_weights=w, background_reg=reg)
        got = [float(g) for g in got]
        assert abs(got[0] - want_p) <= 1e-13 * abs(want_p)
        assert abs(got[1] - want_d) <= 1e-13 * abs(want_d)
        assert abs(got[2] - (w[0] * want_p + w[1] * want_d)) <= 1e-13 * abs(got[2])


# ---- scope
@pytest.mark.parametrize("kw, word", [
    (dict(n_classes=2), "n_classes"),
    (dict(n_channel_in=3), "n_channel_in"),
    (dict(unet_batch_norm=True), "unet_batch_norm"),
    (dict(train_dist_loss="iou"), "train_dist_loss"),
    (dict(train_shape_completion=True), "train_shape_completion"),
    (dict(unet_n_filter_base=48), "unet_n_filter_base"),
    (dict(unet_dropout=0.1), "unet_dropout"),
    (dict(unet_kernel_size=(5, 5)), "unet_kernel_size"),
    (dict(unet_activation="elu"), "unet_activation"),
])
def test_out_of_scope_raises(kw, word):
    from stardist_amd.models import Config2D, StarDist2D
    m = StarDist2D(Config2D(n_rays=8, **kw), basedir=None, device="cpu")
    X = [np.zeros((64, 64), np.float32)]
    Y = [np.zeros((64, 64), np.int32)]
    with pytest.raises(NotImplementedError, match=word):
        m.train(X, Y, validation_data=(X, Y), epochs=1, steps_per_epoch=1)


def test_in_scope_config_passes_the_check():
    from stardist_amd.models import Config2D
    from stardist_amd.training import check_trainable
    check_trainable(Config2D(n_rays=32, grid=(2, 2)))
    check_trainable(Config2D(n_rays=17, grid=(1, 4), train_dist_loss="mse", unet_n_filter_base=64, unet_n_depth=2))
