"""CPU: the host side of StarDist3D.train (stardist_amd/training3d.py).
  * patch sampling: the reference's sample_patches / get_valid_inds (stardist/sample_patches.py) and StarDistDataBase.get_valid_inds
    (stardist/models/base.py), executed from its sources at run time (test_cpu_training's sampler: StarDistData3D.__getitem__ draws
    its patches as StarDistData2D does, model3d.py:51-58), give the same patches as TrainData3D.sample after the same np.random.seed,
    for foreground_prob 0, 0.9 and 1 and anisotropic patch sizes;
  * scope: check_trainable3d raises NotImplementedError naming each setting outside it; the default Config3D and the 3D_demo
    configuration pass."""
import json
import os

import numpy as np
import pytest

from test_cpu_training import _reference_sampler, needs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _volumes(n=3, seed=0):
    rng = np.random.RandomState(seed)
    Y, X = [], []
    for i in range(n):
        shape = (20 + 3 * i, 50 - 4 * i, 44 + 5 * i)
        y = np.zeros(shape, np.int32)
        zz, yy, xx = np.ogrid[:shape[0], :shape[1], :shape[2]]
        for k in range(1, 7):
            c = [rng.randint(0, s) for s in shape]
            r = rng.randint(3, 8)
            y[(2 * (zz - c[0])) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 < r * r] = k
        if i == 0:
            y[:, :, :25] = 0                # a region without foreground near the border
        Y.append(y)
        X.append(rng.rand(*shape).astype(np.float32))
    return X, Y


@needs_ref
@pytest.mark.parametrize("foreground_prob", [0.0, 0.9, 1.0])
@pytest.mark.parametrize("ps", [(8, 32, 24), (16, 16, 40)])
def test_patches_equal_reference(foreground_prob, ps):
    from stardist_amd.rays3d import Rays_GoldenSpiral
    from stardist_amd.training3d import TrainData3D
    X, Y = _volumes()
    bs = 2
    for seed in (0, 7):
        np.random.seed(seed)
        ref = _reference_sampler(X, Y, ps, bs, foreground_prob)
        want = [ref(i) for i in range(5)]
        np.random.seed(seed)
        d = TrainData3D(X, Y, batch_size=bs, rays=Rays_GoldenSpiral(8, anisotropy=(2, 1, 1)), length=5, patch_size=ps, grid=(1, 2, 2),
                        anisotropy=(2, 1, 1), foreground_prob=foreground_prob)
        got = [d.sample(i) for i in range(5)]
        for (xw, yw), (xg, yg) in zip(want, got):
            assert len(xw) == len(xg) == bs
            for a, b in zip(xw + yw, xg + yg):
                assert a.shape == tuple(ps) and a.dtype == b.dtype and np.array_equal(a, b)


def test_rejects_2d_data():
    from stardist_amd.rays3d import Rays_GoldenSpiral
    from stardist_amd.training3d import TrainData3D
    with pytest.raises(ValueError, match="3D"):
        TrainData3D([np.zeros((32, 32), np.float32)], [np.zeros((32, 32), np.int32)], batch_size=1, rays=Rays_GoldenSpiral(8), length=1,
                    patch_size=(16, 16))


# ---- scope
OUT_OF_SCOPE = [
    (dict(n_classes=2), "n_classes"),
    (dict(n_channel_in=2), "n_channel_in"),
    (dict(train_dist_loss="iou"), "train_dist_loss"),
    (dict(unet_batch_norm=True), "unet_batch_norm"),
    (dict(unet_dropout=0.1), "unet_dropout"),
    (dict(unet_kernel_size=(5, 5, 5)), "unet_kernel_size"),
    (dict(unet_n_filter_base=48), "unet_n_filter_base"),
    (dict(unet_n_depth=5), "unet_n_depth"),
    (dict(unet_pool=(1, 4, 4)), "unet_pool"),
    (dict(unet_activation="elu"), "unet_activation"),
    (dict(unet_last_activation="sigmoid"), "unet_last_activation"),
    (dict(net_conv_after_unet=48), "net_conv_after_unet"),
    (dict(net_conv_after_unet=0), "net_conv_after_unet"),
    (dict(backbone="resnet", resnet_batch_norm=True), "resnet_batch_norm"),
    (dict(backbone="resnet", resnet_kernel_size=(5, 5, 5)), "resnet_kernel_size"),
    (dict(backbone="resnet", resnet_n_filter_base=40), "resnet_n_filter_base"),
    (dict(backbone="resnet", resnet_n_filter_base=512, grid=(1, 2, 2)), "resnet_n_filter_base"),
    (dict(backbone="resnet", resnet_n_conv_per_block=1), "resnet_n_conv_per_block"),
    (dict(backbone="resnet", resnet_activation="tanh"), "resnet_activation"),
    (dict(backbone="resnet", net_conv_after_resnet=0), "net_conv_after_resnet"),
]


@pytest.mark.parametrize("kw, word", OUT_OF_SCOPE)
def test_out_of_scope_raises(kw, word):
    from stardist_amd.models import Config3D
    from stardist_amd.training3d import check_trainable3d
    with pytest.raises(NotImplementedError, match="^StarDist3D.train on the native kernels does not support .*%s" % word):
        check_trainable3d(Config3D(n_rays=8, **kw))


def test_grid_not_power_of_two_raises():
    from stardist_amd.models import Config3D
    from stardist_amd.training3d import check_trainable3d
    c = Config3D(n_rays=8)
    c.grid = (1, 3, 3)
    with pytest.raises(NotImplementedError, match="grid"):
        check_trainable3d(c)


def test_train_checks_the_scope_first():
    from stardist_amd.models import Config3D, StarDist3D
    m = StarDist3D(Config3D(n_rays=8, train_dist_loss="iou"), basedir=None, device="cpu")
    X = [np.zeros((16, 32, 32), np.float32)]
    Y = [np.zeros((16, 32, 32), np.int32)]
    with pytest.raises(NotImplementedError, match="train_dist_loss"):
        m.train(X, Y, validation_data=(X, Y), epochs=1, steps_per_epoch=1)


def test_in_scope_configs_pass_the_check():
    from stardist_amd.models import Config3D
    from stardist_amd.training3d import check_trainable3d
    check_trainable3d(Config3D())
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "pretrained", "StarDist3D", "3D_demo", "config.json")))
    demo = Config3D(**{k: v for k, v in cfg.items() if k not in ("n_dim", "n_channel_out", "rays_json")}, rays=cfg["n_rays"])
    assert demo.backbone == "resnet" and tuple(demo.grid) == (1, 2, 2) and demo.n_rays == 96
    check_trainable3d(demo)
    check_trainable3d(Config3D(backbone="resnet", grid=(2, 2, 2), n_rays=73))
    check_trainable3d(Config3D(backbone="resnet", grid=(1, 2, 4), n_rays=33, train_dist_loss="mse"))
    check_trainable3d(Config3D(grid=(2, 1, 1), n_rays=7, unet_pool=(1, 2, 2), unet_n_filter_base=64, unet_activation="linear"))
