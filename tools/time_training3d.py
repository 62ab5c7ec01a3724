"""Time one StarDist3D training step on the library's kernels (stardist_amd/training3d.py) for two configurations:
  * the 3D_demo topology: ResNet, 4 blocks of 3 convolutions, 32 filters, grid (1, 2, 2), anisotropy (2, 1, 1), 96 rays; batch 2 of
    48 x 96 x 96 patches;
  * the default Config3D U-Net (depth 2, 32 filters, 96 rays, grid (1, 1, 1)), same batch and patches;
split into data (patch sampling + targets), forward, backward and optimiser, next to the same step under plain torch autograd of
StarDistNet on the device (the framework's library conv3d) for scale.  The native forward includes the fused loss kernel; on the
library side the network's forward and the loss expression (training.reference_losses) are timed as separate phases.
Writes profiles/training3d_times.json.  Usage: python tools/time_training3d.py [--reps 10]"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def balls(shape, n, seed):
    rng = np.random.RandomState(seed)
    y = np.zeros(shape, np.int32)
    zz, yy, xx = np.ogrid[:shape[0], :shape[1], :shape[2]]
    for i in range(1, n + 1):
        r = rng.randint(5, 10)
        c = [rng.randint(0, s) for s in shape]
        y[(2 * (zz - c[0]) / r) ** 2 + ((yy - c[1]) / r) ** 2 + ((xx - c[2]) / r) ** 2 < 1] = i
    return (y > 0).astype(np.float32) + 0.1 * rng.randn(*shape).astype(np.float32), y


def time_config(name, cfg, X, Y, reps, dev):
    from stardist_amd.models import StarDist3D
    from stardist_amd.rays3d import rays_from_json
    from stardist_amd.training import Adam, reference_losses
    from stardist_amd.training3d import TrainData3D, train_loss3d
    model = StarDist3D(cfg, basedir=None, device=dev, seed=0)
    B = int(cfg.train_batch_size)
    np.random.seed(0)
    data = TrainData3D(X, Y, batch_size=B, rays=rays_from_json(cfg.rays_json), length=10 ** 6, patch_size=cfg.train_patch_size,
                       grid=cfg.grid, anisotropy=cfg.anisotropy, foreground_prob=0.9)
    net = model.net
    params = list(net.parameters())
    for p in params:
        p.requires_grad_(True)
    opt = Adam(params, 3e-4)
    sync = torch.cuda.synchronize

    def clock(fn):
        sync(); t0 = time.perf_counter(); r = fn(); sync(); return r, time.perf_counter() - t0

    rows = {"data": [], "forward": [], "backward": [], "optimiser": []}
    for i in range(reps + 2):
        (x, pt, dtm), td = clock(lambda: data.batch_device(i, dev))
        for p in params:
            p.grad = None
        (loss, _), tf = clock(lambda: train_loss3d(net, cfg, x, pt, dtm))
        _, tb = clock(lambda: loss.backward())
        _, to = clock(opt.step)
        if i >= 2:
            for k, v in zip(rows, (td, tf, tb, to)):
                rows[k].append(v * 1e3)
    for p in params:
        p.grad = None
    # the same step under torch autograd of the plain modules (library conv3d), float32 channels-last on the device
    ref = copy.deepcopy(net)
    ref.train()
    xr = x.permute(0, 4, 1, 2, 3).contiguous(memory_format=torch.channels_last_3d)
    topt = torch.optim.Adam(ref.parameters(), lr=3e-4, eps=1e-7)
    lib = {"forward": [], "loss": [], "backward": [], "optimiser": []}
    for i in range(reps + 2):
        topt.zero_grad(set_to_none=True)
        out, tf = clock(lambda: ref(xr))
        prob, dist = out[:2]
        l2, tl = clock(lambda: reference_losses(prob[:, 0], dist.permute(0, 2, 3, 4, 1), pt, dtm, dist_loss=cfg.train_dist_loss,
                                                 loss_weights=cfg.train_loss_weights, background_reg=cfg.train_background_reg)[2])
        _, tb = clock(lambda: l2.backward())
        _, to = clock(topt.step)
        if i >= 2:
            for k, v in zip(lib, (tf, tl, tb, to)):
                lib[k].append(v * 1e3)
    med = lambda v: float(np.median(v))
    r = {"native": {k: med(v) for k, v in rows.items()}, "torch_autograd_library_conv3d": {k: med(v) for k, v in lib.items()}}
    r["native"]["step"] = sum(r["native"].values())
    r["torch_autograd_library_conv3d"]["step"] = sum(r["torch_autograd_library_conv3d"].values())
    r["backward_ratio_native_over_library"] = r["native"]["backward"] / r["torch_autograd_library_conv3d"]["backward"]
    del model, net, ref, opt, topt
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "training3d_times.json"))
    a = ap.parse_args()
    from stardist_amd.models import Config3D
    dev = torch.device("cuda:0")
    X, Y = zip(*[balls((64, 160, 160), 150, s) for s in range(4)])
    configs = {
        "3D_demo_resnet": Config3D(backbone="resnet", n_rays=96, grid=(1, 2, 2), anisotropy=(2, 1, 1), resnet_n_blocks=4, resnet_n_filter_base=32,
                                   resnet_n_conv_per_block=3, net_conv_after_resnet=128, train_patch_size=(48, 96, 96), train_batch_size=2),
        "default_unet": Config3D(n_rays=96, train_patch_size=(48, 96, 96), train_batch_size=2),
    }
    res = {
        "what": "one training step, batch 2 of 48 x 96 x 96 patches; median of %d steps after 2 warm-up steps, wall clock around each "
                "synchronised phase, ms.  native forward = network + heads + fused loss kernel; library forward = the network alone, "
                "its loss expression timed as 'loss'; both backward phases include the loss's gradient" % a.reps,
        "device": torch.cuda.get_device_name(0),
    }
    for name, cfg in configs.items():
        res[name] = time_config(name, cfg, list(X), list(Y), a.reps, dev)
        print(name, json.dumps(res[name]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
