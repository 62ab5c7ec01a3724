"""Time one StarDist2D training step (2D_demo topology: grid (2, 2), 32 rays, depth 3, 32 filters; batch 4 of 256^2 patches) on the
library's kernels (stardist_amd/training.py), split into data (patch sampling + targets), forward, backward and optimiser, next to the
same step under plain torch autograd of StarDistNet on the device (the framework's library convolutions) for scale.  The native forward
includes the fused loss kernel; on the library side the network's forward and the loss expression (training.reference_losses, torch
element-wise ops with a boolean-mask gather that synchronises) are timed as separate phases.
Writes profiles/training_times.json.  Usage: python tools/time_training.py [--reps 20]"""
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


def discs(S, n, seed):
    rng = np.random.RandomState(seed)
    y = np.zeros((S, S), np.int32)
    for i in range(1, n + 1):
        r, cy, cx = rng.randint(4, 11), rng.randint(0, S), rng.randint(0, S)
        yy, xx = np.ogrid[:S, :S]
        y[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = i
    return (y > 0).astype(np.float32) + 0.1 * rng.randn(S, S).astype(np.float32), y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "training_times.json"))
    a = ap.parse_args()
    from stardist_amd.models import Config2D, StarDist2D
    from stardist_amd.training import Adam, TrainData2D, reference_losses, train_loss
    dev = torch.device("cuda:0")
    B, S = 4, 256
    cfg = Config2D(n_rays=32, grid=(2, 2), train_patch_size=(S, S), train_batch_size=B)
    model = StarDist2D(cfg, basedir=None, device=dev, seed=0)
    X, Y = zip(*[discs(512, 120, s) for s in range(8)])
    np.random.seed(0)
    data = TrainData2D(list(X), list(Y), batch_size=B, n_rays=32, length=10 ** 6, patch_size=(S, S), grid=(2, 2), foreground_prob=0.9)
    net = model.net
    params = list(net.parameters())
    for p in params:
        p.requires_grad_(True)
    opt = Adam(params, 3e-4)
    sync = torch.cuda.synchronize

    def clock(fn):
        sync(); t0 = time.perf_counter(); r = fn(); sync(); return r, time.perf_counter() - t0

    rows = {"data": [], "forward": [], "backward": [], "optimiser": []}
    for i in range(a.reps + 3):
        (x, pt, dtm), td = clock(lambda: data.batch_device(i, dev))
        for p in params:
            p.grad = None
        (loss, _), tf = clock(lambda: train_loss(net, cfg, x, pt, dtm))
        _, tb = clock(lambda: loss.backward())
        _, to = clock(opt.step)
        if i >= 3:
            for k, v in zip(rows, (td, tf, tb, to)):
                rows[k].append(v * 1e3)
    # the same step under torch autograd of the plain modules (library convolutions), float32 channels-last on the device
    ref = copy.deepcopy(net)
    ref.train()
    xr = x.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
    topt = torch.optim.Adam(ref.parameters(), lr=3e-4, eps=1e-7)
    lib = {"forward": [], "loss": [], "backward": [], "optimiser": []}
    for i in range(a.reps + 3):
        topt.zero_grad(set_to_none=True)

        (prob, dist), tf = clock(lambda: ref(xr))
        l2, tl = clock(lambda: reference_losses(prob[:, 0], dist.permute(0, 2, 3, 1), pt, dtm, dist_loss=cfg.train_dist_loss,
                                                 loss_weights=cfg.train_loss_weights, background_reg=cfg.train_background_reg)[2])
        _, tb = clock(lambda: l2.backward())
        _, to = clock(topt.step)
        if i >= 3:
            for k, v in zip(lib, (tf, tl, tb, to)):
                lib[k].append(v * 1e3)
    med = lambda v: float(np.median(v))
    res = {
        "what": "one training step of the 2D_demo topology (grid (2, 2), 32 rays, depth 3, 32 filters), batch %d of %d^2 patches; "
                "median of %d steps after 3 warm-up steps, wall clock around each synchronised phase, ms.  native forward = network + heads + "
                "fused loss kernel; library forward = the network alone, its loss expression timed as 'loss'; both backward phases "
                "include the loss's gradient" % (B, S, a.reps),
        "device": torch.cuda.get_device_name(0),
        "native": {k: med(v) for k, v in rows.items()},
        "torch_autograd_library_convolutions": {k: med(v) for k, v in lib.items()},
    }
    res["native"]["step"] = sum(res["native"].values())
    res["backward_ratio_native_over_library"] = res["native"]["backward"] / res["torch_autograd_library_convolutions"]["backward"]
    lib_ms = res["torch_autograd_library_convolutions"]
    res["forward_ratio_native_over_library"] = res["native"]["forward"] / (lib_ms["forward"] + lib_ms["loss"])
    res["forward_ratio_note"] = "native forward (with its fused loss) / (library forward + library loss)"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
