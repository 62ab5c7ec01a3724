"""Time one training step on the library's kernels (stardist_amd/training.py, training3d.py), split into data (patch sampling +
targets), forward, backward and optimiser, next to the same step under plain torch autograd of StarDistNet on the device (the
framework's library convolutions) for scale.  The native forward includes the fused loss kernel; on the library side the network's
forward and the loss expression (training.reference_losses, torch element-wise ops with a boolean-mask gather that synchronises) are
timed as separate phases.
  --dim 2   the 2D_demo topology (U-Net, grid (2, 2), 32 rays, depth 3, 32 filters), batch 4 of 256^2 patches; 20 steps after 3 warm-up
            steps -> profiles/training_times.json
  --dim 3   batch 2 of 48 x 96 x 96 patches; 10 steps after 2 warm-up steps -> profiles/training3d_times.json, one entry per --backbone:
            resnet  the 3D_demo topology: 4 blocks of 3 convolutions, 32 filters, grid (1, 2, 2), anisotropy (2, 1, 1), 96 rays
            unet    the default Config3D U-Net (depth 2, 32 filters, 96 rays, grid (1, 1, 1))
            both    (default) the two of them
  --classes K   instead: what the class head of a model with K classes adds to a step.  The same topology (--dim 2: 2D_demo, --dim 3:
            the 3D_demo ResNet) as a single-class and as a K-class model, on the same seeded patches, one step of each in turn
            (data, forward, backward, optimiser; wall clock around the synchronised step), medians -> one entry of
            profiles/training_classes_times.json.  The single-class step launches what it launched before the class head existed
            (tests/test_cpu_training_calls.py pins its calls), so it is the baseline.
Usage: python tools/time_training.py --dim {2,3} [--backbone {resnet,unet,both}] [--classes K] [--reps N] [--out FILE]"""
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


def balls(shape, n, seed):
    rng = np.random.RandomState(seed)
    y = np.zeros(shape, np.int32)
    zz, yy, xx = np.ogrid[:shape[0], :shape[1], :shape[2]]
    for i in range(1, n + 1):
        r = rng.randint(5, 10)
        c = [rng.randint(0, s) for s in shape]
        y[(2 * (zz - c[0]) / r) ** 2 + ((yy - c[1]) / r) ** 2 + ((xx - c[2]) / r) ** 2 < 1] = i
    return (y > 0).astype(np.float32) + 0.1 * rng.randn(*shape).astype(np.float32), y


def time_config(model, data, loss_fn, reps, warm):
    """medians (ms) of the phases of `reps` steps after `warm` warm-up steps: (native, library)"""
    from stardist_amd.training import Adam, reference_losses
    cfg, dev, net = model.config, model.device, model.net
    params = list(net.parameters())
    for p in params:
        p.requires_grad_(True)
    opt = Adam(params, 3e-4)
    sync = torch.cuda.synchronize

    def clock(fn):
        sync(); t0 = time.perf_counter(); r = fn(); sync(); return r, time.perf_counter() - t0

    rows = {"data": [], "forward": [], "backward": [], "optimiser": []}
    for i in range(reps + warm):
        (x, pt, dtm), td = clock(lambda: data.batch_device(i, dev))
        for p in params:
            p.grad = None
        (loss, _), tf = clock(lambda: loss_fn(net, cfg, x, pt, dtm))
        _, tb = clock(lambda: loss.backward())
        _, to = clock(opt.step)
        if i >= warm:
            for k, v in zip(rows, (td, tf, tb, to)):
                rows[k].append(v * 1e3)
    for p in params:
        p.grad = None
    # the same step under torch autograd of the plain modules (library convolutions), float32 channels-last on the device
    ref = copy.deepcopy(net)
    ref.train()
    nd = x.ndim - 2
    to_first, to_last = (0, nd + 1) + tuple(range(1, nd + 1)), (0,) + tuple(range(2, nd + 2)) + (1,)
    xr = x.permute(*to_first).contiguous(memory_format=torch.channels_last if nd == 2 else torch.channels_last_3d)
    topt = torch.optim.Adam(ref.parameters(), lr=3e-4, eps=1e-7)
    lib = {"forward": [], "loss": [], "backward": [], "optimiser": []}
    for i in range(reps + warm):
        topt.zero_grad(set_to_none=True)
        out, tf = clock(lambda: ref(xr))
        prob, dist = out[:2]
        l2, tl = clock(lambda: reference_losses(prob[:, 0], dist.permute(*to_last), pt, dtm, dist_loss=cfg.train_dist_loss,
                                                 loss_weights=cfg.train_loss_weights, background_reg=cfg.train_background_reg)[2])
        _, tb = clock(lambda: l2.backward())
        _, to = clock(topt.step)
        if i >= warm:
            for k, v in zip(lib, (tf, tl, tb, to)):
                lib[k].append(v * 1e3)
    med = lambda v: float(np.median(v))
    native, library = {k: med(v) for k, v in rows.items()}, {k: med(v) for k, v in lib.items()}
    native["step"] = sum(native.values())
    del ref, opt, topt
    torch.cuda.empty_cache()
    return native, library


def time_classes(make_model, make_data, loss_fn, K, reps, warm):
    """medians (ms) of one whole step of the single-class and of the K-class model, taken in turn"""
    from stardist_amd.training import Adam
    sync = torch.cuda.synchronize
    runs = []
    for n_classes in (None, K):
        model = make_model(n_classes)
        params = list(model.net.parameters())
        for p in params:
            p.requires_grad_(True)
        np.random.seed(0)
        runs.append((model, params, Adam(params, 3e-4), make_data(n_classes), []))
    for i in range(reps + warm):
        for model, params, opt, data, times in runs:
            sync(); t0 = time.perf_counter()
            x, pt, dtm, *pc = data.batch_device(i, model.device)
            for p in params:
                p.grad = None
            loss, _ = loss_fn(model.net, model.config, x, pt, dtm, **(dict(prob_class_true=pc[0]) if pc else {}))
            loss.backward()
            opt.step()
            sync()
            if i >= warm:
                times.append((time.perf_counter() - t0) * 1e3)
    for r in runs:
        if r[3].class_tables is not None:
            r[3].class_tables.check()
    single, multi = (float(np.median(r[4])) for r in runs)
    spread = [float(np.percentile(r[4], 75) - np.percentile(r[4], 25)) for r in runs]
    return {"single_class_step_ms": single, "multi_class_step_ms": multi, "extra_ms": multi - single, "ratio": multi / single,
            "interquartile_range_ms": {"single_class": spread[0], "multi_class": spread[1]}, "n_classes": K, "steps": reps, "warm_up": warm}


def main_classes(a):
    dev = torch.device("cuda:0")
    out = a.out or os.path.join(ROOT, "profiles", "training_classes_times.json")
    K = a.classes
    if a.dim == 2:
        from stardist_amd.models import Config2D, StarDist2D
        from stardist_amd.training import TrainData2D, train_loss
        name, B, S = "2D_demo", 4, 256
        X, Y = zip(*[discs(512, 120, s) for s in range(8)])
        make_model = lambda n: StarDist2D(Config2D(n_rays=32, grid=(2, 2), n_classes=n, train_patch_size=(S, S), train_batch_size=B),
                                          basedir=None, device=dev, seed=0)
        make_data = lambda n: TrainData2D(list(X), list(Y), batch_size=B, n_rays=32, length=10 ** 6, patch_size=(S, S), grid=(2, 2),
                                          foreground_prob=0.9, n_classes=n,
                                          classes=None if n is None else [{k: 1 + k % n for k in range(1, 121)} for _ in X])
        res = time_classes(make_model, make_data, train_loss, K, a.reps or 20, 3)
        res["what"] = "2D_demo topology (U-Net, grid (2, 2), 32 rays, depth 3, 32 filters), batch %d of %d^2 patches" % (B, S)
    else:
        from stardist_amd.models import Config3D, StarDist3D
        from stardist_amd.rays3d import rays_from_json
        from stardist_amd.training3d import TrainData3D, train_loss3d
        name = "3D_demo_resnet"
        X, Y = zip(*[balls((64, 160, 160), 150, s) for s in range(4)])
        kw = dict(backbone="resnet", n_rays=96, grid=(1, 2, 2), anisotropy=(2, 1, 1), resnet_n_blocks=4, resnet_n_filter_base=32,
                  resnet_n_conv_per_block=3, net_conv_after_resnet=128, train_patch_size=(48, 96, 96), train_batch_size=2)
        make_model = lambda n: StarDist3D(Config3D(n_classes=n, **kw), basedir=None, device=dev, seed=0)
        rays = rays_from_json(Config3D(**kw).rays_json)
        make_data = lambda n: TrainData3D(list(X), list(Y), batch_size=2, rays=rays, length=10 ** 6, patch_size=(48, 96, 96), grid=(1, 2, 2),
                                          anisotropy=(2, 1, 1), foreground_prob=0.9, n_classes=n,
                                          classes=None if n is None else [{k: 1 + k % n for k in range(1, 151)} for _ in X])
        res = time_classes(make_model, make_data, train_loss3d, K, a.reps or 10, 2)
        res["what"] = "3D_demo topology (ResNet, 4 blocks of 3 convolutions, 32 filters, grid (1, 2, 2), 96 rays), batch 2 of 48 x 96 x 96 patches"
    res["what"] += ("; one whole training step (data, forward, backward, optimiser) of the single-class and of the multi-class model in "
                    "turn, wall clock around each synchronised step, median ms")
    res["device"] = torch.cuda.get_device_name(0)
    allres = {}
    if os.path.exists(out):
        with open(out) as fh:
            allres = json.load(fh)
    allres[name] = res
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(allres, fh, indent=1)
    print(json.dumps({name: res}, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, choices=(2, 3), required=True)
    ap.add_argument("--backbone", choices=("resnet", "unet", "both"), default="both", help="--dim 3 only")
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--classes", type=int, default=None, help="time the step of a model with this many classes next to the single-class one")
    a = ap.parse_args()
    if a.classes is not None:
        return main_classes(a)
    dev = torch.device("cuda:0")
    what = ("; median of %d steps after %d warm-up steps, wall clock around each synchronised phase, ms.  native forward = network + heads + "
            "fused loss kernel; library forward = the network alone, its loss expression timed as 'loss'; both backward phases include "
            "the loss's gradient")
    if a.dim == 2:
        from stardist_amd.models import Config2D, StarDist2D
        from stardist_amd.training import TrainData2D, train_loss
        reps, warm, out = a.reps or 20, 3, a.out or os.path.join(ROOT, "profiles", "training_times.json")
        B, S = 4, 256
        cfg = Config2D(n_rays=32, grid=(2, 2), train_patch_size=(S, S), train_batch_size=B)
        X, Y = zip(*[discs(512, 120, s) for s in range(8)])
        np.random.seed(0)
        data = TrainData2D(list(X), list(Y), batch_size=B, n_rays=32, length=10 ** 6, patch_size=(S, S), grid=(2, 2), foreground_prob=0.9)
        native, library = time_config(StarDist2D(cfg, basedir=None, device=dev, seed=0), data, train_loss, reps, warm)
        res = {
            "what": "one training step of the 2D_demo topology (grid (2, 2), 32 rays, depth 3, 32 filters), batch %d of %d^2 patches" % (B, S)
                    + what % (reps, warm),
            "device": torch.cuda.get_device_name(0),
            "native": native,
            "torch_autograd_library_convolutions": library,
            "backward_ratio_native_over_library": native["backward"] / library["backward"],
            "forward_ratio_native_over_library": native["forward"] / (library["forward"] + library["loss"]),
            "forward_ratio_note": "native forward (with its fused loss) / (library forward + library loss)",
        }
    else:
        from stardist_amd.models import Config3D, StarDist3D
        from stardist_amd.rays3d import rays_from_json
        from stardist_amd.training3d import TrainData3D, train_loss3d
        reps, warm, out = a.reps or 10, 2, a.out or os.path.join(ROOT, "profiles", "training3d_times.json")
        X, Y = zip(*[balls((64, 160, 160), 150, s) for s in range(4)])
        configs = {
            "3D_demo_resnet": Config3D(backbone="resnet", n_rays=96, grid=(1, 2, 2), anisotropy=(2, 1, 1), resnet_n_blocks=4,
                                       resnet_n_filter_base=32, resnet_n_conv_per_block=3, net_conv_after_resnet=128,
                                       train_patch_size=(48, 96, 96), train_batch_size=2),
            "default_unet": Config3D(n_rays=96, train_patch_size=(48, 96, 96), train_batch_size=2),
        }
        res = {"what": "one training step, batch 2 of 48 x 96 x 96 patches" + what % (reps, warm), "device": torch.cuda.get_device_name(0)}
        for name, cfg in configs.items():
            if a.backbone not in ("both", cfg.backbone):
                continue
            np.random.seed(0)
            data = TrainData3D(list(X), list(Y), batch_size=2, rays=rays_from_json(cfg.rays_json), length=10 ** 6,
                               patch_size=cfg.train_patch_size, grid=cfg.grid, anisotropy=cfg.anisotropy, foreground_prob=0.9)
            native, library = time_config(StarDist3D(cfg, basedir=None, device=dev, seed=0), data, train_loss3d, reps, warm)
            library["step"] = sum(library.values())
            res[name] = {"native": native, "torch_autograd_library_conv3d": library,
                         "backward_ratio_native_over_library": native["backward"] / library["backward"]}
            print(name, json.dumps(res[name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
