"""Time the "data" phase of a training step (TrainData.batch_device: patch sampling, augmentation, uploads, targets) with and without
augmentation, on the host route and on the device route of stardist_amd.augment, in the configurations of tools/time_training.py:

  2d   batch 4 of 256^2 patches, grid (2, 2), 32 rays (the 2D_demo data of time_training.py --dim 2)
  3d   batch 2 of 48 x 96 x 96 patches, grid (1, 2, 2), anisotropy (2, 1, 1), 96 rays (time_training.py --dim 3, 3D_demo_resnet)

Variants:  none     no augmenter
           chain    Compose([FlipRot90, IntensityScaleShift, AdditiveNoise]), the reference notebooks' chain
           elastic  the same plus Warp(elastic_grid=5, elastic_amount=4)
           each of the last two on the host route (the object behind a plain callable: numpy / scipy per sample, then the uploads) and
           on the device route (the object itself: draws on the host, one launch, targets from the device labels).
Every (variant, route) has its own generator over the same images.  An entry's batches run back to back, as a training run asks for
them: --warmup batches, then --steps / 2 timed ones (host clock around batch_device and a device synchronise), entry after entry, and
the whole sequence twice, so that every entry is timed early and late in the run; median, minimum and maximum over its --steps
batches.  (One batch of each entry in turn would time every device-route batch right after 0.1 - 0.3 s of host-only work of a
host-route batch, on a device that has gone idle.)  `augment_call` is Compose.apply_device alone on a resident batch, by device events.

--package ROOT imports stardist_amd from another tree (a checkout of the parent commit, built): without stardist_amd.augment there,
only `none` is timed -- the figure this commit's `none` (alone: --only-none) is compared with.

Writes profiles/augment_times.json (or --out).  Needs a HIP device: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = 2
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), n=len(ms))


def augmenters(only_none=False):
    """name -> the Compose (None for `none`); `none` alone where the package has no augment module, or when asked"""
    try:
        from stardist_amd import augment as A
    except ImportError:
        only_none = True
    if only_none:
        return {"none": None}
    chain = lambda: [A.FlipRot90(), A.IntensityScaleShift(), A.AdditiveNoise()]
    return {"none": None, "chain": A.Compose(chain()), "elastic": A.Compose(chain() + [A.Warp(elastic_grid=5, elastic_amount=4.0)])}


def generators(dim, only_none=False):
    """(label -> a TrainData over the same images, the batch shape, the augmenters)"""
    from time_training import balls, discs
    augs = augmenters(only_none)
    if dim == 2:
        from stardist_amd.training import TrainData2D
        X, Y = zip(*[discs(512, 120, s) for s in range(8)])
        make = lambda a: TrainData2D(list(X), list(Y), batch_size=4, n_rays=32, length=10 ** 6, patch_size=(256, 256), grid=(2, 2),
                                     foreground_prob=0.9, augmenter=a)
        shape = (4, 256, 256)
    else:
        from stardist_amd.rays3d import Rays_GoldenSpiral
        from stardist_amd.training3d import TrainData3D
        X, Y = zip(*[balls((64, 160, 160), 150, s) for s in range(4)])
        rays = Rays_GoldenSpiral(96, anisotropy=(2, 1, 1))
        make = lambda a: TrainData3D(list(X), list(Y), batch_size=2, rays=rays, length=10 ** 6, patch_size=(48, 96, 96), grid=(1, 2, 2),
                                     anisotropy=(2, 1, 1), foreground_prob=0.9, augmenter=a)
        shape = (2, 48, 96, 96)
    out = {"none": make(None)}
    for name, aug in augs.items():
        if aug is not None:
            out[name + "/host"] = make(lambda x, y, aug=aug: aug(x, y))
            out[name + "/device"] = make(aug)
    return out, shape, augs


def time_dim(torch, dim, steps, warmup, only_none=False):
    dev = torch.device("cuda:0")
    gens, shape, augs = generators(dim, only_none)
    np.random.seed(0)
    rows, at = {k: [] for k in gens}, {k: 0 for k in gens}
    for part in range(PASSES):
        for k, g in gens.items():
            for j in range(warmup + steps // PASSES):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                g.batch_device(at[k], dev)
                torch.cuda.synchronize()
                at[k] += 1
                if j >= warmup:
                    rows[k].append((time.perf_counter() - t0) * 1e3)
    res = {"batch": list(shape), "data_phase": {k: stats(v) for k, v in rows.items()}}
    # the augmentation call alone, on a resident batch
    calls = {}
    for name, aug in augs.items():
        if aug is None:
            continue
        x = torch.rand(shape, device=dev)
        y = (torch.rand(shape, device=dev) * 50).to(torch.int32)
        ms, wall = [], []
        for i in range(warmup + steps):
            params = [aug.draw(shape[1:]) for _ in range(shape[0])]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); aug.apply_device(x, y, params); e1.record()
            e1.synchronize()
            if i >= warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(e0.elapsed_time(e1))
        calls[name] = dict(device_events=stats(ms), host_clock=stats(wall))
    if calls:
        res["augment_call"] = calls
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dims", default="2,3")
    ap.add_argument("--only-none", action="store_true", help="time the variant without an augmenter alone")
    ap.add_argument("--package", default=ROOT, help="the tree stardist_amd is imported from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_times.json"))
    args = ap.parse_args(argv)
    if args.steps < 20 or args.warmup < 5 or args.steps % PASSES:
        ap.error("at least 20 timed batches (an even number) after 5 warm-up batches")
    sys.path.insert(0, os.path.abspath(args.package))
    import torch
    from stardist_amd.lib import _native as N
    N.require_device()
    res = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup,
               what="ms per batch; data_phase: host clock around TrainData.batch_device and a synchronise, an entry's batches back to back, "
                    "every entry in two blocks of steps / 2 after `warmup` batches each; "
                    "augment_call: Compose.apply_device alone")
    for dim in (int(d) for d in args.dims.split(",")):
        res["%dd" % dim] = time_dim(torch, dim, args.steps, args.warmup, args.only_none)
        print("%dd" % dim, json.dumps(res["%dd" % dim]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
