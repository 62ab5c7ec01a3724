"""Time the device zoom (csrc/zoom.hip) and what it buys predict_instances(img, scale=...).

  (a) sd_zoom_linear_device alone on float32 images of 2048^2 and 16384^2 elements, factors 0.5 and 2.0 (16384^2 by 0.5 only: its
      double is 4 GiB of output): device events, median of --reps timed calls after --warmup, with the bytes moved counted from the
      shapes (the input once plus the output once) and the achieved bandwidth against the 6.29 TB/s of a float4 copy on the MI355X;
  (b) raw host image -> labels: predict_instances(raw, scale=s), the image uploaded raw and resampled on the device;
  (c) the same call on the host path -- scipy.ndimage.zoom on the host array, then the upload: the line the device path replaces, and
      all there was before it.  (b) and (c) alternate in one run (host clock around calls that end with the labels on the host):
      2048^2 float32 and uint16 (with PercentileNormalizer(1, 99.8)) by 0.5 and 2.0, and 256^3 float32 by 0.5;
  (d) scipy.ndimage.zoom(order=1) alone on the same host arrays.

Writes profiles/scale_times.json (or --out).  Needs a HIP device: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_TBPS = 6.29


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), n=len(ms))


def time_kernel(torch, shape, factor, reps, warmup):
    from stardist_amd.utils import zoom_linear
    dev = torch.device("cuda:0")
    x = torch.rand(shape, device=dev, dtype=torch.float32, generator=torch.Generator(device=dev).manual_seed(shape[0]))
    out = None
    for _ in range(warmup):
        out = zoom_linear(x, factor)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = zoom_linear(x, factor); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    r = stats(ms)
    r["out_shape"] = list(out.shape)
    r["bytes"] = int(x.numel() * 4 + out.numel() * 4)
    r["tb_per_s"] = r["bytes"] / (r["median_ms"] * 1e-3) / 1e12
    r["share_of_copy_bandwidth"] = r["tb_per_s"] / COPY_TBPS
    del x, out
    torch.cuda.empty_cache()
    return r


def time_predict(torch, model, raw, scale, normalizer, reps, warmup):
    from scipy.ndimage import zoom
    kw = dict(scale=scale) if normalizer is None else dict(scale=scale, normalizer=normalizer)

    def device_way():
        return model.predict_instances(raw, **kw)

    def host_way():
        model._zoom_on_device = lambda img: False
        try:
            return model.predict_instances(raw, **kw)
        finally:
            del model._zoom_on_device

    a, b = device_way(), host_way()
    same = bool(np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][k], b[1][k]) for k in ("points", "prob")))
    for _ in range(warmup):
        device_way(); host_way()
    td, th = [], []
    for _ in range(reps):                       # alternating, so that both see the same machine
        for fn, acc in ((device_way, td), (host_way, th)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t0) * 1e3)
    tz = []
    for _ in range(max(3, reps // 3)):
        t0 = time.perf_counter()
        zoom(raw, scale, order=1)
        tz.append((time.perf_counter() - t0) * 1e3)
    return dict(shape=list(raw.shape), dtype=str(raw.dtype), scale=scale, instances=int(len(a[1]["prob"])), identical_results=same,
                device_zoom=stats(td), host_zoom_then_upload=stats(th), scipy_zoom_alone=stats(tz))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_times.json"))
    ap.add_argument("--skip-predict", action="store_true")
    args = ap.parse_args(argv)
    if args.reps < 10 or args.warmup < 1:
        ap.error("at least 10 timed calls after a warm-up")
    import torch
    import bench
    from oracle import synth
    from stardist_amd.lib import _native as N
    from stardist_amd.models import Config2D, Config3D, StarDist2D, StarDist3D
    from stardist_amd.utils import PercentileNormalizer
    N.require_device()
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), copy_bandwidth_tb_per_s=COPY_TBPS, reps=args.reps, warmup=args.warmup, kernel={}, predict={})
    for shape, factor in (((2048, 2048), 0.5), ((2048, 2048), 2.0), ((16384, 16384), 0.5)):
        key = "%s_float32_by_%g" % ("x".join(map(str, shape)), factor)
        res["kernel"][key] = time_kernel(torch, shape, factor, 2 * args.reps, args.warmup + 3)
        print(key, json.dumps(res["kernel"][key]), flush=True)

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")

    write()
    if not args.skip_predict:
        img = synth.s2d_nuclei_image(2048, 2048, seed=0)
        model = StarDist2D(Config2D(n_rays=32), basedir=None, device=dev, seed=0)
        bench.calibrate_heads(model, torch.from_numpy(synth.s2d_nuclei_image(256, 256, seed=1)).to(dev))
        raw16 = np.clip(img.astype(np.float64) * 3000 + 120, 0, 65535).astype(np.uint16)
        for raw, nz, name in ((img, None, "float32"), (raw16, PercentileNormalizer(1, 99.8), "uint16")):
            for scale in (0.5, 2.0):
                key = "2048x2048_%s_by_%g" % (name, scale)
                res["predict"][key] = time_predict(torch, model, raw, scale, nz, args.reps, args.warmup)
                print(key, json.dumps(res["predict"][key]), flush=True)
                write()
        del model
        vol = np.ascontiguousarray(np.tile(synth.s3d_nuclei_image(64, seed=1), (4, 4, 4)))
        model = StarDist3D(Config3D(rays=32), basedir=None, device=dev, seed=0)
        model.thresholds = dict(prob=0.5, nms=0.3)
        bench.calibrate_heads(model, torch.from_numpy(synth.s3d_nuclei_image(64, seed=0)).to(dev), frac=0.009, radius=8.5, noise=0.03)
        res["predict"]["256x256x256_float32_by_0.5"] = time_predict(torch, model, vol, 0.5, None, args.reps, args.warmup)
        print("256x256x256_float32_by_0.5", json.dumps(res["predict"]["256x256x256_float32_by_0.5"]), flush=True)
        write()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
