"""Time the device normalisation (csrc/normalize.hip) and what it buys a prediction from a raw image.

  (a) sd_percentiles_device + sd_normalize_mi_ma_device on uint16 and float32 images of 2048^2, 256^3 and 16384^2 elements: device
      events, median of --reps timed calls after --warmup, with the bytes each entry point moves (counted from the shapes: one read of
      the image per histogram pass -- 1 for uint16, 3 for float32 -- plus one read and one float32 write for the rescale) and the
      achieved bandwidth against the 6.29 TB/s of a float4 copy on the MI355X;
  (b) raw host image -> labels: predict_instances(raw, normalizer=PercentileNormalizer(1, 99.8)) (upload raw, normalise on the device);
  (c) the same on the host, as before the device path: normalize(raw, 1, 99.8) with numpy, then predict_instances.
      (b) and (c) alternate in one run on a 2048^2 image (host clock around calls that end with the labels on the host).

Writes profiles/normalize_times.json (or --out).  Needs a HIP device: there is no fallback."""
import argparse
import ctypes
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


def time_kernels(torch, N, shape, dtype, reps, warmup):
    dev = torch.device("cuda:0")
    n = int(np.prod(shape))
    g = torch.Generator(device=dev).manual_seed(n % 9973)
    if dtype == "uint16":                       # a camera-like histogram: a few thousand grey levels and a saturated tail
        x = (torch.randn(n, device=dev, generator=g) * 400 + 2500).clamp_(0, 65535)
        x[torch.rand(n, device=dev, generator=g) < 0.002] = 65535
        x = x.to(torch.int32).to(torch.uint16)
        code, passes, isz = 1, 1, 2
    else:
        x = torch.rand(n, device=dev, generator=g, dtype=torch.float32)
        code, passes, isz = 2, 3, 4
    p = torch.empty(2, dtype=torch.float32, device=dev)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    q = (ctypes.c_double * 2)(1.0, 99.8)
    vp = ctypes.c_void_p

    def perc():
        N.dcall(x, "sd_percentiles_device", vp(x.data_ptr()), code, n, 1, ctypes.cast(q, vp), 2, 1, vp(p.data_ptr()))

    def resc():
        N.dcall(x, "sd_normalize_mi_ma_device", vp(x.data_ptr()), code, n, 1, vp(p.data_ptr()), vp(p.data_ptr() + 4), 1e-20, 0, vp(out.data_ptr()))

    res = {}
    for name, fn, nbytes in (("percentiles", perc, passes * n * isz), ("rescale", resc, n * isz + n * 4),
                             ("both", lambda: (perc(), resc()), (passes + 1) * n * isz + n * 4)):
        for _ in range(warmup):
            fn()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        r = stats(ms)
        r["bytes"] = int(nbytes)
        r["tb_per_s"] = nbytes / (r["median_ms"] * 1e-3) / 1e12
        r["share_of_copy_bandwidth"] = r["tb_per_s"] / COPY_TBPS
        res[name] = r
    res["image_reads"] = passes + 1
    res["image_writes_float32"] = 1
    del x, out
    torch.cuda.empty_cache()
    return res


def time_predict(torch, dtype, reps, warmup):
    import bench
    from oracle import synth
    from stardist_amd.models import Config2D, StarDist2D
    from stardist_amd.utils import PercentileNormalizer, normalize
    dev = torch.device("cuda:0")
    img = synth.s2d_nuclei_image(2048, 2048, seed=0)
    raw = np.clip(img.astype(np.float64) * 3000 + 120, 0, 65535)
    raw = raw.astype(np.uint16) if dtype == "uint16" else raw.astype(np.float32)
    model = StarDist2D(Config2D(n_rays=32), basedir=None, device=dev, seed=0)
    bench.calibrate_heads(model, torch.from_numpy(normalize(raw, 1, 99.8)).to(dev))
    nz = PercentileNormalizer(1, 99.8)

    def device_way():
        return model.predict_instances(raw, normalizer=nz)

    def host_way():
        return model.predict_instances(normalize(raw, 1, 99.8))

    a, b = device_way(), host_way()
    same = bool(np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][k], b[1][k]) for k in ("coord", "points", "prob")))
    for _ in range(warmup):
        device_way(); host_way()
    td, th = [], []
    for _ in range(reps):                       # alternating, so that both see the same machine
        for fn, acc in ((device_way, td), (host_way, th)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t0) * 1e3)
    tn = []
    for _ in range(max(5, reps // 4)):
        t0 = time.perf_counter()
        normalize(raw, 1, 99.8)
        tn.append((time.perf_counter() - t0) * 1e3)
    return dict(shape=[2048, 2048], instances=int(len(a[1]["prob"])), identical_results=same, device_normalizer=stats(td),
                host_normalize_then_predict=stats(th), host_normalize_alone=stats(tn))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normalize_times.json"))
    ap.add_argument("--skip-predict", action="store_true")
    args = ap.parse_args(argv)
    if args.reps < 20 or args.warmup < 5:
        ap.error("at least 20 timed calls after 5 warm-ups")
    import torch
    from stardist_amd.lib import _native as N
    N.require_device()
    res = dict(device=torch.cuda.get_device_name(0), copy_bandwidth_tb_per_s=COPY_TBPS, reps=args.reps, warmup=args.warmup, kernels={}, predict={})
    for shape in ((2048, 2048), (256, 256, 256), (16384, 16384)):
        for dtype in ("uint16", "float32"):
            key = "%s_%s" % ("x".join(map(str, shape)), dtype)
            res["kernels"][key] = time_kernels(torch, N, shape, dtype, args.reps, args.warmup)
            print(key, json.dumps(res["kernels"][key]["both"]), flush=True)
    if not args.skip_predict:
        for dtype in ("uint16", "float32"):
            res["predict"]["2048x2048_" + dtype] = time_predict(torch, dtype, args.reps, args.warmup)
            print(dtype, json.dumps(res["predict"]["2048x2048_" + dtype]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
