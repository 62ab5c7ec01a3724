"""Time fill_label_holes on the device (csrc/fill_holes.hip) and on the host (the scipy loop of stardist_amd.utils) on the same arrays:

  2048^2       the 12 756 random discs of tools/time_matching.py, every third one hollowed out (so that there are holes to fill);
  16384^2      its ~8.3e5 lattice discs, hollowed the same way;
  128x256x256  a volume of random balls, hollowed the same way.

Device: sd_fill_label_holes_device on an int32 tensor that is already there, device events, median and range of --steps timed calls
after --warmup (likewise sd_label_boxes_device alone, the first pass of the same code and all of calculate_extents); and the Python
call fill_label_holes(tensor) by the host clock (it adds the read of the largest id and the conversions).
Host: fill_label_holes(array), host clock, --host-steps calls (one for the 16384^2 image).  Bytes: one read of the image plus one of
every object's bounding box (the planes are built from it), 4 bytes a pixel, against the 6.29 TB/s of a float4 copy on the MI355X --
the write of the output and the workspace are not counted, so the share is a lower bound on the traffic and says how far from a
copy the call is.  The results of both paths are compared.

Writes profiles/fill_holes_times.json (or --out).  Needs a HIP device: there is no fallback."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
COPY_TBPS = 6.29


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), n=len(ms))


def hollow(a, every=3):
    """cut the core (two erosions deep) out of every `every`-th label"""
    from scipy.ndimage import binary_erosion
    core = binary_erosion((a > 0) & (a % every == 0), iterations=2)
    a[core] = 0
    return a


def scenes():
    from time_matching import lattice_discs, random_discs
    yield "2048x2048", lambda: hollow(random_discs((2048, 2048), 12756, 11))
    yield "128x256x256", lambda: hollow(random_discs((128, 256, 256), 3000, 14, rmin=4, rmax=9))
    yield "16384x16384", lambda: hollow(lattice_discs(16384, 18, 13))


def time_scene(torch, N, a, steps, warmup, host_steps):
    from stardist_amd.utils import fill_label_holes
    vp = ctypes.c_void_p
    t = torch.as_tensor(a, device="cuda:0")
    out = torch.empty_like(t)
    top = int(a.max())
    zyx = ((1,) + a.shape) if a.ndim == 2 else a.shape
    boxes = torch.empty((top + 1, 6), dtype=torch.int32, device=t.device)
    N.dcall(t, "sd_label_boxes_device", vp(t.data_ptr()), *zyx, top, vp(boxes.data_ptr()))
    b = boxes.cpu().numpy().astype(np.int64)
    b = b[b[:, 5] > b[:, 2]]
    box_pixels = int(np.prod(b[:, 3:] - b[:, :3], axis=1).sum())

    def call():
        N.dcall(t, "sd_fill_label_holes_device", vp(t.data_ptr()), *zyx, top, vp(out.data_ptr()))

    def call_boxes():
        N.dcall(t, "sd_label_boxes_device", vp(t.data_ptr()), *zyx, top, vp(boxes.data_ptr()))

    timed = {}
    for key, fn in (("device_call", call), ("boxes_call", call_boxes)):
        for _ in range(warmup):
            fn()
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        timed[key] = stats(ms)
    res = dict(shape=list(a.shape), objects=int(len(b)), **timed)
    nbytes = 4 * (a.size + box_pixels)
    res["bytes"] = int(nbytes)
    res["tb_per_s"] = nbytes / (res["device_call"]["median_ms"] * 1e-3) / 1e12
    res["share_of_copy_bandwidth"] = res["tb_per_s"] / COPY_TBPS
    wall = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fill_label_holes(t)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    res["device_python_call"] = stats(wall)
    filled = got.cpu().numpy()
    res["pixels_filled"] = int((filled != a).sum())
    if host_steps > 0:
        hs = []
        for _ in range(host_steps):
            t0 = time.perf_counter()
            want = fill_label_holes(a)
            hs.append(time.perf_counter() - t0)
        res["host_s"] = dict(median_s=float(np.median(hs)), min_s=float(np.min(hs)), max_s=float(np.max(hs)), n=len(hs))
        res["identical_results"] = bool(np.array_equal(filled, want) and np.array_equal(out.cpu().numpy(), want))
        res["host_over_device"] = res["host_s"]["median_s"] * 1e3 / res["device_python_call"]["median_ms"]
    del t, out, got
    torch.cuda.empty_cache()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated scene names to leave out")
    ap.add_argument("--skip-host", default="", help="comma-separated scene names whose host run is left out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_holes_times.json"))
    args = ap.parse_args(argv)
    if args.steps < 20 or args.warmup < 5:
        ap.error("at least 20 timed calls after 5 warm-ups")
    import torch
    from stardist_amd.lib import _native as N
    N.require_device()
    res = dict(device=torch.cuda.get_device_name(0), copy_bandwidth_tb_per_s=COPY_TBPS, steps=args.steps, warmup=args.warmup, scenes={})
    for name, make in scenes():
        if name in args.skip.split(","):
            continue
        host_steps = 0 if name in args.skip_host.split(",") else (1 if name == "16384x16384" else args.host_steps)
        res["scenes"][name] = time_scene(torch, N, make(), args.steps, args.warmup, host_steps)
        print(name, json.dumps(res["scenes"][name]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
