"""Time measure_labels on the device (csrc/measure.hip with the box and centroid-sum kernels) and on the host (the numpy loop of
stardist_amd.utils) on the same arrays, with a uint16 and a float32 image each:

  2048^2       the 12 756 random discs of tools/time_matching.py;
  128x256x256  a volume of 3 000 random balls;
  16384^2      its ~8.3e5 lattice discs.

Device, on tensors that are already there, by device events, median and range of --steps timed calls after --warmup:
  device_call   the three entry points of one call (sd_label_boxes_device, sd_label_centroid_sums_device,
                sd_label_intensity_stats_device) back to back
  stats_call    sd_label_intensity_stats_device alone: the new kernels
and by the host clock around a synchronise:
  device_python_call          measure_labels(tensor, tensor, as_tensors=True): adds the read of the largest id, the row selection
                              and the derived columns
  device_python_call_numpy    measure_labels(tensor, tensor): adds the read-back of the table
Host: measure_labels(array, array), host clock, --host-steps calls (one, with the uint16 image only, for the 16384^2 image; the float32
table is there compared in its integer columns and, for the sums, with np.bincount).  The tables of both routes are compared: every
column identical for uint16; for float32 every column but sum / mean / std identical and the largest relative difference of the sums
reported.  Bytes a call must move: one read of the labels for boxes and centroid sums (the call makes two passes, one per entry point:
`label_passes`), one read of the label and of the value per box pixel, and the tables; given as a share of the 6.29 TB/s of a float4
copy on the MI355X (profiles/normalize_times.json).

Writes profiles/measure_times.json (or --out).  Needs a HIP device: there is no fallback."""
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
CODE = {"uint16": 1, "float32": 2}


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), n=len(ms))


def scenes():
    from time_matching import lattice_discs, random_discs
    yield "2048x2048", lambda: random_discs((2048, 2048), 12756, 11)
    yield "128x256x256", lambda: random_discs((128, 256, 256), 3000, 14, rmin=4, rmax=9)
    yield "16384x16384", lambda: lattice_discs(16384, 18, 13)


def image(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == "uint16":
        return rng.integers(0, 65536, shape, dtype=np.uint16)
    return (1e3 * rng.standard_normal(shape, dtype=np.float32) + 500).astype(np.float32)


def events(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return stats(ms)


def wall(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ms, got = [], None
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms), got


def time_scene(torch, N, a, dtype, steps, warmup, host_steps, host_table=None):
    from stardist_amd.utils import measure_labels
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    img = image(a.shape, dtype, 21)
    t, x = torch.as_tensor(a, device="cuda:0"), torch.as_tensor(img, device="cuda:0")
    top = int(a.max())
    zyx = ((1,) + a.shape) if a.ndim == 2 else a.shape
    boxes = torch.empty((top + 1, 6), dtype=torch.int32, device=t.device)
    sums = torch.empty((top + 1, 4), dtype=torch.int64, device=t.device)
    acc = torch.empty((top + 1, 1, 2), dtype=torch.float64 if dtype == "float32" else torch.int64, device=t.device)
    mm = torch.empty((top + 1, 1, 2), dtype=torch.float32 if dtype == "float32" else torch.int32, device=t.device)
    isum, fsum = (None, vp(acc)) if dtype == "float32" else (vp(acc), None)

    def call_stats():
        N.dcall(t, "sd_label_intensity_stats_device", vp(t), *zyx, top, vp(boxes), vp(x), CODE[dtype], 1, isum, fsum, vp(mm))

    def call():
        N.dcall(t, "sd_label_boxes_device", vp(t), *zyx, top, vp(boxes))
        N.dcall(t, "sd_label_centroid_sums_device", vp(t), *zyx, top, vp(sums))
        call_stats()

    call()
    b = boxes.cpu().numpy().astype(np.int64)
    b = b[b[:, 5] > b[:, 2]]
    box_pixels = int(np.prod(b[:, 3:] - b[:, :3], axis=1).sum())
    res = dict(shape=list(a.shape), dtype=dtype, objects=int(len(b)), box_pixels=box_pixels, label_passes=2)
    res["device_call"] = events(torch, call, steps, warmup)
    res["stats_call"] = events(torch, call_stats, steps, warmup)
    tables = (top + 1) * (6 * 4 + 4 * 8 + 2 * 8 + 2 * 4)
    res["bytes"] = int(4 * a.size + box_pixels * (4 + img.itemsize) + tables)
    res["stats_bytes"] = int(box_pixels * (4 + img.itemsize) + (top + 1) * (6 * 4 + 2 * 8 + 2 * 4))
    for key, nbytes in (("device_call", res["bytes"]), ("stats_call", res["stats_bytes"])):
        tbps = nbytes / (res[key]["median_ms"] * 1e-3) / 1e12
        res[key]["tb_per_s"] = tbps
        res[key]["share_of_copy_bandwidth"] = tbps / COPY_TBPS
    res["device_python_call"], got_t = wall(torch, lambda: measure_labels(t, x, as_tensors=True), steps, 2)
    res["device_python_call_numpy"], got = wall(torch, lambda: measure_labels(t, x), steps, 2)
    res["tensor_and_numpy_tables_identical"] = bool(all(np.array_equal(v.cpu().numpy(), got[k], equal_nan=True) for k, v in got_t.items()))
    again = measure_labels(t, x)
    res["repeatable_bits"] = bool(all(got[k].tobytes() == again[k].tobytes() for k in got))
    want = host_table
    if host_steps > 0:
        hs = []
        for _ in range(host_steps):
            t0 = time.perf_counter()
            want = measure_labels(a, img)
            hs.append(time.perf_counter() - t0)
        res["host_s"] = dict(median_s=float(np.median(hs)), min_s=float(np.min(hs)), max_s=float(np.max(hs)), n=len(hs))
        res["host_over_device"] = res["host_s"]["median_s"] * 1e3 / res["device_python_call_numpy"]["median_ms"]
    if want is not None:
        approx = ("sum_intensity", "mean_intensity", "std_intensity") if dtype == "float32" else ()
        shared = [k for k in got if not k.endswith("_intensity")] if host_steps <= 0 else [k for k in got if k not in approx]
        res["identical_columns"] = bool(all(np.array_equal(got[k], want[k]) for k in shared))
        res["columns_compared_exactly"] = shared
        if dtype == "float32":
            ref = want["sum_intensity"] if host_steps > 0 else \
                np.bincount(a.ravel(), weights=img.ravel().astype(np.float64), minlength=top + 1)[got["label"]]
            scale = np.bincount(a.ravel(), weights=np.abs(img.ravel()).astype(np.float64), minlength=top + 1)[got["label"]]
            res["sum_max_difference_over_sum_abs"] = float((np.abs(got["sum_intensity"] - ref) / scale).max())
    del t, x
    torch.cuda.empty_cache()
    return res, (want if host_steps > 0 else None)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated scene names to leave out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measure_times.json"))
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
        a = make()
        big = name == "16384x16384"
        table = None
        for dtype in ("uint16", "float32"):
            host_steps = (1 if dtype == "uint16" else 0) if big else args.host_steps
            res["scenes"]["%s/%s" % (name, dtype)], table = time_scene(torch, N, a, dtype, args.steps, args.warmup, host_steps, table)
            print(name, dtype, json.dumps(res["scenes"]["%s/%s" % (name, dtype)]), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1, sort_keys=True)
                fh.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
