"""Time point_neighbors on the device (csrc/point_neighbors.hip) against its host route on the same points, with identical results asserted.
The points are the centroids (measure_labels on the device) of the three scenes of the other label tools:

  2048^2       12 756 random discs (12 435 objects after overlaps);
  128x256x256  a volume of 3 000 random balls;
  16384^2      ~8.3e5 lattice discs.

Per scene, for k = 1, k = 8, a radius that gives about 20 neighbours (from the mean density), and that radius with count_only:
  device_call   sd_point_neighbors_device alone (through its one Python driver, on a float64 tensor that is on the device) by device events
                around the call, which synchronises the stream itself (once for the box, once more for the lists' total); median and range
                of --steps timed calls after --warmup
  tensors / numpy   the public function on that tensor, as_tensors=True / numpy columns, host clock around a synchronise
  host_workers_1 / host_workers_16   the host route (scipy's cKDTree for candidates, d2 recomputed) on the same array, the tree's queries
                with workers=1 (what the public function uses) and with workers=16; --host-steps calls (one at 16384^2)
The first and the last device call's results are compared bit for bit, and all routes with the host route's.

Writes profiles/point_neighbors_times.json (or --out).  Needs a HIP device: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), n=len(ms))


def scenes():
    from time_matching import lattice_discs, random_discs

    return {"2048x2048": lambda: random_discs((2048, 2048), 12756, 11), "128x256x256": lambda: random_discs((128, 256, 256), 3000, 14, rmin=4, rmax=9),
            "16384x16384": lambda: lattice_discs(16384, 18, 13)}


def device_events(torch, call, steps, warmup):
    first = call()
    for _ in range(warmup - 1):
        call()
    ms, out = [], first
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = call(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return stats(ms), first, out


def host_clock(torch, fn, steps, warmup=2):
    for _ in range(warmup):
        fn()
    ms, out = [], None
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms), out


def host_seconds(fn, steps):
    hs, out = [], None
    for _ in range(steps):
        t0 = time.perf_counter()
        out = fn()
        hs.append(time.perf_counter() - t0)
    return dict(median_s=float(np.median(hs)), min_s=float(np.min(hs)), max_s=float(np.max(hs)), n=len(hs)), out


def same(got, want):
    host = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else v
    return list(got) == list(want) and all(host(got[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes() for k in want)


def time_scene(torch, name, lbl, steps, warmup, host_steps):
    from stardist_amd import label_ops
    from stardist_amd import utils as U
    t = torch.as_tensor(np.ascontiguousarray(lbl.astype(np.int32)), device="cuda:0")
    table = U.measure_labels(t, as_tensors=True)
    nd = t.dim()
    P = torch.stack([table["centroid-%d" % d] for d in range(nd)], dim=1).contiguous()
    del t, table
    pts = U.to_host(P)
    n = len(pts)
    density = n / float(np.prod(lbl.shape))
    radius = float(np.sqrt(20 / (np.pi * density)) if nd == 2 else (20 / (4 / 3 * np.pi * density)) ** (1 / 3))
    res = dict(shape=list(lbl.shape), points=n, radius=radius)
    print(name, json.dumps(res), flush=True)
    for label, k, r, count_only in (("k1", 1, None, False), ("k8", 8, None, False), ("radius", None, radius, False), ("radius_count", None, radius, True)):
        rec = {}
        r2 = None if r is None else float(np.float64(r) * np.float64(r))
        mode = 1 if count_only else 0 if k is not None else 2
        cell = []
        rec["device_call"], first, last = device_events(torch, lambda: label_ops._point_neighbors_device(P, None, mode, k, r2, 0.0, cell), steps, warmup)
        first, last = (first, last) if isinstance(first, tuple) else ((first,), (last,))
        rec["same_bits_from_call_to_call"] = all(torch.equal(a, b) for a, b in zip(first, last))
        rec["cell_size"] = cell[0]
        kw = dict(count_only=count_only)
        for workers in (1, 16):
            label_ops._POINT_NEIGHBORS_WORKERS = workers
            rec["host_workers_%d" % workers], want = host_seconds(lambda: U.point_neighbors(pts, k, r, **kw), host_steps)
        label_ops._POINT_NEIGHBORS_WORKERS = 1
        rec["tensors"], got = host_clock(torch, lambda: U.point_neighbors(P, k, r, as_tensors=True, **kw), steps)
        rec["identical_to_host"] = same(got, want)
        rec["numpy"], got = host_clock(torch, lambda: U.point_neighbors(P, k, r, **kw), steps)
        rec["identical_to_host"] = bool(rec["identical_to_host"] and same(got, want))
        if r is not None:
            rec["mean_neighbours"] = float(want["counts"].mean() if count_only else np.diff(want["offsets"]).mean())
        rec["host_1_over_device_numpy"] = rec["host_workers_1"]["median_s"] * 1e3 / rec["numpy"]["median_ms"]
        rec["host_16_over_device_numpy"] = rec["host_workers_16"]["median_s"] * 1e3 / rec["numpy"]["median_ms"]
        assert rec["identical_to_host"] and rec["same_bits_from_call_to_call"], (name, label)
        print(name, label, json.dumps(rec), flush=True)
        res[label] = rec
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--scenes", default="2048x2048,128x256x256,16384x16384")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_neighbors_times.json"))
    args = ap.parse_args()
    import torch
    from stardist_amd.lib import _native as N
    N.require_device()
    out = dict(tool="tools/time_point_neighbors.py", device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup,
               note="device_call: device events around sd_point_neighbors_device; tensors / numpy: the public call, host clock; host_workers_*: "
                    "the host route with that many threads in cKDTree's queries; untuned, no per-kernel trace was made")
    make = scenes()
    for name in args.scenes.split(","):
        out[name] = time_scene(torch, name, make[name](), args.steps, args.warmup, 1 if name == "16384x16384" else args.host_steps)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
