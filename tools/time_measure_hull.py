"""Time measure_labels(hull=True) on the device (csrc/measure_hull.hip beside the box and centroid-sum kernels) and on the host (the
Python-integer code of stardist_amd.label_ops) on the two 2D label images of tools/time_measure.py:

  2048^2       the 12 756 random discs of tools/time_matching.py;
  16384^2      its ~8.3e5 lattice discs.

Device, on tensors that are already there, median and range of --steps timed calls after --warmup:
  hull_call                   sd_label_hull_device alone, by device events (the call synchronises once itself: two scalars size
                              its row table, so the figure holds that round trip)
and by the host clock around a synchronise:
  device_python_call          measure_labels(tensor, hull=True, as_tensors=True)
  device_python_call_numpy    measure_labels(tensor, hull=True): adds the read-back of the table
  plain_python_call_numpy     measure_labels(tensor): the same call without hull
Host: measure_labels(array, hull=True), host clock, --host-steps calls (one for the 16384^2 image).  The tables of both routes are
compared: every column identical.  Bytes the entry point must move: one read of the labels, the box table, the row table written
(emptied, then the extremes) and read, and its own table; given as a share of the 6.29 TB/s of a float4 copy on the MI355X
(profiles/normalize_times.json).

Writes profiles/measure_hull_times.json (or --out).  Needs a HIP device: there is no fallback."""
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


def time_scene(torch, N, a, steps, warmup, host_steps):
    from stardist_amd.utils import measure_labels
    from time_measure import events, wall
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    t = torch.as_tensor(a, device="cuda:0")
    top = int(a.max())
    boxes = torch.empty((top + 1, 6), dtype=torch.int32, device=t.device)
    table = torch.empty((top + 1, 2), dtype=torch.int64, device=t.device)
    N.dcall(t, "sd_label_boxes_device", vp(t), 1, *a.shape, top, vp(boxes))
    b = boxes.cpu().numpy().astype(np.int64)
    rows = int(np.maximum(b[:, 4] - b[:, 1], 0).sum())
    res = dict(shape=list(a.shape), objects=int(len(np.unique(a)) - 1), object_rows=rows)
    res["hull_call"] = events(torch, lambda: N.dcall(t, "sd_label_hull_device", vp(t), *a.shape, top, vp(boxes), vp(table)), steps, warmup)
    res["hull_call"]["bytes"] = int(4 * a.size + (top + 1) * (6 * 4 + 2 * 8 + 4 * 8) + rows * 8 * 3)
    tbps = res["hull_call"]["bytes"] / (res["hull_call"]["median_ms"] * 1e-3) / 1e12
    res["hull_call"]["tb_per_s"] = tbps
    res["hull_call"]["share_of_copy_bandwidth"] = tbps / COPY_TBPS
    res["device_python_call"], got_t = wall(torch, lambda: measure_labels(t, hull=True, as_tensors=True), steps, warmup)
    res["device_python_call_numpy"], got = wall(torch, lambda: measure_labels(t, hull=True), steps, warmup)
    res["plain_python_call_numpy"], _ = wall(torch, lambda: measure_labels(t), steps, warmup)
    res["tensor_and_numpy_tables_identical"] = bool(all(np.array_equal(v.cpu().numpy(), got[k]) for k, v in got_t.items()))
    again = measure_labels(t, hull=True)
    res["repeatable_bits"] = bool(all(got[k].tobytes() == again[k].tobytes() for k in got))
    del t
    torch.cuda.empty_cache()
    if host_steps > 0:
        hs = []
        for _ in range(host_steps):
            t0 = time.perf_counter()
            want = measure_labels(a, hull=True)
            hs.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        measure_labels(a)
        res["host_plain_s"] = time.perf_counter() - t0
        res["host_s"] = dict(median_s=float(np.median(hs)), min_s=float(np.min(hs)), max_s=float(np.max(hs)), n=len(hs))
        res["host_over_device"] = res["host_s"]["median_s"] * 1e3 / res["device_python_call_numpy"]["median_ms"]
        res["identical_columns"] = bool(list(got) == list(want) and all(np.array_equal(got[k], want[k]) for k in want))
        assert res["identical_columns"], "the device table differs from the host table"
    assert res["tensor_and_numpy_tables_identical"] and res["repeatable_bits"]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated scene names to leave out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measure_hull_times.json"))
    args = ap.parse_args(argv)
    if args.steps < 20 or args.warmup < 5:
        ap.error("at least 20 timed calls after 5 warm-ups")
    import torch
    from stardist_amd.lib import _native as N
    from time_measure import scenes
    N.require_device()
    todo = [(name, make) for name, make in scenes() if name not in args.skip.split(",") and name.count("x") == 1]
    res = dict(copy_bandwidth_tb_per_s=COPY_TBPS, steps=args.steps, warmup=args.warmup, python_call_warmup=args.warmup, scenes={}, device=torch.cuda.get_device_name(0))
    if os.path.exists(args.out):                                           # a run of some parts keeps the others
        with open(args.out) as fh:
            res["scenes"] = json.load(fh).get("scenes", {})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
    for name, make in todo:
        res["scenes"][name] = time_scene(torch, N, make(), args.steps, args.warmup, 1 if name == "16384x16384" else args.host_steps)
        print(name, json.dumps(res["scenes"][name]), flush=True)
        save()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
