"""Time measure_labels(shape=True) on the device (csrc/measure_shape.hip beside the box, centroid-sum kernels) and on the host (the
numpy code of stardist_amd.label_ops) on the label images of tools/time_measure.py:

  2048^2       the 12 756 random discs of tools/time_matching.py;
  128x256x256  a volume of 3 000 random balls;
  16384^2      its ~8.3e5 lattice discs.

Device, on tensors that are already there, by device events, median and range of --steps timed calls after --warmup:
  moments_call   sd_label_moment_sums_device alone (one read of the labels and a gather from the box table)
  contour_call   sd_label_contour_counts_device alone (2D; one read of the labels, the tile halos from L2)
and by the host clock around a synchronise:
  device_python_call          measure_labels(tensor, shape=True, as_tensors=True)
  device_python_call_numpy    measure_labels(tensor, shape=True): adds the read-back of the table
  plain_python_call_numpy     measure_labels(tensor): the same call without shape
Host: measure_labels(array, shape=True), host clock, --host-steps calls (one for the 16384^2 image).  The tables of both routes are
compared: every column identical.  Bytes an entry point must move: one read of the labels and its table; given as a share of the
6.29 TB/s of a float4 copy on the MI355X (profiles/normalize_times.json).

--parent TREE adds the "unchanged" check against a built checkout of the parent commit in TREE: child processes, alternating between
TREE and this tree in one run, time measure_labels without shape (2048^2 labels and a uint16 image, to numpy) and run
`bench.py --gpus 1 --steps 20 --warmup 5` for its headline (ms per step, as the neighbouring profiles record it); recorded are every
run's figure and whether this tree's median lies inside the spread of the parent's own runs (--first this: a second run whose alternations start with this tree, against drift within a run).

Writes profiles/measure_shape_times.json (or --out).  Needs a HIP device: there is no fallback."""
import argparse
import ctypes
import json
import os
import subprocess
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
    zyx = ((1,) + a.shape) if a.ndim == 2 else a.shape
    boxes = torch.empty((top + 1, 6), dtype=torch.int32, device=t.device)
    m2 = torch.empty((top + 1, 6), dtype=torch.int64, device=t.device)
    counts = torch.empty((top + 1, 18), dtype=torch.int64, device=t.device)
    N.dcall(t, "sd_label_boxes_device", vp(t), *zyx, top, vp(boxes))
    res = dict(shape=list(a.shape), objects=int(len(np.unique(a)) - 1))
    calls = [("moments_call", lambda: N.dcall(t, "sd_label_moment_sums_device", vp(t), *zyx, top, vp(boxes), vp(m2)), 6 * 4 + 6 * 8)]
    if a.ndim == 2:
        calls.append(("contour_call", lambda: N.dcall(t, "sd_label_contour_counts_device", vp(t), *a.shape, top, vp(counts)), 18 * 8))
    for key, fn, row_bytes in calls:
        res[key] = events(torch, fn, steps, warmup)
        res[key]["bytes"] = int(4 * a.size + (top + 1) * row_bytes)
        tbps = res[key]["bytes"] / (res[key]["median_ms"] * 1e-3) / 1e12
        res[key]["tb_per_s"] = tbps
        res[key]["share_of_copy_bandwidth"] = tbps / COPY_TBPS
    res["device_python_call"], got_t = wall(torch, lambda: measure_labels(t, shape=True, as_tensors=True), steps, 2)
    res["device_python_call_numpy"], got = wall(torch, lambda: measure_labels(t, shape=True), steps, 2)
    res["plain_python_call_numpy"], _ = wall(torch, lambda: measure_labels(t), steps, 2)
    libm = ("orientation",) if a.ndim == 2 else ("equivalent_diameter",)      # the columns that call atan2 / pow
    res["tensor_and_numpy_tables_identical_but_libm"] = bool(all(np.array_equal(v.cpu().numpy(), got[k]) for k, v in got_t.items() if k not in libm))
    res["libm_columns_max_difference"] = float(max(np.abs(got_t[k].cpu().numpy() - got[k]).max() for k in libm))
    again = measure_labels(t, shape=True)
    res["repeatable_bits"] = bool(all(got[k].tobytes() == again[k].tobytes() for k in got))
    del t
    torch.cuda.empty_cache()
    if host_steps > 0:
        hs = []
        for _ in range(host_steps):
            t0 = time.perf_counter()
            want = measure_labels(a, shape=True)
            hs.append(time.perf_counter() - t0)
        res["host_s"] = dict(median_s=float(np.median(hs)), min_s=float(np.min(hs)), max_s=float(np.max(hs)), n=len(hs))
        res["host_over_device"] = res["host_s"]["median_s"] * 1e3 / res["device_python_call_numpy"]["median_ms"]
        res["identical_columns"] = bool(list(got) == list(want) and all(np.array_equal(got[k], want[k]) for k in want))
    return res


def worker_plain(steps, warmup):
    """one child of the "unchanged" check: measure_labels without shape of the tree it runs in; prints one JSON line"""
    import torch
    from stardist_amd.utils import measure_labels
    from time_matching import random_discs
    from time_measure import image, wall
    a = random_discs((2048, 2048), 12756, 11)
    t, x = torch.as_tensor(a, device="cuda:0"), torch.as_tensor(image(a.shape, "uint16", 21), device="cuda:0")
    st, got = wall(torch, lambda: measure_labels(t, x), steps, warmup)
    st["columns"] = list(got)
    st["checksum"] = float(sum(np.asarray(v, np.float64).sum() for v in got.values()))
    print(json.dumps(st), flush=True)


def child(tree, argv, limit):
    r = subprocess.run([sys.executable] + argv, cwd=tree, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise RuntimeError("%s in %s failed (%d):\n%s" % (argv, tree, r.returncode, (r.stdout + r.stderr)[-2000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def unchanged(parent, rounds, steps, warmup, bench_steps, bench_warmup, bench_rounds, first="parent"):
    """alternating child processes, parent tree first; {what: {parent: [...], this: [...], this_median_inside_parent_spread}}"""
    out = {}
    plans = (("measure_labels_plain_ms", ["tools/time_measure_shape.py", "--worker-plain", "--steps", str(steps), "--warmup", str(warmup)],
              lambda r: r["median_ms"], rounds, 300),
             ("bench_headline_ms_per_step", ["bench.py", "--gpus", "1", "--steps", str(bench_steps), "--warmup", str(bench_warmup)],
              lambda r: r["ms_per_step"], bench_rounds, 600))
    for what, argv, pick, n, limit in plans:
        runs = {"parent": [], "this": []}
        checks = {"parent": [], "this": []}
        for k in range(n):
            for side, tree in (("parent", parent), ("this", ROOT))[::1 if first == "parent" else -1]:
                if side == "parent" and what.startswith("measure") and not os.path.exists(os.path.join(tree, "tools", "time_measure_shape.py")):
                    r = child(tree, [os.path.join(ROOT, argv[0])] + argv[1:] + ["--tree", tree], limit)   # the parent has no such tool
                else:
                    r = child(tree, argv, limit)
                runs[side].append(float(pick(r)))
                checks[side].append(r.get("checksum"))
                print(what, k, side, runs[side][-1], flush=True)
        lo, hi, med = min(runs["parent"]), max(runs["parent"]), float(np.median(runs["this"]))
        out[what] = dict(parent=runs["parent"], this=runs["this"], parent_median=float(np.median(runs["parent"])), this_median=med,
                         this_median_inside_parent_spread=bool(lo <= med <= hi))
        if what.startswith("measure"):
            out[what]["same_table"] = bool(len(set(checks["parent"] + checks["this"])) == 1)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated scene names to leave out")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: adds the unchanged check")
    ap.add_argument("--first", choices=("parent", "this"), default="parent", help="which tree every alternation starts with; a run that starts "
                    "with this tree is recorded beside the other, as unchanged_this_first")
    ap.add_argument("--rounds", type=int, default=5, help="child processes per tree for measure_labels without shape")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--worker-plain", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measure_shape_times.json"))
    args = ap.parse_args(argv)
    if args.steps < 20 or args.warmup < 5 or args.bench_steps < 20 or args.bench_warmup < 5:
        ap.error("at least 20 timed calls after 5 warm-ups")
    if args.worker_plain:
        if args.tree:                                                      # run by path from another tree: import that tree's package
            sys.path[:2] = [args.tree, os.path.join(args.tree, "tools")]
        worker_plain(args.steps, args.warmup)
        return 0
    from time_measure import scenes
    todo = [(name, make) for name, make in scenes() if name not in args.skip.split(",")]
    res = dict(copy_bandwidth_tb_per_s=COPY_TBPS, steps=args.steps, warmup=args.warmup, scenes={})
    if todo:                                                               # (the unchanged check alone leaves the device to its children)
        import torch
        from stardist_amd.lib import _native as N
        N.require_device()
        res["device"] = torch.cuda.get_device_name(0)
    if os.path.exists(args.out):                                           # a run of some parts keeps the others
        with open(args.out) as fh:
            old = json.load(fh)
        res["scenes"] = old.get("scenes", {})
        res.update({k: v for k, v in old.items() if k.startswith("unchanged") or k == "device"})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
    for name, make in todo:
        res["scenes"][name] = time_scene(torch, N, make(), args.steps, args.warmup, 1 if name == "16384x16384" else args.host_steps)
        print(name, json.dumps(res["scenes"][name]), flush=True)
        save()
    if args.parent:
        res["unchanged" if args.first == "parent" else "unchanged_this_first"] = unchanged(
            os.path.abspath(args.parent), args.rounds, args.steps, args.warmup, args.bench_steps, args.bench_warmup, args.bench_rounds, args.first)
        save()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
