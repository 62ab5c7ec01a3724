"""Time expand_labels on the device (csrc/edt_feature.hip) against scikit-image's composition on scipy on the host
(distance_transform_edt(lbl == 0, return_indices=True) and the gather: the host route of stardist_amd.utils.expand_labels), on the same
label images, with identical results asserted:

  2048^2       12 435 random discs (the label image of tools/time_relabel.py and tools/time_measure.py), distance 5;
  128x256x256  a volume of 3 000 random balls, distance 3;
  16384^2      ~8.3e5 lattice discs, distance 5 (the host composition runs once).

Every label image is an int32 tensor that is already on the device:
  device_call         sd_expand_labels_device by device events, median and range of --steps timed calls after --warmup
  device_python_call  expand_labels(tensor), host clock around a synchronise (it includes the label policy's reduction and read-back)
  passes              per-launch kernel times of the passes (first, middle, last): the tool starts itself once more under
                      `rocprofv3 --kernel-trace` (a child process that only repeats the native call) and takes every launch's duration
                      from the trace.  Without rocprofv3 the record says so and carries no pass figures.
  host_s              the host route, host clock, --host-steps calls (one for the 16384^2 image)
Bytes a call must move: one read of the labels and one write of the result, given as a share of the 6.29 TB/s of a float4 copy on the
MI355X (profiles/normalize_times.json); a pass's `bytes` is what its launches read and write at the least (a carried pixel is a
float64 and an int32).

Writes profiles/expand_labels_times.json (or --out).  Needs a HIP device: there is no fallback."""
import argparse
import csv
import ctypes
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
COPY_TBPS = 6.29
PASSES = (("first", "k_first"), ("middle", "k_middle"), ("last", "k_last"))
DISTANCE = {"2048x2048": 5.0, "128x256x256": 3.0, "16384x16384": 5.0}


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), n=len(ms))


def scenes():
    from time_matching import lattice_discs, random_discs
    return {"2048x2048": lambda: random_discs((2048, 2048), 12756, 11), "128x256x256": lambda: random_discs((128, 256, 256), 3000, 14, rmin=4, rmax=9),
            "16384x16384": lambda: lattice_discs(16384, 18, 13)}


def native_call(torch, N, t, distance):
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    out = torch.empty_like(t)
    zyx = ((1,) + tuple(t.shape)) if t.dim() == 2 else tuple(t.shape)
    return (lambda: N.dcall(t, "sd_expand_labels_device", vp(t), *zyx, 1.0, 1.0, 1.0, distance, vp(out))), out


def kernels_child(name, rounds):
    """what the traced child runs: 2 warm-up calls and `rounds` calls of the native entry point, nothing else on the device"""
    import torch
    from stardist_amd.lib import _native as N
    t = torch.as_tensor(scenes()[name](), device="cuda:0")
    call, _ = native_call(torch, N, t, DISTANCE[name])
    for _ in range(2 + rounds):
        call()
        torch.cuda.synchronize()
    return 0


def trace_passes(name, rounds, pixels, volume):
    prof = shutil.which("rocprofv3") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "rocprofv3")
    if not os.path.exists(prof):
        return dict(error="rocprofv3 not found")
    d = tempfile.mkdtemp(prefix="expand_labels_trace_")
    try:
        cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__),
               "--kernels-child", name, "--steps", str(rounds)]
        run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=400)
        if run.returncode < 0 or run.returncode in (124, 134, 137, 139):
            raise SystemExit("the traced child died (%d): nothing more is started on the device\n%s"
                             % (run.returncode, run.stdout.decode(errors="replace")[-2000:]))
        if run.returncode != 0:
            return dict(error="rocprofv3 run failed (%d): %s" % (run.returncode, run.stdout.decode(errors="replace")[-400:]))
        recs = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(f) as fh:
                recs += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    recs.sort()
    times = {p: [(e - s) * 1e-6 for s, e, k in recs if key in k][2:] for p, key in PASSES}
    if len(times["first"]) != rounds or len(times["last"]) != rounds or len(times["middle"]) != (rounds if volume else 0):
        return dict(error="expected %d calls in the trace, found %r" % (2 + rounds, {p: len(v) for p, v in times.items()}))
    # least traffic per pass for int32 labels: first reads the labels and writes the carried pixels; middle reads and writes them;
    # last reads them, gathers a label and writes the result
    nbytes = dict(first=(4 + 12) * pixels, middle=(12 + 12) * pixels, last=(12 + 4 + 4) * pixels)
    out = dict(source="rocprofv3 --kernel-trace of %d calls of the native entry point (2 warm-up calls before them dropped)" % rounds)
    for p, _ in PASSES:
        if not times[p]:
            continue
        out[p] = stats(times[p])
        out[p]["bytes"] = int(nbytes[p])
        out[p]["share_of_copy_bandwidth"] = nbytes[p] / (out[p]["median_ms"] * 1e-3) / 1e12 / COPY_TBPS
    return out


def time_scene(torch, N, name, lbl, steps, warmup, host_steps):
    from stardist_amd.utils import expand_labels
    distance = DISTANCE[name]
    t = torch.as_tensor(lbl, device="cuda:0")
    call, out = native_call(torch, N, t, distance)
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    res = dict(shape=list(lbl.shape), dtype="int32", distance=distance, spacing=1.0, objects=int(len(np.unique(lbl)) - 1),
               labelled=float((lbl != 0).mean()), device_call=stats(ms))
    res["bytes"] = int(8 * lbl.size)
    res["device_call"]["tb_per_s"] = res["bytes"] / (res["device_call"]["median_ms"] * 1e-3) / 1e12
    res["device_call"]["share_of_copy_bandwidth"] = res["device_call"]["tb_per_s"] / COPY_TBPS
    wall = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = expand_labels(t, distance)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    res["device_python_call"] = stats(wall)
    res["repeatable_bits"] = bool(torch.equal(got, out))
    hs, want = [], None
    for _ in range(host_steps):
        t0 = time.perf_counter()
        want = expand_labels(lbl, distance)
        hs.append(time.perf_counter() - t0)
    res["host_s"] = dict(median_s=float(np.median(hs)), min_s=float(np.min(hs)), max_s=float(np.max(hs)), n=len(hs))
    res["host_over_device"] = res["host_s"]["median_s"] * 1e3 / res["device_python_call"]["median_ms"]
    res["labelled_after"] = float((want != 0).mean())
    res["identical_to_host"] = bool(np.array_equal(got.cpu().numpy(), want))
    assert res["identical_to_host"], name
    del t, out, got
    torch.cuda.empty_cache()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated scene names to leave out")
    ap.add_argument("--skip-kernels", action="store_true", help="no rocprofv3 child: no pass times")
    ap.add_argument("--kernels-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expand_labels_times.json"))
    args = ap.parse_args(argv)
    if args.kernels_child:
        return kernels_child(args.kernels_child, args.steps)
    if args.steps < 20 or args.warmup < 5:
        ap.error("at least 20 timed calls after 5 warm-ups")
    # the traced children run first, one at a time, before this process opens the device
    made = {name: make() for name, make in scenes().items() if name not in args.skip.split(",")}
    passes = {name: (dict(error="skipped") if args.skip_kernels else trace_passes(name, 10, lbl.size, lbl.ndim == 3)) for name, lbl in made.items()}
    import torch
    from stardist_amd.lib import _native as N
    N.require_device()
    res = dict(device=torch.cuda.get_device_name(0), copy_bandwidth_tb_per_s=COPY_TBPS, steps=args.steps, warmup=args.warmup, scenes={})
    for name, lbl in made.items():
        res["scenes"][name] = time_scene(torch, N, name, lbl, args.steps, args.warmup, 1 if name == "16384x16384" else args.host_steps)
        res["scenes"][name]["passes"] = passes[name]
        print(name, json.dumps(res["scenes"][name]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
