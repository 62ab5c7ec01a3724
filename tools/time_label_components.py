"""Time label_components on the device (csrc/label_cc.hip) against scipy.ndimage.label on the host, on the same masks, with identical
results asserted:

  2048^2       the nuclei mask of oracle/synth.py (s2d_nuclei_labels > 0);
  128x256x256  a volume of 3 000 random balls;
  16384^2      ~8.3e5 lattice discs.

Every mask is labelled at connectivity 1 as a bool (uint8) tensor that is already on the device:
  device_call         sd_label_components_device by device events, median and range of --steps timed calls after --warmup
  device_python_call  label_components(tensor), host clock around a synchronise
  phases              per-launch kernel times of the four phases (tile, border, flatten, number = scan + numbering): the tool starts itself
                      once more under `rocprofv3 --kernel-trace` (a child process that only repeats the native call) and takes every
                      launch's duration from the trace.  Without rocprofv3 the record says so and carries no phase figures.
  host_s              scipy.ndimage.label, host clock, --host-steps calls (one for the 16384^2 mask)
Bytes a call must move: one read of the mask and one write of the labels, given as a share of the 6.29 TB/s of a float4 copy on the
MI355X (profiles/normalize_times.json); a phase's `bytes` is what its launches read and write at the least.

Writes profiles/label_components_times.json (or --out).  Needs a HIP device: there is no fallback."""
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
PHASES = (("tile", "k_tile"), ("border", "k_border"), ("flatten", "k_flatten"), ("number", ""))     # number: every other kernel of the call


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), n=len(ms))


def scenes():
    from time_matching import lattice_discs, random_discs

    def nuclei():
        from oracle.synth import s2d_nuclei_labels
        return s2d_nuclei_labels(2048, 2048)[0] > 0
    return {"2048x2048": nuclei, "128x256x256": lambda: random_discs((128, 256, 256), 3000, 14, rmin=4, rmax=9) > 0,
            "16384x16384": lambda: lattice_discs(16384, 18, 13) > 0}


def native_call(torch, N, t):
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    out = torch.empty(t.shape, dtype=torch.int32, device=t.device)
    n = torch.zeros(1, dtype=torch.int32, device=t.device)
    zyx = ((1,) + tuple(t.shape)) if t.dim() == 2 else tuple(t.shape)
    return (lambda: N.dcall(t, "sd_label_components_device", vp(t), 0, *zyx, 1, 0, vp(out), vp(n))), out, n


def kernels_child(name, rounds):
    """what the traced child runs: 2 warm-up calls and `rounds` calls of the native entry point, nothing else on the device"""
    import torch
    from stardist_amd.lib import _native as N
    t = torch.as_tensor(scenes()[name](), device="cuda:0").view(torch.uint8)
    call, _, _ = native_call(torch, N, t)
    for _ in range(2 + rounds):
        call()
        torch.cuda.synchronize()
    return 0


def trace_phases(name, rounds, pixels):
    prof = shutil.which("rocprofv3") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "rocprofv3")
    if not os.path.exists(prof):
        return dict(error="rocprofv3 not found")
    d = tempfile.mkdtemp(prefix="label_components_trace_")
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
    starts = [i for i, r in enumerate(recs) if "k_tile" in r[2]]
    if len(starts) != 2 + rounds:
        return dict(error="expected %d calls in the trace, found %d" % (2 + rounds, len(starts)))
    times = {p: [] for p, _ in PHASES}
    for a, b in list(zip(starts, starts[1:] + [len(recs)]))[2:]:
        call = recs[a:b]                                                    # the child launches nothing else
        for p, key in PHASES:
            own = [r for r in call if (key and key in r[2]) or (not key and not any(k and k in r[2] for _, k in PHASES))]
            times[p].append(sum(e - s for s, e, _ in own) * 1e-6)
    # least traffic per phase for a uint8 mask: tile reads the mask and writes the parents; flatten reads and writes them; the scan
    # reads them and writes the ranks; numbering reads parents, gathers ranks and writes the labels; border touches the tile faces only
    nbytes = dict(tile=5 * pixels, border=None, flatten=8 * pixels, number=8 * pixels + 12 * pixels)
    out = dict(source="rocprofv3 --kernel-trace of %d calls of the native entry point (2 warm-up calls before them dropped)" % rounds)
    for p, _ in PHASES:
        out[p] = stats(times[p])
        if nbytes[p]:
            out[p]["bytes"] = int(nbytes[p])
            out[p]["share_of_copy_bandwidth"] = nbytes[p] / (out[p]["median_ms"] * 1e-3) / 1e12 / COPY_TBPS
    return out


def time_scene(torch, N, name, mask, steps, warmup, host_steps):
    from scipy import ndimage
    from stardist_amd.utils import label_components
    t = torch.as_tensor(mask, device="cuda:0")
    call, out, n = native_call(torch, N, t.view(torch.uint8))
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    res = dict(shape=list(mask.shape), dtype="bool", connectivity=1, foreground=float(mask.mean()), device_call=stats(ms))
    res["bytes"] = int(5 * mask.size)
    res["device_call"]["tb_per_s"] = res["bytes"] / (res["device_call"]["median_ms"] * 1e-3) / 1e12
    res["device_call"]["share_of_copy_bandwidth"] = res["device_call"]["tb_per_s"] / COPY_TBPS
    wall = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = label_components(t, 1)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    res["device_python_call"] = stats(wall)
    res["components"] = int(n)
    res["repeatable_bits"] = bool(torch.equal(got, out))
    hs, want = [], None
    for _ in range(host_steps):
        t0 = time.perf_counter()
        want, m = ndimage.label(mask)
        hs.append(time.perf_counter() - t0)
    res["host_s"] = dict(median_s=float(np.median(hs)), min_s=float(np.min(hs)), max_s=float(np.max(hs)), n=len(hs))
    res["host_over_device"] = res["host_s"]["median_s"] * 1e3 / res["device_python_call"]["median_ms"]
    res["identical_to_scipy"] = bool(m == int(n) and np.array_equal(got.cpu().numpy(), want))
    assert res["identical_to_scipy"], name
    del t, out, got
    torch.cuda.empty_cache()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated scene names to leave out")
    ap.add_argument("--skip-kernels", action="store_true", help="no rocprofv3 child: no phase times")
    ap.add_argument("--kernels-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_components_times.json"))
    args = ap.parse_args(argv)
    if args.kernels_child:
        return kernels_child(args.kernels_child, args.steps)
    if args.steps < 20 or args.warmup < 5:
        ap.error("at least 20 timed calls after 5 warm-ups")
    # the traced children run first, one at a time, before this process opens the device
    made = {name: make() for name, make in scenes().items() if name not in args.skip.split(",")}
    phases = {name: (dict(error="skipped") if args.skip_kernels else trace_phases(name, 10, mask.size)) for name, mask in made.items()}
    import torch
    from stardist_amd.lib import _native as N
    N.require_device()
    res = dict(device=torch.cuda.get_device_name(0), copy_bandwidth_tb_per_s=COPY_TBPS, steps=args.steps, warmup=args.warmup, scenes={})
    for name, mask in made.items():
        res["scenes"][name] = time_scene(torch, N, name, mask, args.steps, args.warmup, 1 if name == "16384x16384" else args.host_steps)
        res["scenes"][name]["phases"] = phases[name]
        print(name, json.dumps(res["scenes"][name]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
