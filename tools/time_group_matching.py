"""Time group_matching_labels on the host (per frame: dense matching with report_matches + a repaint loop over find_objects) and on the
device (one stack overlap call csrc/overlap.hip, the id maps from the sparse lists on the host, one stack relabel call csrc/relabel.hip;
stardist_amd.matching_sparse) for a synthetic stack:
  8 frames of 2048^2 with 12 756 discs on a lattice (radius 3..6), each frame the one before shifted by 1-2 px with 5 objects dropped.
Prints one JSON line: median and spread (min, max) of the host call, of the device call and of its phases (wall clock, device idle at both
ends) -- overlap call, read-back of the lists, host assignment and tables, relabel call (table upload included).  The two bandwidth
kernels are timed on their own: the tool starts itself once more under `rocprofv3 --kernel-trace` (a child process that only repeats the
two native calls) and takes every launch's duration from the trace -- k_stack_runs<false> (count pass) and k_stack_runs<true> (append
pass) of the overlap call, k_relabel_stack of the relabel call, and the sum of the other kernels of each call (sort, reduce-by-key,
table fill, ...).  Each kernel's bytes (the frames it must read and write) over its median duration is rated against the 6.29 TB/s copy
rate that profiles/normalize_times.json measures.  Without rocprofv3 the record says so and carries no kernel figures.

    python tools/time_group_matching.py [--repeat 9] [--host-repeat 3] [--skip-host] [--skip-kernels] [--out profiles/group_matching_times.json]
"""
import argparse
import json
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE_GBS = 6290.0                                                  # profiles/normalize_times.json: device-to-device copy


def lattice_discs(size, cell, seed):
    """one disc per cell of a size x size image (radius 3..6, centre jittered by 1 px, >= 4 px between discs): the generator of
    tests/test_gpu_matching.py"""
    rng = np.random.RandomState(seed)
    k = size // cell - 1
    n = k * k
    rad = rng.randint(3, 7, n)
    cy = (np.arange(n) // k + 1) * cell + rng.randint(-1, 2, n)
    cx = (np.arange(n) % k + 1) * cell + rng.randint(-1, 2, n)
    y = np.zeros((size, size), np.int32)
    for r in range(3, 7):
        dy, dx = np.nonzero(np.add.outer(np.arange(-r, r + 1) ** 2, np.arange(-r, r + 1) ** 2) < r * r)
        ids = np.flatnonzero(rad == r)
        y[(cy[ids, None] + dy - r), (cx[ids, None] + dx - r)] = ids[:, None].astype(np.int32) + 1
    return y


def lattice_stack(frames=8, size=2048, cell=17, seed=13, drop=5, keep=12756):
    """the timing scene (tests/_group_cases.py takes it from here): the first `keep` discs of the lattice, then every frame the one before
    shifted by 1-2 px with `drop` objects removed"""
    rng = np.random.RandomState(seed)
    first = lattice_discs(size, cell, seed)
    ys = [np.where(first <= keep, first, 0)]                            # the first `keep` discs of the lattice
    for _ in range(frames - 1):
        y = np.roll(ys[-1], (int(rng.randint(1, 3)), int(rng.randint(1, 3))), axis=(0, 1))
        present = np.unique(y[y > 0])
        ys.append(np.where(np.isin(y, rng.choice(present, drop, replace=False)), 0, y).astype(np.int32))
    return np.stack(ys)


def stats(xs):
    return dict(median_s=float(np.median(xs)), min_s=float(np.min(xs)), max_s=float(np.max(xs)))


KERNELS = {"count_pass": ("k_stack_runs<false>", "k_stack_runsILb0E"), "append_pass": ("k_stack_runs<true>", "k_stack_runsILb1E"),
           "relabel": ("k_relabel_stack",)}
MARK = "k_stack_init"                                                   # first kernel of an overlap call


def kernels_child(args):
    """what the trace is taken of: the two native calls alone, repeated; tables and frames are staged before"""
    import torch
    from stardist_amd import matching_sparse as S
    dev = torch.device("cuda:0")
    ys = lattice_stack(args.frames, args.size)
    a = torch.from_numpy(ys).to(dev)
    flat = a.reshape(len(ys), -1)
    keys, counts, offs, mm = S._overlap_stack_call(flat)
    tables = S.group_tables_from_overlaps(S._split_lists(keys.cpu().numpy(), counts.cpu().numpy(), offs), mm[0, 1], 1e-10, "iou")
    for _ in range(2 + args.repeat):                                    # two warm-up rounds, dropped by the parent
        S._overlap_stack_call(flat)
        S.relabel_stack_device(a, tables, mm[:, 1])
    torch.cuda.synchronize(dev)


def trace_kernels(args, frame_bytes):
    """per-launch durations of the kernels of the two native calls from a rocprofv3 kernel trace of a child process"""
    prof = shutil.which("rocprofv3") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "rocprofv3")
    if not os.path.exists(prof):
        return dict(error="rocprofv3 not found")
    d = tempfile.mkdtemp(prefix="group_matching_trace_")
    try:
        cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__),
               "--kernels-child", "--repeat", str(args.repeat), "--frames", str(args.frames), "--size", str(args.size)]
        run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        if run.returncode != 0:
            return dict(error="rocprofv3 run failed (%d): %s" % (run.returncode, run.stdout.decode(errors="replace")[-400:]))
        recs = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(f) as fh:
                recs += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    recs.sort()
    marks = [i for i, r in enumerate(recs) if MARK in r[2]]
    if len(marks) < 3 + args.repeat:
        return dict(error="the trace holds %d overlap calls, %d expected" % (len(marks), 3 + args.repeat))
    rounds = [recs[lo:hi] for lo, hi in zip(marks, marks[1:] + [len(recs)])][-args.repeat:]
    K = args.frames
    # what a kernel must move: a pass of the overlap call reads every frame once; the relabel kernel reads and writes every frame once
    nbytes = dict(count_pass=K * frame_bytes, append_pass=K * frame_bytes, relabel=2 * K * frame_bytes)
    out = dict(source="rocprofv3 --kernel-trace of %d rounds of the two native calls (2 warm-up rounds before them dropped)" % args.repeat)
    times = {k: [] for k in list(KERNELS) + ["overlap_other_kernels", "relabel_other_kernels"]}
    for rnd in rounds:
        cut = next((i for i, r in enumerate(rnd) if "k_fill_tables" in r[2] or any(p in r[2] for p in KERNELS["relabel"])), len(rnd))
        for part, other in ((rnd[:cut], "overlap_other_kernels"), (rnd[cut:], "relabel_other_kernels")):
            rest = 0.0
            for s0, s1, name in part:
                hit = [k for k, pats in KERNELS.items() if any(p in name for p in pats)]
                if hit:
                    times[hit[0]].append((s1 - s0) / 1e9)
                else:
                    rest += (s1 - s0) / 1e9
            times[other].append(rest)
    for k, xs in times.items():
        if len(xs) != args.repeat:
            return dict(error="%d launches of %s in %d rounds" % (len(xs), k, args.repeat))
        out[k] = stats(xs)
        if k in nbytes:
            gbs = nbytes[k] / float(np.median(xs)) / 1e9
            out[k].update(bytes=nbytes[k], GBs=gbs, fraction_of_copy_rate=gbs / COPY_RATE_GBS)
    both = nbytes["count_pass"] + nbytes["append_pass"]
    gbs = both / float(np.median(np.add(times["count_pass"], times["append_pass"]))) / 1e9
    out["overlap_passes"] = dict(bytes=both, GBs=gbs, fraction_of_copy_rate=gbs / COPY_RATE_GBS)
    out["copy_rate_GBs"] = COPY_RATE_GBS
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--host-repeat", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--kernels-child", action="store_true", help="internal: the run that is traced")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernels_child:
        return kernels_child(args)
    # the traced child runs first, while this process has not opened the device
    kernels = None if args.skip_kernels else trace_kernels(args, args.size * args.size * 4)
    import torch
    from stardist_amd import matching as M
    from stardist_amd import matching_sparse as S
    dev = torch.device("cuda:0")
    ys = lattice_stack(args.frames, args.size)
    K = len(ys)
    a = torch.from_numpy(ys).to(dev)
    flat = a.reshape(K, -1)
    sync = lambda: torch.cuda.synchronize(dev)
    thresh, crit = 1e-10, "iou"
    res = M.group_matching_labels(a)                                    # warm-up (workspace, kernels)
    M.group_matching_labels(a)
    t_dev, t_ov, t_rb, t_host, t_rl = [], [], [], [], []
    for _ in range(args.repeat):
        sync()
        t0 = time.perf_counter()
        res = M.group_matching_labels(a)
        sync()
        t_dev.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        keys, counts, offs, mm = S._overlap_stack_call(flat)
        sync()
        t1 = time.perf_counter()
        lists = S._split_lists(keys.cpu().numpy(), counts.cpu().numpy(), offs)
        t2 = time.perf_counter()
        tables = S.group_tables_from_overlaps(lists, mm[0, 1], thresh, crit)
        t3 = time.perf_counter()
        out = S.relabel_stack_device(a, tables, mm[:, 1])
        sync()
        t4 = time.perf_counter()
        t_ov.append(t1 - t0); t_rb.append(t2 - t1); t_host.append(t3 - t2); t_rl.append(t4 - t3)
        assert torch.equal(out, res)
    pairs = int(len(keys))
    rec = dict(scene="%d x %dx%d lattice discs" % (K, args.size, args.size), objects_first_frame=int(len(np.unique(ys[0])) - 1), pairs=pairs,
               groups=int(len(np.unique(res.cpu().numpy())) - 1), thresh=thresh, criterion=crit, repeat=args.repeat,
               device=stats(t_dev), overlap_call=stats(t_ov), read_back=stats(t_rb), host_tables=stats(t_host), relabel_call=stats(t_rl),
               kernels=kernels)
    if not args.skip_host:
        t_h = []
        for _ in range(args.host_repeat):
            t0 = time.perf_counter()
            h = M.group_matching_labels(ys)
            t_h.append(time.perf_counter() - t0)
        rec.update(host=stats(t_h), host_repeat=args.host_repeat, host_equal=bool(np.array_equal(h, res.cpu().numpy())),
                   host_over_device=float(np.median(t_h) / np.median(t_dev)))
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="tools/time_group_matching.py", device=torch.cuda.get_device_name(0), cpus=len(os.sched_getaffinity(0)), results=[rec]),
                      fh, indent=1)


if __name__ == "__main__":
    main()
