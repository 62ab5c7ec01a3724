"""Time label_contacts and measure_labels(neighbors=) on the device (csrc/label_contacts.hip) against their host routes on the same label
images, with identical results asserted:

  2048^2       12 756 random discs (12 435 objects after overlaps), the image of the other label tools;
  128x256x256  a volume of 3 000 random balls;
  16384^2      ~8.3e5 lattice discs.

Every image goes through expand_labels(lbl, --grow) on the device first, so that objects touch, and is then an int32 tensor that is
already on the device.  Per image and connectivity (1 and full):
  device_call         sd_label_contacts_device alone (with the background's pairs) by device events around the call, which synchronises
                      the stream twice itself; median and range of --steps timed calls after --warmup; with the number of runs the
                      append pass wrote, the number of contacts (emissions) and of table rows
  label_contacts_tensors / label_contacts_numpy   the public function on the tensor, as_tensors=True / numpy columns, host clock around
                      a synchronise
  measure_labels / measure_labels_neighbors       the table without and with neighbors=, numpy columns, host clock
  host_s              the host routes on the same array, host clock, --host-steps calls (one for the 16384^2 image); measure_labels'
                      host route walks the objects one by one and is left out on the 16384^2 image unless --host-measure-16k: there the
                      neighbour columns are compared with the ones derived from the host route's contact table
Bytes the entry point must move, given as a share of the 6.29 TB/s of a float4 copy on the MI355X (profiles/normalize_times.json): one
read of the labels (4 B / pixel) and the table (16 B / row).  It moves more: two passes over the labels, and 16 B written plus the
sort's traffic per run.

Writes profiles/label_contacts_times.json (or --out).  Needs a HIP device: there is no fallback."""
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
NEIGHBOR_NAMES = ("neighbors", "contact_objects", "contact_background")


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), n=len(ms))


def scenes():
    from time_matching import lattice_discs, random_discs

    return {"2048x2048": lambda: random_discs((2048, 2048), 12756, 11), "128x256x256": lambda: random_discs((128, 256, 256), 3000, 14, rmin=4, rmax=9),
            "16384x16384": lambda: lattice_discs(16384, 18, 13)}


def device_events(torch, call, steps, warmup):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return stats(ms)


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


def same_table(got, want):
    return list(got) == list(want) and all(np.array_equal(got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k], want[k]) for k in want)


def time_scene(torch, N, name, lbl, grow, steps, warmup, host_steps, host_measure):
    from stardist_amd import label_ops
    from stardist_amd import utils as U
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    t = U.expand_labels(torch.as_tensor(np.ascontiguousarray(lbl.astype(np.int32)), device="cuda:0"), grow)
    lbl = U.to_host(t)
    zyx = ((1,) + tuple(t.shape)) if t.dim() == 2 else tuple(t.shape)
    nd, n = t.dim(), t.numel()
    res = dict(shape=list(lbl.shape), dtype="int32", grown_by=grow, objects=int(len(np.unique(lbl)) - 1), background_share=float((lbl == 0).mean()))
    print(name, json.dumps(res), flush=True)
    for c in (1, nd):
        rec = {}
        count, runs, mm = ctypes.c_longlong(0), ctypes.c_longlong(0), (ctypes.c_int32 * 2)()
        N.dcall(t, "sd_label_contacts_device", vp(t), nd, *zyx, c, 1, 0, None, None, ctypes.byref(count), mm, ctypes.byref(runs))
        cap = count.value
        keys = torch.empty(max(cap, 1), dtype=torch.int64, device=t.device)
        counts = torch.empty(max(cap, 1), dtype=torch.int64, device=t.device)
        entry = lambda: N.dcall(t, "sd_label_contacts_device", vp(t), nd, *zyx, c, 1, cap, vp(keys), vp(counts), ctypes.byref(count), mm,
                                ctypes.byref(runs))
        rec["device_call"] = device_events(torch, entry, steps, warmup)
        nbytes = 4 * n + 16 * cap
        rec["device_call"].update(rows=int(cap), runs=int(runs.value), contacts=int(counts[:cap].sum()), bytes=int(nbytes),
                                  tb_per_s=nbytes / (rec["device_call"]["median_ms"] * 1e-3) / 1e12)
        rec["device_call"]["share_of_copy_bandwidth"] = rec["device_call"]["tb_per_s"] / COPY_TBPS
        print(name, c, "device_call", json.dumps(rec["device_call"]), flush=True)
        rec["host_s"], want = host_seconds(lambda: U.label_contacts(lbl, c, background=True, symmetric=True), host_steps)
        rec["label_contacts_tensors"], got = host_clock(torch, lambda: U.label_contacts(t, c, background=True, symmetric=True, as_tensors=True), steps)
        rec["identical_to_host"] = same_table(got, want)
        rec["label_contacts_numpy"], got = host_clock(torch, lambda: U.label_contacts(t, c, background=True, symmetric=True), steps)
        rec["identical_to_host"] = bool(rec["identical_to_host"] and same_table(got, want))
        rec["host_over_device"] = rec["host_s"]["median_s"] * 1e3 / rec["label_contacts_numpy"]["median_ms"]
        assert rec["identical_to_host"], (name, c)
        print(name, c, "label_contacts", json.dumps({k: rec[k] for k in rec if k != "device_call"}), flush=True)
        m = {}
        m["measure_labels"], plain = host_clock(torch, lambda: U.measure_labels(t), steps)
        m["measure_labels_neighbors"], got = host_clock(torch, lambda: U.measure_labels(t, neighbors=c), steps)
        assert list(got) == list(plain) + list(NEIGHBOR_NAMES) and all(np.array_equal(got[k], plain[k]) for k in plain)
        if host_measure:
            m["host_s"], ref = host_seconds(lambda: U.measure_labels(lbl, neighbors=c), host_steps)
            m["host_over_device"] = m["host_s"]["median_s"] * 1e3 / m["measure_labels_neighbors"]["median_ms"]
            m["identical_to_host"] = same_table(got, ref)
        else:
            m["host_s"] = "not run (see the tool's docstring); the neighbour columns are compared with the host contact table's"
            plain_table = U.label_contacts(lbl, c, background=True)
            ref = label_ops._neighbor_columns(got["label"], plain_table["label_a"], plain_table["label_b"], plain_table["contacts"])
            m["identical_to_host"] = all(np.array_equal(got[k], r) for k, r in zip(NEIGHBOR_NAMES, ref))
        assert m["identical_to_host"], (name, c)
        rec["measure"] = m
        print(name, c, "measure", json.dumps(m), flush=True)
        res["connectivity_%d" % c] = rec
        del keys, counts
    del t
    torch.cuda.empty_cache()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--grow", type=float, default=4.0, help="the distance of the expand_labels call before the measurement")
    ap.add_argument("--skip", default="", help="comma-separated scene names to leave out")
    ap.add_argument("--host-measure-16k", action="store_true", help="run measure_labels' host route on the 16384^2 image too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_contacts_times.json"))
    args = ap.parse_args(argv)
    if args.steps < 20 or args.warmup < 5:
        ap.error("at least 20 timed calls after 5 warm-ups")
    import torch
    from stardist_amd.lib import _native as N
    N.require_device()
    res = dict(device=torch.cuda.get_device_name(0), copy_bandwidth_tb_per_s=COPY_TBPS, steps=args.steps, warmup=args.warmup, scenes={})
    for name, make in scenes().items():
        if name in args.skip.split(","):
            continue
        big = name == "16384x16384"
        res["scenes"][name] = time_scene(torch, N, name, make(), args.grow, args.steps, args.warmup, 1 if big else args.host_steps,
                                         not big or args.host_measure_16k)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
