"""Time find_boundaries, clear_border, remove_small_objects and select_labels on the device (csrc/label_edit.hip and the entry points
behind them) against their host routes on the same label images, with identical results asserted:

  2048^2       12 756 random discs (12 435 objects after overlaps), the image of the other label tools;
  128x256x256  a volume of 3 000 random balls;
  16384^2      ~8.3e5 lattice discs.

Every image is an int32 tensor that is already on the device.  Per function:
  device_call         the entry points alone by device events, median and range of --steps timed calls after --warmup:
                      sd_find_boundaries_device (mode inner, connectivity 1; mode outer, full connectivity); the clear pass
                      sd_label_clear_flagged_device with the flags of remove_small_objects (values and keys one image) and in
                      clear_border's shape (the keys another image: the components); sd_label_border_flags_device on the band of
                      buffer_size 0 and on a mask
  device_python_call  the public function on the tensor, host clock around a synchronise
  host_s              the host route on the same array, host clock, --host-steps calls (one for the 16384^2 image); clear_border's host
                      route on the 16384^2 image builds a pixel graph of 2.7e8 nodes and is left out unless --host-clear-border-16k
Bytes a call must move, given as a share of the 6.29 TB/s of a float4 copy on the MI355X (profiles/normalize_times.json):
find_boundaries reads the labels once and writes one byte per pixel (5 B / pixel), the clear pass reads values and keys and writes
the result (12 B / pixel; in remove_small_objects values and keys are one image, which the cache serves once, so its share can pass 1).

Writes profiles/label_edit_times.json (or --out).  Needs a HIP device: there is no fallback."""
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


def host_clock(torch, fn, steps):
    ms, out = [], None
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms), out


def with_bandwidth(rec, nbytes):
    rec["bytes"] = int(nbytes)
    rec["tb_per_s"] = nbytes / (rec["median_ms"] * 1e-3) / 1e12
    rec["share_of_copy_bandwidth"] = rec["tb_per_s"] / COPY_TBPS
    return rec


def time_scene(torch, N, name, lbl, steps, warmup, host_steps, host_clear_border):
    from stardist_amd import utils as U
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    lbl = np.ascontiguousarray(lbl.astype(np.int32))
    t = torch.as_tensor(lbl, device="cuda:0")
    zyx = ((1,) + tuple(t.shape)) if t.dim() == 2 else tuple(t.shape)
    nd, n, top = t.dim(), t.numel(), int(lbl.max())
    res = dict(shape=list(lbl.shape), dtype="int32", objects=int(len(np.unique(lbl)) - 1))

    def host(fn):
        hs, out = [], None
        for _ in range(host_steps):
            t0 = time.perf_counter()
            out = fn()
            hs.append(time.perf_counter() - t0)
        return dict(median_s=float(np.median(hs)), min_s=float(np.min(hs)), max_s=float(np.max(hs)), n=len(hs)), out

    def record(key, python_call, host_call, entry=None, nbytes=None):
        rec = {}
        if entry is not None:
            rec["device_call"] = with_bandwidth(device_events(torch, entry, steps, warmup), nbytes)
        for _ in range(2):
            python_call()
        rec["device_python_call"], got = host_clock(torch, python_call, steps)
        if host_call is None:
            rec["host_s"] = "not run (see the tool's docstring)"
        else:
            rec["host_s"], want = host(host_call)
            rec["host_over_device"] = rec["host_s"]["median_s"] * 1e3 / rec["device_python_call"]["median_ms"]
            rec["identical_to_host"] = bool(np.array_equal(got.cpu().numpy(), want))
            assert rec["identical_to_host"], (name, key)
        res[key] = rec
        print(name, key, json.dumps(rec), flush=True)

    out8 = torch.empty(t.shape, dtype=torch.uint8, device=t.device)
    for key, c, mode, code in (("find_boundaries_inner_c1", 1, "inner", 1), ("find_boundaries_outer_full", nd, "outer", 2)):
        record(key, lambda: U.find_boundaries(t, c, mode), lambda: U.find_boundaries(lbl, c, mode),
               lambda: N.dcall(t, "sd_find_boundaries_device", vp(t), *zyx, c, code, 0, 2 ** 31 - 1, vp(out8)), 5 * n)
    del out8
    sizes = torch.bincount(t.reshape(-1), minlength=top + 1)
    flags = (sizes < 64).to(torch.uint8).contiguous()
    out32 = torch.empty_like(t)
    record("remove_small_objects_64", lambda: U.remove_small_objects(t, 64), lambda: U.remove_small_objects(lbl, 64),
           lambda: N.dcall(t, "sd_label_clear_flagged_device", vp(t), vp(t), vp(flags), top + 1, n, 0, vp(out32)), 12 * n)
    del out32, flags
    big = torch.nonzero(sizes > 64).reshape(-1)
    big_host = big.cpu().numpy()
    record("select_labels_relabel", lambda: U.select_labels(t, big, relabel=True), lambda: U.select_labels(lbl, big_host, relabel=True))
    comp = U.label_components(t, nd)
    flags = torch.empty(n + 1, dtype=torch.uint8, device=t.device)
    mask = torch.ones(t.shape, dtype=torch.uint8, device=t.device)
    out32 = torch.empty_like(t)
    band = 2 * sum(n // s for s in t.shape)                                 # an upper bound of the band's pixels, 4 B read each
    res["border_flags_band"] = dict(device_call=with_bandwidth(device_events(
        torch, lambda: N.dcall(t, "sd_label_border_flags_device", vp(comp), *zyx, nd, 0, None, n + 1, vp(flags)), steps, warmup), n + 1 + 4 * band))
    res["border_flags_mask"] = dict(device_call=with_bandwidth(device_events(
        torch, lambda: N.dcall(t, "sd_label_border_flags_device", vp(comp), *zyx, nd, 0, vp(mask), n + 1, vp(flags)), steps, warmup), n + 1 + n))
    N.dcall(t, "sd_label_border_flags_device", vp(comp), *zyx, nd, 0, None, n + 1, vp(flags))
    res["clear_pass_keys_apart"] = dict(device_call=with_bandwidth(device_events(
        torch, lambda: N.dcall(t, "sd_label_clear_flagged_device", vp(t), vp(comp), vp(flags), n + 1, n, 0, vp(out32)), steps, warmup), 12 * n))
    for key in ("border_flags_band", "border_flags_mask", "clear_pass_keys_apart"):
        print(name, key, json.dumps(res[key]), flush=True)
    del comp, flags, mask, out32
    run_host = name != "16384x16384" or host_clear_border
    record("clear_border", lambda: U.clear_border(t), (lambda: U.clear_border(lbl)) if run_host else None)
    del t
    torch.cuda.empty_cache()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated scene names to leave out")
    ap.add_argument("--host-clear-border-16k", action="store_true", help="run clear_border's host route on the 16384^2 image too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_edit_times.json"))
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
        res["scenes"][name] = time_scene(torch, N, name, make(), args.steps, args.warmup, 1 if name == "16384x16384" else args.host_steps,
                                         args.host_clear_border_16k)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
