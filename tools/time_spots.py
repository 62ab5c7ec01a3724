"""Time the spot functions on the device (csrc/spots.hip) against their host routes on the same arrays, with identical results asserted.
The label images are the three scenes of the other label tools (2048^2: 12 756 random discs; 128x256x256: 3 000 random balls; 16384^2:
~8.3e5 lattice discs); the image of a scene is uint16 noise around 100 with one bright pixel per 400 pixels, made on the device from a
fixed seed, so that its Gaussian shows foci.

Per scene: gaussian_filter at sigma 1 and 2, difference_of_gaussians(1), and on that difference peak_local_max at min_distance 1 and 3
(threshold_rel 0.1), without and with the labels, and detect_spots(1, min_distance 2, threshold_rel 0.1) on the image.  Per operation:
  device_call   the entry point alone (sd_gaussian_filter_device once or twice; sd_peak_local_max_device + sd_peaks_emit_device, which
                synchronise the stream themselves to size the result) through its Python driver on tensors that are on the device, by
                device events; median and range of --steps timed calls after --warmup
  tensors / numpy   the public function on the device tensor, results as tensors / as numpy arrays, host clock around a synchronise
  host          the host route on the same array; --host-steps calls.  At 16384^2 only sigma 1 and min_distance 1 are run on the host
                (one call each): the others take minutes
  bytes_min / share_of_copy_rate   what the operation must move (Gaussian: per pass one read and one float32 write; peaks: the image, the
                labels if given, the result) and that over the median device_call time, as a share of the 6.29 TB/s copy rate
The first and the last device call's results are compared bit for bit, and every route with the host route's where that ran.

Writes profiles/spots_times.json (or --out).  Needs a HIP device: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_point_neighbors import device_events, host_clock, host_seconds, scenes  # noqa: E402

COPY_RATE = 6.29e12


def bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_floats(a, b):
    nan = np.isnan(b)
    return bool(np.array_equal(np.isnan(a), nan) and np.array_equal(np.where(nan, 0, a.view(np.uint32)), np.where(nan, 0, b.view(np.uint32))))


def time_scene(torch, name, lbl, steps, warmup, host_steps):
    from stardist_amd import spots
    from stardist_amd import utils as U
    large = lbl.size > 2 ** 27
    nd = lbl.ndim
    g = torch.Generator(device="cuda:0").manual_seed(lbl.size % 1000003)
    noise = torch.randn(lbl.shape, device="cuda:0", generator=g) * 6 + 100
    bright = torch.rand(lbl.shape, device="cuda:0", generator=g) < 1 / 400
    img = (noise + bright * (300 + 900 * torch.rand(lbl.shape, device="cuda:0", generator=g))).clamp(0, 32767).round().to(torch.int16).view(torch.uint16)
    del noise, bright
    lab = torch.as_tensor(np.ascontiguousarray(lbl.astype(np.int32)), device="cuda:0")
    host_img, host_lab = U.to_host(img), lbl.astype(np.int32)
    count = img.numel()
    res = dict(shape=list(lbl.shape), pixels=count, objects=int(lbl.max()))
    print(name, json.dumps(res), flush=True)

    def record(label, device_call, public, host, compare, bytes_min, run_host=True):
        rec = {}
        rec["device_call"], first, last = device_events(torch, device_call, steps, warmup)
        first, last = (first, last) if isinstance(first, (tuple, list)) else ((first,), (last,))
        rec["same_bits_from_call_to_call"] = all(torch.equal(bits(a), bits(b)) for a, b in zip(first, last))
        rec["tensors"], got_t = host_clock(torch, lambda: public(True), steps)
        rec["numpy"], got_n = host_clock(torch, lambda: public(False), steps)
        rec["bytes_min"] = int(bytes_min(got_n))
        rec["share_of_copy_rate"] = rec["bytes_min"] / (rec["device_call"]["median_ms"] * 1e-3) / COPY_RATE
        if run_host:
            rec["host"], want = host_seconds(host, 1 if large else host_steps)
            rec["identical_to_host"] = bool(compare(got_n, want) and compare(got_t, want))
            rec["host_over_device_numpy"] = rec["host"]["median_s"] * 1e3 / rec["numpy"]["median_ms"]
            assert rec["identical_to_host"], (name, label)
        else:
            rec["host"] = "not run at this size"
        assert rec["same_bits_from_call_to_call"], (name, label)
        print(name, label, json.dumps(rec), flush=True)
        res[label] = rec

    to_np = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else v
    for sigma in (1.0, 2.0):
        plan = spots._gaussian_plan([sigma] * nd, 4.0)
        record("gaussian_sigma%g" % sigma, lambda: spots._gaussian_device(img, plan),
               lambda as_t: U.gaussian_filter(img if as_t else host_img, sigma, device="cuda:0"), lambda: U.gaussian_filter(host_img, sigma),
               lambda got, want: same_floats(to_np(got), want), lambda got: count * (2 + 4) + (nd - 1) * count * 8,
               run_host=not large or sigma == 1.0)
    low, high = spots._gaussian_plan([1.0] * nd, 4.0), spots._gaussian_plan([1.6] * nd, 4.0)
    record("difference_of_gaussians_1", lambda: spots._gaussian_device(img, low) - spots._gaussian_device(img, high),
           lambda as_t: U.difference_of_gaussians(img if as_t else host_img, 1.0, device="cuda:0"), lambda: U.difference_of_gaussians(host_img, 1.0),
           lambda got, want: same_floats(to_np(got), want), lambda got: 2 * (count * (2 + 4) + (nd - 1) * count * 8) + count * 12,
           run_host=not large)
    dog = U.difference_of_gaussians(img, 1.0)
    host_dog = U.to_host(dog)
    table = lambda got, want: list(got) == list(want) and all(to_np(got[k]).tobytes() == want[k].tobytes() for k in want)
    for d in (1, 3):
        for with_labels in (False, True):
            kw = dict(min_distance=d, threshold_rel=0.1)
            args = spots._peak_args(tuple(dog.shape), d, None, 0.1, True, None, None)
            dl, hl = (lab, host_lab) if with_labels else (None, None)
            record("peaks_d%d%s" % (d, "_labels" if with_labels else ""),
                   lambda: spots._peaks_device(dog, dl, args[0], args[1], args[2], args[3], args[5], args[4]),
                   lambda as_t: U.peak_local_max(dog, labels=dl, return_table=True, as_tensors=as_t, **kw),
                   lambda: U.peak_local_max(host_dog, labels=hl, return_table=True, **kw), table,
                   lambda got: count * (4 + 4 * with_labels) + len(got["coords"]) * (8 + 8 * nd + 4 + 4),
                   run_host=not large or (d == 1 and not with_labels))
            res["peaks_d%d%s" % (d, "_labels" if with_labels else "")]["peaks"] = int(len(U.peak_local_max(dog, labels=dl, **kw)))
    kw = dict(min_distance=2, threshold_rel=0.1)
    record("detect_spots_1", lambda: tuple(U.detect_spots(img, 1.0, return_table=True, as_tensors=True, **kw).values()),
           lambda as_t: U.detect_spots(img if as_t else host_img, 1.0, return_table=True, as_tensors=as_t, device="cuda:0", **kw),
           lambda: U.detect_spots(host_img, 1.0, return_table=True, **kw), table,
           lambda got: 2 * (count * (2 + 4) + (nd - 1) * count * 8) + count * 12 + count * 4 + len(got["coords"]) * (8 + 8 * nd + 4 + 4),
           run_host=not large)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--scenes", default="2048x2048,128x256x256,16384x16384")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spots_times.json"))
    args = ap.parse_args()
    import torch
    from stardist_amd.lib import _native as N
    N.require_device()
    out = dict(tool="tools/time_spots.py", device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup,
               note="device_call: device events around the entry points' Python driver (for detect_spots the public call to tensors); "
                    "tensors / numpy: the public call, host clock (numpy: the image uploaded and the result read back); host: the numpy "
                    "route; untuned, no per-kernel trace was made")
    make = scenes()
    for name in args.scenes.split(","):
        out[name] = time_scene(torch, name, make[name](), args.steps, args.warmup, args.host_steps)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
