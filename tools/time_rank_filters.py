"""Time the rank filters and grey morphology on the device (csrc/rank_filter.hip) against scipy.ndimage on the same arrays, with
identical results asserted.  The scenes are the three shapes of the other tools (2048^2, 128x256x256, 16384^2); the image of a scene is
noise around 100 with one bright pixel per 400 pixels, made on the device from a fixed seed, as uint16 and as float32.

Per scene and dtype: minimum_filter(size 3 / 15), median_filter(size 3 / 5 / 9), median_filter under a disc of radius 7 (a ball of
radius 3 in 3D), white_tophat(size 15), and the chain median_filter(3) -> white_tophat(15) -> detect_spots(1.5).  Per operation:
  device_call   the entry points alone (sd_minmax_box_device / sd_rank_filter_device through their Python driver, on a tensor that is
                on the device), by device events; median and range of --steps timed calls after --warmup.  For the chain: the public
                calls to tensors
  tensors / numpy   the public function on the device tensor / on the numpy array with device=, host clock around a synchronise
  host          scipy.ndimage (the host route) on the same array; --host-steps calls.  At 16384^2 only minimum_filter(3),
                median_filter(3) and white_tophat(15) are run on the host, once: the others take minutes
  bytes_min / share_of_copy_rate   one read and one write of the image, and that over the median device_call time as a share of the
                6.29 TB/s copy rate
The first and the last device call's results are compared bit for bit, and every route with scipy's where that ran.

Writes profiles/rank_filter_times.json (or --out); scenes that an earlier run wrote there stay.  Needs a HIP device: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_point_neighbors import device_events, host_clock, host_seconds  # noqa: E402

COPY_RATE = 6.29e12
SHAPES = {"2048x2048": (2048, 2048), "128x256x256": (128, 256, 256), "16384x16384": (16384, 16384)}


def disc(r, nd):
    g = np.mgrid[tuple(slice(-r, r + 1) for _ in range(nd))]
    return (g ** 2).sum(0) <= r * r


def same(a, b):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return bool(a.dtype == b.dtype and np.array_equal(a, b, equal_nan=b.dtype.kind == "f"))


def make_image(torch, shape, dtype):
    g = torch.Generator(device="cuda:0").manual_seed(int(np.prod(shape)) % 1000003)
    img = torch.randn(shape, device="cuda:0", generator=g) * 6 + 100
    bright = torch.rand(shape, device="cuda:0", generator=g) < 1 / 400
    img += bright * (300 + 900 * torch.rand(shape, device="cuda:0", generator=g))
    if dtype == "float32":
        return img
    return img.clamp(0, 32767).round().to(torch.int16).view(torch.uint16)


def time_scene(torch, name, shape, dtype, steps, warmup, host_steps):
    import scipy.ndimage as ndi
    from stardist_amd import rank_filters as RF
    from stardist_amd import utils as U
    nd = len(shape)
    img = make_image(torch, shape, dtype)
    host_img = U.to_host(img)
    count = img.numel()
    large = count > 2 ** 27
    res = dict(shape=list(shape), dtype=dtype, pixels=count)
    print(name, dtype, json.dumps(res), flush=True)
    ball = disc(7 if nd == 2 else 3, nd)
    ops = [("minimum_3", "minimum_filter", dict(size=3), True), ("minimum_15", "minimum_filter", dict(size=15), False),
           ("median_3", "median_filter", dict(size=3), True), ("median_5", "median_filter", dict(size=5), False),
           ("median_9" if nd == 2 else "median_5x5x5", "median_filter", dict(size=9 if nd == 2 else 5), False),
           ("median_disc7" if nd == 2 else "median_ball3", "median_filter", dict(footprint=ball), False),
           ("white_tophat_15", "white_tophat", dict(size=15), True)]
    for label, fn, kw, host_when_large in ops:
        rec = {}
        plan, fuse, mode, cval = RF._plan(fn, nd, dtype, kw.get("size"), kw.get("footprint"), "reflect", 0)
        rec["device_call"], first, last = device_events(torch, lambda: RF._device_plan(img, plan, fuse, mode, float(cval), False), steps, warmup)
        rec["same_bits_from_call_to_call"] = bool(torch.equal(first.view(torch.uint8), last.view(torch.uint8)))
        rec["tensors"], got_t = host_clock(torch, lambda: getattr(U, fn)(img, **kw), steps)
        rec["numpy"], got_n = host_clock(torch, lambda: getattr(U, fn)(host_img, device="cuda:0", **kw), steps)
        rec["bytes_min"] = 2 * count * host_img.itemsize
        rec["share_of_copy_rate"] = rec["bytes_min"] / (rec["device_call"]["median_ms"] * 1e-3) / COPY_RATE
        if not large or host_when_large:
            rec["host"], want = host_seconds(lambda: getattr(ndi, fn)(host_img, **kw), 1 if large else host_steps)
            rec["identical_to_scipy"] = same(got_t, want) and same(got_n, want) and same(first, want)
            rec["host_over_device_numpy"] = rec["host"]["median_s"] * 1e3 / rec["numpy"]["median_ms"]
            rec["host_over_device_call"] = rec["host"]["median_s"] * 1e3 / rec["device_call"]["median_ms"]
            assert rec["identical_to_scipy"], (name, dtype, label)
        else:
            rec["host"] = "not run at this size"
        assert rec["same_bits_from_call_to_call"], (name, dtype, label)
        print(name, dtype, label, json.dumps(rec), flush=True)
        res[label] = rec
        del first, last, got_t, got_n
    # the chain that the functions were built for
    kw = dict(min_distance=2, threshold_rel=0.1, return_table=True)
    chain = lambda x, **how: U.detect_spots(U.white_tophat(U.median_filter(x, 3), size=15), 1.5, **how, **kw)
    rec = {}
    rec["device_call"], first, last = device_events(torch, lambda: tuple(chain(img, as_tensors=True).values()), steps, warmup)
    rec["same_bits_from_call_to_call"] = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(first, last))
    rec["tensors"], _ = host_clock(torch, lambda: chain(img, as_tensors=True), steps)
    rec["numpy"], got = host_clock(torch, lambda: chain(torch.as_tensor(host_img, device="cuda:0")), steps)      # one upload, the table read back
    rec["spots"] = int(len(got["coords"]))
    if not large:
        through_scipy = lambda: U.detect_spots(ndi.white_tophat(ndi.median_filter(host_img, size=3), size=15), 1.5, **kw)
        rec["host"], want = host_seconds(through_scipy, host_steps)
        rec["identical_to_host"] = bool(list(got) == list(want) and all(got[k].tobytes() == want[k].tobytes() for k in want))
        rec["host_over_device_numpy"] = rec["host"]["median_s"] * 1e3 / rec["numpy"]["median_ms"]
        assert rec["identical_to_host"], (name, dtype, "chain")
    else:
        rec["host"] = "not run at this size"
    assert rec["same_bits_from_call_to_call"], (name, dtype, "chain")
    print(name, dtype, "median_tophat_detect_spots", json.dumps(rec), flush=True)
    res["median_tophat_detect_spots"] = rec
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--scenes", default="2048x2048,128x256x256,16384x16384")
    ap.add_argument("--dtypes", default="uint16,float32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_filter_times.json"))
    args = ap.parse_args()
    import torch
    from stardist_amd.lib import _native as N
    N.require_device()
    out = dict(tool="tools/time_rank_filters.py", device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup,
               note="device_call: device events around the entry points' Python driver (for the chain the public calls to tensors); "
                    "tensors / numpy: the public call, host clock (numpy: the image uploaded and the result read back); host: scipy.ndimage "
                    "on the same array; untuned, no per-kernel trace was made")
    if os.path.exists(args.out):                                            # scenes measured in an earlier run stay
        with open(args.out) as f:
            out = dict(json.load(f), **out)
    for name in args.scenes.split(","):
        for dtype in args.dtypes.split(","):
            out["%s %s" % (name, dtype)] = time_scene(torch, name, SHAPES[name], dtype, args.steps, args.warmup, args.host_steps)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
