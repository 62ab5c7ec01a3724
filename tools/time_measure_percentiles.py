"""Time measure_labels(percentiles=) on the device (csrc/measure_rank.hip) and on the host (np.percentile per object) on the same arrays,
with a uint16 and a float32 image each and percentiles (50,) and (25, 50, 75):

  2048^2       the 12 756 random discs of tools/time_matching.py;
  128x256x256  a volume of 3 000 random balls;
  16384^2      its ~8.3e5 lattice discs;
  4096^2/one   one object that covers the whole image (uint16, float32): the chunked tier, spread over the grid.

Device, on tensors that are already there, median and range of --steps timed calls after --warmup:
  rank_call                   sd_label_percentiles_device alone (device events): the new kernels, on a box table made before
  device_python_call          measure_labels(tensor, tensor, percentiles=q, as_tensors=True) (host clock around a synchronise)
  device_python_call_numpy    measure_labels(tensor, tensor, percentiles=q): adds the read-back of the table and of the percentile block
  plain_python_call / plain_python_call_numpy   the same two calls without percentiles: the yardstick, same run, same arrays
Host: measure_labels(array, array, percentiles=q), host clock, once per scene, image type and q (at 16384^2 once in all: uint16, (50,),
whose table also checks the p50 column of (25, 50, 75); every 16384^2 table is besides compared with np.percentile on a sample of
2 000 objects).  The tool asserts that device and host give identical tables
(== and equal NaN positions in the percentile columns; the other columns as tools/time_measure.py compares them).  The single-object
scene is compared with np.percentile of the whole image, and timed against it.

Bytes a rank_call must move: per box pixel and pass one label (4 bytes) and one value -- one pass for a box of the sort tier, one per
8-bit digit (uint16: 2, float32: 4) for the others -- plus the box table and the result table; given as a share of the 6.29 TB/s of a
float4 copy on the MI355X (profiles/normalize_times.json).

Writes profiles/measure_percentiles_times.json (or --out).  Needs a HIP device: there is no fallback."""
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
from time_measure import COPY_TBPS, CODE, events, image, scenes, stats, wall  # noqa: E402

MR_SORT_KEYS, MS_CHUNK_PIXELS = 1024, 65536                                 # csrc/measure_rank.h, csrc/measure.h
PASSES = {"uint16": 2, "float32": 4}
NUMPY_2 = int(np.__version__.split(".")[0]) >= 2
QS = ((50,), (25, 50, 75))


def same(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return bool(a.dtype == b.dtype and np.array_equal(na, nb) and (a[~na] == b[~nb]).all())


def rank_call_of(torch, N, t, x, dtype, qs):
    """(the call, its output table, the bytes it must move, box pixels per tier) for label tensor t and image tensor x"""
    vp = lambda v: ctypes.c_void_p(v.data_ptr())
    top = int(t.max())
    zyx = ((1,) + tuple(t.shape)) if t.dim() == 2 else tuple(t.shape)
    boxes = torch.empty((top + 1, 6), dtype=torch.int32, device=t.device)
    out = torch.empty((top + 1, 1, len(qs)), dtype=torch.float64, device=t.device)
    q = (ctypes.c_double * len(qs))(*[float(v) for v in qs])
    N.dcall(t, "sd_label_boxes_device", vp(t), *zyx, top, vp(boxes))
    interp = 1 if (NUMPY_2 and dtype == "float32") else 0

    def call():
        N.dcall(t, "sd_label_percentiles_device", vp(t), *zyx, top, vp(boxes), vp(x), CODE[dtype], 1, ctypes.cast(q, ctypes.c_void_p), len(qs),
                interp, vp(out))

    b = boxes.cpu().numpy().astype(np.int64)
    b = b[b[:, 5] > b[:, 2]]
    pixels = np.prod(b[:, 3:] - b[:, :3], axis=1)
    tiers = dict(sort=int(pixels[pixels <= MR_SORT_KEYS].sum()), block=int(pixels[(pixels > MR_SORT_KEYS) & (pixels <= MS_CHUNK_PIXELS)].sum()),
                 chunked=int(pixels[pixels > MS_CHUNK_PIXELS].sum()))
    per_pixel = 4 + x.element_size()
    nbytes = per_pixel * (tiers["sort"] + PASSES[dtype] * (tiers["block"] + tiers["chunked"])) + (top + 1) * (24 + 8 * len(qs))
    return call, out, int(nbytes), tiers, int(len(b))


def time_scene(torch, N, a, dtype, qs, steps, warmup, host, sample=None):
    from stardist_amd.utils import measure_labels
    img = image(a.shape, dtype, 21)
    t, x = torch.as_tensor(a, device="cuda:0"), torch.as_tensor(img, device="cuda:0")
    call, out, nbytes, tiers, objects = rank_call_of(torch, N, t, x, dtype, qs)
    res = dict(shape=list(a.shape), dtype=dtype, percentiles=list(qs), objects=objects, box_pixels_by_tier=tiers, rank_bytes=nbytes)
    res["rank_call"] = events(torch, call, steps, warmup)
    tbps = nbytes / (res["rank_call"]["median_ms"] * 1e-3) / 1e12
    res["rank_call"].update(tb_per_s=tbps, share_of_copy_bandwidth=tbps / COPY_TBPS)
    res["device_python_call"], got_t = wall(torch, lambda: measure_labels(t, x, percentiles=qs, as_tensors=True), steps, 2)
    res["device_python_call_numpy"], got = wall(torch, lambda: measure_labels(t, x, percentiles=qs), steps, 2)
    res["plain_python_call"], _ = wall(torch, lambda: measure_labels(t, x, as_tensors=True), steps, 2)
    res["plain_python_call_numpy"], plain = wall(torch, lambda: measure_labels(t, x), steps, 2)
    names = ["p%g_intensity" % q for q in qs]
    assert list(got) == list(plain) + names and all(got[k].tobytes() == plain[k].tobytes() for k in plain)
    assert all(same(got_t[k].cpu().numpy(), got[k]) for k in names)
    again = measure_labels(t, x, percentiles=qs)
    res["repeatable_bits"] = bool(all(got[k].tobytes() == again[k].tobytes() for k in got))
    if host is not None and not isinstance(host, dict):
        t0 = time.perf_counter()
        host = measure_labels(a, img, percentiles=qs)
        res["host_s"] = time.perf_counter() - t0
        res["host_over_device"] = res["host_s"] * 1e3 / res["device_python_call_numpy"]["median_ms"]
    if isinstance(host, dict):
        assert np.array_equal(got["label"], host["label"]) and all(same(got[k], host[k]) for k in names if k in host), "device and host differ"
        res["percentile_columns_identical_to_host"] = [k for k in names if k in host]
    if sample:
        rng = np.random.default_rng(5)
        rows = rng.choice(len(got["label"]), size=min(sample, len(got["label"])), replace=False)
        bb = [got["bbox-%d" % k] for k in range(2 * a.ndim)]
        for r in rows:
            box = tuple(slice(int(bb[d][r]), int(bb[d + a.ndim][r])) for d in range(a.ndim))
            v = img[box][a[box] == got["label"][r]]
            for q, k in zip(qs, names):
                want = np.percentile(v, float(q))
                assert got[k][r] == got[k].dtype.type(want), "device and np.percentile differ"
        res["sampled_objects_identical_to_numpy"] = int(len(rows))
    del t, x
    torch.cuda.empty_cache()
    return res, host


def time_single_object(torch, N, dtype, qs, steps, warmup):
    """one label over a whole 4096^2 image: 256 chunks, worked off by the grid one digit pass at a time"""
    from stardist_amd.utils import measure_labels
    a = np.ones((4096, 4096), np.int32)
    img = image(a.shape, dtype, 22)
    t, x = torch.as_tensor(a, device="cuda:0"), torch.as_tensor(img, device="cuda:0")
    call, out, nbytes, tiers, objects = rank_call_of(torch, N, t, x, dtype, qs)
    res = dict(shape=list(a.shape), dtype=dtype, percentiles=list(qs), objects=objects, box_pixels_by_tier=tiers, rank_bytes=nbytes)
    res["rank_call"] = events(torch, call, steps, warmup)
    tbps = nbytes / (res["rank_call"]["median_ms"] * 1e-3) / 1e12
    res["rank_call"].update(tb_per_s=tbps, share_of_copy_bandwidth=tbps / COPY_TBPS)
    res["device_python_call_numpy"], got = wall(torch, lambda: measure_labels(t, x, percentiles=qs), steps, 2)
    hs = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = [np.percentile(img.ravel(), float(q)) for q in qs]
        hs.append(time.perf_counter() - t0)
    res["numpy_percentile_whole_image"] = stats(np.array(hs) * 1e3)
    assert all(got["p%g_intensity" % q][0] == got["p%g_intensity" % q].dtype.type(w) for q, w in zip(qs, want)), "device and np.percentile differ"
    res["identical_to_numpy"] = True
    del t, x
    torch.cuda.empty_cache()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip", default="", help="comma-separated scene names to leave out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measure_percentiles_times.json"))
    args = ap.parse_args(argv)
    if args.steps < 20 or args.warmup < 5:
        ap.error("at least 20 timed calls after 5 warm-ups")
    import torch
    from stardist_amd.lib import _native as N
    N.require_device()
    res = dict(device=torch.cuda.get_device_name(0), copy_bandwidth_tb_per_s=COPY_TBPS, steps=args.steps, warmup=args.warmup, scenes={})

    def keep(key, value):
        res["scenes"][key] = value
        print(key, json.dumps(value), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")

    if "4096x4096/one" not in args.skip.split(","):
        for dtype in ("uint16", "float32"):
            keep("4096x4096/one/%s/%s" % (dtype, "-".join("%g" % q for q in QS[1])), time_single_object(torch, N, dtype, QS[1], args.steps, args.warmup))
    for name, make in scenes():
        if name in args.skip.split(","):
            continue
        a = make()
        big = name == "16384x16384"
        for dtype in ("uint16", "float32"):
            table = None
            for qs in QS:                                                   # at 16384^2 the host table of (50,) also serves (25, 50, 75)'s p50
                host = True if not big else (True if (dtype == "uint16" and table is None) else table)
                print("%s %s %s ..." % (name, dtype, qs), flush=True)
                got, table = time_scene(torch, N, a, dtype, qs, args.steps, args.warmup, host, sample=2000 if big else None)
                if not big:
                    table = None
                keep("%s/%s/%s" % (name, dtype, "-".join("%g" % q for q in qs)), got)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
