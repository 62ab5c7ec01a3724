"""Time relabel_image_stardist / relabel_image_stardist3D on label images that are device tensors (csrc/relabel_star.hip: centroid sums,
star distances at the centroids only, then the rasterisers' tensor paths) and the host function on the same arrays:

  2048^2       the 12 756 random discs of tools/time_matching.py, 32 rays;
  128x256x256  a volume of 3000 random balls, Rays_GoldenSpiral(96);
  16384^2      its ~8.3e5 lattice discs, 32 rays -- the device path only: the host function needs the dense (16384, 16384, 32) float32
               distances, 34 GB, on the device and on the host.

Device: the Python call on an int32 tensor that is already there, by the host clock around a synchronised call (it holds the read-backs
of the largest id, of the number of objects and of the point kernel's status), median and range of --steps timed calls after --warmup;
and the two new entry points alone by device events (sd_label_centroid_sums_device; the point entry on the centroids).
Host: the same function on the numpy array (the dense star_dist on the device, its copy to the host, the per-object centroid loop, the
rasteriser's host entry), host clock, --host-steps calls.  Bytes: the image read once and the result written once, 4 bytes a pixel
each, against the 6.29 TB/s of a float4 copy on the MI355X.  The results of both paths are compared.

Writes profiles/relabel_times.json (or --out).  Needs a HIP device: there is no fallback."""
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
    from stardist_amd.rays3d import Rays_GoldenSpiral
    yield "2048x2048", lambda: random_discs((2048, 2048), 12756, 11), 32
    yield "128x256x256", lambda: random_discs((128, 256, 256), 3000, 14, rmin=4, rmax=9), Rays_GoldenSpiral(96)
    yield "16384x16384", lambda: lattice_discs(16384, 18, 13), 32


def time_scene(torch, N, a, rays, steps, warmup, host_steps):
    from stardist_amd.geometry import relabel_image_stardist, relabel_image_stardist3D
    from stardist_amd.geometry.geom2d import _region_centroids_device
    vp = ctypes.c_void_p
    nd = a.ndim
    relabel = (lambda x: relabel_image_stardist(x, rays)) if nd == 2 else (lambda x: relabel_image_stardist3D(x, rays))
    t = torch.as_tensor(np.ascontiguousarray(a, np.int32), device="cuda:0")
    top = int(a.max())
    zyx = ((1,) + a.shape) if nd == 2 else a.shape
    sums = torch.empty((top + 1, 4), dtype=torch.int64, device=t.device)
    labs, points = _region_centroids_device(t, top)
    n, n_rays = int(len(labs)), (rays if nd == 2 else len(rays))
    dist = torch.empty((n, n_rays), dtype=torch.float32, device=t.device)
    if nd == 3:
        dz, dy, dx = (torch.as_tensor(np.ascontiguousarray(v, np.float32), device=t.device) for v in rays.vertices.T)

    def call_sums():
        N.dcall(t, "sd_label_centroid_sums_device", vp(t.data_ptr()), *zyx, top, vp(sums.data_ptr()))

    def call_points():
        if nd == 2:
            N.dcall(t, "sd_star_dist2d_points_device", vp(t.data_ptr()), *a.shape, vp(points.data_ptr()), n, n_rays, vp(dist.data_ptr()))
        else:
            N.dcall(t, "sd_star_dist3d_points_device", vp(t.data_ptr()), *a.shape, vp(points.data_ptr()), n, vp(dz.data_ptr()), vp(dy.data_ptr()),
                    vp(dx.data_ptr()), n_rays, ctypes.c_float(1e-3), vp(dist.data_ptr()))

    timed = {}
    for key, fn in (("centroid_sums_call", call_sums), ("points_call", call_points)):
        for _ in range(warmup):
            fn()
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        timed[key] = stats(ms)
    res = dict(shape=list(a.shape), objects=n, n_rays=int(n_rays), **timed)
    for _ in range(warmup):
        got = relabel(t)
    wall = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = relabel(t)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    res["device_python_call"] = stats(wall)
    nbytes = 2 * 4 * a.size
    res["bytes"] = int(nbytes)
    res["tb_per_s"] = nbytes / (res["device_python_call"]["median_ms"] * 1e-3) / 1e12
    res["share_of_copy_bandwidth"] = res["tb_per_s"] / COPY_TBPS
    kernels_ms = res["centroid_sums_call"]["median_ms"] + res["points_call"]["median_ms"]
    res["new_kernels_share_of_copy_bandwidth"] = 4 * a.size / (kernels_ms * 1e-3) / 1e12 / COPY_TBPS
    out = got.cpu().numpy()
    res["pixels_labelled"] = int((out > 0).sum())
    if host_steps > 0:
        hs = []
        for _ in range(host_steps):
            t0 = time.perf_counter()
            want = relabel(a)
            hs.append(time.perf_counter() - t0)
        res["host_s"] = dict(median_s=float(np.median(hs)), min_s=float(np.min(hs)), max_s=float(np.max(hs)), n=len(hs))
        res["identical_results"] = bool(np.array_equal(out, np.asarray(want)))
        res["host_over_device"] = res["host_s"]["median_s"] * 1e3 / res["device_python_call"]["median_ms"]
    del t, got
    torch.cuda.empty_cache()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated scene names to leave out")
    ap.add_argument("--skip-host", default="16384x16384", help="comma-separated scene names whose host run is left out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relabel_times.json"))
    args = ap.parse_args(argv)
    if args.steps < 20 or args.warmup < 5:
        ap.error("at least 20 timed calls after 5 warm-ups")
    import torch
    from stardist_amd.lib import _native as N
    N.require_device()
    res = dict(device=torch.cuda.get_device_name(0), copy_bandwidth_tb_per_s=COPY_TBPS, steps=args.steps, warmup=args.warmup, scenes={})
    for name, make, rays in scenes():
        if name in args.skip.split(","):
            continue
        host_steps = 0 if name in args.skip_host.split(",") else args.host_steps
        res["scenes"][name] = time_scene(torch, N, make(), rays, args.steps, args.warmup, host_steps)
        print(name, json.dumps(res["scenes"][name]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
