"""Time matching(y_true, y_pred, thresh=[0.3, 0.5, 0.7]) on the host (dense overlap + linear_sum_assignment) and on the device (sparse
overlap kernel csrc/overlap.hip + exact host finishing, stardist_amd.matching_sparse) for two synthetic pairs:
  2048^2:  12 756 random discs (radius 3..9) against the same discs shifted by (2, 1) with 2 000 random discs cut out;
  16384^2: ~8.3e5 discs on a lattice against the same image shifted by (1, 2) (device only: the dense host path cannot hold it).
Prints one JSON line per pair: median wall time of the host call and of the device call, and the device call split into the overlap
kernel (upload excluded, read-back of the list included) and the host finishing.

    python tools/time_matching.py [--repeat 5] [--skip-host] [--out profiles/matching_times.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THRESH = [0.3, 0.5, 0.7]


def random_discs(shape, n, seed, rmin=3, rmax=10):
    rng = np.random.RandomState(seed)
    y = np.zeros(shape, np.int32)
    for i in range(1, n + 1):
        r = rng.randint(rmin, rmax)
        c = [rng.randint(0, s) for s in shape]
        sl = tuple(slice(max(0, ci - r), min(s, ci + r + 1)) for ci, s in zip(c, shape))
        g = np.ogrid[sl]
        y[sl][sum((gi - ci) ** 2 for gi, ci in zip(g, c)) < r * r] = i
    return y


def lattice_discs(size, cell, seed):
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


def pair_2048():
    a = random_discs((2048, 2048), 12756, 11)
    b = np.roll(a, (2, 1), axis=(0, 1))
    b[random_discs((2048, 2048), 2000, 12) > 0] = 0
    return a, b


def pair_16384():
    a = lattice_discs(16384, 18, 13)
    return a, np.roll(a, (1, 2), axis=(0, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from stardist_amd import matching as M
    from stardist_amd import matching_sparse as S
    dev = torch.device("cuda:0")
    lines = []
    for name, make, host_ok in (("2048x2048", pair_2048, True), ("16384x16384", pair_16384, False)):
        a, b = make()
        ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        rec = dict(pair=name, n_true=int(len(np.unique(a)) - 1), n_pred=int(len(np.unique(b)) - 1), thresh=THRESH)
        del a, b
        M.matching(ta, tb, thresh=THRESH)                                # warm-up (workspace, kernels)
        dev_t, ker_t, fin_t = [], [], []
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = M.matching(ta, tb, thresh=THRESH)
            dev_t.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            (t, p, c), _, _ = S.label_overlap_device(ta, tb)
            t1 = time.perf_counter()
            S.matching_from_overlap(t, p, c, ta.numel(), thresh=THRESH)
            t2 = time.perf_counter()
            ker_t.append(t1 - t0)
            fin_t.append(t2 - t1)
        rec.update(device_s=float(np.median(dev_t)), device_overlap_kernel_s=float(np.median(ker_t)), device_host_finish_s=float(np.median(fin_t)),
                   pairs=int(len(t)), tp=[s.tp for s in res], repeat=args.repeat)
        if host_ok and not args.skip_host:
            a, b = ta.cpu().numpy(), tb.cpu().numpy()
            t0 = time.perf_counter()
            h = M.matching(a, b, thresh=THRESH)
            rec.update(host_s=time.perf_counter() - t0, host_equal=all(x == y for x, y in zip(h, res)))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del ta, tb
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="tools/time_matching.py", device=torch.cuda.get_device_name(0), cpus=len(os.sched_getaffinity(0)), results=lines), fh, indent=1)


if __name__ == "__main__":
    main()
