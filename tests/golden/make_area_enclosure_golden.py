"""Goldens of the 2D NMS's area enclosure (stardist_amd/csrc/area_bounds.h pair_enclosure), recorded on the GPU from the build of ONE
commit so that a later rewrite of the kernel is held to that commit's bits, not to itself.

small_families() and large_family() build the inputs from seeds (tests/_poly_families.py star_polys), so only the outputs are stored:
  area_enclosure_small.npz    per small family "<name>/area", "<name>/band" (uint32 bit patterns of the float32 results),
                              "<name>/usable" (uint8), "<name>/K", "<name>/T" (uint16) of sd2.area_bounds_pairs
  area_enclosure_golden.json  "large": the crc32 of each of the five arrays for the 60 001 pairs of large_family();
                              "nms": per scene of nms_scenes() the stats[0], [9], [10], [11] (pairs, decided by the enclosure, deferred
                              undecided, skipped) of sd2.c_non_max_suppression_inds; "tail_scene": the first candidate of
                              TAIL_CANDIDATES whose run defers undecided pairs to the tail batch (stats[10] > 0)
The small families (pair counts are odd: the last wave's upper half idles; "single_R32" leaves the upper half idle throughout):
  star_R3, star_R7, star_R31       the wrap of the next-edge index and the dead lanes of a half-wave
  star_R32, coincident_R32         radius 10 at (noise 0.1, spread 12) and near-coincident at (0.03, 3): many crossings and strips
  small_R32, tiny_R32              radius 4 and 2.5: zero-length edges, polygons that are not robustly simple
  degenerate_R5                    the nine configurations of tests/test_cpu_area_enclosure.py::test_degenerate_configurations in both
                                   common orientations, then the same with the orientations opposed
  mixed_R32                        star pairs with Q reversed (opposite orientation), with Q moved away by about the window (1023) and far
                                   beyond it, and unchanged
  single_R32                       one pair

usage (GPU): python tests/golden/make_area_enclosure_golden.py
The committed files were written at commit 2d2206f, before pair_enclosure kept a per-edge record of Q; tests/test_gpu_area_enclosure_golden.py and
tests/test_gpu_nms2d_decide_counts.py hold today's kernels to them, tests/test_cpu_area_enclosure_golden.py checks without a GPU that
the set holds the cases it claims to hold.  They are regenerated only by a change that means to alter the enclosure's results."""
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
NPZ = os.path.join(HERE, "area_enclosure_small.npz")
JSON = os.path.join(HERE, "area_enclosure_golden.json")
N_SMALL = 1001
N_LARGE = 60001
ARRAYS = ("area", "band", "usable", "K", "T")
TAIL_CANDIDATES = [dict(H=384, W=384, n_rays=32, prob_thresh=0.85, thr=0.4), dict(H=300, W=280, n_rays=32, prob_thresh=0.85, thr=0.7),
                   dict(H=512, W=512, n_rays=32, prob_thresh=0.85, thr=0.4), dict(H=768, W=768, n_rays=32, prob_thresh=0.8, thr=0.4)]


def _star_polys():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        from _poly_families import star_polys
    finally:
        sys.path.pop(0)
    return star_polys


def _pair(seed, n, R, radius, noise, spread, scale):
    star_polys = _star_polys()
    rng = np.random.RandomState(seed)
    xa, ya = star_polys(rng, n, R, radius, noise, spread)
    xb, yb = star_polys(rng, n, R, radius * scale, noise, spread)
    return xa, ya, xb, yb


def degenerate_pairs():
    """the nine configurations of test_degenerate_configurations, padded to 5 vertices by repeating the last one: both orientations
    in common (18 pairs), then opposed (18 pairs)"""
    sq = lambda x0, y0, w, h: (np.array([x0, x0 + w, x0 + w, x0]), np.array([y0, y0, y0 + h, y0 + h]))
    cases = [(sq(0, 0, 10, 10), sq(0, 0, 10, 10)), (sq(0, 0, 10, 10), sq(10, 0, 10, 10)), (sq(0, 0, 10, 10), sq(0, 0, 5, 10)),
             (sq(0, 0, 10, 10), sq(10, 10, 5, 5)), (sq(0, 0, 10, 10), sq(5, 0, 10, 10)), (sq(0, 0, 10, 10), sq(2, 2, 3, 3)),
             (sq(0, 0, 10, 10), sq(20, 0, 3, 3)),
             ((np.array([0, 10, 5]), np.array([0, 0, 10])), (np.array([5, 10, 0]), np.array([0, 10, 10]))),
             ((np.array([0, 10, 10, 5, 0]), np.array([0, 0, 10, 10, 10])), sq(5, 5, 10, 10))]
    pad = lambda v: np.concatenate([v, np.repeat(v[-1:], 5 - len(v))])
    rows = []
    for opposed in (False, True):
        for (ax, ay), (bx, by) in cases:
            for flip_a in (False, True):
                flip_b = flip_a != opposed
                xa, ya = (ax[::-1], ay[::-1]) if flip_a else (ax, ay)
                xb, yb = (bx[::-1], by[::-1]) if flip_b else (bx, by)
                rows.append([pad(xa), pad(ya), pad(xb), pad(yb)])
    a = np.array(rows, np.int32)
    return tuple(np.ascontiguousarray(a[:, i]) for i in range(4))


def mixed_pairs():
    """61 star pairs: 0..19 with Q reversed, 20..39 with Q moved in x or y by 1000, 1010, ... (the window ends at an extent of 1023 about
    the centre of P's box) and by 5000 / 70000, 40..60 unchanged"""
    xa, ya, xb, yb = _pair(909, 61, 32, 10, 0.1, 12, 0.9)
    xb, yb = xb.copy(), yb.copy()
    xb[:20], yb[:20] = xb[:20, ::-1].copy(), yb[:20, ::-1].copy()
    shifts = [1000, 1005, 1010, 1012, 1014, 1016, 1018, 1020, 1025, 1030, 5000, 70000]
    for k in range(20):
        s = shifts[k % len(shifts)] * (-1 if k % 3 == 2 else 1)
        if k % 2: yb[20 + k] += s
        else: xb[20 + k] += s
    return xa, ya, np.ascontiguousarray(xb), np.ascontiguousarray(yb)


def small_families():
    """name -> (xa, ya, xb, yb) int32 (n_pairs, R), in a fixed order"""
    f = {}
    f["star_R3"] = _pair(903, N_SMALL, 3, 6, 0.5, 12, 0.8)
    f["star_R7"] = _pair(907, N_SMALL, 7, 12, 0.2, 14, 0.8)
    f["star_R31"] = _pair(931, N_SMALL, 31, 10, 0.1, 12, 0.8)
    f["star_R32"] = _pair(932, N_SMALL, 32, 10, 0.1, 12, 0.8)
    f["coincident_R32"] = _pair(933, N_SMALL, 32, 10, 0.03, 3, 0.97)
    f["small_R32"] = _pair(934, N_SMALL, 32, 4, 0.3, 6, 0.8)
    f["tiny_R32"] = _pair(935, N_SMALL, 32, 2.5, 0.3, 4, 1.0)
    f["degenerate_R5"] = degenerate_pairs()
    f["mixed_R32"] = mixed_pairs()
    f["single_R32"] = _pair(936, 1, 32, 10, 0.1, 12, 0.8)
    return f


def large_family():
    return _pair(960, N_LARGE, 32, 10, 0.1, 12, 0.8)


def nms_scenes(tail_scene):
    sc = [dict(H=384, W=384, n_rays=32, prob_thresh=0.85, thr=0.3), dict(H=384, W=384, n_rays=32, prob_thresh=0.85, thr=0.5)]
    return sc + ([dict(tail_scene)] if tail_scene else [])


def encode(out):
    """what sd2.area_bounds_pairs returned -> the stored arrays"""
    area, band, usable, K, T = out
    return {"area": np.ascontiguousarray(area, np.float32).view(np.uint32), "band": np.ascontiguousarray(band, np.float32).view(np.uint32),
            "usable": np.asarray(usable).astype(np.uint8), "K": np.asarray(K).astype(np.uint16), "T": np.asarray(T).astype(np.uint16)}


def crc(a):
    return "%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes())


def run_scene(sc):
    """-> (keep flags, stats) of the 2D NMS on a scene of nms_scenes()"""
    from oracle import synth
    from stardist_amd.lib import stardist2d as sd2
    d, p, s = synth.s2d_uniform(sc["H"], sc["W"], n_rays=sc["n_rays"], prob_thresh=sc["prob_thresh"])
    keep, stats = sd2.c_non_max_suppression_inds(d, p, 1, 1, 0, np.float32(sc["thr"]), return_stats=True)
    return d, p, np.asarray(keep), [int(v) for v in stats]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from stardist_amd.lib import stardist2d as sd2
    small = {}
    for name, polys in small_families().items():
        enc = encode(sd2.area_bounds_pairs(*polys))
        for k in ARRAYS:
            small["%s/%s" % (name, k)] = enc[k]
        print(name, polys[0].shape, "usable", int(enc["usable"].sum()), "K max", int(enc["K"].max()), "T max", int(enc["T"].max()))
    np.savez_compressed(NPZ, **small)
    enc = encode(sd2.area_bounds_pairs(*large_family()))
    gold = {"large": {"n_pairs": N_LARGE, "crc32": {k: crc(enc[k]) for k in ARRAYS}}}
    tail = None
    for sc in TAIL_CANDIDATES:
        st = run_scene(sc)[3]
        print("tail candidate", sc, "deferred undecided", st[10])
        if st[10] > 0:
            tail = sc
            break
    if tail is None:
        raise SystemExit("no candidate scene defers undecided pairs to the tail batch")
    gold["tail_scene"] = tail
    gold["nms"] = []
    for sc in nms_scenes(tail):
        d, p, keep, st = run_scene(sc)
        gold["nms"].append({"scene": sc, "n_candidates": int(len(d)), "n_kept": int(keep.sum()),
                            "stats": {"pairs": st[0], "decided": st[9], "deferred_undecided": st[10], "skipped": st[11]}})
        print(gold["nms"][-1])
    with open(JSON, "w") as fh:
        json.dump(gold, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(gold["large"]), os.path.getsize(NPZ), "bytes of small goldens")
