"""GPU: the pair probe sd_clip_pairs_device (AddPath of both polygons + the tier-1 bound-slot sweep per lane, the general sweep behind it)
on the pair families of tests/host/beam_families_check.cpp -- horizontals on a scan line, exact ties of TopX, vertices at the edge of the
16-bit range, random 3- to 32-gons, identical and touching rings -- mixed pair by pair so that the lanes of a wave differ.  Area and
flags must equal the same header evaluated on the host, and the area the reference's compiled Clipper gave for the same pairs
(tests/golden/beam_families/, recorded with `beam_families_check golden 8192 7`).  And the 2D NMS on one small dense scene, with and
without nms2d_strict: keep flags and pair counts as recorded at the commit before the sweep's per-beam work was cut
(tools/record_nms2d_scene_golden.py)."""
import ctypes
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "beam_families")
N_PAIRS, SEED, R = 8192, 7, 32


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    """the mixed set, its host evaluation (computed once) and Clipper's recorded areas"""
    so = str(tmp_path_factory.mktemp("beamfam") / "libbeam_families_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DNO_CLIPPER_REF", os.path.join(ROOT, "tests", "host", "beam_families_check.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    v = [np.zeros((N_PAIRS, R), np.int32) for _ in range(4)]
    lib.fam_generate(0, ctypes.c_long(N_PAIRS), ctypes.c_uint(SEED), *[vp(a.ctypes.data) for a in v])
    twice = np.zeros(N_PAIRS, np.int64); flags = np.zeros(N_PAIRS, np.int32); joins = np.zeros(N_PAIRS, np.int32); sabs = np.zeros(N_PAIRS, np.int64)
    lib.fam_host_probe(*[vp(a.ctypes.data) for a in v], ctypes.c_long(N_PAIRS), vp(twice.ctypes.data), vp(flags.ctypes.data), vp(joins.ctypes.data), vp(sabs.ctypes.data))
    ref = np.fromfile(os.path.join(GOLD, "clipper_area_mixed_seed7_n8192.f32"), np.float32)
    assert len(ref) == N_PAIRS
    for a in v + [twice, flags, joins, sabs, ref]:
        a.setflags(write=False)
    return v, twice, flags, joins, sabs, ref


def test_host_evaluation_equals_recorded_clipper(pairs):
    """the set is the one the golden was recorded on, and the host side of the comparison below is itself right"""
    v, twice, flags, joins, sabs, ref = pairs
    assert "%08x" % zlib.crc32(np.stack(v).tobytes()) == "b14c5a61"
    exact = ((flags & 256) != 0) | (sabs < (1 << 24))          # (the reference sums in float: a bound-slot area is comparable below 2^24)
    assert exact.all()
    assert np.array_equal(np.float32(0.5) * twice.astype(np.float32), ref)
    assert (joins != 0).sum() > 100 and ((flags & 256) != 0).sum() > 1000 and ((flags & 512) != 0).sum() > 1000


@pytest.mark.parametrize("n", [1, 63, 64, 65, N_PAIRS])
def test_device_probe_equals_host_and_clipper(pairs, n):
    from stardist_amd.lib import stardist2d as sd2
    v, twice, flags, joins, sabs, ref = pairs
    got, fl = sd2.clip_pairs(*[np.array(a[:n]) for a in v])
    bad = np.flatnonzero((got != twice[:n]) | (fl != flags[:n]))
    assert len(bad) == 0, "%d of %d pairs differ from the host, first: pair %d device (%d, %d) host (%d, %d)" % (
        len(bad), n, bad[0], got[bad[0]], fl[bad[0]], twice[bad[0]], flags[bad[0]])
    assert ((fl & 256) != 0)[joins[:n] != 0].all()             # a pair with join records is the general path's
    assert np.array_equal(np.float32(0.5) * got.astype(np.float32), ref[:n])


def nms_scene():
    """about 3 000 candidates of radius 10 +- 10 % on a 330 x 330 field, in score order: every polygon overlaps a few dozen others"""
    rng = np.random.RandomState(11)
    n = 3000
    dist = (10.0 * (1 + 0.1 * rng.uniform(-1, 1, (n, R)))).astype(np.float32)
    points = np.floor(rng.uniform(20, 350, (n, 2))).astype(np.float32)
    return np.ascontiguousarray(dist), np.ascontiguousarray(points)


STAT_NAMES = {0: "pairs", 1: "general", 8: "spilled", 9: "decided", 10: "deferred", 11: "skipped"}


def run_nms_scene(strict):
    from stardist_amd.lib import _native, stardist2d as sd2
    import torch
    dist, points = nms_scene()
    dev = torch.device("cuda")
    _native.check(_native.lib().sd_set_option(b"nms2d_strict", 1 if strict else 0))
    try:                                                                        # (device tensors: sd_nms2d_device)
        keep, stats = sd2.c_non_max_suppression_inds(torch.from_numpy(dist).to(dev), torch.from_numpy(points).to(dev), 1, 1, 0, np.float32(0.4), return_stats=True)
        torch.cuda.synchronize()
    finally:
        _native.check(_native.lib().sd_set_option(b"nms2d_strict", 0))
    keep = keep.cpu().numpy().astype(np.uint8)
    return {"inputs_crc": "%08x" % zlib.crc32(dist.tobytes() + points.tobytes()), "kept": int(keep.sum()), "keep_crc": "%08x" % zlib.crc32(keep.tobytes()),
            "keep_bits": np.packbits(keep).tobytes().hex(), **{name: int(stats[i]) for i, name in STAT_NAMES.items()}}


@pytest.mark.parametrize("strict", [0, 1])
def test_nms_scene_keeps_and_counts_as_recorded(strict):
    with open(os.path.join(GOLD, "nms2d_scene_parent.json")) as fh:
        want = json.load(fh)["strict" if strict else "default"]
    got = run_nms_scene(strict)
    assert got["inputs_crc"] == want["inputs_crc"]
    assert got["keep_bits"] == want["keep_bits"], (got["kept"], want["kept"])
    assert {k: got[k] for k in STAT_NAMES.values()} == {k: want[k] for k in STAT_NAMES.values()}
    assert want["pairs"] > 4000 and 0 < want["kept"] < 3000
