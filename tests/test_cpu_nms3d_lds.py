"""CPU: the dynamic-LDS layouts of the 3D NMS kernels (csrc/nms3d_lds.h through tests/host/nms3d_lds_check.cpp).

The kernels take their pointers and the host its byte counts from one description per stage; here that description is walked with a host
compiler for every ray count the library accepts: regions disjoint (except the documented alias: vertex staging, ray-cast vectors and,
in the lean form, pos / orig inside the workspace), doubles 8-aligned, the 16-aligned regions 16-aligned, bytes() = the end of the last
region.  TOTALS pins the byte counts and the branch every ray count takes to what the hand-written formulas gave before the layouts
existed (evaluated from that code, not from the header)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COLS = ("ws3", "lds3", "lds3_small", "lds3_lean", "lds3x", "lds4", "lds4_small", "lds4_lean", "lds4x", "ldsH", "lds5", "lds_rows", "ws3_small",
        "refined_once", "refined_twice", "optin3", "split3", "split4", "rejected")
# n_rays, n_faces = 2 n_rays - 4, then COLS.  The small / lean forms are those of the bounds pass over the mesh the call would choose
# (refined once where that fits).  Branches: the mesh refined twice fits up to 171 rays, refined once up to 227; stage 3 needs the opt-in
# for more than 64 KiB from 252 rays on; the four-wave exact pass of stage 3 fits up to 298 rays (stage 4: 296); the rows of k_pre1 /
# k_pre2 are staged up to 299 rays; stage 3 alone would fit up to 776 rays, stage 4 (and with it the call) up to 774.
TOTALS = [
    (4, 4, 23552, 23888, 608, 528, 94624, 24224, 944, 784, 95024, 324, 144, 2560, 272, 1, 1, 0, 1, 1, 0),
    (96, 188, 23552, 39344, 25632, 21872, 113024, 39680, 25968, 22128, 113424, 9984, 4560, 49664, 9840, 1, 1, 0, 1, 1, 0),
    (171, 338, 23552, 51944, 46024, 39264, 128032, 52280, 46360, 39520, 128432, 20992, 8160, 88064, 17632, 1, 1, 0, 1, 1, 0),
    (172, 340, 23552, 52112, 46304, 39504, 128224, 52448, 46640, 39760, 128624, 21156, 8208, 88576, 17744, 1, 0, 0, 1, 1, 0),
    (227, 450, 23552, 61352, 61256, 52256, 139232, 61688, 61592, 52512, 139632, 7264, 10848, 116736, 23456, 1, 0, 0, 1, 1, 0),
    (228, 452, 23552, 61520, 43904, 34864, 139424, 61856, 44240, 35120, 139824, 7296, 10896, 117248, 5936, 0, 0, 0, 1, 1, 0),
    (251, 498, 23552, 65384, 48360, 38400, 144032, 65720, 48696, 38656, 144432, 8032, 12000, 129024, 6528, 0, 0, 0, 1, 1, 0),
    (252, 500, 23552, 65552, 48560, 38560, 144224, 65888, 48896, 38816, 144624, 8064, 12048, 129536, 6560, 0, 0, 1, 1, 1, 0),
    (256, 508, 23552, 66224, 49328, 39168, 145024, 66560, 49664, 39424, 145424, 8192, 12240, 131584, 6656, 0, 0, 1, 1, 1, 0),
    (298, 592, 23552, 73280, 57488, 45648, 153424, 73616, 57824, 45904, 153824, 9536, 14256, 153088, 7760, 0, 0, 1, 1, 0, 0),
    (299, 594, 23552, 73448, 57672, 45792, 153632, 73784, 58008, 46048, 154032, 9568, 14304, 153600, 7776, 0, 0, 1, 0, 0, 0),
    (300, 596, 23552, 73616, 57872, 45952, 153824, 73952, 58208, 46208, 154224, 9600, 14352, 0, 7808, 0, 0, 1, 0, 0, 0),
    (774, 1544, 23552, 153248, 149824, 118944, 248624, 153584, 150160, 119200, 249024, 24768, 37104, 0, 20128, 0, 0, 1, 0, 0, 0),
    (775, 1546, 23552, 153416, 150024, 119104, 248832, 153752, 150360, 119360, 249232, 24800, 37152, 0, 20160, 0, 0, 1, 0, 0, 1),
    (776, 1548, 23552, 153584, 150208, 119248, 249024, 153920, 150544, 119504, 249424, 24832, 37200, 0, 20176, 0, 0, 1, 0, 0, 1),
    (777, 1550, 23552, 153752, 150408, 119408, 249232, 154088, 150744, 119664, 249632, 24864, 37248, 0, 20208, 0, 0, 1, 0, 0, 1),
    (800, 1596, 23552, 157616, 154864, 122944, 253824, 157952, 155200, 123200, 254224, 25600, 38352, 0, 20800, 0, 0, 1, 0, 0, 1),
]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("nms3dlds") / "libnms3dlds.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                    os.path.join(ROOT, "tests", "host", "nms3d_lds_check.cpp"), "-o", so], check=True)
    l = ctypes.CDLL(so)
    l.sdl_check.restype = ctypes.c_int
    l.sdl_check.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    l.sdl_totals.restype = None
    l.sdl_totals.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)]
    return l


def _totals(lib, R, F):
    out = (ctypes.c_longlong * len(COLS))()
    lib.sdl_totals(R, F, out)
    return dict(zip(COLS, out))


def test_regions_disjoint_aligned_and_summed(lib):
    msg = ctypes.create_string_buffer(256)
    for R in range(4, 801):
        assert lib.sdl_check(R, 2 * R - 4, msg, 256) == 0, msg.value.decode()
    for R in (4, 17, 96, 192, 193, 300, 800):                    # face counts that are not those of a closed mesh over the rays
        for F in (4, 5, 100, 333, 1596, 4000):
            assert lib.sdl_check(R, F, msg, 256) == 0, msg.value.decode()


@pytest.mark.parametrize("row", TOTALS, ids=lambda r: "rays%d" % r[0])
def test_totals_are_those_of_the_hand_written_formulas(lib, row):
    R, F = row[:2]
    assert F == 2 * R - 4
    assert _totals(lib, R, F) == dict(zip(COLS, row[2:]))


def test_branches_switch_where_recorded(lib):
    t = {R: _totals(lib, R, 2 * R - 4) for R in range(4, 801)}
    first = lambda col, val: min(R for R in t if t[R][col] == val)
    assert first("refined_twice", 0) == 172 and first("refined_once", 0) == 228
    assert first("optin3", 1) == 252 and t[252]["lds3"] > 65536 >= t[251]["lds3"]
    assert first("split3", 0) == 299 and first("split4", 0) == 297
    assert first("lds_rows", 0) == 300
    assert first("rejected", 1) == 775 and t[776]["lds3"] <= 150 * 1024 < t[777]["lds3"]
    for R in range(5, 801):                                      # each switch happens once
        for col in ("refined_once", "refined_twice", "split3", "split4"):
            assert t[R][col] <= t[R - 1][col]
        for col in ("optin3", "rejected"):
            assert t[R][col] >= t[R - 1][col]
    # the bounds-only forms are smaller than the full one wherever the driver launches them (workspace smaller than the full one)
    for R in t:
        if t[R]["ws3_small"] < t[R]["ws3"]:
            assert t[R]["lds3_lean"] < t[R]["lds3_small"] < t[R]["lds3"]
