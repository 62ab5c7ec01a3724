"""CPU: the bit-plane arithmetic of the device fill_label_holes (csrc/fill_holes.h through tests/host/fill_holes_check.cpp: boxes, planes,
passes to the fixpoint, max rule) against the host function stardist_amd.utils.fill_label_holes, exactly, on the scenes of
tests/_fill_cases.py; the box-free statement the kernels implement against the host function; and the routing of host input."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import _fill_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i = ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fillholes") / "libfillholes.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host", "fill_holes_check.cpp"), "-o", so],
                   check=True)
    l = ctypes.CDLL(so)
    l.fh_lds_words.restype = _i
    l.fh_boxes.restype = _i
    l.fh_boxes.argtypes = [_vp, _i, _i, _i, _i, _vp]
    l.fh_fill.restype = _i
    l.fh_fill.argtypes = [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]
    l.fh_fill_row.restype = _i
    l.fh_fill_row.argtypes = [_vp, _vp, _i]
    return l


def zyx(a, fill=False):
    """the extents as the library takes them: Z = 1 says "a 2D image"; to fill one plane given as a volume (where, as in the host
    function, every pixel lies on the outer layer along z and nothing is a hole) it goes in as (Y, 1, X), as stardist_amd.utils does"""
    if a.ndim == 2:
        return (1,) + a.shape
    return (a.shape[1], 1, a.shape[2]) if (fill and a.shape[0] == 1) else a.shape


def harness_fill(lib, a, max_label=None):
    """(filled image, rounds of the slowest object, objects within the LDS budget, objects beyond it)"""
    a = np.ascontiguousarray(a, np.int32)
    out = np.full(a.shape, -7, np.int32)
    info = (ctypes.c_int * 3)()
    rc = lib.fh_fill(a.ctypes.data, *zyx(a, fill=True), max(int(a.max()), 0) if max_label is None else max_label, out.ctypes.data,
                     ctypes.addressof(info), ctypes.addressof(info) + 4, ctypes.addressof(info) + 8)
    assert rc == 0
    return out, info[0], info[1], info[2]


def statement_fill(a):
    """the box-free statement of csrc/fill_holes.h, with scipy's labelling: out = max(lbl, 0); per label L, the components of
    (lbl != L) on bbox(L) (cross structure) that hold no pixel of the box's outermost layer get max(out, L)"""
    out = np.maximum(a, 0)
    for k, box in enumerate(ndimage.find_objects(np.maximum(a, 0)), 1):
        if box is None:
            continue
        free = a[box] != k
        comp, n = ndimage.label(free)
        outer = np.zeros(free.shape, bool)
        for ax in range(free.ndim):
            sl = [slice(None)] * free.ndim
            sl[ax] = 0
            outer[tuple(sl)] = True
            sl[ax] = -1
            outer[tuple(sl)] = True
        open_ids = np.unique(comp[outer & free])
        hole = free & ~np.isin(comp, open_ids)
        view = out[box]
        view[hole] = np.maximum(view[hole], k)
    return out


def test_budget_constant_is_the_header_s(lib):
    txt = open(os.path.join(ROOT, "stardist_amd", "csrc", "fill_holes.h")).read()
    found = re.findall(r"\bFH_LDS_WORDS\s*=\s*(\d+)", txt)
    assert found == [str(C.FH_LDS_WORDS)]
    assert lib.fh_lds_words() == C.FH_LDS_WORDS
    assert re.findall(r"\bFH_WAVE_WORDS\s*=\s*(\d+)", txt) == [str(C.FH_WAVE_WORDS)]


def test_every_tier_of_the_kernel_has_scenes():
    """planes within FH_WAVE_WORDS, within FH_LDS_WORDS and beyond: each in 2D, the first two in 3D too"""
    def tiers(a):
        got = set()
        for box in ndimage.find_objects(np.maximum(a, 0)):
            if box is not None and min(s.stop - s.start for s in box[-2:]) >= 3:
                ext = [s.stop - s.start for s in box]
                words = 2 * int(np.prod(ext[:-1])) * -(-ext[-1] // 32)
                got.add(0 if words <= C.FH_WAVE_WORDS else (1 if words <= C.FH_LDS_WORDS else 2))
        return got
    S = C.all_int32_scenes()
    assert tiers(S["ring_200"]) == {0, 1} and tiers(C.budget_scene(False)) == {0, 2}
    in3d = set().union(*[tiers(a) for a in S.values() if a.ndim == 3])
    assert in3d == {0, 1}


def test_statement_equals_host_function_on_random_scenes():
    changed = 0
    for s in range(C.N_RANDOM):
        a = C.random_scene(s)
        want = C.expected("random_%02d" % s, a)
        assert np.array_equal(statement_fill(a), want), s
        changed += int((want != np.maximum(a, 0)).sum())
    assert changed > 500                                                    # the scenes do have holes


def test_harness_equals_host_function(lib):
    for name, a in C.all_int32_scenes().items():
        got = harness_fill(lib, a)[0]
        assert np.array_equal(got, C.expected(name, a)), name


def test_scenes_are_what_they_say(lib):
    S = C.all_int32_scenes()
    same = lambda n: np.array_equal(C.expected(n, S[n]), np.maximum(S[n], 0))
    for side in range(4):
        assert same("cavity_reaches_border_%d" % side)
    assert not same("ring_on_border_closed") and (C.expected("ring_on_border_closed", S["ring_on_border_closed"])[1:5, 5:8] == 6).all()
    assert C.expected("smaller_id_erased", S["smaller_id_erased"])[2].tolist() == [0, 5, 5, 5, 5, 5, 0]
    assert C.expected("larger_id_kept", S["larger_id_kept"])[2].tolist() == [0, 1, 7, 1, 0]
    assert C.expected("diagonal_leak", S["diagonal_leak"])[4, 4] == 8
    assert same("spiral_open") and not same("spiral_closed")
    assert (C.expected("spiral_closed", S["spiral_closed"])[3:67, 5:69] == 4).all()
    assert harness_fill(lib, S["spiral_open"])[1] >= 12                     # one round cannot walk the corridor
    for w in C.WORD_WIDTHS:
        for leak in ("left", "right"):
            assert same("words_%d_%s_open" % (w, leak)) and not same("words_%d_%s_closed" % (w, leak))
    assert not same("shell_closed") and same("torus") and same("shell_pinhole") and not same("shell_diagonal_leak")
    assert all(same(n) for n in S if n.startswith("shell_cut_"))
    m = S["many_objects"]
    assert len(np.unique(m)) > 5500 and not same("many_objects")


def test_budget_scenes_take_the_global_planes(lib):
    for opened in (False, True):
        a = C.budget_scene(opened)
        got, _, n_lds, n_big = harness_fill(lib, a)
        box = ndimage.find_objects(a)[59]
        words = 2 * (box[0].stop - box[0].start) * -(-(box[1].stop - box[1].start) // 32)
        assert C.FH_LDS_WORDS < words < 1.1 * C.FH_LDS_WORDS
        assert n_big == 1 and n_lds == len(np.unique(a)) - 2 >= 20
        want = C.expected("budget_%d" % opened, a)
        assert np.array_equal(got, want)
        assert (int((want != a).sum()) > 100000) != opened


def test_harness_boxes_equal_find_objects(lib):
    for s in range(C.N_RANDOM):
        a = C.random_scene(s)
        top = max(int(a.max()), 0) + 3
        boxes = np.empty((top + 1, 6), np.int32)
        assert lib.fh_boxes(a.ctypes.data, *zyx(a), top, boxes.ctypes.data) == 0
        found = ndimage.find_objects(np.maximum(a, 0), max_label=top)
        assert boxes[0].tolist() == [2 ** 31 - 1] * 3 + [0] * 3
        for k, sl in enumerate(found, 1):
            if sl is None:
                assert boxes[k].tolist() == [2 ** 31 - 1] * 3 + [0] * 3
            else:
                sl = ((slice(0, 1),) + sl) if a.ndim == 2 else sl
                assert boxes[k].tolist() == [s_.start for s_ in sl] + [s_.stop for s_ in sl]


def test_row_pass_carries_across_words(lib):
    """random rows of 1 to 4 words: every run of free bits that holds a seed becomes reach, nothing else"""
    rng = np.random.default_rng(5)
    for _ in range(400):
        wx = int(rng.integers(1, 5))
        bits = rng.random(32 * wx) < rng.choice([0.5, 0.9, 0.98])
        seed = bits & (rng.random(32 * wx) < 0.03)
        want = np.zeros_like(bits)
        runs, _n = ndimage.label(bits)
        want[np.isin(runs, np.unique(runs[seed]))] = True
        want &= bits
        pack = lambda b: np.packbits(b.reshape(wx, 32), axis=1, bitorder="little").view("<u4").ravel().copy()
        fr, rc = pack(bits), pack(seed)
        changed = lib.fh_fill_row(rc.ctypes.data, fr.ctypes.data, wx)
        assert np.array_equal(rc, pack(want))
        assert bool(changed) == (not np.array_equal(want, seed))
    ones = np.full(4, 0xffffffff, np.uint32)                                # one run across four words, seeded at either end
    for at in (0, 127):
        rc = np.zeros(4, np.uint32)
        rc[at // 32] = np.uint32(1) << np.uint32(at % 32)
        lib.fh_fill_row(rc.ctypes.data, ones.ctypes.data, 4)
        assert np.array_equal(rc, ones)


def test_labels_beyond_max_label_are_background(lib):
    a = C.hand_2d()["larger_id_kept"]
    got = harness_fill(lib, a, max_label=1)[0]
    assert got[2].tolist() == [0, 1, 1, 1, 0]
    assert lib.fh_fill(None, 1, 2, 2, 1, None, None, None, None) == -1


def test_host_input_takes_the_host_code(monkeypatch):
    """numpy in without device=: scipy's calls as before, no native code, kwargs passed on"""
    from stardist_amd import label_ops, utils
    monkeypatch.setattr(label_ops, "_fill_label_holes_device", lambda *a, **k: pytest.fail("device path taken"))
    a = C.hand_2d()["diagonal_leak"]
    got = utils.fill_label_holes(a)
    assert isinstance(got, np.ndarray) and got.dtype == a.dtype and got[4, 4] == 8
    assert utils.fill_label_holes(a, structure=np.ones((3, 3)))[4, 4] == 0
    assert utils.fill_label_holes(a, device=None)[4, 4] == 8
    assert np.array_equal(utils.fill_label_holes(a.astype(np.uint16)), got.astype(np.uint16))
    assert utils.calculate_extents(a).tolist() == [5.0, 5.0]
