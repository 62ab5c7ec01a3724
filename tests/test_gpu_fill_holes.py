"""GPU: fill_label_holes and calculate_extents on device input (csrc/fill_holes.hip) against the host functions of stardist_amd.utils,
exactly (np.array_equal), on the scenes of tests/_fill_cases.py; sd_label_boxes_device against scipy.ndimage.find_objects; the calling
forms, the id policy and the C ABI's argument checks.

Not as the issue words it: "a volume with Z = 1 equals the 2D result" holds for the library call (Z = 1 is how a 2D image is passed);
a (1, Y, X) array given to the Python function is a volume, and the host function -- the reference of every test here -- fills nothing
in it, because along z every pixel touches the outside.  Both are pinned in test_one_plane_volume."""
import ctypes

import numpy as np
import pytest
from scipy import ndimage

import _fill_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = [2 ** 31 - 1] * 3 + [0] * 3


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def fill(a, **kw):
    from stardist_amd.utils import fill_label_holes
    return fill_label_holes(a, **kw)


def device_fill(torch, a):
    """the device result of a numpy scene, through a tensor, back as numpy"""
    t = torch.as_tensor(a, device="cuda")
    keep = t.clone()
    got = fill(t)
    assert got.is_cuda and got.dtype == t.dtype and got.shape == t.shape and got.data_ptr() != t.data_ptr()
    assert torch.equal(t, keep)                                             # the input is not written
    return got.cpu().numpy()


SCENES = C.all_int32_scenes()
GROUPS = {
    "random": [n for n in SCENES if n.startswith("random_")],
    "hand_2d": list(C.hand_2d()),
    "word_boundaries": list(C.word_boundary_cases()),
    "volumes": list(C.volumes()),
    "many_objects": ["many_objects"],
}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_scenes_equal_host_function(torch, group):
    assert len(GROUPS[group]) >= 1
    for name in GROUPS[group]:
        a = SCENES[name]
        assert np.array_equal(device_fill(torch, a), C.expected(name, a)), name


def test_scenes_cover_what_the_issue_lists():
    assert len(GROUPS["random"]) == 40 and any(1 in SCENES[n].shape for n in GROUPS["random"])
    assert sum(SCENES[n].ndim == 3 for n in GROUPS["random"]) == 16 and any((SCENES[n] < 0).any() for n in GROUPS["random"])
    assert len([n for n in GROUPS["hand_2d"] if n.startswith("concentric_")]) == 6
    assert len(GROUPS["word_boundaries"]) == 4 * len(C.WORD_WIDTHS)
    assert len(np.unique(SCENES["many_objects"])) > 5500


@pytest.mark.parametrize("opened", (False, True))
def test_box_beyond_the_lds_budget(torch, opened):
    a = C.budget_scene(opened)
    box = ndimage.find_objects(a)[59]
    assert 2 * (box[0].stop - box[0].start) * -(-(box[1].stop - box[1].start) // 32) > C.FH_LDS_WORDS
    want = C.expected("budget_%d" % opened, a)
    assert (int((want != a).sum()) > 100000) != opened
    assert np.array_equal(device_fill(torch, a), want)


def test_one_plane_volume(torch):
    from stardist_amd.lib import _native as N
    a = C.hand_2d()["concentric_259"]
    want2d = C.expected("concentric_259", a)
    assert not np.array_equal(want2d, a)
    vol = a[None]
    assert np.array_equal(fill(vol), vol)                                   # the host function: nothing is a hole in a one-plane volume
    assert np.array_equal(device_fill(torch, vol), vol)
    assert np.array_equal(device_fill(torch, np.ascontiguousarray(a[:, None])), a[:, None])
    t = torch.as_tensor(a, device="cuda")
    out = torch.empty_like(t)
    N.dcall(t, "sd_fill_label_holes_device", ctypes.c_void_p(t.data_ptr()), 1, a.shape[0], a.shape[1], int(a.max()),
            ctypes.c_void_p(out.data_ptr()))
    assert np.array_equal(out.cpu().numpy(), want2d)                        # the library call: Z = 1 is the 2D image


def test_ids_dense_table_and_compaction(torch):
    a = C.hand_2d()["larger_id_kept"].copy()
    a[a == 7] = 1000000                                                     # 25 pixels: 1 000 000 > 4 * size + 1024, compacted
    assert np.array_equal(device_fill(torch, a), fill(a))
    big = np.zeros((600, 500), np.int32)                                    # 4 * 300 000 + 1024 > 1 000 000: the dense table
    big[10:15, 10:15] = 1
    big[12, 12] = 0
    big[100:109, 100:109] = 1000000
    big[102:107, 102:107] = 0
    big[104, 104] = 1
    got = device_fill(torch, big)
    assert np.array_equal(got, fill(big)) and got[12, 12] == 1 and got[104, 104] == 1000000
    # ids beyond int32: scipy's find_objects allocates one entry per id up to the largest, so the host function cannot take them; the
    # reference is the host result on the small ids, renamed in the same ascending order (2 < 5 < 9 -> 7 < 2^31 + 11 < 2^40 + 3)
    small = C.hand_2d()["concentric_592"]
    rename = np.zeros(10, np.int64)
    rename[[2, 5, 9]] = [7, 2 ** 31 + 11, 2 ** 40 + 3]
    h, want = rename[small], rename[C.expected("concentric_592", small)]
    assert h.dtype == np.int64 and h.max() == 2 ** 40 + 3 and not np.array_equal(want, h)
    got = fill(torch.as_tensor(h, device="cuda"))
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    got = fill(h, device="cuda")
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want)


def test_calling_forms(torch):
    a = SCENES["random_01"]
    want = C.expected("random_01", a)
    for dt in (torch.int32, torch.int64):
        t = torch.as_tensor(a, device="cuda").to(dt)
        got = fill(t)
        assert got.device == t.device and got.dtype == dt and np.array_equal(got.cpu().numpy(), want)
    for dt in (np.int32, np.uint16, np.int64):
        x = np.abs(a).astype(dt)
        got = fill(x, device="cuda")
        assert isinstance(got, np.ndarray) and got.dtype == dt and np.array_equal(got, fill(x))
    base = torch.as_tensor(np.repeat(np.repeat(a, 2, axis=0), 2, axis=1), device="cuda")
    view = base[::2, ::2]                                                   # a strided view
    assert not view.is_contiguous() and np.array_equal(fill(view).cpu().numpy(), want)
    tr = torch.as_tensor(np.ascontiguousarray(a.T), device="cuda").T        # a transposed view
    assert not tr.is_contiguous() and np.array_equal(fill(tr).cpu().numpy(), want)
    assert np.array_equal(base.cpu().numpy(), np.repeat(np.repeat(a, 2, axis=0), 2, axis=1))
    t = torch.as_tensor(a, device="cuda")
    one, two = fill(t), fill(t)
    assert one.data_ptr() != two.data_ptr() and torch.equal(one, two)
    s = np.ones((3, 3))
    d = C.hand_2d()["diagonal_leak"]
    got = fill(torch.as_tensor(d, device="cuda"), structure=s)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), fill(d, structure=s)) and got[4, 4] == 0
    with pytest.raises(ValueError):
        fill(torch.zeros((2, 3, 4, 5), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        fill(np.zeros(7, np.int32), device="cuda")
    e = fill(torch.zeros((0, 5), dtype=torch.int32, device="cuda"))
    assert e.shape == (0, 5) and e.is_cuda


def boxes_of(torch, a, top):
    from stardist_amd.lib import _native as N
    t = torch.as_tensor(np.ascontiguousarray(a, np.int32), device="cuda")
    boxes = torch.full((top + 1, 6), -5, dtype=torch.int32, device="cuda")
    zyx = ((1,) + a.shape) if a.ndim == 2 else a.shape
    N.dcall(t, "sd_label_boxes_device", ctypes.c_void_p(t.data_ptr()), *zyx, top, ctypes.c_void_p(boxes.data_ptr()))
    return boxes.cpu().numpy()


def test_label_boxes_equal_find_objects(torch):
    for name in GROUPS["random"] + ["many_objects", "words_97_left_open"]:
        a = SCENES[name]
        top = max(int(a.max()), 0) + 3                                      # three ids that are absent for certain
        boxes = boxes_of(torch, a, top)
        found = ndimage.find_objects(np.maximum(a, 0), max_label=top)
        assert boxes[0].tolist() == SENTINEL and all(boxes[k].tolist() == SENTINEL for k in range(top - 2, top + 1))
        for k, sl in enumerate(found, 1):
            if sl is None:
                assert boxes[k].tolist() == SENTINEL, (name, k)
            else:
                sl = ((slice(0, 1),) + sl) if a.ndim == 2 else sl
                assert boxes[k].tolist() == [s.start for s in sl] + [s.stop for s in sl], (name, k)
    wide = np.zeros((3, 300), np.int32)                                     # one run across several 64-column cuts
    wide[1, 7:291] = 2
    assert boxes_of(torch, wide, 2)[2].tolist() == [0, 1, 7, 1, 2, 291]


@pytest.mark.parametrize("func", (np.median, np.mean))
def test_calculate_extents_on_device_input(torch, func):
    from stardist_amd.utils import calculate_extents
    dev = lambda x: torch.as_tensor(x, device="cuda")
    two, three = np.abs(SCENES["random_02"]), np.abs(SCENES["random_30"])
    for a in (two, three, np.zeros((6, 7), np.int32), np.zeros((3, 4, 5), np.int32)):
        want, got = calculate_extents(a, func), calculate_extents(dev(a), func)
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and np.array_equal(got, want)
    crop = lambda v: np.pad(v, [(0, max(0, m - n)) for n, m in zip(v.shape, (10, 12, 14))])[:10, :12, :14]
    stack = np.stack([crop(np.abs(SCENES["random_%02d" % s])) for s in (26, 28, 29)])
    assert stack.shape == (3, 10, 12, 14)
    assert np.array_equal(calculate_extents(dev(stack), func), calculate_extents(stack, func))
    many = [two, np.abs(SCENES["random_04"]), np.zeros((5, 5), np.int32)]
    assert np.array_equal(calculate_extents([dev(x) for x in many], func), calculate_extents(many, func))
    assert np.array_equal(calculate_extents(dev(two.astype(np.int64)), func), calculate_extents(two, func))


def test_bad_arguments(torch):
    from stardist_amd.lib import _native as N
    t = torch.zeros((4, 5), dtype=torch.int32, device="cuda")
    out = torch.zeros_like(t)
    boxes = torch.zeros((3, 6), dtype=torch.int32, device="cuda")
    p, o, b = (ctypes.c_void_p(x.data_ptr()) for x in (t, out, boxes))
    bad = [(None, 1, 4, 5, 2), (p, 0, 4, 5, 2), (p, 1, 0, 5, 2), (p, 1, 4, -1, 2), (p, 1, 4, 5, -1)]
    for name, dst in (("sd_fill_label_holes_device", o), ("sd_label_boxes_device", b)):
        fn = getattr(N.lib(), name)
        for src, Z, Y, X, top in bad:
            assert fn(src, Z, Y, X, top, dst, N.current_stream()) == -1
            assert name[:-len("_device")] in N.lib().sd_last_error().decode()
        assert fn(p, 1, 4, 5, 2, None, N.current_stream()) == -1
        assert fn(p, 1, 4, 5, 2, dst, N.current_stream()) == 0
    torch.cuda.synchronize()
    assert out.abs().sum().item() == 0
