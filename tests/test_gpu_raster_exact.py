"""GPU: what the rasterisers (csrc/raster2d.hip, csrc/raster3d.hip) do around the point test, compared EXACTLY (np.array_equal, no exemption)
with plain references on the cases of _raster_cases.py -- windows (crops of the whole-image reference), the polygon / polyhedron stride loops
behind the block caps, vertex staging beyond 256 rays, the LDS opt-in, and the label rules (last painter wins in 2D, label -1 erases; first
painter wins in 3D, overlap_label from two covers on, a non-zero voxel of the in/out buffer stays or becomes overlap_label, a zero label or
overlap_label takes the sequential path).  2D reference: oracle.port (float64 restatement of scikit-image, pinned by the committed goldens);
3D reference: the compiled reference, and its label rule composed in numpy where its wrapper cannot be asked (test_cpu_raster_cases.py
proves the composition).  Every buffer that the package allocates with torch.empty starts as -7: a pixel that no kernel writes shows up."""
import contextlib

import numpy as np
import pytest
import torch

import _raster_cases as RC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
K = RC.source_constants()


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


@contextlib.contextmanager
def dirty_empty():
    """torch.empty gives integer tensors full of -7 while the package allocates"""
    empty = torch.empty

    def dirty(*a, **k):
        t = empty(*a, **k)
        return t if t.is_floating_point() else t.fill_(-7)
    torch.empty = dirty
    try:
        yield
    finally:
        torch.empty = empty


def _same(got, want, tag):
    assert got.dtype == np.int32 and np.array_equal(got, want), "%s: %s" % (tag, RC.describe(got, want))


# ---- 2D ------------------------------------------------------------------------------------------------------------------------------------
def _paint2d(coord, labels, shape=RC.SHAPE2, window=None):
    from stardist_amd.lib import stardist2d as sd2
    with dirty_empty():
        out = sd2.c_polygons_to_label(_t(coord, np.float32), _t(labels, np.int32), shape, window=window)
    assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == tuple(shape if window is None else window[1])
    return out.cpu().numpy()


def test_windows2d_whole_image():
    coord, labels = RC.windows2d_scene()
    _same(_paint2d(coord, labels), RC.windows2d_want(), "whole image")


@pytest.mark.parametrize("name", [n for n, _ in RC.WINDOWS2D])
def test_windows2d_equal_the_crop(name):
    coord, labels = RC.windows2d_scene()
    win = dict(RC.WINDOWS2D)[name]
    got = _paint2d(coord, labels, window=win)
    _same(got, RC.crop(RC.windows2d_want(), win), name)
    if name == "empty":
        assert not got.any()


@pytest.mark.parametrize("name", ("stars32", "stars8_small", "stars64_big", "stars5_int"))
def test_windows2d_of_the_skimage_goldens(name):
    """the committed images of the real scikit-image, through windows"""
    coord, labels, shape, gold = RC.golden2d(name)
    for win in RC.golden_windows(shape):
        _same(_paint2d(coord, labels, shape, window=win), RC.crop(gold, win), "%s %s" % (name, win))


def test_windows2d_outside_the_image_raise():
    from stardist_amd.lib import _native as N
    coord, labels = RC.windows2d_scene()
    for win in RC.BAD_WINDOWS2D:
        with pytest.raises(N.NativeError, match="window outside the image"):
            _paint2d(coord, labels, window=win)
    _same(_paint2d(coord, labels), RC.windows2d_want(), "after the refusals")


def test_windows2d_without_polygons_are_zero():
    from stardist_amd.lib import stardist2d as sd2
    for win in (((7, 11), (23, 31)), ((0, 0), RC.SHAPE2), ((63, 79), (1, 1))):
        stale = torch.full(win[1], 12345, dtype=torch.int32, device=DEV)            # the wrapper's torch.empty may get this block back
        del stale
        out = sd2.c_polygons_to_label(torch.zeros((0, 2, 32), dtype=torch.float32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), RC.SHAPE2, window=win)
        assert tuple(out.shape) == win[1] and out.dtype == torch.int32 and not out.any().item()
        with dirty_empty():
            out = sd2.c_polygons_to_label(torch.zeros((0, 2, 32), dtype=torch.float32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), RC.SHAPE2, window=win)
        assert not out.any().item()


@pytest.mark.parametrize("order", ("given", "reversed"))
@pytest.mark.parametrize("name", ("perm", "dup", "neg_mid", "neg_last"))
def test_labels2d_last_painter_wins(name, order):
    """400 polygons on the same 20 x 20 pixels: the block that comes last in the ORDER wins whenever it runs; label -1 paints 0"""
    coord, labs = RC.stack2d()
    masks, labels = RC.stack2d_masks(), labs[name]
    if order == "reversed":
        coord, masks, labels = coord[::-1], masks[::-1], labels[::-1]
    want = RC.paint2d(masks, labels)
    _same(_paint2d(coord, labels), want, name)
    win = ((RC.STACK2[0][0] + 3, RC.STACK2[0][1] - 2), (11, 17))
    _same(_paint2d(coord, labels, window=win), RC.crop(want, win), name + " window")


@pytest.mark.parametrize("R", RC.RAYS2D + (K["rays2d"],))
def test_rays2d_staging(R):
    coord, labels = RC.rays2d_case(R)
    want = RC.rays2d_want(R)
    _same(_paint2d(coord, labels), want, "R=%d" % R)
    win = ((9, 14), (37, 41))
    _same(_paint2d(coord, labels, window=win), RC.crop(want, win), "R=%d window" % R)


def test_rays2d_beyond_the_limit_raise():
    from stardist_amd.lib import _native as N
    R = K["rays2d"] + 1
    rs = np.random.RandomState(1)
    coord = RC.star_coord(rs, np.array([[30.2, 40.4]]), np.array([12.0]), R)
    with pytest.raises(N.NativeError, match="n_rays=%d too large" % R):
        _paint2d(coord, np.zeros(1, np.int32))


def test_loop2d_polygons_beyond_the_block_cap():
    """cap + 3000 triangles with labels arange(n): the pixels whose last painter has an index at or beyond the cap show it"""
    base, assign, want = RC.loop2d_case()
    n = len(assign)
    assert n > K["cap2d"] and (want > K["cap2d"]).any()
    got = _paint2d(base[assign], np.arange(n, dtype=np.int32))
    _same(got, want, "%d triangles" % n)


# ---- 3D ------------------------------------------------------------------------------------------------------------------------------------
def _paint3d(dist, points, rays, labels, mode, shape, overlap=None, window=None):
    from stardist_amd.lib import stardist3d as sd3
    V, F = RC.rays(rays)
    out = sd3.c_polyhedron_to_label(_t(dist, np.float32), _t(points, np.float32), _t(V, np.float32), _t(F, np.int32), _t(labels, np.int32), mode, 0,
                                    int(overlap is not None), int(0 if overlap is None else overlap), shape, window=window)
    assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == tuple(shape if window is None else window[1])
    return out.cpu().numpy()


def _paint3d_into(buf, dist, points, rays, labels, mode, overlap=None):
    """_LIB_polyhedron_to_label, the reference's C ABI on host pointers: paints into the caller's buffer as it is"""
    from stardist_amd.lib import _native as N
    V, F = RC.rays(rays)
    a = np.ascontiguousarray
    dist, points, labels = a(dist, np.float32), a(points, np.float32), a(labels, np.int32)
    assert buf.dtype == np.int32 and buf.flags["C_CONTIGUOUS"]
    N.require_device()
    N.lib()._LIB_polyhedron_to_label(N.ptr(dist), N.ptr(points), N.ptr(V), N.ptr(F), len(dist), dist.shape[1], len(F), N.ptr(labels), *buf.shape, int(mode), 0,
                                     int(overlap is not None), int(0 if overlap is None else overlap), N.ptr(buf))
    return buf


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("name", [n for n, _ in RC.WINDOWS3D])
def test_windows3d_equal_the_crop(refmods, name, mode):
    d, p, labels, _ = RC.windows3d_scene()
    win = dict(RC.WINDOWS3D)[name]
    got = _paint3d(d, p, "golden32", labels, mode, RC.SHAPE3, window=win)
    _same(got, RC.crop(RC.windows3d_want(refmods, mode), win), "%s mode %d" % (name, mode))
    if name == "empty":
        assert not got.any()


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_windows3d_whole_volume(refmods, mode):
    """no window argument, and the host-array route: the whole volume, polyhedra wholly below the volume included"""
    from stardist_amd.lib import stardist3d as sd3
    d, p, labels, _ = RC.windows3d_scene()
    want = RC.windows3d_want(refmods, mode)
    _same(_paint3d(d, p, "golden32", labels, mode, RC.SHAPE3), want, "device, mode %d" % mode)
    V, F = RC.rays("golden32")
    if mode != 2:
        _same(sd3.c_polyhedron_to_label(d, p, V, F, labels, mode, 0, 0, 0, RC.SHAPE3), want, "host, mode %d" % mode)


def test_windows3d_outside_the_volume_raise(refmods):
    from stardist_amd.lib import _native as N
    d, p, labels, _ = RC.windows3d_scene()
    for win in RC.BAD_WINDOWS3D:
        with pytest.raises(N.NativeError, match="window outside the volume"):
            _paint3d(d, p, "golden32", labels, 1, RC.SHAPE3, window=win)
    win = dict(RC.WINDOWS3D)["interior-a"]
    _same(_paint3d(d, p, "golden32", labels, 1, RC.SHAPE3, window=win), RC.crop(RC.windows3d_want(refmods, 1), win), "after the refusals")


@pytest.mark.parametrize("name", [n for n, _ in RC.FAR_WINDOWS] + ["whole"])
def test_far3d_beyond_8192(refmods, name):
    """centres and vertices beyond 8192: the cone map's unsafe path, window-relative stores far from the origin"""
    d, p, labels = RC.far3d_scene()
    want = RC.far3d_want(refmods)
    win = dict(RC.FAR_WINDOWS).get(name)
    got = _paint3d(d, p, "golden32", labels, 0, RC.FAR_SHAPE, window=win)
    _same(got, want if win is None else RC.crop(want, win), name)
    assert got.any()


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("ov", RC.OVERLAPS)
@pytest.mark.parametrize("name", ("perm", "dup", "neg"))
def test_labels3d_first_painter_and_overlap(refmods, name, ov, mode):
    d, p, labs = RC.labels3d_scene()
    o = RC.overlap_value(ov, labs[name])
    want = RC.ref3d(refmods, d, p, *RC.rays("golden32"), labs[name], mode, RC.SHAPE3L, overlap=o)
    _same(_paint3d(d, p, "golden32", labs[name], mode, RC.SHAPE3L, overlap=o), want, "%s overlap %s mode %d" % (name, o, mode))
    _same(_paint3d(d[::-1], p[::-1], "golden32", labs[name][::-1], mode, RC.SHAPE3L, overlap=o),
          RC.compose3d(RC.labels3d_masks(refmods, mode)[::-1], labs[name][::-1], o, np.zeros(RC.SHAPE3L, np.int32)), "%s reversed" % name)


@pytest.mark.parametrize("name,ov,mode", [("perm", None, 0), ("perm", 77, 0), ("dup", "label", 0), ("neg", -5, 0), ("perm", None, 1), ("dup", 77, 1),
                                          ("zero_mid", None, 0), ("perm", 0, 0)])
def test_labels3d_into_a_prefilled_buffer(refmods, name, ov, mode):
    """a voxel that is non-zero before the call keeps its value, or becomes overlap_label (:1511-1517)"""
    d, p, labs = RC.labels3d_scene()
    o = RC.overlap_value(ov, labs[name])
    pre = RC.prefill3d()
    want = RC.compose3d(RC.labels3d_masks(refmods, mode), labs[name], o, pre)
    got = _paint3d_into(pre.copy(), d, p, "golden32", labs[name], mode, overlap=o)
    _same(got, want, "%s overlap %s mode %d" % (name, o, mode))
    assert not np.array_equal(got, pre)


@pytest.mark.parametrize("name,ov,mode", [("zero_first", None, 0), ("zero_first", 9, 0), ("zero_mid", None, 0), ("zero_mid", 9, 0), ("zero_last", None, 0),
                                          ("zero_last", 9, 0), ("zero_mid", -5, 1), ("perm", 0, 0), ("dup", 0, 0), ("neg", 0, 1), ("zero_mid", 0, 0)])
def test_labels3d_zero_labels_take_the_sequential_path(refmods, name, ov, mode):
    """a label of 0 leaves its voxels open for later polyhedra, an overlap_label of 0 re-opens covered ones: polyhedron by polyhedron"""
    d, p, labs = RC.labels3d_scene()
    want = RC.compose3d(RC.labels3d_masks(refmods, mode), labs[name], ov, np.zeros(RC.SHAPE3L, np.int32))
    _same(_paint3d(d, p, "golden32", labs[name], mode, RC.SHAPE3L, overlap=ov), want, "%s overlap %s mode %d" % (name, ov, mode))
    win = ((5, 7, 9), (19, 17, 23))
    _same(_paint3d(d, p, "golden32", labs[name], mode, RC.SHAPE3L, overlap=ov, window=win), RC.crop(want, win), "%s window" % name)


@pytest.mark.parametrize("R,mode", RC.RAYS3D)
def test_rays3d_staging_and_lds(refmods, R, mode):
    d, p, labels = RC.rays3d_case(R)
    want = RC.rays3d_want(refmods, R, mode)
    _same(_paint3d(d, p, "golden%d" % R, labels, mode, RC.SHAPE3R), want, "R=%d mode %d" % (R, mode))
    win = ((3, 11, 6), (31, 23, 29))
    _same(_paint3d(d, p, "golden%d" % R, labels, mode, RC.SHAPE3R, window=win), RC.crop(want, win), "R=%d mode %d window" % (R, mode))


@pytest.mark.parametrize("R,mode,text", [(K["hull_rays"] + 1, 0, "hull_planes: n_rays=%d unsupported" % (K["hull_rays"] + 1)),
                                         (RC.OVER_LIMIT_RAYS, 1, "too large for LDS staging")])
def test_rays3d_beyond_the_limits_raise(refmods, R, mode, text):
    from stardist_amd.lib import _native as N
    rs = np.random.RandomState(R)
    d, p = RC.polys3d(rs, rs.uniform(10, 30, (2, 3)), rs.uniform(6, 9, 2), R)
    with pytest.raises(N.NativeError, match=text):
        _paint3d(d, p, "golden%d" % R, np.array([1, 2], np.int32), mode, RC.SHAPE3R)
    dd, pp, labels = RC.rays3d_case(257)
    _same(_paint3d(dd, pp, "golden257", labels, 1, RC.SHAPE3R), RC.rays3d_want(refmods, 257, 1), "after the refusal")


@pytest.mark.parametrize("mode", (0, 1))
def test_loop3d_polyhedra_beyond_the_block_cap(refmods, mode):
    """cap + 600 polyhedra with labels 1 .. n: the voxels whose first painter has an index at or beyond the cap show it"""
    d, p, labels = RC.loop3d_case()
    want = RC.loop3d_want(refmods, mode)
    assert len(d) > K["cap3d"] and (want > K["cap3d"]).any()
    _same(_paint3d(d, p, "octo1", labels, mode, RC.SHAPE3R), want, "%d polyhedra, mode %d" % (len(d), mode))
