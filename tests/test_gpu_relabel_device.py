"""GPU: `relabel_image_stardist` / `relabel_image_stardist3D` on label images that are device tensors (csrc/relabel_star.hip: per-object
centroid sums in one pass, star distances at the centroids only), against the host path of the same functions on the same arrays,
exactly: the sums against np.bincount, the star representation against `_region_centroids` and the dense star_dist / star_dist3D of this
package, the results against the host function's and against tests/golden/relabel_reference.npz (under that file's rules, as in
tests/test_gpu_relabel.py).  The host entry of the 3D rasteriser uploads and runs the kernels of the tensor path, so the 3D results are
compared voxel for voxel without exemption.  Scenes: tests/_relabel_cases.py."""
import ctypes
import os

import numpy as np
import pytest

import _relabel_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "relabel_reference.npz"))


def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.array(a, dtype=dtype, order="C"), device="cuda")          # a copy: the scenes are read-only


def sums_device(lbl, top):
    import torch
    from stardist_amd.lib import _native as N
    t = _dev(lbl, np.int32)
    out = torch.full((top + 1, 4), -3, dtype=torch.int64, device="cuda")
    Z, Y, X = ((1,) + lbl.shape) if lbl.ndim == 2 else lbl.shape
    N.dcall(t, "sd_label_centroid_sums_device", N.tptr(t), Z, Y, X, top, N.tptr(out))
    return out.cpu().numpy()


# ---- centroid sums -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["multi2d", "one_pixel_image", "multi3d", "wide", "full_image", "last_pixel"])
def test_centroid_sums_equal_bincount(name):
    lbl = C.centroid_scenes()[name]
    top = int(lbl.max())
    want = C.centroid_sums_np(lbl, top)
    got = sums_device(lbl, top)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(sums_device(lbl, top), got)                      # the same bits from call to call
    if name == "last_pixel":
        assert np.flatnonzero(got[:, 0]).tolist() == [top] and got[top].tolist() == [1, 0, 60, 129]
    if name == "wide":
        assert got[2, 3] > 2 ** 32


def test_centroid_sums_max_label_bounds_the_objects():
    """labels beyond max_label and negative values are background; a larger max_label leaves the extra slots 0"""
    lbl = C.multi2d().copy()
    lbl[0, 0] = -4
    assert np.array_equal(sums_device(lbl, 40), C.centroid_sums_np(lbl, 40))
    assert np.array_equal(sums_device(lbl, 500), C.centroid_sums_np(lbl, 500))
    assert sums_device(lbl, 0).tolist() == [[0, 0, 0, 0]]
    from stardist_amd.lib import _native as N
    t = _dev(lbl)
    assert N.lib().sd_label_centroid_sums_device(N.tptr(t), 1, 61, 130, 5, None, None) == -1
    assert N.lib().sd_label_centroid_sums_device(N.tptr(t), 1, 0, 130, 5, N.tptr(t), None) == -1
    assert N.lib().sd_label_centroid_sums_device(N.tptr(t), 1, 61, 130, -1, N.tptr(t), None) == -1


# ---- point rows: the kernels against the host march and the dense entry points --------------------------------------------------------
def test_point_kernels_equal_host_rows_and_dense_rows():
    import torch
    from stardist_amd.lib import _native as N
    from stardist_amd.lib.stardist2d import c_star_dist
    from stardist_amd.lib.stardist3d import c_star_dist3d
    lbl = C.multi2d()
    pts = C.probe_points(lbl)
    t, p = _dev(lbl), _dev(pts)
    for R in (17, 32):
        d = torch.full((len(pts), R), -5.0, device="cuda")
        N.dcall(t, "sd_star_dist2d_points_device", N.tptr(t), 61, 130, N.tptr(p), len(pts), R, N.tptr(d))
        h = np.full((len(pts), R), -5, np.float32)
        assert N.lib().sd_star_dist2d_points_host(N.ptr(lbl), 61, 130, N.ptr(pts), len(pts), R, N.ptr(h)) == 0
        dense = c_star_dist(lbl, R, 1, 1)[tuple(pts.T)]
        assert np.array_equal(d.cpu().numpy(), dense) and np.array_equal(h, dense)
    vol, rays = C.multi3d(), C.rays3d()
    pts = C.probe_points(vol)
    t, p = _dev(vol), _dev(pts)
    dz, dy, dx = (np.ascontiguousarray(v, np.float32) for v in rays.vertices.T)
    tz, ty, tx = _dev(dz), _dev(dy), _dev(dx)
    dense = c_star_dist3d(vol, dz, dy, dx, len(rays), 1, 1, 1)[tuple(pts.T)]
    for floor in (0.0, 1e-3):
        d = torch.full((len(pts), len(rays)), -5.0, device="cuda")
        N.dcall(t, "sd_star_dist3d_points_device", N.tptr(t), 20, 37, 45, N.tptr(p), len(pts), N.tptr(tz), N.tptr(ty), N.tptr(tx), len(rays),
                ctypes.c_float(floor), N.tptr(d))
        h = np.full((len(pts), len(rays)), -5, np.float32)
        assert N.lib().sd_star_dist3d_points_host(N.ptr(vol), 20, 37, 45, N.ptr(pts), len(pts), N.ptr(dz), N.ptr(dy), N.ptr(dx), len(rays),
                                                  ctypes.c_float(floor), N.ptr(h)) == 0
        want = np.maximum(dense, np.float32(floor))
        assert np.array_equal(d.cpu().numpy(), want) and np.array_equal(h, want)


def test_point_kernels_refuse_points_outside_and_take_no_points():
    import torch
    from stardist_amd.lib import _native as N
    lbl = C.multi2d()
    t = _dev(lbl)
    d = torch.full((2, 8), -5.0, device="cuda")
    s = N.current_stream()
    for bad in ([61, 0], [0, -1], [2 ** 40, 3]):
        p = _dev(np.array([[14, 20], bad], np.int64))
        assert N.lib().sd_star_dist2d_points_device(N.tptr(t), 61, 130, N.tptr(p), 2, 8, N.tptr(d), s) == -1
        assert b"outside" in N.lib().sd_last_error()
        got = d.cpu().numpy()
        assert (got[0] > 0).all() and (got[1] == 0).all()                  # the good row is written, the bad one is zeros
    assert N.lib().sd_star_dist2d_points_device(N.tptr(t), 61, 130, None, 0, 8, None, s) == 0
    vol, rays = C.multi3d(), C.rays3d()
    tv = _dev(vol)
    tz, ty, tx = (_dev(np.ascontiguousarray(v, np.float32)) for v in rays.vertices.T)
    d = torch.full((2, 24), -5.0, device="cuda")
    p = _dev(np.array([[9, 12, 12], [0, 37, 0]], np.int64))
    args = (N.tptr(tz), N.tptr(ty), N.tptr(tx), 24, ctypes.c_float(0.0), N.tptr(d), s)
    assert N.lib().sd_star_dist3d_points_device(N.tptr(tv), 20, 37, 45, N.tptr(p), 2, *args) == -1
    assert N.lib().sd_star_dist3d_points_device(N.tptr(tv), 20, 37, 45, None, 0, *args) == 0


# ---- the star representation ------------------------------------------------------------------------------------------------------------
def _host_representation(lbl, rays):
    from stardist_amd import star_dist, star_dist3D
    from stardist_amd.geometry.geom2d import _region_centroids
    labs, cen = _region_centroids(lbl)
    pts = cen.astype(int)
    if lbl.ndim == 2:
        dist = np.asarray(star_dist(lbl, rays))[tuple(pts.T)]
    else:
        dist = np.maximum(np.asarray(star_dist3D(lbl, rays))[tuple(pts.T)].reshape(len(pts), len(rays)), np.float32(1e-3))
    return labs, pts, dist


@pytest.mark.parametrize("name,n_rays", [(n, 32) for n in sorted(C.scenes2d())] + [("multi2d", 17), ("ell", 17)])
def test_star_representation_2d_equals_host(name, n_rays):
    from stardist_amd.geometry.geom2d import _star_representation_device
    lbl = C.scenes2d()[name]
    labs, pts, dist = _star_representation_device(_dev(lbl), n_rays)
    want = _host_representation(lbl, n_rays)
    assert labs.dtype == pts.dtype == __import__("torch").int64 and dist.dtype == __import__("torch").float32
    assert np.array_equal(labs.cpu().numpy(), want[0]) and np.array_equal(pts.cpu().numpy(), want[1])
    assert dist.cpu().numpy().shape == want[2].shape and np.array_equal(dist.cpu().numpy(), want[2])
    if name == "ell":
        assert (want[2] == 0).all()                                        # the centroid pixel is background
    if name == "ring_disc":
        assert np.array_equal(want[1][0], want[1][1]) and np.array_equal(want[2][0], want[2][1])
    if name == "u16_zero":
        assert (want[2][1] == 0).all() and (want[2][0] > 0).all()
    if name == "u16_pair":
        assert want[2][0, 0] > 50 and want[2][2, n_rays // 2] > 50         # the rays cross the seam between 7 and 65543


def test_star_representation_3d_equals_host():
    from stardist_amd.geometry.geom2d import _star_representation_device
    lbl, rays = C.multi3d(), C.rays3d()
    labs, pts, dist = _star_representation_device(_dev(lbl), rays)
    want = _host_representation(lbl, rays)
    assert np.array_equal(labs.cpu().numpy(), want[0]) and np.array_equal(pts.cpu().numpy(), want[1])
    assert np.array_equal(dist.cpu().numpy(), want[2]) and dist.cpu().numpy().min() >= np.float32(1e-3)
    labs, pts, dist = _star_representation_device(_dev(np.zeros((3, 4, 5), np.int32)), rays)
    assert tuple(labs.shape) == (0,) and tuple(pts.shape) == (0, 3) and tuple(dist.shape) == (0, 24)


# ---- whole functions --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.scenes2d()))
def test_relabel_2d_tensor_in_equals_host_function(name):
    import torch
    from stardist_amd import relabel_image_stardist
    lbl = C.scenes2d()[name]
    t = _dev(lbl)
    before = t.clone()
    out = relabel_image_stardist(t, 32)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == lbl.shape
    assert torch.equal(t, before)                                           # the input is not written
    assert np.array_equal(out.cpu().numpy(), relabel_image_stardist(lbl, 32))


def test_relabel_3d_tensor_in_equals_host_function():
    import torch
    from stardist_amd import relabel_image_stardist3D
    lbl, rays = C.multi3d(), C.rays3d()
    t = _dev(lbl)
    before = t.clone()
    out = relabel_image_stardist3D(t, rays)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == lbl.shape
    assert torch.equal(t, before)
    want = np.asarray(relabel_image_stardist3D(lbl, rays))
    assert np.array_equal(out.cpu().numpy(), want)                          # voxel for voxel: both entries run the same kernels
    assert set(np.unique(want)) - {0} <= set(np.unique(lbl))


@pytest.mark.parametrize("k", range(int(G["n2d"])))
def test_relabel_2d_device_equals_reference(k):
    from stardist_amd import relabel_image_stardist
    lbl = G["in2d_%d" % k]
    out = relabel_image_stardist(_dev(lbl, np.int32), int(G["rays2d_%d" % k]))
    assert np.array_equal(out.cpu().numpy(), G["out2d_%d" % k]), str(G["name2d_%d" % k])


@pytest.mark.parametrize("k", range(int(G["n3d"])))
def test_relabel_3d_device_equals_reference(k):
    """the rules of tests/test_gpu_relabel.py: voxel for voxel except at most two voxels per object that lie exactly on its hull"""
    from test_gpu_relabel import _on_hull_boundary
    from stardist_amd import Rays_GoldenSpiral, relabel_image_stardist3D
    lbl = G["in3d_%d" % k]
    rays = Rays_GoldenSpiral(int(G["rays3d_%d" % k]), anisotropy=tuple(1.0 / G["eps3d_%d" % k]))
    out = relabel_image_stardist3D(_dev(lbl, np.int32), rays).cpu().numpy()
    assert np.array_equal(out, np.asarray(relabel_image_stardist3D(lbl, rays)))
    diff = np.argwhere(out != G["out3d_%d" % k])
    if len(diff):
        assert len(diff) <= 2 * len(G["lab3d_%d" % k]), (str(G["name3d_%d" % k]), len(diff))
        assert _on_hull_boundary(diff, lbl, rays).all(), (str(G["name3d_%d" % k]), diff[:8])


@pytest.mark.parametrize("dtype", ["int16", "int32", "int64", "uint8"])
def test_relabel_label_dtypes(dtype):
    import torch
    from stardist_amd import relabel_image_stardist, relabel_image_stardist3D
    lbl = np.minimum(C.multi2d(), 250).astype(dtype)                        # 333 -> 250: fits uint8
    out = relabel_image_stardist(_dev(lbl), 32)
    assert out.dtype == torch.int32 and np.array_equal(out.cpu().numpy(), relabel_image_stardist(lbl, 32))
    vol, rays = C.multi3d().astype(dtype), C.rays3d()
    out = relabel_image_stardist3D(_dev(vol), rays)
    assert out.dtype == torch.int32 and np.array_equal(out.cpu().numpy(), relabel_image_stardist3D(vol, rays))


def test_numpy_in_with_device_gives_numpy_out():
    from stardist_amd import relabel_image_stardist, relabel_image_stardist3D
    lbl = C.multi2d()
    out = relabel_image_stardist(lbl, 32, device="cuda")
    assert isinstance(out, np.ndarray) and out.dtype == np.int32 and np.array_equal(out, relabel_image_stardist(lbl, 32))
    vol, rays = C.multi3d(), C.rays3d()
    out = relabel_image_stardist3D(vol.astype(np.uint16), rays, device="cuda:0")
    assert isinstance(out, np.ndarray) and np.array_equal(out, relabel_image_stardist3D(vol, rays))


def test_tensor_with_kwargs_or_compacted_ids_comes_back_as_a_tensor():
    import torch
    from stardist_amd import relabel_image_stardist, relabel_image_stardist3D
    lbl = C.multi2d()
    want = relabel_image_stardist(lbl, 32)
    out = relabel_image_stardist(_dev(lbl), 32, grid=(1, 1))
    assert isinstance(out, torch.Tensor) and out.is_cuda and np.array_equal(out.cpu().numpy(), want)
    sparse = np.where(lbl == 333, 70000, lbl)                               # would be compacted: the host function, ids as uint16 there
    out = relabel_image_stardist(_dev(sparse), 32)
    assert out.is_cuda and np.array_equal(out.cpu().numpy(), relabel_image_stardist(sparse, 32))
    vol, rays = C.multi3d(), C.rays3d()
    out = relabel_image_stardist3D(_dev(vol), rays, grid=(1, 1, 1))
    assert out.is_cuda and np.array_equal(out.cpu().numpy(), relabel_image_stardist3D(vol, rays))


def test_empty_images(capsys):
    import torch
    from stardist_amd import polyhedron_to_label, relabel_image_stardist, relabel_image_stardist3D
    out = relabel_image_stardist(torch.zeros((33, 70), dtype=torch.int16, device="cuda"), 32)
    assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (33, 70) and int(out.abs().sum()) == 0
    out = relabel_image_stardist(np.zeros((33, 70), np.uint16), 32, device="cuda")
    assert isinstance(out, np.ndarray) and out.shape == (33, 70) and not out.any()
    rays = C.rays3d()
    empty = torch.zeros((0, 24), device="cuda")
    want = polyhedron_to_label(empty, torch.zeros((0, 3), device="cuda"), rays, shape=(5, 6, 7), verbose=False)
    capsys.readouterr()
    out = relabel_image_stardist3D(torch.zeros((5, 6, 7), dtype=torch.int32, device="cuda"), rays)
    assert capsys.readouterr().out == ""
    assert type(out) is type(want) and out.dtype == want.dtype and out.shape == want.shape and not np.asarray(out).any()
    relabel_image_stardist3D(torch.zeros((5, 6, 7), dtype=torch.int32, device="cuda"), rays, verbose=True)
    assert "empty list of points" in capsys.readouterr().out


def test_a_stream_of_images_gives_the_bits_of_single_calls():
    import torch
    from stardist_amd import relabel_image_stardist
    imgs = [C.multi2d(), np.ascontiguousarray(C.multi2d()[::-1, ::-1]), np.roll(C.multi2d(), 17, axis=1)]
    single = [relabel_image_stardist(_dev(a), 32).cpu().numpy() for a in imgs]
    tensors = [_dev(a) for a in imgs]
    outs = [relabel_image_stardist(t, 32) for t in tensors]                  # back to back, nothing read in between
    torch.cuda.synchronize()
    for got, want, a in zip(outs, single, imgs):
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(want, relabel_image_stardist(a, 32))


def test_result_feeds_matching_on_the_device():
    from stardist_amd.matching import matching
    lbl = C.multi2d()
    y = _dev(lbl)
    from stardist_amd import relabel_image_stardist
    y2 = relabel_image_stardist(y, 32)
    assert y2.is_cuda and y2.data_ptr() != y.data_ptr()
    got = matching(y, y2)
    want = matching(lbl, relabel_image_stardist(lbl, 32))
    assert got.n_true == want.n_true == 9 and got.n_pred == want.n_pred and got.tp == want.tp and got.fp == want.fp
    assert abs(got.mean_true_score - want.mean_true_score) < 1e-6
