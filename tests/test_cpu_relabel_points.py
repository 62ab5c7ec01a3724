"""CPU: star distances at given pixels only (sd_star_dist2d_points_host / sd_star_dist3d_points_host: the march of csrc/relabel_star.h
run by the host, the same function the point kernels run), the integer centroid rule of `_region_centroids_device`, and the routing of
`relabel_image_stardist(..., device=)` / `relabel_image_stardist3D(..., device=)`.

The dense rows the point rows must equal are those of c_star_dist / c_star_dist3d.  The library's dense entry points
(sd_star_dist2d_host / sd_star_dist3d_host) launch kernels and need a device, so here the dense side is their line-by-line float32
statement tests/_target_cases.py (star_dist2d_np / star_dist3d_np), which tests/test_gpu_target_cases.py holds equal to those kernels
bit for bit; tests/test_gpu_relabel_device.py compares the same point rows with the dense entry points themselves."""
import ctypes

import numpy as np
import pytest

import _relabel_cases as C
import _target_cases as T


def _lib():
    import __graft_entry__  # noqa: F401
    from stardist_amd.build import build_lib
    build_lib(verbose=False)
    from stardist_amd.lib import _native as N
    return N


def points2d_host(lbl, pts, n_rays):
    N = _lib()
    lbl = np.ascontiguousarray(lbl, np.int32); pts = np.ascontiguousarray(pts, np.int64).reshape(-1, 2)
    out = np.full((len(pts), n_rays), -5, np.float32)
    rc = N.lib().sd_star_dist2d_points_host(N.ptr(lbl), lbl.shape[0], lbl.shape[1], N.ptr(pts), len(pts), n_rays, N.ptr(out))
    return rc, out


def points3d_host(lbl, pts, rays, floor=0.0):
    N = _lib()
    lbl = np.ascontiguousarray(lbl, np.int32); pts = np.ascontiguousarray(pts, np.int64).reshape(-1, 3)
    dz, dy, dx = (np.ascontiguousarray(v, np.float32) for v in rays.vertices.T)
    out = np.full((len(pts), len(rays)), -5, np.float32)
    rc = N.lib().sd_star_dist3d_points_host(N.ptr(lbl), *lbl.shape, N.ptr(pts), len(pts), N.ptr(dz), N.ptr(dy), N.ptr(dx), len(rays),
                                            ctypes.c_float(floor), N.ptr(out))
    return rc, out


# ---- point rows against the dense function ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rays", (17, 32))
def test_point_rows_2d_equal_the_dense_rows(n_rays):
    lbl = C.multi2d()
    assert lbl.shape == (61, 130)
    pts = C.probe_points(lbl)
    vals = lbl[tuple(pts.T)]
    on_border = (pts == 0).any(1) | (pts == np.array(lbl.shape) - 1).any(1)
    assert (vals[on_border] > 0).any() and (vals == 0).any() and len(np.unique(vals[vals > 0])) == len(np.unique(lbl)) - 1
    rc, got = points2d_host(lbl, pts, n_rays)
    assert rc == 0
    dense = T.star_dist2d_np(lbl, n_rays)
    assert np.array_equal(got, dense[tuple(pts.T)])
    assert (got[vals == 0] == 0).all() and (got[vals > 0] > 0).all()


def test_point_rows_3d_equal_the_dense_rows_and_floor():
    lbl, rays = C.multi3d(), C.rays3d()
    assert lbl.shape == (20, 37, 45) and len(rays) == 24
    pts = C.probe_points(lbl)
    vals = lbl[tuple(pts.T)]
    on_border = (pts == 0).any(1) | (pts == np.array(lbl.shape) - 1).any(1)
    assert (vals[on_border] > 0).any() and (vals == 0).any() and len(np.unique(vals[vals > 0])) == len(np.unique(lbl)) - 1
    dense = T.star_dist3d_np(lbl, rays.vertices)[tuple(pts.T)]
    rc, got = points3d_host(lbl, pts, rays)
    assert rc == 0 and np.array_equal(got, dense)
    assert (dense == 0).any()                                             # background rows, and rays that stop within half a voxel
    rc, got = points3d_host(lbl, pts, rays, floor=1e-3)
    assert rc == 0 and np.array_equal(got, np.maximum(dense, np.float32(1e-3)))
    rc, got = points3d_host(lbl, pts, rays, floor=2.5)
    assert rc == 0 and np.array_equal(got, np.maximum(dense, np.float32(2.5))) and (got == 2.5).any() and (got > 2.5).any()


def test_no_points_and_points_outside():
    N = _lib()
    lbl, rays = C.multi2d(), C.rays3d()
    rc, got = points2d_host(lbl, np.zeros((0, 2), np.int64), 8)
    assert rc == 0 and got.shape == (0, 8)
    rc, got = points3d_host(C.multi3d(), np.zeros((0, 3), np.int64), rays)
    assert rc == 0 and got.shape == (0, 24)
    for bad in ([61, 0], [0, 130], [-1, 5], [5, -1], [2 ** 40, 3]):
        rc, _ = points2d_host(lbl, np.array([[14, 20], bad]), 8)
        assert rc == -1 and b"outside" in N.lib().sd_last_error()
    for bad in ([20, 0, 0], [0, 37, 0], [0, 0, 45], [0, -1, 0], [0, 0, 2 ** 33]):
        rc, _ = points3d_host(C.multi3d(), np.array([[9, 12, 12], bad]), rays)
        assert rc == -1 and b"outside" in N.lib().sd_last_error()
    assert points2d_host(lbl, np.array([[14, 20]]), 0)[0] == -1           # no rays
    still = T.Rays(np.vstack([rays.vertices[:3], np.zeros((1, 3))]))      # a ray without a direction would never end
    assert points3d_host(C.multi3d(), np.array([[9, 12, 12]]), still)[0] == -1 and b"direction" in N.lib().sd_last_error()


# ---- ids are compared as unsigned short -----------------------------------------------------------------------------------------------
def test_ids_equal_modulo_65536_are_one_object_to_a_ray():
    a = C.u16_pair()
    pts = np.array([[60, 40], [60, 80], [110, 20], [0, 0]], np.int64)     # in 7, in 65543, in 8, background
    rc, got = points2d_host(a, pts, 32)
    assert rc == 0
    merged = np.where(a == 65543, 7, a)
    assert np.array_equal(T._as_u16(a), merged.astype(np.uint16))          # what the cast of geom2d.py:31 makes of the int32 image
    assert np.array_equal(got, T.star_dist2d_np(a, 32)[tuple(pts.T)])
    assert np.array_equal(got, points2d_host(merged, pts, 32)[1])
    assert got[0, 0] > 50 and got[1, 16] > 50                             # the rays along +x / -x cross the seam between the two ids
    assert (got[3] == 0).all()


def test_a_multiple_of_65536_is_background_to_a_ray():
    a = C.u16_zero()
    pts = np.array([[40, 40], [100, 70]], np.int64)                       # in 65536, in 2
    rc, got = points2d_host(a, pts, 32)
    assert rc == 0 and (got[0] == 0).all() and (got[1] > 0).all()
    assert np.array_equal(got, T.star_dist2d_np(a, 32)[tuple(pts.T)])


# ---- the centroid rule -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.centroid_scenes()))
def test_integer_centroids_equal_truncated_float_centroids(name):
    from stardist_amd.geometry.geom2d import _region_centroids
    lbl = C.centroid_scenes()[name]
    labs, cen = _region_centroids(lbl)
    got_labs, got = C.centroid_rule_np(lbl)
    assert np.array_equal(got_labs, labs) and len(labs) == len(np.unique(lbl[lbl > 0]))
    assert np.array_equal(got, cen.astype(int))


def test_centroid_scenes_are_what_they_say():
    S = C.centroid_scenes()
    labs, pts = C.centroid_rule_np(S["multi2d"])
    assert labs.tolist() == [3, 7, 12, 40, 41, 90, 91, 200, 333] and (np.diff(labs) > 1).any()
    assert (C.centroid_sums_np(S["multi2d"])[:, 0] == 1).sum() == 2                                 # one-pixel objects
    for name in ("ell",):
        labs, pts = C.centroid_rule_np(S[name])
        assert S[name][tuple(pts[0])] == 0                                                          # the L's centroid is background
    labs, pts = C.centroid_rule_np(S["ring_disc"])
    assert labs.tolist() == [4, 9] and pts[0].tolist() == pts[1].tolist() and S["ring_disc"][tuple(pts[0])] == 4
    s = C.centroid_sums_np(S["wide"])
    assert s[2].tolist() == [400000, 0, 400000 * 39 // 2, 40 * (60000 + 69999) * 10000 // 2] and s[2, 3] > 2 ** 32
    assert C.centroid_rule_np(S["u16_pair"])[0].tolist() == [7, 8, 65543] and C.centroid_rule_np(S["u16_zero"])[0].tolist() == [2, 65536]
    assert C.centroid_rule_np(S["multi3d"])[0].tolist() == [2, 5, 11, 30, 31, 50]


# ---- dispatch -------------------------------------------------------------------------------------------------------------------------
class _RecordingLib(object):
    """stands in for the loaded library: records (name, integer arguments) of every call and reports success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, tuple(a for a in args if isinstance(a, int))))
            return 1 if name == "sd_device_count" else 0
        return fn


def _record(monkeypatch):
    N = _lib()
    fake = _RecordingLib()
    monkeypatch.setattr(N, "lib", lambda: fake)
    return fake


def test_host_input_makes_the_native_calls_it_made_before(monkeypatch):
    from stardist_amd.geometry import geom2d, geom3d
    for fn in ("_star_representation_device", "_region_centroids_device"):
        monkeypatch.setattr(geom2d, fn, lambda *a, **k: pytest.fail("device path taken"))
    fake = _record(monkeypatch)
    lbl = C.multi2d()
    for kw in ({}, {"device": None}):
        del fake.calls[:]
        out = geom2d.relabel_image_stardist(lbl, 17, **kw)
        assert isinstance(out, np.ndarray) and out.shape == lbl.shape and out.dtype == np.int32
        assert fake.calls == [("sd_device_count", ()), ("sd_star_dist2d_host", (61, 130, 17, 1, 1)),
                              ("sd_device_count", ()), ("sd_polygons_to_label_host", (9, 17, 61, 130))]
    del fake.calls[:]
    geom2d.relabel_image_stardist(lbl, 8, grid=(1, 1), mode="cpp")         # kwargs go to star_dist, as before
    assert fake.calls[1] == ("sd_star_dist2d_host", (61, 130, 8, 1, 1))
    with pytest.raises(ValueError, match="Unknown mode"):
        geom2d.relabel_image_stardist(lbl, 8, mode="no such mode")
    vol, rays = C.multi3d(), C.rays3d()
    for kw in ({}, {"device": None}):
        del fake.calls[:]
        out = geom3d.relabel_image_stardist3D(vol, rays, **kw)
        assert isinstance(out, np.ndarray) and out.shape == vol.shape
        assert [c[0] for c in fake.calls] == ["sd_device_count", "sd_star_dist3d_host", "sd_device_count", "_LIB_polyhedron_to_label"]
        assert fake.calls[1][1] == (20, 37, 45, 24, 1, 1, 1) and fake.calls[3][1][:3] == (6, 24, len(rays.faces))


def test_kwargs_and_compacted_ids_take_the_host_function(monkeypatch):
    """with device=: a numpy array with kwargs, or with ids that would be compacted, still runs the host code"""
    from stardist_amd.geometry import geom2d, geom3d
    from stardist_amd._route import _ids_need_compaction
    for fn in ("_star_representation_device", "_region_centroids_device"):
        monkeypatch.setattr(geom2d, fn, lambda *a, **k: pytest.fail("device path taken"))
    fake = _record(monkeypatch)
    lbl = C.multi2d()
    geom2d.relabel_image_stardist(lbl, 8, device="cuda", grid=(1, 1))
    geom2d.relabel_image_stardist(lbl, 8, device="cuda", mode="cpp")
    sparse = np.where(lbl == 333, 70000, lbl)                             # 70000 > 4 * 61 * 130 + 1024
    assert _ids_need_compaction(70000, sparse.size) and not _ids_need_compaction(333, lbl.size)
    geom2d.relabel_image_stardist(sparse, 8, device="cuda")
    assert [c[0] for c in fake.calls] == ["sd_device_count", "sd_star_dist2d_host", "sd_device_count", "sd_polygons_to_label_host"] * 3
    del fake.calls[:]
    vol = C.multi3d()
    geom3d.relabel_image_stardist3D(vol, C.rays3d(), device="cuda", grid=(1, 1, 1))
    geom3d.relabel_image_stardist3D(np.where(vol == 50, 10 ** 6, vol), C.rays3d(), device="cuda")
    assert [c[0] for c in fake.calls] == ["sd_device_count", "sd_star_dist3d_host", "sd_device_count", "_LIB_polyhedron_to_label"] * 2


def test_tensors_with_kwargs_or_compacted_ids_go_through_the_host_function(monkeypatch):
    import torch
    from stardist_amd.geometry import geom2d, geom3d
    for fn in ("_star_representation_device", "_region_centroids_device"):
        monkeypatch.setattr(geom2d, fn, lambda *a, **k: pytest.fail("device path taken"))
    fake = _record(monkeypatch)
    lbl = C.multi2d()
    t = torch.from_numpy(lbl.copy())
    for out in (geom2d.relabel_image_stardist(t, 8, device="cpu", grid=(1, 1)),
                geom2d.relabel_image_stardist(torch.from_numpy(np.where(lbl == 333, 70000, lbl)), 8, device="cpu"),
                geom2d.relabel_image_stardist(t, 8)):                      # a host tensor without device=
        assert isinstance(out, torch.Tensor) and out.dtype == torch.int32 and tuple(out.shape) == lbl.shape
    assert [c[0] for c in fake.calls] == ["sd_device_count", "sd_star_dist2d_host", "sd_device_count", "sd_polygons_to_label_host"] * 3
    del fake.calls[:]
    out = geom3d.relabel_image_stardist3D(torch.from_numpy(C.multi3d().copy()), C.rays3d(), device="cpu", grid=(1, 1, 1))
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == C.SHAPE_3D
    assert [c[0] for c in fake.calls] == ["sd_device_count", "sd_star_dist3d_host", "sd_device_count", "_LIB_polyhedron_to_label"]


def test_the_reference_s_value_errors_on_every_kind_of_input():
    import torch
    from stardist_amd.geometry import relabel_image_stardist, relabel_image_stardist3D
    rays = C.rays3d()
    for dev in ({}, {"device": "cuda"}):
        for wrap in (np.asarray, torch.as_tensor):
            with pytest.raises(ValueError, match="non-negative integers"):
                relabel_image_stardist(wrap(np.zeros((4, 4), np.float32)), 8, **dev)
            with pytest.raises(ValueError, match="non-negative integers"):
                relabel_image_stardist3D(wrap(np.zeros((4, 4, 4), np.float32)), rays, **dev)
            with pytest.raises(ValueError, match="non-negative integers"):
                relabel_image_stardist(wrap(-np.ones((4, 4), np.int32)), 8, **dev)
            with pytest.raises(ValueError, match="non-negative integers"):
                relabel_image_stardist3D(wrap(-np.ones((4, 4, 4), np.int64)), rays, **dev)
            with pytest.raises(ValueError, match="2 dimensional"):
                relabel_image_stardist(wrap(np.zeros((4, 4, 4), np.int32)), 8, **dev)
            with pytest.raises(ValueError, match="3 dimensional"):
                relabel_image_stardist3D(wrap(np.zeros((4, 4), np.int16)), rays, **dev)
