"""Mirror of stardist/geometry/geom2d.py (hot-path functions) on top of the HIP natives."""
import numpy as np

from .. import _route as R
from ..lib import _native as N
from ..utils import _normalize_grid, to_host


_SC_CACHE = {}


def ray_angles(n_rays=32):
    """geom2d.py:214-215"""
    return np.linspace(0, 2 * np.pi, n_rays, endpoint=False)


def star_dist(a, n_rays=32, grid=(1, 1), mode="hip"):
    """geom2d.py:73-85. 'a' is a label image (0 = background). mode 'hip' replaces 'cpp'/'opencl'."""
    from ..lib.stardist2d import c_star_dist
    n_rays >= 3 or (_ for _ in ()).throw(ValueError("need 'n_rays' >= 3"))
    if mode not in ("hip", "cpp", "opencl"):
        raise ValueError("Unknown mode %s" % mode)
    grid = _normalize_grid(grid, 2)
    if N.is_torch(a):
        import torch
        return c_star_dist(a.to(torch.uint16) if a.dtype != torch.uint16 else a, np.int32(n_rays), np.int32(grid[0]), np.int32(grid[1]))
    return c_star_dist(a.astype(np.uint16, copy=False), np.int32(n_rays), np.int32(grid[0]), np.int32(grid[1]))


def _dist_to_coord_old(rhos, grid=(1, 1)):
    """geom2d.py:88-109: dense polar -> cartesian for one image (3-D) or several (4-D): coord (..., h, w, 2, n_rays) in the dtype of rhos."""
    grid = _normalize_grid(grid, 2)
    rhos = np.asarray(rhos)
    is_single_image = rhos.ndim == 3
    if is_single_image:
        rhos = np.expand_dims(rhos, 0)
    assert rhos.ndim == 4
    n_images, h, w, n_rays = rhos.shape
    coord = np.empty((n_images, h, w, 2, n_rays), dtype=rhos.dtype)
    start = np.indices((h, w))
    for i in range(2):
        coord[..., i, :] = grid[i] * np.broadcast_to(start[i].reshape(1, h, w, 1), (n_images, h, w, n_rays))
    phis = ray_angles(n_rays).reshape(1, 1, 1, n_rays)
    coord[..., 0, :] += rhos * np.sin(phis)   # row coordinate
    coord[..., 1, :] += rhos * np.cos(phis)   # col coordinate
    return coord[0] if is_single_image else coord


def _polygons_to_label_old(coord, prob, points, shape=None, thr=-np.inf):
    """geom2d.py:112-127: paint the polygons of the dense coordinate map at `points` with increasing probability (ids 1, 2, ... in
    that order); the per-polygon skimage.draw.polygon loop runs as one call of the HIP rasteriser."""
    coord = np.asarray(coord); prob = np.asarray(prob); points = np.asarray(points)
    sh = coord.shape[:2] if shape is None else shape
    if len(points) == 0:
        return np.zeros(sh, np.int32)
    pr = prob[points[:, 0], points[:, 1]]
    ind = np.argsort(pr)
    points = points[ind]
    points = points[prob[points[:, 0], points[:, 1]] >= thr]
    c = np.ascontiguousarray(coord[points[:, 0], points[:, 1]], np.float32)
    return polygons_to_label_coord(c, sh, labels=np.arange(len(points)))


def dist_to_coord(dist, points, scale_dist=(1, 1)):
    """geom2d.py:130-146: polar -> cartesian, coord (n_polys, 2, n_rays) float32."""
    assert dist.ndim == 2 and points.ndim == 2 and len(dist) == len(points) and points.shape[1] == 2 and len(scale_dist) == 2
    n_rays = dist.shape[1]
    phis = ray_angles(n_rays)
    sc = np.array([np.sin(phis), np.cos(phis)])           # float64 (2, n_rays)
    if N.is_torch(dist) and dist.is_cuda and dist.dtype == __import__("torch").float32 and N.is_torch(points):
        # one launch in numpy's arithmetic (sd_dist_to_coord_device): f32 * f64 products rounded to f32, the centre added in f64 and
        # rounded once; the (sin, cos) table is the host libm's, uploaded once per (n_rays, device)
        import torch
        key = (n_rays, str(dist.device))
        sct = _SC_CACHE.get(key)
        if sct is None:
            sct = _SC_CACHE[key] = torch.as_tensor(np.ascontiguousarray(sc), device=dist.device)
        d = dist.contiguous()
        p = points.to(torch.float64).contiguous()
        coord = torch.empty((d.shape[0], 2, n_rays), dtype=torch.float32, device=dist.device)
        if d.shape[0]:
            import ctypes
            N.dcall(d, "sd_dist_to_coord_device", N.tptr(d), N.tptr(p), N.tptr(sct), int(d.shape[0]), int(n_rays),
                    ctypes.c_double(float(scale_dist[0])), ctypes.c_double(float(scale_dist[1])), N.tptr(coord))
        return coord
    if N.is_torch(dist):
        import torch
        sct = torch.as_tensor(sc, device=dist.device)                      # float64
        coord = (dist[:, None].to(torch.float64) * sct).to(torch.float32)  # f32*f64 product -> f32, as numpy does
        sd = torch.as_tensor(np.asarray(scale_dist, np.float64).reshape(1, 2, 1), device=dist.device)
        coord = (coord.to(torch.float64) * sd).to(torch.float32) if tuple(scale_dist) != (1, 1) else coord
        # numpy's in-place `coord += points[..., None]` adds in the common type of both operands and rounds ONCE to float32
        # (points may be int64 / float64): add in float64, cast once
        coord = (coord.to(torch.float64) + points[..., None].to(torch.float64)).to(torch.float32)
        return coord
    dist = np.asarray(dist); points = np.asarray(points)
    coord = (dist[:, np.newaxis] * sc).astype(np.float32)
    coord *= np.asarray(scale_dist).reshape(1, 2, 1)
    coord += points[..., np.newaxis]
    return coord


def polygons_to_label_coord(coord, shape, labels=None, window=None):
    """geom2d.py:149-166: paint polygons in the given order (later overwrite earlier), value labels[i]+1.
    window = ((y0, x0), (h, w)) (device tensors): only that part of the image is rendered and returned."""
    from ..lib.stardist2d import c_polygons_to_label
    assert coord.ndim == 3 and coord.shape[1] == 2
    n = len(coord)
    if N.is_torch(coord):
        import torch
        if labels is None:
            labels = torch.arange(n, device=coord.device)
        assert len(labels) == n
        if window is not None and n:                               # polygons whose bounding box misses the window are dropped up front
            (y0, x0), (h, w) = window
            lo, hi = coord.amin(dim=2), coord.amax(dim=2)
            hit = (hi[:, 0] >= y0 - 1) & (lo[:, 0] <= y0 + h) & (hi[:, 1] >= x0 - 1) & (lo[:, 1] <= x0 + w)
            coord, labels = coord[hit], labels[hit]
        return c_polygons_to_label(coord, labels.to(torch.int32), shape, window=window)
    assert window is None, "window rendering takes device tensors"
    coord = np.asarray(coord)
    if labels is None:
        labels = np.arange(n)
    labels = np.asarray(labels)
    if not (np.issubdtype(labels.dtype, np.integer) or labels.dtype == bool):
        raise ValueError("labels must be an array of integers")
    assert len(labels) == n
    return c_polygons_to_label(coord, labels.astype(np.int32), shape)


def polygons_to_label(dist, points, shape, prob=None, thr=-np.inf, scale_dist=(1, 1), window=None):
    """geom2d.py:169-197: label ids are consecutive and adhere to the order given."""
    assert dist.ndim == 2 and points.ndim == 2 and len(dist) == len(points) and points.shape[1] == 2
    if N.is_torch(dist):
        import torch
        prob = torch.full((len(points),), float("inf"), device=dist.device) if prob is None else prob
        ind = prob > thr
        points, dist, prob = points[ind], dist[ind], prob[ind]
        ind = torch.sort(prob, stable=True)[1]
        points, dist = points[ind], dist[ind]
        coord = dist_to_coord(dist, points, scale_dist=scale_dist)
        return polygons_to_label_coord(coord, shape=shape, labels=ind, window=window)
    assert window is None, "window rendering takes device tensors"
    dist = np.asarray(dist); points = np.asarray(points)
    prob = np.inf * np.ones(len(points)) if prob is None else np.asarray(prob)
    assert len(points) == len(prob) and prob.ndim == 1
    ind = prob > thr
    points, dist, prob = points[ind], dist[ind], prob[ind]
    ind = np.argsort(prob, kind="stable")
    points, dist = points[ind], dist[ind]
    coord = dist_to_coord(dist, points, scale_dist=scale_dist)
    return polygons_to_label_coord(coord, shape=shape, labels=ind)


def _region_centroids(lbl):
    """(labels, centroids): what `skimage.measure.regionprops(lbl)` yields as (r.label, r.centroid) -- the labels present in ascending
    order, the centroid = the mean of the region's pixel coordinates (skimage: `coords.mean(axis=0)`, a float64 quotient of an exactly
    representable integer sum and the pixel count; reproduced here as that quotient, so the truncation `astype(int)` the callers apply
    sees the very same float64).  Per object on its bounding box (scipy.ndimage.find_objects), like regionprops: no image-sized temporaries."""
    from scipy.ndimage import find_objects
    lbl = np.asarray(lbl)
    boxes = [(i, sl) for i, sl in enumerate(find_objects(lbl), 1) if sl is not None]
    labs = np.array([i for i, _ in boxes], np.int64)
    cen = np.empty((len(boxes), lbl.ndim), np.float64)
    for k, (lab, sl) in enumerate(boxes):
        m = lbl[sl] == lab
        n = int(m.sum())
        for d in range(lbl.ndim):
            along = m.sum(axis=tuple(a for a in range(lbl.ndim) if a != d), dtype=np.int64)           # pixels of the object per coordinate
            cen[k, d] = int((along * np.arange(sl[d].start, sl[d].stop, dtype=np.int64)).sum()) / n    # exact integer sum, one rounding
    return labs, cen


def _check_label_array(y, name=None):
    """matching.py:23-35 (the non-sequential form the geometry functions use)"""
    y = np.asarray(y)
    if not np.issubdtype(y.dtype, np.integer) or (y.size and y.min() < 0):
        raise ValueError("%s must be an array of non-negative integers." % ("labels" if name is None else name))
    return True


def _region_centroids_device(lab, top):
    """(labs, points) of a contiguous int32 label tensor on a HIP device whose objects are the labels 1 .. top: the labels present in
    ascending order and the pixel under each one's centroid, `sums[:, 1:] // count` of sd_label_centroid_sums_device, as int64 tensors
    ((n,) and (n, lab.dim())) on that device.  The integer division equals the host's truncation of the float64 quotient
    (`_region_centroids(lbl)[1].astype(int)`) wherever a coordinate sum is below 2**53, where the float64 sum is the integer: every
    image that int32 offsets address satisfies this (fewer than 2**31 pixels, coordinates below 2**31 / count).  One scalar comes to the
    host, the number of objects (in torch.nonzero)."""
    import torch
    sums = R.label_tables(lab, int(top), sums=True)[1]
    labs = torch.nonzero(sums[:, 0]).reshape(-1)
    s = sums.index_select(0, labs)
    return labs, torch.div(s[:, 4 - lab.dim():], s[:, :1], rounding_mode="floor").contiguous()


def _star_representation_device(lbl, rays):
    """(labs, points, dist) of the objects of a 2D / 3D label image on a HIP device, as relabel_image_stardist / relabel_image_stardist3D
    use them: the labels present (ascending), the pixel under each centroid (int64) and the row of star_dist(lbl, rays) (`rays` an int:
    2D) or of star_dist3D(lbl, rays) (a Rays_* object: 3D; clamped below at 1e-3, geom3d.py:214) at that pixel, float32, evaluated
    there only (sd_star_dist2d_points_device / sd_star_dist3d_points_device).  lbl: an integer tensor without negative values whose ids
    need no compaction (stardist_amd._route._ids_need_compaction); nothing but the number of objects and the kernels' status come to
    the host."""
    import ctypes
    import torch
    N.require_device()
    lab = lbl.to(torch.int32).contiguous()
    top = int(lab.max()) if lab.numel() else 0
    dev = lab.device
    if lab.numel() == 0 or top <= 0:
        n_rays = rays if np.isscalar(rays) else len(rays)
        return (torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros((0, lab.dim()), dtype=torch.int64, device=dev),
                torch.zeros((0, int(n_rays)), dtype=torch.float32, device=dev))
    labs, points = _region_centroids_device(lab, top)
    n = int(points.shape[0])
    if lab.dim() == 2:
        n_rays = int(rays)
        dist = torch.empty((n, n_rays), dtype=torch.float32, device=dev)
        N.dcall(lab, "sd_star_dist2d_points_device", N.tptr(lab), int(lab.shape[0]), int(lab.shape[1]), N.tptr(points), n, n_rays, N.tptr(dist))
    else:
        n_rays = len(rays)
        dz, dy, dx = (torch.as_tensor(np.ascontiguousarray(v, np.float32), device=dev) for v in rays.vertices.T)
        dist = torch.empty((n, n_rays), dtype=torch.float32, device=dev)
        N.dcall(lab, "sd_star_dist3d_points_device", N.tptr(lab), *(int(v) for v in lab.shape), N.tptr(points), n, N.tptr(dz), N.tptr(dy),
                N.tptr(dx), n_rays, ctypes.c_float(1e-3), N.tptr(dist))
    return labs, points, dist


def _relabel_route(lbl, ndim, device, kwargs):
    """how relabel_image_stardist / relabel_image_stardist3D treat their input, after the reference's own checks (integer values, none
    negative, `ndim` axes: ValueError).  -> (route, image): 'host' = the host code on the numpy array `image`; 'via_host' = the host
    function on a copy of the tensor, the result back as a tensor; 'device' = `image` is the label tensor on the device (an uploaded
    numpy array comes back as numpy: the caller sees that from its own argument)."""
    lbl, is_t, on_device = R.classify(lbl, device)
    if not is_t:
        _check_label_array(lbl, "lbl")
        if not lbl.ndim == ndim:
            raise ValueError("lbl image should be %d dimensional" % ndim)
        if not on_device or kwargs or (lbl.size and R._ids_need_compaction(int(lbl.max()), lbl.size)):
            return "host", lbl
        return "device", R.to_device_tensor(lbl.astype(np.int32), device)
    import torch
    if lbl.is_floating_point() or lbl.is_complex() or lbl.dtype == torch.bool:
        raise ValueError("lbl must be an array of non-negative integers.")
    lo, hi = (int(v) for v in torch.stack(torch.aminmax(lbl)).tolist()) if lbl.numel() else (0, 0)
    if lo < 0:
        raise ValueError("lbl must be an array of non-negative integers.")
    if not lbl.dim() == ndim:
        raise ValueError("lbl image should be %d dimensional" % ndim)
    if kwargs or not on_device or str(lbl.dtype) not in R._DEVICE_LABEL_DTYPES or R._ids_need_compaction(hi, lbl.numel()):
        return "via_host", lbl
    return "device", R.to_device_tensor(lbl, device)


def relabel_image_stardist(lbl, n_rays, *, device=None, **kwargs):
    """geom2d.py:200-211: relabel each label region in `lbl` with its star representation (star_dist at the truncated region
    centroid -> polygons_to_label).  Label ids of the result are 1..n in the order of the regions' ids, as in the reference.

    Routing: DESIGN.md section 3p; the host code is the one below.  The device route takes integer images: centroids and the star
    distances at the centroids only (`_star_representation_device`), then the tensor path of polygons_to_label; the result is int32
    and equals the host result.  Its own (exception 8 there): with any **kwargs (grid, mode), or ids that
    stardist_amd._route._device_labels would compact (the compaction loses the low 16 bits the rays compare), a tensor goes through
    the host function and comes back as a tensor where it lives, whatever `device=` says; a numpy array takes the host code."""
    route, img = _relabel_route(lbl, 2, device, kwargs)
    if route == "via_host":
        return R.via_host(relabel_image_stardist, img, n_rays, **kwargs)
    if route == "device":
        import torch
        _, points, dist = _star_representation_device(img, int(n_rays))
        shape = tuple(int(v) for v in img.shape)
        out = polygons_to_label(dist, points, shape=shape) if len(points) else torch.zeros(shape, dtype=torch.int32, device=img.device)
        return out if N.is_torch(lbl) else to_host(out)
    lbl = img
    dist = star_dist(lbl, n_rays, **kwargs)
    points = _region_centroids(lbl)[1].astype(int)
    if len(points) == 0:
        dist, points = np.zeros((0, n_rays), np.float32), np.zeros((0, 2), int)
    else:
        dist = dist[tuple(points.T)]
    return polygons_to_label(dist, points, shape=lbl.shape)
