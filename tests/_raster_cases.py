"""Cases, data and host models of the exact tests of the rasterisers (stardist_amd/csrc/raster2d.hip, raster3d.hip): what the kernels do AROUND the
point test -- windows, the polygon / polyhedron stride loops, vertex staging, the LDS opt-in, the label rules.  numpy only, importable
without a GPU; test_cpu_raster_cases.py asserts that every case reaches the regime it is named for and proves the references,
test_gpu_raster_exact.py runs the cases through the kernels and compares with np.array_equal.

  source_constants   block caps, LDS and ray limits read from the launch code (never retyped)
  clip2d, clip3d     the kernels' bounding-box arithmetic (float32 min / max, trunc / ceil in 2D, round-half-even in 3D; image, then window)
  lds3d              the launch's LDS byte count
  2D references      oracle.port.polygon / polygons_to_label_coord (float64 restatement of scikit-image's rule); a window's expected value is
                     the crop of the whole-image reference
  3D references      the compiled reference (`ref` = the oracle.ref module of the refmods fixture); pre-filled buffers and zero labels never
                     reach it through its wrapper: compose3d applies its rule (stardist3d_impl.cpp:1511-1517) to the masks it paints for one
                     polyhedron at a time

Every centre and distance is a random, non-lattice float: no vertex, edge or hull facet lies on a pixel, the comparison has no exemption."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stardist_amd", "csrc")


# ---- the launch arithmetic, from the source ----------------------------------------------------------------------------------------------
def _prod(s):
    return int(np.prod([int(v) for v in s.split("*")], dtype=np.int64))


@functools.lru_cache(None)
def source_constants():
    """dict(cap2d, rays2d, cap3d, optin3d, limit3d, hull_rays) read from sd_polygons_to_label_window_device, sd_polyhedron_to_label_window_device
    and hull_planes; asserts that the loops behind the caps are the stride loops this file models"""
    s2 = open(os.path.join(CSRC, "raster2d.hip")).read()
    s3 = open(os.path.join(CSRC, "raster3d.hip")).read()
    sn = open(os.path.join(CSRC, "nms3d.hip")).read()
    m = re.search(r"const int blocks = n_polys < ([\d *]+) \? n_polys : ([\d *]+);", s2)
    assert _prod(m.group(1)) == _prod(m.group(2))
    cap2d = _prod(m.group(1))
    m = re.search(r"\(size_t\)n_rays \* 2 \* sizeof\(double\) > (\d+)\)", s2)
    rays2d = int(m.group(1)) // 16                                                  # the largest n_rays with 2 * 8 * n_rays <= the limit
    m = re.search(r"const int blocks = n_polys < ([\d *]+) \? n_polys : ([\d *]+);", s3)
    assert _prod(m.group(1)) == _prod(m.group(2))
    cap3d = _prod(m.group(1))
    limit3d = _prod(re.search(r"if \(lds > ([\d *]+)\) \{ sd::set_error", s3).group(1))
    optin3d = _prod(re.search(r"if \(lds > ([\d *]+)\) SD_CHECK\(hipFuncSetAttribute", s3).group(1))
    hull_rays = int(re.search(r"if \(R < 4 \|\| R > (\d+)\) \{ sd::set_error\(\"hull_planes", sn).group(1))
    for text, src in (("for (int p = blockIdx.x; p < n_polys; p += gridDim.x)", s2), ("for (int k = threadIdx.x; k < R; k += blockDim.x)", s2),
                      ("for (int p = p0 + blockIdx.x; p < p1; p += gridDim.x)", s3), ("for (int j = threadIdx.x; j < n_rays; j += blockDim.x)", s3),
                      ("for (int k = threadIdx.x; k < 3 * n_faces; k += blockDim.x)", s3), ("dim3(blocks), dim3(256)", s2), ("dim3(blocks), dim3(256)", s3),
                      ("const int hullCapL = need_hull ? 2 * n_rays : 0;", s3),
                      ("(size_t)(n_faces + hullCapL) * 4 * sizeof(double) + (size_t)n_rays * 3 * sizeof(float) + (size_t)n_faces * 3 * sizeof(int)", s3),
                      ("fabsf(cz) < 8192.f && fabsf(cy) < 8192.f && fabsf(cx) < 8192.f", s3)):
        assert text in src, text
    return dict(cap2d=cap2d, rays2d=rays2d, cap3d=cap3d, optin3d=optin3d, limit3d=limit3d, hull_rays=hull_rays)


THREADS = 256                  # both paint kernels: one block of 256 threads per polygon / polyhedron
UNSAFE = 8192.0                # geom3d.h: the cone map is used below this coordinate only


def lds3d(n_rays, n_faces, mode):
    """the dynamic LDS of k_paint3d: half-spaces of the faces (and of up to 2 * n_rays hull facets in modes 0 and 2) in double, the vertices in
    float, the face list in int"""
    hull = 2 * n_rays if mode in (0, 2) else 0
    return (n_faces + hull) * 4 * 8 + n_rays * 3 * 4 + n_faces * 3 * 4


def clip2d(coord, shape, window=None):
    """k_paint's box per polygon: (minr, maxr, minc, maxc) after the image and the window clip, `culled`, and the float32 extremes
    (rmin, rmax, cmin, cmax) it starts from"""
    c = np.asarray(coord, np.float32)
    HI, WI = shape
    (y0, x0), (h, w) = ((0, 0), (HI, WI)) if window is None else window
    ext = np.stack([c[:, 0].min(1), c[:, 0].max(1), c[:, 1].min(1), c[:, 1].max(1)], 1)
    minr = np.maximum(np.float32(0), ext[:, 0]).astype(np.int64); minc = np.maximum(np.float32(0), ext[:, 2]).astype(np.int64)      # truncation
    maxr = np.minimum(np.ceil(ext[:, 1]).astype(np.int64), HI - 1); maxc = np.minimum(np.ceil(ext[:, 3]).astype(np.int64), WI - 1)
    minr = np.maximum(minr, y0); minc = np.maximum(minc, x0)
    maxr = np.minimum(maxr, y0 + h - 1); maxc = np.minimum(maxc, x0 + w - 1)
    return np.stack([minr, maxr, minc, maxc], 1), (maxr < minr) | (maxc < minc), ext


def clip3d(dist, points, verts, shape, window=None):
    """k_paint3d's box per polyhedron: (zlo, zhi, ylo, yhi, xlo, xhi) after both clips, `culled`, the rounded box before any clip
    (polyhedron_bbox, stardist3d_impl.cpp:536-567: float32 centre + dist * ray, lrint), and `unsafe` (the cone-map preconditions fail)"""
    d, p, V = np.asarray(dist, np.float32), np.asarray(points, np.float32), np.asarray(verts, np.float32)
    pv = p[:, None, :] + d[:, :, None] * V[None]                                     # float32, product rounded, then the sum
    assert pv.dtype == np.float32
    r = np.rint(pv).astype(np.int64)
    raw = np.stack([r[..., 0].min(1), r[..., 0].max(1), r[..., 1].min(1), r[..., 1].max(1), r[..., 2].min(1), r[..., 2].max(1)], 1)
    o, s = ((0, 0, 0), tuple(shape)) if window is None else window
    box = raw.copy()
    for a in range(3):
        box[:, 2 * a] = np.maximum(np.maximum(0, raw[:, 2 * a]), o[a])
        box[:, 2 * a + 1] = np.minimum(np.minimum(shape[a] - 1, raw[:, 2 * a + 1]), o[a] + s[a] - 1)
    culled = (box[:, 1::2] < box[:, 0::2]).any(1)
    unsafe = (np.abs(p) >= UNSAFE).any(1) | ~(d >= 1).all(1) | ~(np.abs(pv).max((1, 2)) < UNSAFE)
    return box, culled, raw, unsafe


def straddles(lo, hi, w0, wn):
    """per shape (given its box [lo, hi] on one axis BEFORE the window clip): it is cut by the low / by the high face of the window [w0, w0 + wn)"""
    return (lo < w0) & (hi >= w0), (hi > w0 + wn - 1) & (lo <= w0 + wn - 1)


def crop(a, window):
    o, s = window
    return a[tuple(slice(int(i), int(i) + int(n)) for i, n in zip(o, s))]


def describe(got, want, k=6):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shape %s != %s" % (got.shape, want.shape)
    bad = np.argwhere(got != want)
    return "%d of %d differ; (index, got, want): %s" % (len(bad), got.size, [(tuple(int(v) for v in i), int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:k]])


# ---- 2D ------------------------------------------------------------------------------------------------------------------------------------
SHAPE2 = (64, 80)
EMPTY2 = ((40, 52), (8, 10))          # the window that no polygon of the window scene reaches


def star_coord(rs, points, radius, R, noise=0.3, phase=None):
    """(n, 2, R) float32 vertices of star polygons: row 0 = r, row 1 = c (geom2d.dist_to_coord's layout), random radii per ray"""
    n = len(points)
    phi = np.linspace(0, 2 * np.pi, R, endpoint=False)[None] + (0 if phase is None else np.asarray(phase)[:, None])
    d = (np.asarray(radius).reshape(n, 1) * (1 + noise * rs.uniform(-1, 1, (n, R))))
    coord = np.stack([d * np.sin(phi), d * np.cos(phi)], 1) + np.asarray(points, np.float64)[:, :, None]
    return np.ascontiguousarray(coord, np.float32)


def _dist_to_box(p, origin, size):
    """distance of the points p (n, nd) to the box [origin, origin + size - 1]"""
    lo, hi = np.asarray(origin, np.float64), np.asarray(origin, np.float64) + np.asarray(size) - 1
    return np.sqrt((np.maximum(np.maximum(lo - p, p - hi), 0) ** 2).sum(1))


def _away(rs, n, lo, hi, reach, origin, size):
    """n uniform points of [lo, hi) whose distance to the box exceeds their `reach`"""
    nd = len(origin)
    p = rs.uniform(lo, hi, (n, nd))
    for _ in range(200):
        bad = _dist_to_box(p, origin, size) <= reach + 1
        if not bad.any():
            return p
        p[bad] = rs.uniform(lo, hi, (int(bad.sum()), nd))
    raise AssertionError("no room beside the empty window")


@functools.lru_cache(None)
def windows2d_scene():
    """(coord (150, 2, 32), labels): 118 ordinary stars with centres up to 6 px outside the image (cut by every border), 24 wholly outside
    (six beyond every border), 8 slivers longer than the image is wide whose boxes exceed it on all four sides; nothing reaches EMPTY2;
    shuffled, labels a permutation"""
    rs = np.random.RandomState(20250)
    H, W = SHAPE2
    rad = rs.uniform(3, 9, 118)
    pts = _away(rs, 118, (-6, -6), (H + 6, W + 6), rad * 1.3, *EMPTY2)
    parts = [star_coord(rs, pts, rad, 32)]
    out = []
    for a, side in ((0, -1), (0, 1), (1, -1), (1, 1)):
        p = np.stack([rs.uniform(0, H, 6), rs.uniform(0, W, 6)], 1)
        p[:, a] = (-rs.uniform(12, 30, 6)) if side < 0 else ((H, W)[a] + rs.uniform(12, 30, 6))
        out.append(p)
    parts.append(star_coord(rs, np.concatenate(out), rs.uniform(3, 6, 24), 32))
    # slivers: r(phi) of an ellipse with half axes 160 and 3, turned so that the long axis misses EMPTY2
    phi = np.linspace(0, 2 * np.pi, 32, endpoint=False)
    sl = []
    mid = np.asarray(EMPTY2[0]) + (np.asarray(EMPTY2[1]) - 1) / 2.0
    while len(sl) < 8:
        c = np.array([rs.uniform(20, H - 20), rs.uniform(25, W - 25)])
        th = rs.uniform(0.5, 1.1) * (1 if rs.rand() < 0.5 else -1)                 # 29 to 63 degrees against the c axis: both extents exceed the image
        u = np.array([np.sin(th), np.cos(th)])
        off = mid - c
        if abs(off[0] * u[1] - off[1] * u[0]) < 20:                                # distance of the window's middle to the long axis
            continue
        a, b = 160.0, 3.0
        r = a * b / np.sqrt((b * np.cos(phi - th)) ** 2 + (a * np.sin(phi - th)) ** 2) * (1 + 0.05 * rs.uniform(-1, 1, 32))
        k = rs.randint(0, 16)
        r[k] = r[k + 16] = a * rs.uniform(0.9, 1.1)                                 # two opposite rays ...
        ph = phi.copy(); ph[k] = th; ph[k + 16] = th + np.pi                        # ... exactly along the long axis
        order = np.argsort(ph % (2 * np.pi))
        sl.append(np.stack([c[0] + r * np.sin(ph), c[1] + r * np.cos(ph)])[:, order])
    parts.append(np.asarray(sl, np.float32))
    coord = np.concatenate(parts)
    perm = rs.permutation(len(coord))
    return np.ascontiguousarray(coord[perm]), rs.permutation(len(coord)).astype(np.int32)


WINDOWS2D = [("full", ((0, 0), SHAPE2)), ("interior-a", ((7, 11), (23, 31))), ("interior-b", ((33, 5), (17, 51))), ("pixel", ((29, 37), (1, 1))),
             ("pixel-corner", ((63, 79), (1, 1))), ("row", ((13, 0), (1, 80))), ("column", ((0, 41), (64, 1))), ("corner-00", ((0, 0), (9, 13))),
             ("corner-01", ((0, 67), (9, 13))), ("corner-10", ((55, 0), (9, 13))), ("corner-11", ((55, 67), (9, 13))), ("empty", EMPTY2)]
BAD_WINDOWS2D = [((-1, 0), (5, 5)), ((0, -1), (5, 5)), ((60, 0), (5, 5)), ((0, 76), (5, 5)), ((0, 0), (65, 80)), ((0, 0), (64, 81))]


def want2d(coord, labels, shape=SHAPE2):
    from oracle import port
    return port.polygons_to_label_coord(coord, shape, labels=np.asarray(labels))


@functools.lru_cache(None)
def windows2d_want():
    return want2d(*windows2d_scene())


def golden2d(name):
    """(coord, labels, shape, golden label image) of a committed scikit-image golden, in the order geom2d.polygons_to_label paints"""
    from oracle import port
    g = np.load(os.path.join(ROOT, "tests", "golden", "raster2d_reference.npz"))
    dist, points, prob = g[name + "_dist"], g[name + "_points"], g[name + "_prob"]
    ind = prob > 0.2
    points, dist, prob = points[ind], dist[ind], prob[ind]
    ind = np.argsort(prob, kind="stable")
    coord = port.dist_to_coord(dist[ind], points[ind])
    return np.ascontiguousarray(coord, np.float32), ind.astype(np.int32), tuple(int(v) for v in g[name + "_shape"]), g[name + "_labels"]


def golden_windows(shape):
    H, W = shape
    return [((0, 0), (H, W)), ((3, 5), (H // 2 + 1, W // 3)), ((H // 2, W // 2), (1, 1)), ((H - 7, W - 9), (7, 9)), ((0, W - 1), (H, 1)), ((H // 3, 0), (1, W))]


STACK2 = ((22, 30), (20, 20))          # the region the label-rule stack is piled on
STACK2_DEPTH = 100                      # the stated depth: that many of the 400 polygons cover one pixel


@functools.lru_cache(None)
def stack2d():
    """(coord (400, 2, 32), dict name -> labels): 400 stars of radius 5 to 11 with centres inside a 20 x 20 region"""
    rs = np.random.RandomState(20251)
    n = 400
    (y0, x0), (h, w) = STACK2
    pts = np.stack([rs.uniform(y0, y0 + h, n), rs.uniform(x0, x0 + w, n)], 1)
    coord = star_coord(rs, pts, rs.uniform(5, 11, n), 32)
    perm = rs.permutation(n).astype(np.int32)
    dup = rs.randint(0, 7, n).astype(np.int32)
    neg_mid = perm.copy(); neg_mid[150:260:3] = -1                                   # label -1 paints 0: it erases
    neg_last = neg_mid.copy(); neg_last[-1] = -1; neg_last[0] = -1
    return coord, dict(perm=perm, dup=dup, neg_mid=neg_mid, neg_last=neg_last)


@functools.lru_cache(None)
def stack2d_masks():
    from oracle import port
    return [port.polygon(*c, SHAPE2) for c in stack2d()[0]]


def paint2d(masks, labels, shape=SHAPE2):
    """geom2d.py:149-166 on precomputed skimage.draw.polygon results: in order, lbl[rr, cc] = label + 1"""
    lbl = np.zeros(shape, np.int32)
    for (rr, cc), l in zip(masks, labels):
        lbl[rr, cc] = l + 1
    return lbl


RAYS2D = (3, 5, 255, 256, 257, 300)     # and source_constants()["rays2d"], the largest count the native takes


@functools.lru_cache(None)
def rays2d_case(R):
    """(coord, labels): a few overlapping stars of R rays, some cut by the border"""
    rs = np.random.RandomState(3000 + R)
    n = 3 if R > 1000 else 6
    pts = np.stack([rs.uniform(-3, SHAPE2[0] + 3, n), rs.uniform(-3, SHAPE2[1] + 3, n)], 1)
    pts[0] = (30.3, 41.7)
    coord = star_coord(rs, pts, rs.uniform(8, 22, n), R, noise=0.4, phase=rs.uniform(0, 1, n))
    return coord, rs.permutation(n).astype(np.int32)


@functools.lru_cache(None)
def rays2d_want(R):
    return want2d(*rays2d_case(R))


LOOP2_EXTRA, LOOP2_BASE = 3000, 4000


def loop2d(n, n_base, seed=20252, tail=(LOOP2_EXTRA, 150)):
    """(base (n_base, 2, 3), assign (n,)): n triangles, polygon i a copy of base[assign[i]], assign random -- the last copies of the base
    triangles are scattered over the whole order.  tail = (k, m): the last k polygons are copies of the first m base triangles only, so that
    they repaint a part of the image and leave the rest to earlier polygons"""
    rs = np.random.RandomState(seed)
    pts = np.stack([rs.uniform(-3, SHAPE2[0] + 3, n_base), rs.uniform(-3, SHAPE2[1] + 3, n_base)], 1)
    base = star_coord(rs, pts, rs.uniform(1.5, 5, n_base), 3, noise=0.5, phase=rs.uniform(0, 2 * np.pi, n_base))
    assign = rs.randint(0, n_base, n)
    assign[n - tail[0]:] = rs.randint(0, tail[1], tail[0])
    return base, assign


def loop2d_last(assign, n_base):
    """position of the last copy of every base triangle (-1: never used)"""
    last = np.full(n_base, -1, np.int64)
    np.maximum.at(last, assign, np.arange(len(assign)))
    return last


def loop2d_want(base, assign, shape=SHAPE2):
    """the image after painting base[assign] in order with labels arange(n): every pixel shows the LAST polygon that covers it, i.e. of the
    base triangles that cover it the one whose last copy comes latest, with that copy's position + 1"""
    from oracle import port
    last = loop2d_last(assign, len(base))
    lbl = np.zeros(shape, np.int32)
    for b in np.argsort(last, kind="stable"):
        if last[b] >= 0:
            rr, cc = port.polygon(*base[b], shape)
            lbl[rr, cc] = last[b] + 1
    return lbl




@functools.lru_cache(None)
def loop2d_case():
    """(base, assign, want) of the polygon-loop case: cap + 3000 triangles"""
    base, assign = loop2d(source_constants()["cap2d"] + LOOP2_EXTRA, LOOP2_BASE)
    return base, assign, loop2d_want(base, assign)


# ---- 3D ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def rays(name):
    """(vertices float32 (R, 3), faces int32 (F, 3)) of "golden<n>" or "octo1" """
    from stardist_amd.rays3d import Rays_GoldenSpiral, Rays_Octo
    r = Rays_Octo(1) if name == "octo1" else Rays_GoldenSpiral(int(name[6:]))
    return np.ascontiguousarray(r.vertices, np.float32), np.ascontiguousarray(r.faces, np.int32)


def polys3d(rs, points, radius, R, noise=0.3):
    n = len(points)
    d = np.asarray(radius).reshape(n, 1) * (1 + noise * rs.uniform(-1, 1, (n, R)))
    return np.ascontiguousarray(d, np.float32), np.ascontiguousarray(points, np.float32)


def ref3d(ref, dist, points, V, F, labels, mode, shape, overlap=None):
    """the compiled reference, all polyhedra at once into a zeroed volume"""
    a = np.ascontiguousarray
    return ref.stardist3d().c_polyhedron_to_label(a(dist, np.float32), a(points, np.float32), a(V, np.float32), a(F, np.int32), a(labels, np.int32), int(mode), 0,
                                                  int(overlap is not None), int(0 if overlap is None else overlap), tuple(int(s) for s in shape))


def masks3d(ref, dist, points, V, F, mode, shape):
    """what the compiled reference paints for every polyhedron on its own"""
    one = np.ones(1, np.int32)
    return [ref3d(ref, dist[i:i + 1], points[i:i + 1], V, F, one, mode, shape) != 0 for i in range(len(dist))]


def compose3d(masks, labels, overlap, start):
    """stardist3d_impl.cpp:1511-1517, polyhedron by polyhedron in the given order:
    result = result == 0 ? label : (use_overlap ? overlap_label : result)"""
    res = np.array(start, np.int32)
    for m, l in zip(masks, labels):
        free = m & (res == 0)
        taken = m & (res != 0)
        res[free] = l
        if overlap is not None:
            res[taken] = overlap
    return res


SHAPE3 = (40, 44, 48)
EMPTY3 = ((29, 3, 34), (7, 8, 9))
WINDOWS3D = [("full", ((0, 0, 0), SHAPE3)), ("interior-a", ((3, 5, 7), (17, 21, 19))), ("interior-b", ((21, 1, 13), (15, 33, 9))),
             ("voxel", ((19, 22, 25), (1, 1, 1))), ("plane-z", ((11, 0, 0), (1, 44, 48))), ("plane-x", ((0, 0, 31), (40, 44, 1))),
             ("line-y", ((8, 0, 17), (1, 44, 1))), ("corner-000", ((0, 0, 0), (9, 11, 13))), ("corner-111", ((31, 33, 35), (9, 11, 13))), ("empty", EMPTY3)]
BAD_WINDOWS3D = [((-1, 0, 0), (4, 4, 4)), ((0, -1, 0), (4, 4, 4)), ((0, 0, -1), (4, 4, 4)), ((37, 0, 0), (4, 4, 4)), ((0, 41, 0), (4, 4, 4)),
                 ((0, 0, 45), (4, 4, 4)), ((0, 0, 0), (41, 44, 48))]


@functools.lru_cache(None)
def windows3d_scene():
    """(dist (50, 32), points, labels, below): 36 ordinary polyhedra with centres up to 4 voxels outside the volume, 6 wholly beyond the upper
    faces, 4 wholly beyond the LOWER faces (`below`), 4 spiky ones whose boxes exceed the volume on all six sides (three rays of 60 along the
    main diagonal, the others short); nothing reaches EMPTY3.

    `below`: the reference's loops run `for (uint64_t z = max(0, bbox[0]); z <= (uint64_t) min(nz - 1, bbox[1]); ...)` (:1461-1463); with a
    negative upper bound the cast wraps and the loop does not end.  By its own rule such a polyhedron paints nothing, so the reference is
    given the scene without them; the kernels get all 50."""
    rs = np.random.RandomState(20253)
    V, F = rays("golden32")
    S = np.asarray(SHAPE3, np.float64)
    rad = rs.uniform(4, 9, 36)
    pts = _away(rs, 36, (-4, -4, -4), tuple(S + 4), rad * 1.3, *EMPTY3)
    up = rs.uniform(5, S - 5, (6, 3)); lo = rs.uniform(5, S - 5, (4, 3))
    for i in range(6):
        up[i, i % 3] = S[i % 3] + rs.uniform(12, 25)
    for i in range(4):
        lo[i, i % 3] = -rs.uniform(12, 25)
    d0, p0 = polys3d(rs, np.concatenate([pts, up, lo]), np.concatenate([rad, rs.uniform(3, 6, 10)]), 32)
    u = np.ones(3) / np.sqrt(3)
    along = np.abs(V.astype(np.float64) @ u)
    spike = np.argsort(along)[-3:]
    assert (np.sign(V[spike].astype(np.float64) @ u) > 0).any() and (np.sign(V[spike].astype(np.float64) @ u) < 0).any()
    d1 = rs.uniform(1.5, 3, (4, 32)); d1[:, spike] = rs.uniform(58, 66, (4, 3))
    p1 = np.asarray([(19.3, 22.6, 22.4), (22.7, 20.2, 25.1), (18.4, 23.3, 21.6), (20.9, 21.1, 24.8)])
    dist = np.concatenate([d0, d1.astype(np.float32)]); points = np.concatenate([p0, p1.astype(np.float32)])
    below = np.zeros(50, bool); below[42:46] = True
    perm = rs.permutation(50)
    return np.ascontiguousarray(dist[perm]), np.ascontiguousarray(points[perm]), (rs.permutation(50) + 1).astype(np.int32), below[perm]


@functools.lru_cache(None)
def windows3d_want(ref, mode):
    d, p, lab, below = windows3d_scene()
    return ref3d(ref, d[~below], p[~below], *rays("golden32"), lab[~below], mode, SHAPE3)


FAR_SHAPE = (8300, 24, 24)
FAR_WINDOWS = [("far", ((8240, 0, 0), (40, 24, 24))), ("across-8192", ((8172, 0, 0), (40, 24, 24)))]


@functools.lru_cache(None)
def far3d_scene():
    """(dist (18, 32), points, labels): 12 polyhedra with centres beyond 8192 (inside the window at z0 = 8240), 3 with the centre below 8192
    and vertices beyond it, 3 wholly below it (the cone map's safe path in the same launch)"""
    rs = np.random.RandomState(20254)
    z = np.concatenate([rs.uniform(8243, 8277, 12), rs.uniform(8187, 8191.5, 3), rs.uniform(8174, 8180, 3)])
    pts = np.stack([z, rs.uniform(4, 20, 18), rs.uniform(4, 20, 18)], 1)
    rad = np.concatenate([rs.uniform(3, 7, 12), rs.uniform(7, 9, 3), rs.uniform(3, 4.5, 3)])
    d, p = polys3d(rs, pts, rad, 32, noise=0.25)
    return d, p, (rs.permutation(18) + 1).astype(np.int32)


@functools.lru_cache(None)
def far3d_want(ref):
    d, p, lab = far3d_scene()
    return ref3d(ref, d, p, *rays("golden32"), lab, 0, FAR_SHAPE)


SHAPE3L = (32, 36, 40)
STACK3_DEPTH = 4
OVERLAPS = (None, 77, -5, "label")      # "label": the value of labels[3]


@functools.lru_cache(None)
def labels3d_scene():
    """(dist (60, 32), points, dict name -> labels): 60 polyhedra of radius 5 to 9 inside a 32 x 36 x 40 volume: most voxels are covered more
    than once.  zero_*: a zero label first, in the middle, last (the sequential path)"""
    rs = np.random.RandomState(20255)
    S = np.asarray(SHAPE3L, np.float64)
    d, p = polys3d(rs, rs.uniform(5, S - 5, (60, 3)), rs.uniform(5, 9, 60), 32)
    perm = (rs.permutation(60) + 1).astype(np.int32)
    dup = rs.randint(1, 6, 60).astype(np.int32)
    neg = perm.copy(); neg[rs.rand(60) < 0.4] *= -1
    zf, zm, zl = perm.copy(), perm.copy(), perm.copy()
    zf[0] = 0; zm[[20, 31, 32]] = 0; zl[-1] = 0
    return d, p, dict(perm=perm, dup=dup, neg=neg, zero_first=zf, zero_mid=zm, zero_last=zl)


def overlap_value(ov, labels):
    return int(labels[3]) if ov == "label" else ov


@functools.lru_cache(None)
def labels3d_masks(ref, mode):
    d, p, _ = labels3d_scene()
    return masks3d(ref, d, p, *rays("golden32"), mode, SHAPE3L)


def prefill3d(shape=SHAPE3L):
    """a buffer that is already labelled on two voxels of three: positive and negative values, 7 among them (a label of `dup`, too)"""
    g = np.indices(shape).sum(0)
    vals = np.array([0, 7, -2, 0, 1000, 7, 0, -31, 5], np.int32)
    return vals[g % len(vals)].copy()


SHAPE3R = (40, 40, 40)
RAYS3D = [(257, 0), (257, 1), (300, 0), (300, 1), (300, 2), (420, 0), (420, 2), (672, 1)]      # (n_rays, render mode)


@functools.lru_cache(None)
def rays3d_case(R):
    rs = np.random.RandomState(4000 + R)
    n = 8
    d, p = polys3d(rs, rs.uniform(4, 36, (n, 3)), rs.uniform(6, 12, n), R, noise=np.repeat([0.05, 0.35], n // 2)[:, None])      # smooth ones: a kernel worth painting
    return d, p, (rs.permutation(n) + 1).astype(np.int32)


@functools.lru_cache(None)
def rays3d_want(ref, R, mode):
    d, p, lab = rays3d_case(R)
    return ref3d(ref, d, p, *rays("golden%d" % R), lab, mode, SHAPE3R)


OVER_LIMIT_RAYS = 1540                  # render mode 1: more LDS than the launch allows
LOOP3_EXTRA = 600


@functools.lru_cache(None)
def loop3d_case():
    """(dist (cap + 600, 6), points, labels = 1 .. n): Rays_Octo(1), radii 1.5 to 3; the first `cap` centres keep to z < 29, the others are
    anywhere: the first painter of the voxels above comes from beyond the cap"""
    rs = np.random.RandomState(20256)
    cap = source_constants()["cap3d"]
    n = cap + LOOP3_EXTRA
    pts = rs.uniform(0, 40, (n, 3))
    pts[:cap, 0] = rs.uniform(0, 29, cap)
    return rs.uniform(1.5, 3, (n, 6)).astype(np.float32), np.ascontiguousarray(pts, np.float32), np.arange(1, n + 1, dtype=np.int32)


@functools.lru_cache(None)
def loop3d_want(ref, mode):
    d, p, lab = loop3d_case()
    return ref3d(ref, d, p, *rays("octo1"), lab, mode, SHAPE3R)
