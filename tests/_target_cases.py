"""Cases, data and plain references of the exact tests of the training targets (csrc/edt.hip, csrc/star_dist.hip and the host code that
drives them: utils.edt_prob, targets.stardist_targets, training.targets_device, training3d.targets_device3d).  Nothing here needs a GPU or
scipy; test_cpu_target_cases.py proves the references against scipy / the reference sources / the compiled reference and asserts that the
case lists reach the regimes they are named for, test_gpu_targets_exact.py runs every case through the kernels and compares with ==.

  label generators   seeded, deterministic, int32
  edt_prob_box       float64 reference of stardist/utils.py:98-125 (_edt_prob_scipy)
  star_dist2d_np     float32 restatement of c_star_dist (stardist/lib/stardist2d.cpp:55-124), vectorised over pixels, stepping along the ray
  star_dist3d_np     the same of c_star_dist3d (stardist/lib/stardist3d.cpp:245-346)
  targets_ref        the target lines of StarDistData2D / 3D.__getitem__ (model2d.py:63-104, model3d.py:66-104) on those pieces
  EDT2D, EDT3D, SD2D, SD3D, BATCH2D, BATCH3D   the case lists; every entry is a dict with an `id`"""
import ctypes
import ctypes.util
import functools
import warnings

import numpy as np

GRID_CAP_THREADS = 8192 * 256                    # star_dist.hip grid_for(): at most 8192 blocks of 256 threads, the rest by the stride loop


# ---- label generators ----------------------------------------------------------------------------------------------------------------
def _coords(shape):
    return np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1)


def ellipses(shape, n, seed, rmin=3.0, rfrac=0.4, rcap=None):
    """n ellipses / ellipsoids, later ones painted over earlier ones, radii up to rfrac of the extent (and rcap)"""
    rs = np.random.RandomState(seed)
    lab = np.zeros(shape, np.int32)
    g = _coords(shape)
    for k in range(1, n + 1):
        c = np.array([rs.uniform(0, s) for s in shape])
        hi = np.array([max(rmin, rfrac * s) for s in shape])
        if rcap is not None:
            hi = np.minimum(hi, rcap)
        r = np.array([rs.uniform(min(rmin, h), h) for h in hi])
        lab[(((g - c) / r) ** 2).sum(-1) <= 1.0] = k
    return lab


def band(shape, axes, seed=0):
    """object 1 spans the FULL extent of every axis in `axes` (it reaches both borders there: the +inf of the first EDT pass) and is a
    slab in the middle of the others; object 2 is a small box beside it"""
    lab = np.zeros(shape, np.int32)
    sl = tuple(slice(None) if a in axes else slice(s // 3, max(s // 3 + 1, 2 * s // 3)) for a, s in enumerate(shape))
    lab[sl] = 1
    lab[tuple(slice(0, max(1, s // 5)) for s in shape)] = 2
    return lab


def one_other_pixel(shape, other, seed=0):
    """one object everywhere except ONE pixel, which is background (other = 0) or a second object (other = 2)"""
    rs = np.random.RandomState(seed)
    lab = np.ones(shape, np.int32)
    lab[tuple(int(rs.randint(0, s)) for s in shape)] = other
    return lab


def annulus(shape, gap=False):
    """a ring (with gap: a C) in the last two axes around the centre, a full-height tube in 3D; object 2 sits in the hole"""
    g = _coords(shape[-2:]).astype(np.float64)
    c = (np.array(shape[-2:]) - 1) / 2.0
    r = np.sqrt(((g - c) ** 2).sum(-1))
    ro = 0.45 * min(shape[-2:])
    m = (r <= ro) & (r >= 0.6 * ro)
    if gap:
        m &= ~((np.abs(g[..., 0] - c[0]) <= 0.12 * ro) & (g[..., 1] > c[1]))
    lab2 = np.where(m, 1, 0).astype(np.int32)
    lab2[r <= 0.25 * ro] = 2
    return np.broadcast_to(lab2, shape).copy()


def two_components(shape):
    """label 1 in two distant components at both ends of the last axis, object 2 between them"""
    lab = np.zeros(shape, np.int32)
    W = shape[-1]
    lab[..., : max(1, W // 6)] = 1
    lab[..., W - max(1, W // 6):] = 1
    lab[..., W // 2 - max(1, W // 10): W // 2 + max(1, W // 10)] = 2
    lab[tuple(slice(0, max(1, s // 4)) for s in shape[:-1])] = 0
    return lab


def checkerboard(shape):
    """1-pixel objects, every one its own id, on the black squares; background on the white ones"""
    g = _coords(shape).sum(-1)
    lab = np.zeros(shape, np.int32)
    m = g % 2 == 0
    lab[m] = np.arange(1, int(m.sum()) + 1)
    return lab


def cut_by_borders(shape, r=None):
    """a ball at every corner and at the middle of every edge / face of the image: objects cut by every border and every corner"""
    lab = np.zeros(shape, np.int32)
    g = _coords(shape).astype(np.float64)
    r = 0.22 * min(s for s in shape if s > 1) if r is None else r
    k = 0
    for pos in np.ndindex(*(3,) * len(shape)):
        if all(p == 1 for p in pos):
            continue
        k += 1
        c = np.array([(0, (s - 1) / 2.0, s - 1)[p] for p, s in zip(pos, shape)])
        lab[((g - c) ** 2).sum(-1) <= r * r] = k
    return lab


def voronoi(shape, n, seed):
    """every pixel belongs to its nearest seed point: a tiling with no background at all"""
    rs = np.random.RandomState(seed)
    pts = np.stack([rs.uniform(0, s, n) for s in shape], 1)
    g = _coords(shape).astype(np.float64)
    d = ((g[..., None, :] - pts) ** 2).sum(-1)
    return (d.argmin(-1) + 1).astype(np.int32)


def discs_2048(seed=11, n_small=5000, r_large=100):
    """2048 x 2048: many small discs (radius 3 - 8) and one large one (id 1, radius r_large)"""
    rs = np.random.RandomState(seed)
    S = 2048
    lab = np.zeros((S, S), np.int32)
    for k in range(2, n_small + 2):
        cy, cx, r = rs.uniform(0, S), rs.uniform(0, S), rs.uniform(3, 8)
        y0, y1, x0, x1 = max(0, int(cy - r - 1)), min(S, int(cy + r + 2)), max(0, int(cx - r - 1)), min(S, int(cx + r + 2))
        yy, xx = np.mgrid[y0:y1, x0:x1]
        lab[y0:y1, x0:x1][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k
    yy, xx = np.mgrid[0:S, 0:S]
    lab[(yy - 1000.3) ** 2 + (xx - 1100.6) ** 2 <= r_large * r_large] = 1
    return lab


# ---- edt_prob -------------------------------------------------------------------------------------------------------------------------
def edt_prob_box(lbl, anisotropy=None, ids=None, exhaustive=False):
    """stardist/utils.py:98-125 (_edt_prob_scipy) in float64 without scipy: per object, on its bounding box grown by one pixel where it does
    not touch the image border (the box the reference gives to scipy), the distance of every object pixel to the nearest pixel of the box
    that is not the object -- squared axis terms ((index difference) * sampling)^2 summed in axis order (scipy: dt *= sampling; dt * dt;
    np.add.reduce over the axis axis), sqrt, / (max + 1e-10), float32.  A constant positive image is padded with background.
    ids: compute these objects only (everything else stays 0).
    The search runs over the non-object pixels that have an object pixel as a face neighbour: the nearest non-object pixel q of an object
    pixel p always is one (the pixel one step from q towards p along an axis where they differ is strictly nearer to p in that axis term
    and equal in the others, so it is nearer, so it belongs to the object).  exhaustive=True searches every non-object pixel of the box
    instead (the CPU test compares the two)."""
    lbl = np.asarray(lbl)
    nd = lbl.ndim
    samp = np.ones(nd) if anisotropy is None else np.asarray(anisotropy, np.float64)
    constant = lbl.size > 0 and lbl.min() == lbl.max() and lbl.flat[0] > 0
    if constant:
        lbl = np.pad(lbl, ((1, 1),) * nd, mode="constant")
        warnings.warn("EDT of constant label image is ill-defined. (Assuming background around it.)")
    prob = np.zeros(lbl.shape, np.float32)
    todo = np.unique(lbl) if ids is None else np.asarray(ids)
    boxes = _boxes(lbl)
    for l in todo:
        l = int(l)
        if l <= 0 or l not in boxes:
            continue
        lo, hi = boxes[l]
        sl = tuple(slice(max(0, a - 1), min(s, b + 2)) for a, b, s in zip(lo, hi, lbl.shape))
        mask = lbl[sl] == l
        other = ~mask
        if not exhaustive:
            near = np.zeros_like(mask)
            for a in range(nd):
                m = np.moveaxis(mask, a, 0)
                n_ = np.moveaxis(near, a, 0)
                n_[1:] |= m[:-1]
                n_[:-1] |= m[1:]
            other &= near
        pin = np.argwhere(mask).astype(np.float64)
        pot = np.argwhere(other).astype(np.float64)
        d = np.full(len(pin), np.inf)
        if len(pot):
            step = max(1, int(3e6 // len(pot)))
            for a in range(0, len(pin), step):
                acc = None
                for k in range(nd):
                    t = (pin[a:a + step, None, k] - pot[None, :, k]) * samp[k]
                    t *= t
                    acc = t if acc is None else acc + t
                d[a:a + step] = np.sqrt(acc.min(axis=1))
        view = prob[sl]
        view[mask] = d / (d.max() + 1e-10)
    if constant:
        prob = prob[(slice(1, -1),) * nd].copy()
    return prob


def _boxes(lbl):
    """{id: (lo, hi)} inclusive bounding boxes of the positive ids (what scipy.ndimage.find_objects gives the reference)"""
    idx = np.flatnonzero(lbl.reshape(-1) > 0)
    if len(idx) == 0:
        return {}
    v = lbl.reshape(-1)[idx]
    order = np.argsort(v, kind="stable")
    v, idx = v[order], idx[order]
    cut = np.flatnonzero(np.diff(v)) + 1
    starts = np.concatenate(([0], cut))
    co = np.stack(np.unravel_index(idx, lbl.shape), 1)
    lo = np.minimum.reduceat(co, starts, axis=0)
    hi = np.maximum.reduceat(co, starts, axis=0)
    return {int(i): (tuple(a), tuple(b)) for i, a, b in zip(v[starts], lo, hi)}


# ---- star_dist ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _libm():
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for f in (m.cosf, m.sinf):
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
    return m


def dirs2d(n_rays):
    """the direction table of sd_star_dist2d_device (stardist2d.cpp:91-95): phi = k * (float)(2 pi / n_rays) in float, dy = cosf(phi),
    dx = sinf(phi) by the C library (numpy's own float32 sin / cos need not round like it) -> (dy, dx) float32 arrays"""
    m = _libm()
    st = np.float32((2 * np.pi) / n_rays)
    phi = [np.float32(np.float32(k) * st) for k in range(n_rays)]
    return (np.array([m.cosf(float(p)) for p in phi], np.float32), np.array([m.sinf(float(p)) for p in phi], np.float32))


def _as_u16(lbl):
    return np.asarray(lbl).astype(np.int64).astype(np.uint16)            # the cast of geom2d.py:31 / geom3d.py:19: ids wrap modulo 65536


def star_dist2d_np(lbl, n_rays, grid=(1, 1)):
    """c_star_dist (stardist2d.cpp:55-124) line by line in float32: x, y accumulate the float direction, the pixel is lrint(i * gy + x)
    (np.rint: round half to even), the ray stops outside the image or on another id, then the overshoot correction t_corr with separate
    multiply and add, dist = sqrtf(x * x + y * y).  Labels are read as uint16."""
    src = _as_u16(lbl)
    H, W = src.shape
    gy, gx = int(grid[0]), int(grid[1])
    sub = src[::gy, ::gx]
    out = np.zeros(sub.shape + (n_rays,), np.float32)
    fi, fj = np.nonzero(sub)
    val = sub[fi, fj]
    bi, bj = (fi * gy).astype(np.float32), (fj * gx).astype(np.float32)
    cos, sin = dirs2d(n_rays)
    one, half = np.float32(1), np.float32(0.5)
    for k in range(n_rays):
        dy, dx = cos[k], sin[k]
        t_corr = half / max(abs(dx), abs(dy))                             # :108
        cx, cy = (t_corr - one) * dx, (t_corr - one) * dy                 # :109-110, rounded products
        idx = np.arange(len(val))
        x = np.zeros(len(val), np.float32)
        y = np.zeros(len(val), np.float32)
        b_i, b_j, v = bi, bj, val
        while len(idx):
            x = x + dx
            y = y + dy
            ii = np.rint(b_i + x).astype(np.int64)
            jj = np.rint(b_j + y).astype(np.int64)
            inside = (ii >= 0) & (ii < H) & (jj >= 0) & (jj < W)
            stop = ~inside
            w = np.flatnonzero(inside)
            stop[w] = src[ii[w], jj[w]] != v[w]
            if stop.any():
                xs, ys = x[stop] + cx, y[stop] + cy
                out[fi[idx[stop]], fj[idx[stop]], k] = np.sqrt(xs * xs + ys * ys)
                go = ~stop
                idx, x, y, b_i, b_j, v = idx[go], x[go], y[go], b_i[go], b_j[go], v[go]
    assert out.dtype == np.float32
    return out


def star_dist3d_np(lbl, rays_vertices, grid=(1, 1, 1)):
    """c_star_dist3d (stardist3d.cpp:245-346) in float32: as 2D on (z, y, x) with the given (dz, dy, dx) float32 rays; the distance is
    sqrt of the INTEGER sum of the squared rounded offsets, taken in double (:317-320), stored as float"""
    src = _as_u16(lbl)
    Z, Y, X = src.shape
    gz, gy, gx = (int(g) for g in grid)
    V = np.asarray(rays_vertices)
    rz, ry, rx = (V[:, a].astype(np.float32) for a in range(3))
    sub = src[::gz, ::gy, ::gx]
    out = np.zeros(sub.shape + (len(V),), np.float32)
    fi, fj, fk = np.nonzero(sub)
    val = sub[fi, fj, fk]
    bi, bj, bk = (fi * gz).astype(np.float32), (fj * gy).astype(np.float32), (fk * gx).astype(np.float32)
    for n in range(len(V)):
        dz, dy, dx = rz[n], ry[n], rx[n]
        assert dz != 0 or dy != 0 or dx != 0
        idx = np.arange(len(val))
        x, y, z = (np.zeros(len(val), np.float32) for _ in range(3))
        b_i, b_j, b_k, v = bi, bj, bk, val
        while len(idx):
            x = x + dx
            y = y + dy
            z = z + dz
            ii, jj, kk = np.rint(b_i + z).astype(np.int64), np.rint(b_j + y).astype(np.int64), np.rint(b_k + x).astype(np.int64)
            inside = (ii >= 0) & (ii < Z) & (jj >= 0) & (jj < Y) & (kk >= 0) & (kk < X)
            stop = ~inside
            w = np.flatnonzero(inside)
            stop[w] = src[ii[w], jj[w], kk[w]] != v[w]
            if stop.any():
                x2, y2, z2 = (np.rint(t[stop]).astype(np.int64) for t in (x, y, z))
                s = idx[stop]
                out[fi[s], fj[s], fk[s], n] = np.sqrt((x2 * x2 + y2 * y2 + z2 * z2).astype(np.float64)).astype(np.float32)
                go = ~stop
                idx, x, y, z, b_i, b_j, b_k, v = idx[go], x[go], y[go], z[go], b_i[go], b_j[go], b_k[go], v[go]
    return out


class Rays(object):
    """what star_dist3D and targets_device3d use of a Rays_* object: .vertices (n, 3) in (z, y, x) and len()"""

    def __init__(self, vertices):
        self.vertices = np.asarray(vertices, np.float64)

    def __len__(self):
        return len(self.vertices)


def lattice_rays():
    """the 124 non-zero directions with components in {0, +-0.5, +-1} (not normalised: every partial sum along a ray is exact, and the
    half steps land on .5 coordinates where lrint's round-half-even decides the voxel)"""
    c = (-1.0, -0.5, 0.0, 0.5, 1.0)
    return Rays([(a, b, d) for a in c for b in c for d in c if (a, b, d) != (0.0, 0.0, 0.0)])


def golden_spiral(n):
    from stardist_amd.rays3d import Rays_GoldenSpiral
    return Rays_GoldenSpiral(n)


# ---- the generators' target lines -----------------------------------------------------------------------------------------------------
def targets_ref(Y, grid, n_rays=None, rays=None, anisotropy=None, edt=edt_prob_box, sd2=star_dist2d_np, sd3=star_dist3d_np):
    """model2d.py:64-103 / model3d.py:69-104 (no shape completion, no classes): negative labels ON THE GRID switch the clipping of the
    whole batch on; 2D takes the distance transform of the sub-sampled labels, 3D sub-samples the transform of the full volume (with
    anisotropy); dist_and_mask = [dist | prob] before prob is set to -1 at the negative labels.  -> prob (B, ...), dtm (B, ..., R + 1)"""
    Y = [np.asarray(y) for y in Y]
    nd = Y[0].ndim
    ss = tuple(slice(0, None, int(g)) for g in grid)
    neg = [y[ss] < 0 for y in Y]
    has_neg = any(m.any() for m in neg)
    if has_neg:
        Y = [np.maximum(y, 0) for y in Y]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if nd == 2:
            prob = np.stack([edt(y[ss]) for y in Y])
            dist = np.stack([sd2(y, n_rays, grid) for y in Y])
        else:
            prob = np.stack([edt(y, anisotropy)[ss] for y in Y])
            dist = np.stack([sd3(y, rays.vertices, grid) for y in Y])
    dtm = np.concatenate([dist, prob[..., None]], axis=-1).astype(np.float32)
    prob = prob.copy()
    if has_neg:
        prob[np.stack(neg)] = -1
    return prob, dtm


def batch_branch(y, grid, nd):
    """which way one item of a batch goes, in the reference's terms: the array that edt_prob is given (2D: the sub-sampled patch,
    model2d.py:71; 3D: the full patch, model3d.py:86, negative ids clipped only if the batch clips) is 'constant' if it is one positive id
    (utils.py:104), has 'sparse' ids if its largest id exceeds 4 * size + 1024 (the documented limit of the per-id table), is 'empty'
    if it has no positive id, else 'plain'"""
    a = np.asarray(y)
    if nd == 2:
        a = a[tuple(slice(0, None, int(g)) for g in grid)]
    if a.min() == a.max() and a.flat[0] > 0:
        return "constant"
    if a.max() > 4 * a.size + 1024:
        return "sparse"
    return "empty" if a.max() <= 0 else "plain"


# ---- case lists -----------------------------------------------------------------------------------------------------------------------
def _case(id, make, **kw):
    d = dict(id=id, make=make)
    d.update(kw)
    return d


@functools.lru_cache(None)
def labels(id):
    """the label image (or the list of them, for a batch) of case `id`"""
    c = BY_ID[id]
    return c["make"]()


def _edt_cases_2d():
    S, A = (61, 77), [None, (2.0, 0.5), (1.9, 0.7)]
    gens = [("ellipses", lambda: ellipses(S, 9, 1)), ("band-y", lambda: band(S, (0,))), ("band-x", lambda: band(S, (1,))),
            ("one-bg", lambda: one_other_pixel(S, 0, 2)), ("one-obj2", lambda: one_other_pixel(S, 2, 3)), ("annulus", lambda: annulus(S)),
            ("cshape", lambda: annulus(S, gap=True)), ("twocomp", lambda: two_components(S)), ("checker", lambda: checkerboard((24, 31))),
            ("borders", lambda: cut_by_borders(S)), ("voronoi", lambda: voronoi(S, 14, 4))]
    out = [_case("edt2-%s-a%d" % (n, i), f, aniso=a) for n, f in gens for i, a in enumerate(A) if i != 1 or n in ("ellipses", "band-x")]
    out += [_case("edt2-256-a%d" % i, lambda: ellipses((256, 256), 10, 5), aniso=a) for i, a in ((0, None), (2, (1.09, 7.14)))]
    out += [_case("edt2-256-voronoi", lambda: voronoi((256, 256), 9, 6), aniso=None),
            _case("edt2-256-band", lambda: band((256, 256), (1,)), aniso=(1.9, 1.1)),
            _case("edt2-x1", lambda: ellipses((57, 1), 4, 7, rmin=2.0), aniso=(1.1, 0.7)),
            _case("edt2-y1", lambda: ellipses((1, 57), 4, 8, rmin=2.0), aniso=(1.1, 0.7)),
            _case("edt2-const", lambda: np.full((9, 12), 3, np.int32), aniso=(1.9, 0.7)),
            _case("edt2-2048", lambda: discs_2048(), aniso=None, ids=(1,) + tuple(int(v) for v in np.random.RandomState(12).randint(2, 5002, 40)))]
    return out


def _edt_cases_3d():
    S, A = (14, 30, 33), [None, (2.0, 1.0, 0.5), (1.9, 1.1, 0.7), (7.14, 1.0, 1.09)]
    gens = [("ellipses", lambda: ellipses(S, 8, 21, rmin=2.0)), ("band-z", lambda: band(S, (0,))), ("band-zx", lambda: band(S, (0, 2))),
            ("band-yx", lambda: band(S, (1, 2))), ("one-bg", lambda: one_other_pixel(S, 0, 22)), ("one-obj2", lambda: one_other_pixel(S, 2, 23)),
            ("annulus", lambda: annulus(S)), ("cshape", lambda: annulus(S, gap=True)), ("twocomp", lambda: two_components(S)),
            ("checker", lambda: checkerboard((5, 8, 9))), ("borders", lambda: cut_by_borders(S, r=5.0)), ("voronoi", lambda: voronoi(S, 10, 24))]
    out = [_case("edt3-%s-a%d" % (n, i), f, aniso=a) for n, f in gens for i, a in enumerate(A)
           if i in (0, 2) or n in ("ellipses", "band-zx", "voronoi")]
    out += [_case("edt3-train-a%d" % i, lambda: _vol_train(), aniso=a) for i, a in ((0, None), (3, (7.14, 1.0, 1.09)))]
    out += [_case("edt3-z1", lambda: ellipses((1, 33, 40), 6, 25), aniso=(1.9, 1.1, 0.7)),
            _case("edt3-y1", lambda: ellipses((30, 1, 25), 4, 26, rmin=2.0), aniso=(1.9, 1.1, 0.7)),
            _case("edt3-x1", lambda: ellipses((30, 25, 1), 4, 27, rmin=2.0), aniso=(1.9, 1.1, 0.7)),
            _case("edt3-const", lambda: np.full((4, 5, 6), 2, np.int32), aniso=(1.9, 1.1, 0.7))]
    return out


def _vol_train():
    """48 x 96 x 96, the 3D demo's training patch: ellipsoids of radius <= 20 and a slab that spans z and x"""
    lab = ellipses((48, 96, 96), 7, 31, rmin=6.0, rcap=np.array([14.0, 20.0, 20.0]))
    lab[:, 40:46, :] = 8
    return lab


def _wide_ids():
    """ids 1, 65535, 65536, 65537 and 131073 in touching columns: as uint16 they are 1, 65535, 0, 1, 1"""
    lab = np.zeros((40, 60), np.int32)
    for k, v in enumerate((1, 65537, 65535, 65536, 131073, 1)):
        lab[4:36, 6 + 8 * k: 14 + 8 * k] = v
    return lab


def _sd_cases_2d():
    odd = lambda: ellipses((37, 45), 7, 41, rfrac=0.3)                    # noqa: E731
    out = [_case("sd2-r%d" % r, odd, n_rays=r, grid=(1, 1), public=r >= 3) for r in (1, 3, 4, 6, 12, 17, 32, 64, 300)]
    out += [_case("sd2-g%d%d" % g, odd, n_rays=8, grid=g, public=g != (3, 1)) for g in ((2, 2), (1, 4), (3, 1), (4, 4))]
    out += [_case("sd2-256", lambda: ellipses((256, 256), 10, 5), n_rays=32, grid=(1, 1), public=True),
            _case("sd2-256-voronoi-g22", lambda: voronoi((256, 256), 9, 6), n_rays=32, grid=(2, 2), public=True),
            _case("sd2-2048", lambda: discs_2048(), n_rays=32, grid=(1, 1), public=True),
            _case("sd2-h1", lambda: ellipses((1, 57), 4, 8, rmin=2.0), n_rays=12, grid=(1, 1), public=True),
            _case("sd2-w1", lambda: ellipses((57, 1), 4, 7, rmin=2.0), n_rays=12, grid=(1, 2), public=True),
            _case("sd2-borders", lambda: cut_by_borders((61, 77)), n_rays=16, grid=(1, 1), public=True),
            _case("sd2-checker", lambda: checkerboard((24, 31)), n_rays=12, grid=(1, 1), public=True),
            _case("sd2-wide-ids", _wide_ids, n_rays=16, grid=(1, 1), public=True)]
    return out


def _sd_cases_3d():
    S = (14, 30, 33)
    return [_case("sd3-train", _vol_train, rays=lambda: golden_spiral(96), grid=(1, 2, 2)),
            _case("sd3-faces", lambda: cut_by_borders(S, r=5.0), rays=lambda: golden_spiral(24), grid=(1, 1, 1)),
            _case("sd3-lattice", lambda: ellipses(S, 8, 21, rmin=2.0), rays=lattice_rays, grid=(1, 1, 1)),
            _case("sd3-lattice-g212", lambda: voronoi(S, 10, 24), rays=lattice_rays, grid=(2, 1, 2)),
            _case("sd3-z1", lambda: ellipses((1, 33, 40), 6, 25), rays=lambda: golden_spiral(16), grid=(1, 1, 1)),
            _case("sd3-wide-ids", lambda: np.broadcast_to(_wide_ids(), (3, 40, 60)).copy(), rays=lambda: golden_spiral(12), grid=(1, 1, 1))]


def _batch_items(shape, seed, rcap=None):
    """the patches the batches mix, by name"""
    nd = len(shape)
    plain = ellipses(shape, 6, seed, rfrac=0.3, rcap=rcap)
    sparse = np.where(plain > 0, plain.astype(np.int64) * 1000003, 0)      # ids far beyond 4 * size + 1024, below 2^31
    neg_on = ellipses(shape, 5, seed + 1, rfrac=0.3, rcap=rcap)
    neg_on[tuple(slice(4, 9) for _ in shape)] = -1                          # a block: covers grid points of every grid used here
    neg_off = ellipses(shape, 5, seed + 2, rfrac=0.3, rcap=rcap)
    neg_off[(slice(None),) * (nd - 2) + (slice(1, None, 8), slice(1, None, 8))] = -1     # odd rows and columns only
    return dict(plain=plain, zero=np.zeros(shape, np.int32), const=np.full(shape, 7, np.int32), sparse=sparse, neg_on=neg_on,
                neg_off=neg_off, other=voronoi(shape, 5, seed + 3), band=band(shape, (nd - 1,)))


def _batch(shape, names, dtypes, seed, rcap=None):
    it = _batch_items(shape, seed, rcap)
    return [it[n].astype(dt) for n, dt in zip(names, dtypes)]


def _batch_cases_2d():
    S = (72, 88)
    i32, i64, u16 = np.int32, np.int64, np.uint16
    mk = lambda names, dts, seed: (lambda: _batch(S, names, dts, seed))    # noqa: E731
    return [_case("b2-mixed-g11", mk(("plain", "zero", "const", "sparse"), (u16, i32, i32, i64), 51), grid=(1, 1), n_rays=32,
                  want=("plain", "empty", "constant", "sparse")),
            _case("b2-mixed-g22", mk(("const", "plain", "zero", "sparse"), (i64,) * 4, 52), grid=(2, 2), n_rays=16,
                  want=("constant", "plain", "empty", "sparse")),
            _case("b2-negon-g24", mk(("plain", "neg_on", "zero", "other"), (i32,) * 4, 53), grid=(2, 4), n_rays=8,
                  want=("plain", "plain", "empty", "plain")),
            _case("b2-negoff-g22", mk(("neg_off", "band", "const"), (i32,) * 3, 54), grid=(2, 2), n_rays=32,
                  want=("plain", "plain", "constant")),
            _case("b2-negoff-g11-clips", mk(("neg_off", "plain", "zero"), (i64, i64, i64), 55), grid=(1, 1), n_rays=8,
                  want=("plain", "plain", "empty")),
            _case("b2-wide-ids", lambda: [_wide_ids(), np.zeros((40, 60), np.int32), ellipses((40, 60), 5, 56, rfrac=0.3)], grid=(1, 1),
                  n_rays=16, want=("sparse", "empty", "plain")),                    # ids that collide as uint16, in a batch
            _case("b2-256", lambda: [ellipses((256, 256), 10, 5), np.zeros((256, 256), np.int32), voronoi((256, 256), 9, 6)], grid=(1, 1),
                  n_rays=32, want=("plain", "empty", "plain"))]


def _batch_cases_3d():
    S = (12, 24, 32)
    i32, i64, u16 = np.int32, np.int64, np.uint16
    mk = lambda names, dts, seed: (lambda: _batch(S, names, dts, seed, rcap=7.0))    # noqa: E731
    gs = lambda: golden_spiral(16)                                                   # noqa: E731
    return [_case("b3-mixed-g111", mk(("plain", "zero", "const", "sparse"), (u16, i32, i32, i64), 61), grid=(1, 1, 1), rays=gs, aniso=None,
                  want=("plain", "empty", "constant", "sparse")),
            _case("b3-mixed-g122-aniso", mk(("const", "plain", "sparse", "zero"), (i64,) * 4, 62), grid=(1, 2, 2), rays=gs,
                  aniso=(1.9, 1.1, 0.7), want=("constant", "plain", "sparse", "empty")),
            _case("b3-negon-g222", mk(("plain", "neg_on", "other"), (i32,) * 3, 63), grid=(2, 2, 2), rays=gs, aniso=(2.0, 1.0, 1.0),
                  want=("plain", "plain", "plain")),
            _case("b3-negoff-g122", mk(("neg_off", "band", "zero", "const"), (i32,) * 4, 64), grid=(1, 2, 2), rays=gs, aniso=(7.14, 1.0, 1.09),
                  want=("plain", "plain", "empty", "constant")),
            _case("b3-plain-order", mk(("plain", "other", "band"), (i32,) * 3, 65), grid=(1, 1, 1), rays=lattice_rays, aniso=None,
                  want=("plain", "plain", "plain"))]


EDT2D, EDT3D, SD2D, SD3D, BATCH2D, BATCH3D = (_edt_cases_2d(), _edt_cases_3d(), _sd_cases_2d(), _sd_cases_3d(), _batch_cases_2d(),
                                              _batch_cases_3d())
BY_ID = {c["id"]: c for L in (EDT2D, EDT3D, SD2D, SD3D, BATCH2D, BATCH3D) for c in L}
assert len(BY_ID) == sum(len(L) for L in (EDT2D, EDT3D, SD2D, SD3D, BATCH2D, BATCH3D))


def ids(cases):
    return [c["id"] for c in cases]


@functools.lru_cache(None)
def edt_want(id):
    c = BY_ID[id]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return edt_prob_box(labels(id), c["aniso"], ids=c.get("ids"))


@functools.lru_cache(None)
def sd_want(id):
    c = BY_ID[id]
    if "n_rays" in c:
        return star_dist2d_np(labels(id), c["n_rays"], c["grid"])
    return star_dist3d_np(labels(id), c["rays"]().vertices, c["grid"])


@functools.lru_cache(None)
def batch_want(id):
    c = BY_ID[id]
    if "n_rays" in c:
        return targets_ref(labels(id), c["grid"], n_rays=c["n_rays"])
    return targets_ref(labels(id), c["grid"], rays=c["rays"](), anisotropy=c["aniso"])


def describe(got, want, lbl=None, k=5):
    """count, first indices with got / want (and the object id) of a failed exact comparison"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shape %s != %s" % (got.shape, want.shape)
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    rows = []
    for ix in bad[:k]:
        ix = tuple(int(v) for v in ix)
        oid = "" if lbl is None else " id=%s" % (np.asarray(lbl)[ix[:np.asarray(lbl).ndim]],)
        rows.append("%s got %r want %r%s" % (ix, float(got[ix]), float(want[ix]), oid))
    return "%d of %d differ (%d NaN): %s" % (len(bad), got.size, int(np.isnan(got).sum()), "; ".join(rows))
