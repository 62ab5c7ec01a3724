"""Spot detection with a host route and a device route: gaussian_filter (scipy's, bit for bit),
difference_of_gaussians, peak_local_max (a definition of our own that equals scikit-image 0.18.3 wherever that is well defined) and
detect_spots, their composition.  Routing is stardist_amd/_route.py's; the kernels are csrc/spots.hip, the
per-element rules csrc/spots.h.  The public names are re-exported by stardist_amd.utils."""
import ctypes
import itertools
import math

import numpy as np

from . import _route as R
from ._route import _DEVICE_DTYPE_CODE
from .lib import _native as N

# csrc/spots.h
GAUSSIAN_MAX_RADIUS = 512
GAUSSIAN_LDS_RADIUS = 80          # a pass along an axis that is not the last keeps its tile in LDS up to this radius
PEAK_MAX_DISTANCE = 2 ** 20
_PEAK_LDS_BYTES = 48 * 1024
_MAX_PIXELS = 2 ** 32 - 1
_DTYPES = ("uint8", "uint16", "float32")


def peak_window_in_lds(ndim, d):
    """whether the device route of peak_local_max keeps a tile's halo in LDS for min_distance d (one value per axis): tiles are
    1 x 16 x 64 for a 2D image and 4 x 4 x 64 for a 3D one, and (t + 2 d) floats per axis must fit in 48 KiB"""
    t = (1, 16, 64) if ndim == 2 else (4, 4, 64)
    d = (0,) * (3 - len(d)) + tuple(d)
    return math.prod(a + 2 * b for a, b in zip(t, d)) * 4 <= _PEAK_LDS_BYTES


# ----------------------------------------------------------------------------- arguments

def _image(img, who, device):
    img, is_t, on_device = R.classify(img, device)
    name = str(img.dtype)[6:] if is_t else img.dtype.name
    if name not in _DTYPES:
        raise TypeError("%s: the image must be uint8, uint16 or float32, got %s" % (who, name))
    nd = len(img.shape)
    if nd not in (2, 3):
        raise ValueError("%s: the image must be 2D or 3D, got %d axes" % (who, nd))
    if math.prod(int(n) for n in img.shape) > _MAX_PIXELS:
        raise ValueError("%s: more than 2^32 - 1 pixels" % who)
    return img, is_t, on_device


def _real(v, who, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or math.isnan(v):
        raise ValueError("%s: %s must be a real number, got %r" % (who, what, v))
    return float(v)


def _sigmas(sigma, nd, who, what="sigma"):
    try:
        s = np.asarray(sigma, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: %s must be a number or one per axis, got %r" % (who, what, sigma))
    if s.ndim == 0:
        s = np.full(nd, float(s))
    if s.shape != (nd,) or not (np.isfinite(s).all() and (s >= 0).all()):
        raise ValueError("%s: %s must be a finite number >= 0 or one per axis (%d), got %r" % (who, what, nd, sigma))
    return [float(v) for v in s]


def _truncate(truncate, who):
    t = _real(truncate, who, "truncate")
    if not (t > 0 and math.isfinite(t)):
        raise ValueError("%s: truncate must be positive and finite, got %r" % (who, truncate))
    return t


def gaussian_weights(sigma, radius):
    """the 2 radius + 1 weights of scipy.ndimage's Gaussian window (its _gaussian_kernel1d of order 0, restated), float64"""
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def _gaussian_plan(sig, truncate):
    """[(axis, radius, weights)] of the axes that are not skipped"""
    plan = []
    for ax, s in enumerate(sig):
        if s <= 1e-15:
            continue
        r = int(truncate * s + 0.5)
        plan.append((ax, r, gaussian_weights(s, r)))
    return plan


# ----------------------------------------------------------------------------- Gaussian

def _gaussian_host(a, plan):
    cur = a
    with np.errstate(invalid="ignore", over="ignore"):
        for ax, r, w in plan:
            n = cur.shape[ax]
            src = np.moveaxis(cur, ax, -1)
            i = np.arange(-r, n + r) % (2 * n)
            ext = src[..., np.where(i < n, i, 2 * n - 1 - i)].astype(np.float64)
            tmp = ext[..., r:r + n] * w[r]
            for j in range(r, 0, -1):                                       # farthest taps first, every operation rounded
                tmp += (ext[..., r - j:r - j + n] + ext[..., r + j:r + j + n]) * w[r - j]
            cur = np.moveaxis(tmp.astype(np.float32), -1, ax)
        return np.ascontiguousarray(cur) if plan else a.astype(np.float32)


def _gaussian_device(t, plan):
    """sd_gaussian_filter_device on the contiguous device tensor t: a new float32 tensor there"""
    import torch
    N.require_device()
    nd = t.dim()
    out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    if t.numel() == 0:
        return out
    work = torch.empty_like(out) if len(plan) > 1 else None
    radius = np.full(3, -1, np.int32)
    for ax, r, _ in plan:
        radius[ax + 3 - nd] = r
    w = torch.as_tensor(np.concatenate([w for _, _, w in plan]), device=t.device) if plan else None
    N.dcall(t, "sd_gaussian_filter_device", R.ptr(t), _DEVICE_DTYPE_CODE[str(t.dtype)], nd, *R.zyx(t.shape), N.ptr(radius), R.opt_ptr(w),
            R.ptr(out), R.opt_ptr(work))
    return out


def _gaussian(img, is_t, on_device, device, plans):
    """the Gaussians of `plans` of one image, like the input: the image travels once"""
    if on_device and all(r <= GAUSSIAN_MAX_RADIUS for plan in plans for _, r, _ in plan):
        t = R.to_device_tensor(img, device)
        return [_gaussian_device(t, plan) for plan in plans], True
    if is_t:
        return [R.via_host(_gaussian_host, img, plan, to=device) for plan in plans], False
    return [_gaussian_host(img, plan) for plan in plans], False


def _like_input(outs, img, from_device):
    if from_device and isinstance(img, np.ndarray):
        from .utils import to_host_many
        return to_host_many(outs)
    return outs


def gaussian_filter(img, sigma, *, truncate=4.0, device=None):
    """scipy.ndimage.gaussian_filter(img, sigma, output=np.float32, mode="reflect", truncate=truncate), bit for bit, of a 2D or 3D
    uint8, uint16 or float32 image (other dtypes raise TypeError, more than 2^32 - 1 pixels ValueError).  NaN positions are scipy's;
    a NaN's payload and sign are the hardware's.  Other boundary modes and derivative orders are not offered.

    The rule, which both routes follow.  sigma is a number or one per axis; axes are filtered in the order 0, 1, 2 and an axis with
    sigma <= 1e-15 is skipped (all skipped: the input cast to float32).  r = int(truncate * sigma + 0.5); the weights are
    w = phi / phi.sum() with phi = exp(-0.5 / sigma^2 * x^2), x = -r .. r, in float64 in numpy (gaussian_weights).  One output
    element of a line: tmp = in[l] * w[r], then for j = r .. 1: tmp += (in[l - j] + in[l + j]) * w[r - j], in float64, every
    operation rounded, no fused multiply-add; the result is float32(tmp).  An index outside the line is reflected with period 2n
    (i mod 2n, then i < n ? i : 2n - 1 - i).  The first pass reads the image's dtype; between axes the image is float32.

    Routing: DESIGN.md section 3p -- numpy without device= runs the numpy code, a tensor on a HIP device or device= the kernel
    (csrc/spots.hip: one pass per axis, the line segment with its halo in LDS, always along the last axis and up to r = 80 along
    another, read from global memory beyond; the input is not written); the result comes back like the input.  A radius beyond
    512 takes the host code whatever the route."""
    who = "gaussian_filter"
    img, is_t, on_device = _image(img, who, device)
    plan = _gaussian_plan(_sigmas(sigma, len(img.shape), who), _truncate(truncate, who))
    outs, from_device = _gaussian(img, is_t, on_device, device, [plan])
    return _like_input(outs, img, from_device)[0]


def _dog(img, is_t, on_device, device, low_sigma, high_sigma, truncate, who):
    nd = len(img.shape)
    low = _sigmas(low_sigma, nd, who, "low_sigma")
    high = [1.6 * s for s in low] if high_sigma is None else _sigmas(high_sigma, nd, who, "high_sigma")
    t = _truncate(truncate, who)
    (a, b), from_device = _gaussian(img, is_t, on_device, device, [_gaussian_plan(low, t), _gaussian_plan(high, t)])
    with np.errstate(invalid="ignore", over="ignore"):
        return a - b, from_device


def difference_of_gaussians(img, low_sigma, high_sigma=None, *, truncate=4.0, device=None):
    """gaussian_filter(img, low_sigma) - gaussian_filter(img, high_sigma), one float32 subtraction per pixel; high_sigma defaults to
    1.6 * low_sigma per axis (in float64).  This is the project's own definition: scikit-image's function of this name rescales
    integer images and uses another boundary mode.  Routing and the dtypes are gaussian_filter's; the image travels once."""
    who = "difference_of_gaussians"
    img, is_t, on_device = _image(img, who, device)
    out, from_device = _dog(img, is_t, on_device, device, low_sigma, high_sigma, truncate, who)
    return _like_input([out], img, from_device)[0]


# ----------------------------------------------------------------------------- peaks

def _count_arg(v, who, what):
    if v is None or (isinstance(v, float) and v == math.inf):
        return None
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 0:
        raise ValueError("%s: %s must be an integer >= 0 or None, got %r" % (who, what, v))
    return int(v)


def _per_axis_ints(v, nd, who, what):
    if isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)):
        v = (int(v),) * nd
    else:
        try:
            v = tuple(v)
        except TypeError:
            raise ValueError("%s: %s must be an integer or one per axis, got %r" % (who, what, v))
    if len(v) != nd or any(isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) for x in v):
        raise ValueError("%s: %s must be an integer or one per axis (%d), got %r" % (who, what, nd, v))
    if any(x < 0 for x in v):
        raise ValueError("%s: %s must not be negative, got %r" % (who, what, v))
    return tuple(int(x) for x in v)


def _peak_args(shape, min_distance, threshold_abs, threshold_rel, exclude_border, num_peaks, num_peaks_per_label):
    who = "peak_local_max"
    nd = len(shape)
    d = _per_axis_ints(min_distance, nd, who, "min_distance")
    if isinstance(exclude_border, (bool, np.bool_)):
        b = d if exclude_border else (0,) * nd
    else:
        b = _per_axis_ints(exclude_border, nd, who, "exclude_border")
    d = tuple(min(x, max(int(n) - 1, 0)) for x, n in zip(d, shape))         # a wider window holds no more pixels
    if max(d, default=0) > PEAK_MAX_DISTANCE:
        raise ValueError("%s: min_distance beyond 2^20 on an axis that long" % who)
    t_abs = None if threshold_abs is None else _real(threshold_abs, who, "threshold_abs")
    t_rel = None if threshold_rel is None else _real(threshold_rel, who, "threshold_rel")
    return d, b, t_abs, t_rel, _count_arg(num_peaks, who, "num_peaks"), _count_arg(num_peaks_per_label, who, "num_peaks_per_label")


def _labels_host(labels, shape):
    who = "peak_local_max"
    lab = labels.cpu().numpy() if R.is_torch(labels) else np.asarray(labels)
    if lab.dtype.kind not in "iu" or tuple(lab.shape) != tuple(shape):
        raise ValueError("%s: labels must be an integer image of the image's shape" % who)
    if lab.size and (int(lab.min()) < 0 or int(lab.max()) > 2 ** 31 - 1):
        raise ValueError("%s: label ids must be in 0 .. 2^31 - 1" % who)
    return lab


def _labels_device(labels, shape, device):
    import torch
    who = "peak_local_max"
    if not R.is_torch(labels):
        return R.to_device_tensor(_labels_host(labels, shape).astype(np.int32), device)
    if labels.dtype.is_floating_point or labels.dtype == torch.bool or tuple(labels.shape) != tuple(shape):
        raise ValueError("%s: labels must be an integer image of the image's shape" % who)
    t = R.to_device_tensor(labels, device)
    if t.numel():
        lo, hi = (int(v) for v in torch.aminmax(t if t.dtype != torch.uint16 else t.to(torch.int32)))
        if lo < 0 or hi > 2 ** 31 - 1:
            raise ValueError("%s: label ids must be in 0 .. 2^31 - 1" % who)
    return t.to(torch.int32).contiguous()


def _empty_table(nd, dtype):
    return np.zeros((0, nd), np.int64), np.zeros(0, dtype), np.zeros(0, np.int32)


def _peaks_host(a, lab, d, b, t_abs, t_rel, per_label, num_peaks):
    """(coords, values, labels) by the definition, in numpy: the candidates that pass rules 1 - 3, then one vector comparison per
    offset of the window over those that are still unbeaten"""
    nd, shape = a.ndim, a.shape
    if a.size == 0:
        return _empty_table(nd, a.dtype)
    vf = a.astype(np.float64).ravel()
    valid = ~np.isnan(vf)
    if not valid.any():
        return _empty_table(nd, a.dtype)
    lo, hi = vf[valid].min(), vf[valid].max()
    thr = lo if t_abs is None else np.float64(t_abs)
    if t_rel is not None:
        thr = max(thr, np.float64(t_rel) * hi)
    with np.errstate(invalid="ignore"):
        cand = (vf > thr).reshape(shape)
    for ax in range(nd):
        band = [slice(None)] * nd
        w = min(b[ax], shape[ax])
        band[ax] = slice(0, w)
        cand[tuple(band)] = False
        band[ax] = slice(shape[ax] - w, shape[ax])
        cand[tuple(band)] = False
    labf = None
    if lab is not None:
        labf = lab.ravel()
        cand &= lab != 0
    idx = np.flatnonzero(cand)
    pos = np.stack(np.unravel_index(idx, shape), axis=1) if len(idx) else np.zeros((0, nd), np.int64)
    v = vf[idx]
    own = labf[idx] if labf is not None else None
    strides = np.asarray([math.prod(shape[ax + 1:]) for ax in range(nd)], np.int64)
    extent = np.asarray(shape, np.int64)
    offsets = sorted(itertools.product(*[range(-x, x + 1) for x in d]), key=lambda o: max(abs(c) for c in o))
    for step, off in enumerate(offsets):
        if not any(off) or not len(idx):
            continue
        q = pos + np.asarray(off, np.int64)
        inside = ((q >= 0) & (q < extent)).all(axis=1)
        qi = np.where(inside, q @ strides, 0)
        u = vf[qi]
        beats = inside & ((u > v) | ((u == v) & (qi < idx)))
        if own is not None:
            beats &= labf[qi] == own
        if beats.any():
            keep = ~beats
            idx, pos, v = idx[keep], pos[keep], v[keep]
            own = own[keep] if own is not None else None
    order = np.lexsort((idx, -v))
    idx = idx[order]
    if per_label is not None and labf is not None:
        group = labf[idx]
        o = np.argsort(group, kind="stable")
        g = group[o]
        rank = np.arange(len(g)) - np.searchsorted(g, g, side="left")
        keep = np.zeros(len(g), bool)
        keep[o] = rank < per_label
        idx = idx[keep]
    if num_peaks is not None:
        idx = idx[:num_peaks]
    coords = np.stack(np.unravel_index(idx, shape), axis=1).astype(np.int64) if len(idx) else np.zeros((0, nd), np.int64)
    return coords, a.ravel()[idx], (labf[idx].astype(np.int32) if labf is not None else np.zeros(len(idx), np.int32))


def _peaks_device(t, lab, d, b, t_abs, t_rel, per_label, num_peaks):
    """(coords, values, labels) as tensors on t's device: sd_peak_local_max_device, again with room for all where the first guess of
    the number of peaks was too small, then sd_peaks_emit_device"""
    import torch
    N.require_device()
    nd, dev = t.dim(), t.device
    count = int(t.numel())
    coords = lambda n: torch.empty((n, nd), dtype=torch.int64, device=dev)
    if count == 0:
        return coords(0), torch.empty(0, dtype=t.dtype, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    code = _DEVICE_DTYPE_CODE[str(t.dtype)]
    dist = np.asarray((0,) * (3 - nd) + tuple(d), np.int32)
    border = np.asarray((0,) * (3 - nd) + tuple(b), np.int64)
    cap = min(count, max(65536, count // 8 if count <= 2 ** 26 else count // 64))
    found = (ctypes.c_longlong * 2)(0, 0)
    head = (R.ptr(t), code, nd) + tuple(R.zyx(t.shape)) + (R.opt_ptr(lab),)
    while True:
        keys = torch.empty(cap, dtype=torch.int64, device=dev)
        N.dcall(t, "sd_peak_local_max_device", *head, N.ptr(dist), N.ptr(border), int(t_abs is not None),
                ctypes.c_double(0.0 if t_abs is None else t_abs), int(t_rel is not None), ctypes.c_double(0.0 if t_rel is None else t_rel),
                -1 if per_label is None else per_label, -1 if num_peaks is None else num_peaks, cap, R.ptr(keys),
                ctypes.cast(found, ctypes.c_void_p))
        if found[1] >= 0:
            break
        cap = int(found[0])
    n = int(found[1])
    out = coords(n), torch.empty(n, dtype=t.dtype, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        N.dcall(t, "sd_peaks_emit_device", *head, R.ptr(keys), n, R.ptr(out[0]), R.ptr(out[1]), R.ptr(out[2]))
    return out


def _peaks(img, is_t, on_device, device, labels, args, return_table, as_tensors):
    d, b, t_abs, t_rel, num_peaks, per_label = args
    if on_device:
        if labels is not None and not R.is_torch(labels):
            labels = _labels_host(labels, img.shape).astype(np.int32)       # checked before anything travels
        t = R.to_device_tensor(img, device)
        lab = None if labels is None else _labels_device(labels, img.shape, t.device)
        cols = _peaks_device(t, lab, d, b, t_abs, t_rel, per_label, num_peaks)
    else:
        a = img.cpu().numpy() if is_t else img
        cols = _peaks_host(a, None if labels is None else _labels_host(labels, img.shape), d, b, t_abs, t_rel, per_label, num_peaks)
    cols = R.table_exit(cols if return_table else cols[:1], as_tensors, img, device)         # without the table only the coordinates travel
    return dict(zip(("coords", "values", "labels"), cols)) if return_table else cols[0]


def peak_local_max(img, min_distance=1, threshold_abs=None, threshold_rel=None, exclude_border=True, num_peaks=None, *, labels=None,
                   num_peaks_per_label=None, return_table=False, device=None, as_tensors=False):
    """The local peaks of a 2D or 3D uint8, uint16 or float32 image: coords (n, ndim) int64, ordered by (-value, raster index).  With
    return_table=True a dict: coords, values (n, the image's dtype) and labels (n int32; zeros without `labels`).

    The definition, which both routes and the tests' brute-force loop follow.  idx(p) is the raster index of pixel p; d is
    min_distance per axis (an integer >= 0 or one per axis).  Values compare as numbers: -0.0 equals +0.0, a NaN pixel is never a
    peak and never competes.  lo and hi are the least and greatest non-NaN pixel (none: no peaks).  thr = float64(threshold_abs) if
    given, else lo; with threshold_rel, thr = max(thr, fl64(threshold_rel * hi)).  The border widths b: exclude_border=True means d,
    False or 0 none, an integer or a tuple is used as given; negative values raise ValueError.  A pixel p is a peak iff
      1. float64(v(p)) > thr, strictly;
      2. b[a] <= p[a] < n[a] - b[a] on every axis;
      3. with labels: labels(p) != 0;
      4. no pixel q inside the image with |q[a] - p[a]| <= d[a] on every axis beats p -- with labels, only pixels of p's label
         compete -- where q beats p when v(q) > v(p), or v(q) == v(p) and idx(q) < idx(p).
    Pixels in the border band compete under rule 4; they just cannot be peaks.  num_peaks_per_label=k (it needs labels) keeps, per
    label, the first k peaks in the output order; num_peaks then keeps the first num_peaks of what is left.  Label ids go up to
    2^31 - 1; negative ids raise ValueError.

    Relation to scikit-image 0.18.3.  The strict total order gives one peak per plateau and needs no greedy spacing pass, so every
    pixel is decided on its own.  The result equals skimage.feature.peak_local_max, coordinates and order, whenever no two equal
    values lie within the window of each other (tests/golden/peaks_reference.npz).  Departures, on purpose: scikit-image pads windows
    with the value 0 at the image's and at label boxes' borders, so it loses negative peaks near a border; its labels route writes
    finfo.min into the caller's image where bounding boxes overlap and lets border-band pixels inside a trimmed box be peaks; its
    order among equal values is what an unstable argsort gives (and for unsigned images it sorts the wrapped negation); its "trivial
    image" rule is replaced by rule 1 -- a constant image has no peak under the default threshold and, with a lower threshold_abs and
    no border, exactly one, at index 0.

    Routing: DESIGN.md section 3p by the image; labels that are elsewhere are moved to it.  The columns leave as measure_labels' do
    (exception 4 there, R.table_exit): numpy arrays, which the device route reads back with one synchronisation, unless
    as_tensors=True, which makes them tensors -- on the device for the device route, else where the image is or on `device`.  The
    device route (csrc/spots.hip) reduces lo and hi and forms thr on the device,
    tests every pixel in tiles with the window's halo in LDS while that fits in 48 KiB (peak_window_in_lds; 2D with one d: d <= 36)
    and from global memory beyond, appends peaks with one integer atomic per wave, sorts 64-bit keys (value key, index) and applies
    the cuts; integers and comparisons only, so the same bits from call to call.  One scalar comes to the host, the number of peaks
    (a second with num_peaks_per_label, and a second pass over the image if more than max(65536, pixels / 8) peaks were found; for
    tensor labels also their least and greatest id).  The image and the labels are not written."""
    who = "peak_local_max"
    img, is_t, on_device = _image(img, who, device)
    args = _peak_args(tuple(img.shape), min_distance, threshold_abs, threshold_rel, exclude_border, num_peaks, num_peaks_per_label)
    return _peaks(img, is_t, on_device, device, labels, args, bool(return_table), bool(as_tensors))


def detect_spots(img, sigma, *, sigma_ratio=1.6, truncate=4.0, device=None, **peak_kwargs):
    """peak_local_max(difference_of_gaussians(img, sigma, sigma * sigma_ratio), **peak_kwargs): the centres of blobs of about sigma.
    On the device route the filtered image never leaves the device.  The result is peak_local_max's."""
    who = "detect_spots"
    img, is_t, on_device = _image(img, who, device)
    ratio = _real(sigma_ratio, who, "sigma_ratio")
    low = _sigmas(sigma, len(img.shape), who)
    dog, from_device = _dog(img, is_t, on_device, device, low, [s * ratio for s in low], truncate, who)
    if on_device and not from_device:                                       # a radius beyond the kernel's: the peaks still run where asked
        dog = R.to_device_tensor(dog, device)
    if not on_device and is_t:
        dog = dog.cpu().numpy()
    return peak_local_max(dog, device=device if on_device else None, **peak_kwargs)
