"""Rank filters and grey morphology with a host route and a device route: minimum_filter, maximum_filter,
median_filter, rank_filter, percentile_filter (scipy.ndimage's, with ==) and grey_opening, grey_closing, white_tophat, black_tophat,
their compositions.  Routing is stardist_amd/_route.py's; the kernels are csrc/rank_filter.hip, the per-element
rules csrc/rank_filter.h.  The public names are re-exported by stardist_amd.utils.

The definition is scipy's, with two departures.  NaN: an output pixel is NaN if and only if its footprint, after the boundary rule,
covers a NaN (scipy's result there depends on its selection code); compositions apply that at every stage.  cval must be a value of
the image's dtype and not NaN (scipy casts silently, so that -1 becomes 255 for uint8).  Values compare as numbers; which of -0.0 and
+0.0 comes out of a window that holds both is unspecified in scipy, the device orders -0.0 below +0.0 and repeats its bits."""
import math

import numpy as np

from . import _route as R
from ._route import _DEVICE_DTYPE_CODE
from .lib import _native as N

# csrc/rank_filter.h
MAX_WINDOW = 1025                 # a window's length along an axis; longer windows take the host code
MAX_FOOTPRINT = 4096              # elements of a footprint (of a box under a rank that is neither the first nor the last); larger: host code
_LDS_BYTES = 48 * 1024
_MAX_PIXELS = 2 ** 32 - 1
_DTYPES = ("bool", "uint8", "uint16", "float32")
_BYTES = {"bool": 1, "uint8": 1, "uint16": 2, "float32": 4}
_MODES = {"reflect": 0, "nearest": 1, "mirror": 2, "constant": 3}
_FUSE = {None: 0, "ref_minus": 1, "minus_ref": 2, "xor": 3}


def box_window_in_lds(dtype, size, last_axis):
    """whether a pass of the box kernel along an axis keeps its tile and halo in LDS: tiles are 1024 x 1 along the last axis and
    32 x 64 along any other, and (tile + size - 1) lines of the dtype's bytes must fit in 48 KiB"""
    a, i = (1024, 1) if last_axis else (32, 64)
    return (a + size - 1) * i * _BYTES[np.dtype(dtype).name] <= _LDS_BYTES


def footprint_window_in_lds(ndim, dtype, extent):
    """whether the footprint kernel keeps a tile's halo in LDS for a footprint of these extents: tiles are 1 x 16 x 64 for a 2D image
    and 4 x 4 x 64 for a 3D one, and (t + extent - 1) elements per axis of the dtype's bytes must fit in 48 KiB"""
    t = (1, 16, 64) if ndim == 2 else (4, 4, 64)
    e = (1,) * (3 - len(extent)) + tuple(extent)
    return math.prod(a + b - 1 for a, b in zip(t, e)) * _BYTES[np.dtype(dtype).name] <= _LDS_BYTES


# ----------------------------------------------------------------------------- arguments

def _image(img, who, device):
    img, is_t, on_device = R.classify(img, device)
    name = R.dtype_name(img)
    if name not in _DTYPES:
        raise TypeError("%s: the image must be bool, uint8, uint16 or float32, got %s" % (who, name))
    nd = len(img.shape)
    if nd not in (2, 3):
        raise ValueError("%s: the image must be 2D or 3D, got %d axes" % (who, nd))
    if math.prod(int(n) for n in img.shape) > _MAX_PIXELS:
        raise ValueError("%s: more than 2^32 - 1 pixels" % who)
    return img, is_t, on_device, name


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _per_axis(v, nd, who, what):
    if _is_int(v):
        return (int(v),) * nd
    try:
        v = tuple(v)
    except TypeError:
        raise ValueError("%s: %s must be an integer or one per axis, got %r" % (who, what, v))
    if len(v) != nd or not all(_is_int(x) for x in v):
        raise ValueError("%s: %s must be an integer or one per axis (%d), got %r" % (who, what, nd, v))
    return tuple(int(x) for x in v)


def _window(size, footprint, nd, who):
    """(extent per axis, the bool footprint or None for a box)"""
    if (size is None) == (footprint is None):
        raise ValueError("%s: exactly one of size and footprint must be given" % who)
    if footprint is None:
        extent = _per_axis(size, nd, who, "size")
        if min(extent) < 1:
            raise ValueError("%s: size must be positive, got %r" % (who, size))
        return extent, None
    fp = footprint.cpu().numpy() if R.is_torch(footprint) else np.asarray(footprint)
    if fp.dtype.kind not in "biu" or fp.ndim != nd:
        raise ValueError("%s: footprint must be a bool array with the image's %d axes" % (who, nd))
    fp = np.ascontiguousarray(fp.astype(bool))
    if not fp.any():
        raise ValueError("%s: footprint must have at least one true element" % who)
    return tuple(int(n) for n in fp.shape), (None if fp.all() else fp)


def _origins(origin, extent, who):
    o = _per_axis(origin, len(extent), who, "origin")
    if any(not 0 <= s // 2 + x < s for s, x in zip(extent, o)):
        raise ValueError("%s: origin must satisfy 0 <= size // 2 + origin < size on every axis, got %r for %r" % (who, origin, extent))
    return o


def _mode(mode, who):
    if not isinstance(mode, str) or mode not in _MODES:
        raise ValueError("%s: mode must be one of reflect, nearest, mirror, constant (one for all axes), got %r" % (who, mode))
    return mode


def _cval(cval, name, who):
    """cval as a Python value of the image's dtype, exactly"""
    if isinstance(cval, (bool, np.bool_)):
        cval = int(cval)
    if not isinstance(cval, (int, float, np.integer, np.floating)) or math.isnan(cval):
        raise ValueError("%s: cval must be a number and not NaN, got %r" % (who, cval))
    if name == "float32":
        with np.errstate(over="ignore"):
            ok = math.isinf(cval) or float(np.float32(cval)) == float(cval)
        value = float(cval)
    else:
        top = {"bool": 1, "uint8": 255, "uint16": 65535}[name]
        ok = not math.isinf(cval) and float(cval).is_integer() and 0 <= cval <= top
        value = int(cval) if ok else 0
    if not ok:
        raise ValueError("%s: cval %r is not exactly representable in %s" % (who, cval, name))
    return bool(value) if name == "bool" else value


def _rank(rank, n, who):
    if not _is_int(rank) or not -n <= rank < n:
        raise ValueError("%s: rank must be an integer in -%d .. %d for this footprint, got %r" % (who, n, n - 1, rank))
    return int(rank) + (n if rank < 0 else 0)


def _percentile_rank(percentile, n, who):
    """scipy's rule: 100 is added to a negative percentile; exactly 100 is rank n - 1, any other int(float(n) * p / 100.0)"""
    p = percentile
    if isinstance(p, (bool, np.bool_)) or not isinstance(p, (int, float, np.integer, np.floating)) or math.isnan(p):
        raise ValueError("%s: percentile must be a number, got %r" % (who, percentile))
    if p < 0:
        p += 100
    if p < 0 or p > 100:
        raise ValueError("%s: percentile must be in -100 .. 100, got %r" % (who, percentile))
    return n - 1 if p == 100 else int(float(n) * p / 100.0)


def _stage(op, rank, extent, fp, origin):
    """one filter of a plan: ('min' | 'max' | 'rank', rank, extent, footprint or None, origin); the first and the last rank are min / max"""
    n = int(fp.sum()) if fp is not None else math.prod(extent)
    if op == "rank" and rank in (0, n - 1):
        op = "min" if rank == 0 else "max"                                  # n = 1: the element itself either way
    return op, rank, extent, fp, origin


# ----------------------------------------------------------------------------- host route

def _host_stage(a, stage, mode, cval):
    import scipy.ndimage as ndi
    op, rank, extent, fp, origin = stage
    win = dict(size=extent) if fp is None else dict(footprint=fp)

    def run(x):
        if op == "min":
            return ndi.minimum_filter(x, mode=mode, cval=cval, origin=origin, **win)
        if op == "max":
            return ndi.maximum_filter(x, mode=mode, cval=cval, origin=origin, **win)
        return ndi.rank_filter(x, rank, mode=mode, cval=cval, origin=origin, **win)

    nan = np.isnan(a) if a.dtype == np.float32 else None
    if nan is None or not nan.any():
        return run(a)
    out = run(np.where(nan, np.float32(0), a))
    out[ndi.maximum_filter(nan, mode=mode, cval=False, origin=origin, **win)] = np.nan       # the NaN rule, by the same index rules
    return out


def _host_plan(a, plan, fuse, mode, cval):
    """the stages of `plan` one after the other on the numpy array a, then the top-hat's operation against a"""
    if a.size == 0:
        return a.copy()
    cur = np.ascontiguousarray(a)
    for stage in plan:
        cur = _host_stage(cur, stage, mode, cval)
    if fuse is None:
        return cur
    if a.dtype == np.bool_:
        return np.logical_xor(a, cur)
    with np.errstate(invalid="ignore", over="ignore"):
        return a - cur if fuse == "ref_minus" else cur - a


# ----------------------------------------------------------------------------- device route

def _pad3(v, fill):
    return np.asarray((fill,) * (3 - len(v)) + tuple(v), np.int32)


def _device_box(t, is_max, extent, origin, mode, cval, fuse=None, ref=None):
    """sd_minmax_box_device on the contiguous device tensor t: a new tensor like t"""
    import torch
    out = torch.empty_like(t)
    work = torch.empty_like(t) if sum(e > 1 for e in extent) > 1 else None
    N.dcall(t, "sd_minmax_box_device", R.ptr(t), _DEVICE_DTYPE_CODE[str(t.dtype)], t.dim(), *R.zyx(t.shape), N.ptr(_pad3(extent, 1)),
            N.ptr(_pad3(origin, 0)), int(is_max), _MODES[mode], float(cval), _FUSE[fuse], R.opt_ptr(ref), R.ptr(out), R.opt_ptr(work))
    return out


def _device_rank(t, rank, extent, fp, origin, mode, cval):
    """sd_rank_filter_device on the contiguous device tensor t: a new tensor like t"""
    import torch
    out = torch.empty_like(t)
    offsets = np.argwhere(np.ones(extent, bool) if fp is None else fp).astype(np.int32)
    offsets = np.ascontiguousarray(np.concatenate([np.zeros((len(offsets), 3 - t.dim()), np.int32), offsets], axis=1))
    N.dcall(t, "sd_rank_filter_device", R.ptr(t), _DEVICE_DTYPE_CODE[str(t.dtype)], t.dim(), *R.zyx(t.shape), N.ptr(_pad3(extent, 1)),
            N.ptr(_pad3(origin, 0)), N.ptr(offsets), len(offsets), int(rank), _MODES[mode], float(cval), R.ptr(out))
    return out


def _stage_on_device(stage):
    """whether the kernels take this stage: window lengths up to MAX_WINDOW, and up to MAX_FOOTPRINT elements unless it is a box
    minimum / maximum"""
    op, _, extent, fp, _ = stage
    if max(extent) > MAX_WINDOW:
        return False
    return (fp is None and op != "rank") or (int(fp.sum()) if fp is not None else math.prod(extent)) <= MAX_FOOTPRINT


def _device_plan(t, plan, fuse, mode, cval, is_bool):
    """the plan on the contiguous device tensor t (bool as uint8): the intermediate stays on the device; a box minimum / maximum as the
    last stage takes the top-hat's operation into its last pass, any other last stage is followed by one element-wise launch"""
    N.require_device()
    if t.numel() == 0:
        return t.clone()
    if fuse is not None and is_bool:
        fuse = "xor"
    cur = t
    for k, (op, rank, extent, fp, origin) in enumerate(plan):
        last = k == len(plan) - 1
        if fp is None and op != "rank":
            cur = _device_box(cur, op == "max", extent, origin, mode, cval, fuse if last else None, t if last and fuse else None)
            if last:
                fuse = None
        else:
            n = int(fp.sum()) if fp is not None else math.prod(extent)
            cur = _device_rank(cur, {"min": 0, "max": n - 1}.get(op, rank), extent, fp, origin, mode, cval)
    if fuse is not None:
        cur = _device_box(cur, False, (1,) * t.dim(), (0,) * t.dim(), mode, cval, fuse, t)
    return cur


def _run(img, is_t, on_device, device, name, plan, fuse, mode, cval):
    """the plan on the image by its route, the result like the input"""
    is_bool = name == "bool"
    if on_device and all(_stage_on_device(s) for s in plan):
        t = R.to_device_tensor(img, device)
        out = _device_plan(t, plan, fuse, mode, float(cval), is_bool)
        if isinstance(img, np.ndarray):
            from .utils import to_host
            out = to_host(out)
            return out.view(np.bool_) if is_bool else out
        import torch
        return out.view(torch.bool) if is_bool else out
    if is_t:
        return R.via_host(_host_plan, img, plan, fuse, mode, cval, to=device)
    return _host_plan(img, plan, fuse, mode, cval)


_MORPHOLOGY = {"grey_opening": ("min", None), "grey_closing": ("max", None), "white_tophat": ("min", "ref_minus"),
               "black_tophat": ("max", "minus_ref")}


def _plan(who, nd, name, size, footprint, mode, cval, origin=0, rank=None, percentile=None):
    """(stages, fused operation, mode, cval) of the public function `who` on an image of nd axes and dtype `name`, arguments checked.
    The five filters are one stage.  Opening and closing are two, as scipy composes them: F is the footprint, F' its flip along every
    axis, o' is -1 on every axis of even length and 0 on the others; the minimum always runs under (F, origin 0), the maximum under
    (F', o'); the top-hats add their subtraction."""
    extent, fp = _window(size, footprint, nd, who)
    origin = _origins(origin, extent, who)
    mode, cval = _mode(mode, who), _cval(cval, name, who)
    n = int(fp.sum()) if fp is not None else math.prod(extent)
    if who in _MORPHOLOGY:
        first, fuse = _MORPHOLOGY[who]
        flipped = None if fp is None else np.ascontiguousarray(fp[(slice(None, None, -1),) * nd])
        lo = _stage("min", 0, extent, fp, (0,) * nd)
        hi = _stage("max", 0, extent, flipped, tuple(-1 if e % 2 == 0 else 0 for e in extent))
        return ([lo, hi] if first == "min" else [hi, lo]), fuse, mode, cval
    if who == "minimum_filter":
        stage = _stage("min", 0, extent, fp, origin)
    elif who == "maximum_filter":
        stage = _stage("max", 0, extent, fp, origin)
    else:
        r = n // 2 if who == "median_filter" else _rank(rank, n, who) if who == "rank_filter" else _percentile_rank(percentile, n, who)
        stage = _stage("rank", r, extent, fp, origin)
    return [stage], None, mode, cval


def _call(who, img, device, **kw):
    img, is_t, on_device, name = _image(img, who, device)
    plan, fuse, mode, cval = _plan(who, len(img.shape), name, **kw)
    return _run(img, is_t, on_device, device, name, plan, fuse, mode, cval)


# ----------------------------------------------------------------------------- the five filters

def minimum_filter(img, size=None, footprint=None, *, mode="reflect", cval=0, origin=0, device=None):
    """scipy.ndimage.minimum_filter(img, size, footprint, mode=mode, cval=cval, origin=origin) with ==, of a 2D or 3D bool, uint8,
    uint16 or float32 image (other dtypes raise TypeError, more than 2^32 - 1 pixels ValueError); the output has the input's dtype and
    shape, the input is not written.

    Exactly one of size (an int or one per axis) and footprint (a bool array of the image's rank with a true element).  mode is
    reflect, nearest, mirror or constant, scipy's index rules, for windows longer than the axis as well (wrap and one mode per axis
    raise ValueError).  origin is an int or one per axis with 0 <= size // 2 + origin < size.  Departures from scipy, on purpose: cval
    must be a value of the image's dtype and not NaN (ValueError; scipy casts silently); an output pixel is NaN iff its footprint,
    after the boundary rule, covers a NaN.  Values compare as numbers (-0.0 == +0.0; which zero a window with both gives is
    unspecified).  All argument errors are raised before any device work.

    Routing: DESIGN.md section 3p -- numpy without device= runs scipy (the NaN rule by a second filter over the NaN mask), a tensor on
    a HIP device or device= the kernels of csrc/rank_filter.hip; the result comes back like the input.  With size (or a footprint that
    is all true) one separable pass per axis, the tile and its halo in LDS (box_window_in_lds); with any other footprint the
    footprint kernel (footprint_window_in_lds).  A window longer than 1025 on an axis, or a footprint of more than 4096 elements, takes
    the host code whatever the route."""
    return _call("minimum_filter", img, device, size=size, footprint=footprint, mode=mode, cval=cval, origin=origin)


def maximum_filter(img, size=None, footprint=None, *, mode="reflect", cval=0, origin=0, device=None):
    """scipy.ndimage.maximum_filter with ==; arguments, departures and routing are minimum_filter's."""
    return _call("maximum_filter", img, device, size=size, footprint=footprint, mode=mode, cval=cval, origin=origin)


def median_filter(img, size=None, footprint=None, *, mode="reflect", cval=0, origin=0, device=None):
    """scipy.ndimage.median_filter with ==: rank n // 2 of the n footprint elements; arguments and departures are minimum_filter's.
    The device route selects the rank-th element by bisection over the bits of an order-preserving key, 8, 16 or 32 walks over the
    window in LDS; a box of more than 4096 elements takes the host code."""
    return _call("median_filter", img, device, size=size, footprint=footprint, mode=mode, cval=cval, origin=origin)


def rank_filter(img, rank, size=None, footprint=None, *, mode="reflect", cval=0, origin=0, device=None):
    """scipy.ndimage.rank_filter with ==: the rank-th smallest (0-based) of the n footprint elements, a negative rank counts from the
    end; a rank outside -n .. n - 1 raises ValueError.  Rank 0 and n - 1 are minimum_filter and maximum_filter.  Otherwise as
    median_filter."""
    return _call("rank_filter", img, device, size=size, footprint=footprint, mode=mode, cval=cval, origin=origin, rank=rank)


def percentile_filter(img, percentile, size=None, footprint=None, *, mode="reflect", cval=0, origin=0, device=None):
    """scipy.ndimage.percentile_filter with ==: 100 is added to a negative percentile, exactly 100 is rank n - 1, any other is rank
    int(float(n) * percentile / 100.0); outside -100 .. 100 raises ValueError.  Otherwise as median_filter."""
    return _call("percentile_filter", img, device, size=size, footprint=footprint, mode=mode, cval=cval, origin=origin, percentile=percentile)


# ----------------------------------------------------------------------------- grey morphology

def grey_opening(img, size=None, footprint=None, *, mode="reflect", cval=0, device=None):
    """scipy.ndimage.grey_opening(img, size, footprint, mode=mode, cval=cval) with ==: maximum_filter(minimum_filter(img, F, origin 0),
    F', origin o') with F' the footprint flipped along every axis and o' = -1 on every axis of even length.  Image, size, footprint,
    mode, cval, the NaN rule (at every stage) and routing are minimum_filter's; on the device route the intermediate stays there."""
    return _call("grey_opening", img, device, size=size, footprint=footprint, mode=mode, cval=cval)


def grey_closing(img, size=None, footprint=None, *, mode="reflect", cval=0, device=None):
    """scipy.ndimage.grey_closing with ==: minimum_filter(maximum_filter(img, F', origin o'), F, origin 0); otherwise as grey_opening."""
    return _call("grey_closing", img, device, size=size, footprint=footprint, mode=mode, cval=cval)


def white_tophat(img, size=None, footprint=None, *, mode="reflect", cval=0, device=None):
    """scipy.ndimage.white_tophat with ==: img - grey_opening(img) in the image's dtype (xor for bool; unsigned types wrap as numpy's
    do, which happens only under mode constant with a cval above the image; inf - inf is NaN).  With size the subtraction is part of
    the last pass of the opening's maximum.  Otherwise as grey_opening."""
    return _call("white_tophat", img, device, size=size, footprint=footprint, mode=mode, cval=cval)


def black_tophat(img, size=None, footprint=None, *, mode="reflect", cval=0, device=None):
    """scipy.ndimage.black_tophat with ==: grey_closing(img) - img in the image's dtype (xor for bool); otherwise as white_tophat."""
    return _call("black_tophat", img, device, size=size, footprint=footprint, mode=mode, cval=cval)
