"""Small host-side helpers mirrored from the reference (stardist/utils.py, csbdeep.utils)."""
from zipfile import ZIP_DEFLATED

import numpy as np


def gputools_available():
    """stardist/utils.py:40-45 asks whether the OpenCL helpers can be imported (they serve the reference's mode='opencl' of the training targets).
    There is no OpenCL path here -- 'hip' is the one device mode -- so the answer is always False."""
    return False


def _normalize_grid(grid, n):
    """stardist/utils.py:60-68"""
    try:
        grid = tuple(grid)
        (len(grid) == n and all(map(np.isscalar, grid)) and all(map(_is_power_of_2, grid))) or _raise(TypeError())
        return tuple(int(g) for g in grid)
    except (TypeError, AssertionError):
        raise ValueError("grid = {grid} must be a list/tuple of length {n} with values that are power of 2".format(grid=grid, n=n))


def _is_power_of_2(i):
    assert i > 0
    e = np.log2(i)
    return e == int(e)


def _raise(e):
    raise e


def _is_device_tensor(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "is_cuda") and x.is_cuda


# element type codes of sd_percentiles_device / sd_normalize_mi_ma_device / sd_zoom_linear_device
_DEVICE_DTYPE_CODE = {"torch.uint8": 0, "torch.uint16": 1, "torch.float32": 2}
_NUMPY_2 = int(np.__version__.split(".")[0]) >= 2


def _device_segments(x, axis):
    """number of interleaved segments of a device tensor for statistics over `axis`, or None where the kernels do not apply: 1 for
    axis=None (or every axis), the size of the last axis for "every axis but the last" """
    if str(x.dtype) not in _DEVICE_DTYPE_CODE or x.numel() == 0:
        return None
    if axis is None:
        return 1
    try:
        ax = sorted(set(a % x.dim() for a in ((axis,) if np.isscalar(axis) else tuple(axis))))
    except (TypeError, ZeroDivisionError):
        return None
    if ax == list(range(x.dim())):
        return 1
    if x.dim() >= 2 and ax == list(range(x.dim() - 1)):
        return int(x.shape[-1]) if 1 <= int(x.shape[-1]) <= 64 else None
    return None


def _interp_mode(x, q):
    """how np.percentile interpolates for this data and this q (sd_percentiles_device's interp_f32), or None if q is not a plain scalar:
    numpy >= 2.0 divides a Python-scalar q by 100 in the dtype of float data, so for float32 data the virtual index, the weight and the
    interpolation are float32; a numpy float64 or integer scalar is no such weak scalar (np.float64 IS a Python float by inheritance,
    hence the exact types) and makes everything float64, as integer data do.  Other q (np.float32, float16, arrays) go to the host."""
    if type(q) in (int, float):
        return 1 if (_NUMPY_2 and str(x.dtype) == "torch.float32") else 0
    if type(q) is np.float64 or (isinstance(q, np.integer) and not isinstance(q, np.bool_)):
        return 0
    return None


def _percentiles_device(x, qs, n_seg, interp):
    """(n_seg, len(qs)) float32 device tensor of np.percentile values of the contiguous device tensor x (csrc/normalize.hip)"""
    import ctypes
    import torch
    from .lib import _native as N
    out = torch.empty((n_seg, len(qs)), dtype=torch.float32, device=x.device)
    q = (ctypes.c_double * len(qs))(*[float(v) for v in qs])
    N.dcall(x, "sd_percentiles_device", ctypes.c_void_p(x.data_ptr()), _DEVICE_DTYPE_CODE[str(x.dtype)], x.numel() // n_seg, n_seg,
            ctypes.cast(q, ctypes.c_void_p), len(qs), interp, ctypes.c_void_p(out.data_ptr()))
    return out


def _rescale_device(x, mi, ma, n_seg, clip, eps):
    """float32 device tensor (x - mi) / (ma - mi + eps) of the contiguous device tensor x; mi, ma: contiguous float32 device tensors of
    n_seg values"""
    import ctypes
    import torch
    from .lib import _native as N
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    if x.numel():
        N.dcall(x, "sd_normalize_mi_ma_device", ctypes.c_void_p(x.data_ptr()), _DEVICE_DTYPE_CODE[str(x.dtype)], x.numel() // n_seg, n_seg,
                ctypes.c_void_p(mi.data_ptr()), ctypes.c_void_p(ma.data_ptr()), float(np.float32(eps)), int(bool(clip)),
                ctypes.c_void_p(out.data_ptr()))
    return out


def _bound_device(v, x):
    """a normalisation bound (scalar, numpy array or tensor) as (contiguous float32 device tensor, n_seg), or None if its shape is neither
    one value nor one value per entry of x's last axis"""
    import torch
    if np.isscalar(v):
        return torch.tensor([np.float32(v)], dtype=torch.float32, device=x.device), 1
    if not _is_device_tensor(v):
        if type(v).__module__.startswith("torch"):
            v = v.numpy()
        v = torch.as_tensor(np.ascontiguousarray(np.asarray(v).astype(np.float32, copy=False)), device=x.device)
    if v.dim() > x.dim():
        return None
    if v.dtype != torch.float32:
        v = v.to(torch.float32)
    if v.numel() == 1:
        return v.reshape(1).contiguous(), 1
    if x.dim() >= 2 and v.numel() == x.shape[-1] and v.shape[-1] == x.shape[-1]:
        return v.reshape(-1).contiguous(), int(x.shape[-1])
    return None


def _via_host(fn, x, *args, **kwargs):
    """the host function on a device tensor (dtypes and axes the kernels do not cover): same values, device tensor out"""
    import torch
    args = [a.cpu().numpy() if type(a).__module__.startswith("torch") else a for a in args]
    return torch.as_tensor(np.ascontiguousarray(fn(x.cpu().numpy(), *args, **kwargs)), device=x.device)


def normalize_mi_ma(x, mi, ma, clip=False, eps=1e-20, dtype=np.float32):
    """csbdeep.utils.normalize_mi_ma (csbdeep>=0.8.0, caller side of predict_instances).  numpy in -> numpy out.  A tensor on a HIP device
    in -> a float32 tensor on that device out, with the values of the host expression bit for bit: one fused kernel
    (csrc/normalize.hip) for uint8 / uint16 / float32 data with one bound, or one per entry of the last axis; anything else through the
    host expression."""
    if _is_device_tensor(x):
        if dtype is np.float32 and str(x.dtype) in _DEVICE_DTYPE_CODE and np.isscalar(eps):
            lo, hi = _bound_device(mi, x), _bound_device(ma, x)
            if lo is not None and hi is not None and lo[1] == hi[1] and 1 <= lo[1] <= 64:
                return _rescale_device(x.contiguous(), lo[0], hi[0], lo[1], clip, eps)
        return _via_host(normalize_mi_ma, x, mi, ma, clip=clip, eps=eps, dtype=dtype)
    if dtype is not None:
        x = x.astype(dtype, copy=False)
        mi = dtype(mi) if np.isscalar(mi) else mi.astype(dtype, copy=False)
        ma = dtype(ma) if np.isscalar(ma) else ma.astype(dtype, copy=False)
        eps = dtype(eps)
    x = (x - mi) / (ma - mi + eps)
    if clip:
        x = np.clip(x, 0, 1)
    return x


def _normalize_device(x, pmin, pmax, axis, clip, eps, dtype):
    """(normalised float32 tensor, mi, ma) of a device tensor through the two kernels, mi / ma as (n_seg,) float32 device tensors; None
    where they do not apply.  Nothing is copied to the host: the bounds stay on the device and the rescale reads them there."""
    if dtype is not np.float32 or not np.isscalar(eps):
        return None
    n_seg = _device_segments(x, axis)
    mode_lo, mode_hi = _interp_mode(x, pmin), _interp_mode(x, pmax)
    if n_seg is None or mode_lo is None or mode_lo != mode_hi:
        return None
    if not (0 <= pmin <= 100 and 0 <= pmax <= 100):
        raise ValueError("Percentiles must be in the range [0, 100]")
    x = x.contiguous()
    mima = _percentiles_device(x, (pmin, pmax), n_seg, mode_lo)
    if n_seg == 1:
        mi, ma = mima[0, 0:1], mima[0, 1:2]
    else:
        mi, ma = mima[:, 0].contiguous(), mima[:, 1].contiguous()
    return _rescale_device(x, mi, ma, n_seg, clip, eps), mi, ma


def normalize(x, pmin=3, pmax=99.8, axis=None, clip=False, eps=1e-20, dtype=np.float32):
    """csbdeep.utils.normalize: percentile-based image normalization.  numpy in -> numpy out.  A tensor on a HIP device in -> a float32
    tensor on that device out, equal bit for bit to the host result: exact percentiles by radix selection and a fused rescale
    (csrc/normalize.hip) for uint8 / uint16 / float32 data and axis = None or "every axis but the last", asynchronously (no copy to the
    host); any other dtype or axis through the host functions."""
    if _is_device_tensor(x):
        res = _normalize_device(x, pmin, pmax, axis, clip, eps, dtype)
        if res is not None:
            return res[0]
        return _via_host(normalize, x, pmin, pmax, axis=axis, clip=clip, eps=eps, dtype=dtype)
    mi = np.percentile(x, pmin, axis=axis, keepdims=True)
    ma = np.percentile(x, pmax, axis=axis, keepdims=True)
    return normalize_mi_ma(x, mi, ma, clip=clip, eps=eps, dtype=dtype)


# ----------------------------------------------------------------------------- linear resampling (predict_instances(scale=))
_ZOOM_MAX_RANK = 4
_zoom_device_tables = {}


def _zoom_axis_table(n, m):
    """(i0 int32, w0 float64, w1 float64), one entry per output index, of scipy.ndimage.zoom(order=1) along an axis that goes from n to
    m samples (csrc/zoom_linear.h reads them): the source coordinate cc = float64(k) * ((n - 1) / (m - 1)) (ratio 1 for m = 1), i0 =
    floor(cc), w0 = 1 - (cc - i0), w1 = 1 - w0.  Where the product rounds past n - 1 (it can, for the last k) scipy takes the
    coordinate for outside the array and writes 0: i0 = -1 says so."""
    ratio = np.float64(n - 1) / np.float64(m - 1) if m > 1 else np.float64(1.0)
    cc = np.arange(m, dtype=np.float64) * ratio
    lo = np.floor(cc)
    w0 = 1.0 - (cc - lo)
    w1 = 1.0 - w0
    i0 = lo.astype(np.int32)
    i0[cc > n - 1] = -1
    return i0, w0, w1


def _zoom_out_shape(shape, zoom):
    """the output shape scipy.ndimage.zoom gives an array of this shape, or None where the device kernel does not apply (a zoom that is no
    plain number per axis, an empty output, a rank beyond 4): scipy then decides, and raises its own errors"""
    plain = (int, float, np.float64, np.integer)
    if isinstance(zoom, plain) and not isinstance(zoom, (bool, np.bool_)):
        zoom = (zoom,) * len(shape)
    try:
        zoom = tuple(zoom)
    except TypeError:
        return None
    if not 1 <= len(shape) <= _ZOOM_MAX_RANK or len(zoom) != len(shape):
        return None
    if not all(isinstance(z, plain) and not isinstance(z, (bool, np.bool_)) for z in zoom):
        return None
    try:
        out = tuple(int(round(n * z)) for n, z in zip(shape, zoom))         # scipy's expression; Python's round: halves go to even
    except (ValueError, OverflowError):
        return None
    if min(shape) < 1 or min(out) < 1 or max(out) >= 2 ** 31:
        return None
    return out


def _zoom_tables_on(device, in_shape, out_shape):
    """the tables of every axis, concatenated, as three device tensors; built and uploaded once per (shapes, device)"""
    import torch
    key = (tuple(in_shape), tuple(out_shape), str(device))
    t = _zoom_device_tables.get(key)
    if t is None:
        per_axis = [_zoom_axis_table(n, m) for n, m in zip(in_shape, out_shape)]
        t = tuple(torch.as_tensor(np.concatenate([a[j] for a in per_axis]), device=device) for j in range(3))
        while len(_zoom_device_tables) >= 32:
            _zoom_device_tables.pop(next(iter(_zoom_device_tables)))
        _zoom_device_tables[key] = t
    return t


def _scipy_zoom_linear(x, zoom):
    from scipy import ndimage
    return ndimage.zoom(x, zoom, order=1)


def zoom_linear(x, zoom):
    """scipy.ndimage.zoom(x, zoom, order=1): the resampling behind predict_instances(scale=).  numpy in -> numpy out, scipy's own call.
    A uint8 / uint16 / float32 tensor of rank <= 4 on a HIP device in -> a tensor of the same type on that device out, equal to scipy's
    result bit for bit (csrc/zoom.hip: float64 sum in scipy's order, per-axis tables from the host), asynchronously and with no copy to
    the host; a non-contiguous tensor is made contiguous first.  Non-finite pixels spread as in scipy: a NaN or an infinity makes every
    output element NaN that reads it with weight 0 -- along an axis of factor 1 too, and at the far edge through the mirrored sample
    scipy reads there -- only the sign and payload of such a NaN are not scipy's.  Any other tensor (dtype, rank, a host tensor), a zoom
    that is not one plain number per axis and an empty output go through scipy, which raises its own errors."""
    if not type(x).__module__.startswith("torch"):
        return _scipy_zoom_linear(x, zoom)
    out_shape = _zoom_out_shape(tuple(x.shape), zoom) if (x.is_cuda and str(x.dtype) in _DEVICE_DTYPE_CODE) else None
    if out_shape is None:
        return _via_host(_scipy_zoom_linear, x, zoom)
    import ctypes
    import torch
    from .lib import _native as N
    x = x.contiguous()
    i0, w0, w1 = _zoom_tables_on(x.device, x.shape, out_shape)
    out = torch.empty(out_shape, dtype=x.dtype, device=x.device)
    shapes = (ctypes.c_int * len(out_shape))(*x.shape), (ctypes.c_int * len(out_shape))(*out_shape)
    N.dcall(x, "sd_zoom_linear_device", ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), _DEVICE_DTYPE_CODE[str(x.dtype)],
            len(out_shape), ctypes.cast(shapes[0], ctypes.c_void_p), ctypes.cast(shapes[1], ctypes.c_void_p),
            ctypes.c_void_p(i0.data_ptr()), ctypes.c_void_p(w0.data_ptr()), ctypes.c_void_p(w1.data_ptr()))
    return out


# ----------------------------------------------------------------------------- normalisers for predict(..., normalizer=)
class NoNormalizer(object):
    """csbdeep.data.NoNormalizer: leaves the image as it is (before), and the prediction too (after)"""

    def __init__(self, do_after=False):
        self._do_after = do_after

    def before(self, x, axes):
        return x

    before_device = before

    def after(self, mean, scale, axes):
        self.do_after or _raise(ValueError())
        return mean, scale

    @property
    def do_after(self):
        return self._do_after


class PercentileNormalizer(object):
    """csbdeep.data.PercentileNormalizer: `before(x, axes)` normalises with the percentiles pmin / pmax taken over every axis whose letter
    is not 'C' and keeps them as self.mi / self.ma; `after(mean, scale, axes)` maps a prediction back (alpha = ma - mi, beta = mi).
    **kwargs go to normalize_mi_ma (clip, eps).  `before_device` is `before` for a tensor on a HIP device: percentiles and rescale run
    there (stardist_amd.utils.normalize), self.mi / self.ma stay device tensors."""

    def __init__(self, pmin=2, pmax=99.8, do_after=True, dtype=np.float32, **kwargs):
        (np.isscalar(pmin) and np.isscalar(pmax) and 0 <= pmin < pmax <= 100) or _raise(ValueError())
        self.pmin = pmin
        self.pmax = pmax
        self._do_after = do_after
        self.dtype = dtype
        self.kwargs = kwargs

    def before(self, x, axes):
        if _is_device_tensor(x):
            return self.before_device(x, axes)
        self.axes_before = axes
        axis = tuple(d for d, a in enumerate(axes) if a != "C")
        self.mi = np.percentile(x, self.pmin, axis=axis, keepdims=True).astype(self.dtype, copy=False)
        self.ma = np.percentile(x, self.pmax, axis=axis, keepdims=True).astype(self.dtype, copy=False)
        return normalize_mi_ma(x, self.mi, self.ma, dtype=self.dtype, **self.kwargs)

    def before_device(self, x, axes):
        import torch
        self.axes_before = axes
        axis = tuple(d for d, a in enumerate(axes) if a != "C")
        res = None
        if set(self.kwargs) <= {"clip", "eps"} and len(axes) == x.dim() and "C" not in axes[:-1]:
            res = _normalize_device(x, self.pmin, self.pmax, axis if "C" in axes else None, self.kwargs.get("clip", False),
                                    self.kwargs.get("eps", 1e-20), self.dtype)
        if res is None:
            out = torch.as_tensor(np.ascontiguousarray(self.before(x.cpu().numpy(), axes)), device=x.device)
            return out
        keep = tuple(x.shape[d] if a == "C" else 1 for d, a in enumerate(axes))
        self.mi, self.ma = res[1].reshape(keep), res[2].reshape(keep)
        return res[0]

    def after(self, mean, scale, axes):
        self.do_after or _raise(ValueError())
        self.axes_after = axes
        mi, ma = (v.cpu().numpy() if type(v).__module__.startswith("torch") else v for v in (self.mi, self.ma))
        alpha = ma - mi
        beta = mi
        return (alpha * mean + beta).astype(self.dtype, copy=False), \
            (alpha * scale if scale is not None else None)

    @property
    def do_after(self):
        return self._do_after


class MiMaNormalizer(object):
    """Normaliser with fixed bounds: before(x, axes) = normalize_mi_ma(x, mi, ma, ...).  For the block-wise predictors
    (predict_instances_big), where percentiles taken per block would differ from block to block: take mi / ma once for the whole image
    (np.percentile of a sample, or of the image) and pass them here."""

    def __init__(self, mi, ma, do_after=True, dtype=np.float32, **kwargs):
        self.mi = mi
        self.ma = ma
        self._do_after = do_after
        self.dtype = dtype
        self.kwargs = kwargs

    def before(self, x, axes):
        return normalize_mi_ma(x, self.mi, self.ma, dtype=self.dtype, **self.kwargs)

    before_device = before

    def after(self, mean, scale, axes):
        self.do_after or _raise(ValueError())
        alpha = np.asarray(self.ma, self.dtype) - np.asarray(self.mi, self.dtype)
        beta = np.asarray(self.mi, self.dtype)
        return (alpha * mean + beta).astype(self.dtype, copy=False), (alpha * scale if scale is not None else None)

    @property
    def do_after(self):
        return self._do_after


def to_host(t):
    """device tensor -> numpy array through a page-locked staging tensor (PyTorch's caching host allocator re-uses the
    pinned block once the returned array is dropped): ~50 GB/s over PCIe instead of the pageable path's ~5 GB/s."""
    import torch
    if not t.is_cuda:
        return t.numpy()
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return h.numpy()


def to_host_many(tensors):
    """several device tensors -> numpy arrays with ONE stream synchronisation: every copy goes through its own page-locked staging
    tensor (as to_host) and is enqueued non-blocking; None entries and host tensors pass through."""
    import torch
    outs, dev = [], None
    for t in tensors:
        if t is None or not t.is_cuda:
            outs.append(None if t is None else t.numpy())
            continue
        dev = t.device
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t, non_blocking=True)
        outs.append(h)
    if dev is not None:
        torch.cuda.current_stream(dev).synchronize()
    return [o.numpy() if (o is not None and not isinstance(o, np.ndarray)) else o for o in outs]


def to_device(a, device):
    """host numpy array -> device tensor.  Measured on the MI355X box (tools/probe_h2d.py, 2048^2 float32 = 16.8 MB): the plain
    pageable copy 0.32 ms (52 GB/s), a persistent page-locked staging tensor 0.38 ms -- and filling that staging tensor with torch's
    multi-threaded copy_ left 128 worker threads spinning, which slowed every later host-synchronised stage of the step (the whole
    predict_instances went from 20.5 to 30 ms).  So: the runtime's own pageable path, nothing on top."""
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=torch.device(device))


# ----------------------------------------------------------------------------- training-side target: edt_prob
def edt_prob(lbl_img, anisotropy=None):
    """Per-object normalised Euclidean distance transform of a label image (the object-probability training target; what
    stardist/utils.py:71-125 `edt_prob` returns) computed on the GPU by csrc/edt.hip: for every pixel of an object the distance
    (float64, axis spacing `anisotropy`) to the nearest pixel inside the image that carries another label, divided by the object's
    maximum; background 0.  numpy in -> numpy float32 out; a torch device tensor in -> a device tensor out.
    A constant non-zero image is ill-defined; like the reference it is treated as surrounded by background (with a warning)."""
    import ctypes
    import warnings
    import torch
    from .lib import _native as N
    N.require_device()
    as_np = not N.is_torch(lbl_img)
    # label ids: the kernel keeps one table entry per id up to the largest, in int32.  Ids beyond int32, or sparse huge ids (hash-like
    # labels), are first compacted to 1..n -- the result depends on which pixels share a label, not on the ids
    if as_np:
        a = np.ascontiguousarray(lbl_img)
        if a.size and (int(a.max()) >= 2 ** 31 or int(a.max()) > 4 * a.size + 1024):
            u, inv = np.unique(a, return_inverse=True)
            a = inv.reshape(a.shape).astype(np.int64) + (0 if (len(u) and u[0] == 0) else 1)
            if len(u) and u[0] < 0:
                raise ValueError("edt_prob: negative labels")
        lab = torch.from_numpy(a.astype(np.int32, copy=False)).cuda()
    else:
        t = lbl_img
        if t.numel() and (int(t.max()) >= 2 ** 31 or int(t.max()) > 4 * t.numel() + 1024):
            u, inv = torch.unique(t, return_inverse=True)
            t = inv.reshape(t.shape) + (0 if int(u[0]) == 0 else 1)
        lab = t.to(torch.int32).contiguous()
    nd = lab.dim()
    if nd not in (2, 3):
        raise ValueError("edt_prob: label image must be 2D or 3D")
    samp = (1.0,) * nd if anisotropy is None else tuple(float(a) for a in anisotropy)
    if len(samp) != nd:
        raise ValueError("edt_prob: anisotropy must have one entry per axis")
    if lab.numel() == 0:
        out = torch.zeros(lab.shape, dtype=torch.float32, device=lab.device)
        return out.cpu().numpy() if as_np else out
    lo, hi = int(lab.min()), int(lab.max())
    padded = lo == hi and lo > 0
    if padded:
        warnings.warn("EDT of constant label image is ill-defined. (Assuming background around it.)")
        lab = torch.nn.functional.pad(lab, (1, 1) * nd).contiguous()
    Z, Y, X = ((1,) + tuple(lab.shape)) if nd == 2 else tuple(lab.shape)
    sz, sy, sx = ((1.0,) + samp) if nd == 2 else samp
    out = torch.empty(lab.shape, dtype=torch.float32, device=lab.device)
    N.dcall(lab, "sd_edt_prob_device", ctypes.c_void_p(lab.data_ptr()), Z, Y, X, sz, sy, sx, max(hi, 0), ctypes.c_void_p(out.data_ptr()))
    if padded:
        out = out[(slice(1, -1),) * nd].contiguous()
    return out.cpu().numpy() if as_np else out


# ----------------------------------------------------------------------------- ImageJ ROI export
# File layout from ImageJ's ij/io/RoiDecoder.java (all big-endian): 64-byte header -- "Iout", int16 version (>= 217; 227 written),
# byte roi type (0 = polygon) + 1 unused byte, int16 top / left / bottom / right, uint16 n coordinates, ..., int16 options at 50
# (128 = SUB_PIXEL_RESOLUTION), ..., int32 position at 56 -- then n int16 x offsets from `left`, n int16 y offsets from `top` and,
# with the sub-pixel option, n float32 x and n float32 y absolute coordinates.  ImageJ puts the centre of pixel (0, 0) at (0.5, 0.5).
_ROI_HEADER = 64


def polyroi_bytearray(x, y, pos=None, subpixel=True):
    """one ImageJ polygon ROI as bytes (same arguments and bytes as stardist/utils.py:195-251)"""
    import struct
    fx = np.asarray(x, np.float64).ravel() + 0.5
    fy = np.asarray(y, np.float64).ravel() + 0.5
    if fx.shape != fy.shape:
        raise ValueError("x and y must have the same length")
    ix, iy = np.round(fx), np.round(fy)
    n = fx.size
    top, left, bottom, right = int(iy.min()), int(ix.min()), int(iy.max()), int(ix.max())
    head = bytearray(_ROI_HEADER)
    struct.pack_into(">4shBx4hH", head, 0, b"Iout", 227, 0, top, left, bottom, right, n)
    if subpixel:
        struct.pack_into(">h", head, 50, 128)
    if pos is not None:
        struct.pack_into(">i", head, 56, int(pos))
    body = (ix - left).astype(">i2").tobytes() + (iy - top).astype(">i2").tobytes()
    if subpixel:
        body += fx.astype(">f4").tobytes() + fy.astype(">f4").tobytes()
    return head + body


def export_imagej_rois(fname, polygons, set_position=True, subpixel=True, compression=ZIP_DEFLATED):
    """ImageJ ROI archive of predicted polygons (what stardist/utils.py:254-268 writes): `polygons` is the `coord` array of
    predict_instances' dict -- (n, 2, n_rays), rows (y, x) -- or a sequence of such arrays, one per stack position; entry
    'PPP_III.roi' holds polygon III of position PPP (both 1-based)."""
    import zipfile
    groups = (polygons,) if isinstance(polygons, np.ndarray) else polygons
    target = str(fname)
    if not target.endswith(".zip"):
        target += ".zip"
    with zipfile.ZipFile(target, mode="w", compression=ZIP_DEFLATED if compression is None else compression) as zf:
        for pos, group in enumerate(groups, start=1):
            for k, (ys, xs) in enumerate(group, start=1):
                zf.writestr("%03d_%03d.roi" % (pos, k), bytes(polyroi_bytearray(xs, ys, pos=pos if set_position else None, subpixel=subpixel)))


# ----------------------------------------------------------------------------- label-image helpers the reference package exports
# (stardist/__init__.py:13: fill_label_holes, sample_points, calculate_extents).  numpy + scipy like the reference's on host input;
# fill_label_holes and calculate_extents also take label images on a HIP device (csrc/fill_holes.hip).

def _object_boxes(lbl_img):
    """[(label id, bounding-box slices)] of the labels present, ascending (scipy.ndimage.find_objects: entry i - 1 belongs to label i)"""
    from scipy.ndimage import find_objects
    return [(i, sl) for i, sl in enumerate(find_objects(lbl_img), 1) if sl is not None]


_DEVICE_LABEL_DTYPES = ("torch.uint8", "torch.int8", "torch.int16", "torch.int32", "torch.int64")


def _ids_need_compaction(top, size):
    """the id policy of edt_prob: the kernels keep one table entry per id up to the largest, in int32"""
    return top >= 2 ** 31 or top > 4 * size + 1024


def _device_labels(lbl, device=None):
    """(contiguous int32 device tensor with the positive labels of lbl and 0 elsewhere, largest label, ids): lbl a numpy array (uploaded to
    `device`) or a tensor (moved there if it is elsewhere).  ids is None where the labels are the image's own; otherwise they were
    compacted to 1 .. n in ascending order (so the larger of two ids stays the larger) and ids[k] is the original of label k, ids[0] = 0,
    as an array of lbl's kind."""
    import torch
    if isinstance(lbl, np.ndarray):
        a = lbl
        top = int(a.max()) if a.size else 0
        ids = None
        if _ids_need_compaction(top, a.size):
            pos = a > 0
            u, inv = np.unique(a[pos], return_inverse=True)
            lab = np.zeros(a.shape, np.int32)
            lab[pos] = inv.reshape(-1) + 1
            ids = np.concatenate([np.zeros(1, a.dtype), u.astype(a.dtype, copy=False)])
            top = len(u)
        else:
            lab = np.maximum(a, 0).astype(np.int32, copy=False) if a.dtype.kind != "u" else a.astype(np.int32)
        return torch.as_tensor(np.ascontiguousarray(lab), device=torch.device("cuda" if device is None else device)), max(top, 0), ids
    t = lbl if device is None else lbl.to(torch.device(device))
    top = int(t.max()) if t.numel() else 0
    if _ids_need_compaction(top, t.numel()):
        pos = t > 0
        u, inv = torch.unique(t[pos], return_inverse=True)
        lab = torch.zeros(t.shape, dtype=torch.int32, device=t.device)
        lab[pos] = (inv + 1).to(torch.int32)
        return lab, int(u.numel()), torch.cat([torch.zeros(1, dtype=t.dtype, device=t.device), u])
    return t.clamp(min=0).to(torch.int32).contiguous(), max(top, 0), None


def _zyx(shape):
    return ((1,) + tuple(shape)) if len(shape) == 2 else tuple(shape)


def _fill_label_holes_device(lbl_img, device=None):
    """fill_label_holes through sd_fill_label_holes_device; numpy in (uploaded to `device`) -> numpy out, tensor in -> tensor out, of the
    input's dtype and shape; the input is never written"""
    import ctypes
    import torch
    from .lib import _native as N
    N.require_device()
    as_np = isinstance(lbl_img, np.ndarray)
    if lbl_img.ndim not in (2, 3):
        raise ValueError("fill_label_holes: a label image on the device must be 2D or 3D")
    lab, top, ids = _device_labels(lbl_img, device)
    out = torch.empty_like(lab)
    if lab.numel():
        Z, Y, X = _zyx(lab.shape)
        if lab.dim() == 3 and Z == 1:
            # one plane given as a volume: along z every pixel lies on the box's outer layer, so nothing is a hole (the host function
            # says the same); the library takes Z = 1 for a 2D image, so the plane goes in as the volume (Y, 1, X) -- the same memory
            Z, Y = Y, 1
        N.dcall(lab, "sd_fill_label_holes_device", ctypes.c_void_p(lab.data_ptr()), Z, Y, X, top, ctypes.c_void_p(out.data_ptr()))
    if as_np:
        res = out.cpu().numpy()
        return ids[res] if ids is not None else res.astype(lbl_img.dtype, copy=False)
    res = ids[out.long()] if ids is not None else out.to(lbl_img.dtype)
    return res.to(lbl_img.device)


def _label_boxes_device(t):
    """(n present, ndim) int64 numpy array of the bounding-box sizes of the labels of a 2D / 3D device tensor, by ascending label
    (sd_label_boxes_device; only the box table comes to the host)"""
    import ctypes
    import torch
    from .lib import _native as N
    N.require_device()
    nd = t.dim()
    if t.numel() == 0:
        return np.zeros((0, nd), np.int64)
    if str(t.dtype) not in _DEVICE_LABEL_DTYPES:
        t = t.to(torch.int64)
    lab, top, _ = _device_labels(t)
    boxes = torch.empty((top + 1, 6), dtype=torch.int32, device=lab.device)
    N.dcall(lab, "sd_label_boxes_device", ctypes.c_void_p(lab.data_ptr()), *_zyx(lab.shape), top, ctypes.c_void_p(boxes.data_ptr()))
    b = boxes.cpu().numpy().astype(np.int64)
    b = b[b[:, 5] > b[:, 2]]
    return (b[:, 3:] - b[:, :3])[:, 3 - nd:]


def fill_label_holes(lbl_img, *, device=None, **kwargs):
    """Fill the holes of every labelled object (stardist/utils.py:137-153): per object, `binary_fill_holes` of its mask on its bounding
    box grown by one pixel on every side that is not an image border -- a cavity that reaches the image border stays open, as there.
    **kwargs go to scipy.ndimage.binary_fill_holes.

    numpy in without `device` -> the host code.  A 2D / 3D integer tensor on a HIP device in -> a tensor of the same dtype and shape on
    that device out, equal to the host result (csrc/fill_holes.hip: bounding boxes in one pass, then per object two bit planes and a
    flood from the box's outer layer; the input is not written).  numpy in with `device=` -> uploaded, filled there, numpy out.  The
    kernels implement the default structure: with any **kwargs a device tensor goes through the host function and comes back as a
    tensor.  Ids beyond int32, or sparse huge ids, are compacted in ascending order for the call and mapped back."""
    if type(lbl_img).__module__.startswith("torch"):
        on_device = lbl_img.is_cuda or device is not None
        if kwargs or not on_device or str(lbl_img.dtype) not in _DEVICE_LABEL_DTYPES:
            return _via_host(fill_label_holes, lbl_img, **kwargs)
        return _fill_label_holes_device(lbl_img, device)
    lbl_img = np.asarray(lbl_img)
    if device is not None and not kwargs and lbl_img.dtype.kind in "iu":
        return _fill_label_holes_device(lbl_img, device)
    from scipy.ndimage import binary_fill_holes
    out = np.zeros_like(lbl_img)
    for lab, box in _object_boxes(lbl_img):
        room = [(s.start > 0, s.stop < n) for s, n in zip(box, lbl_img.shape)]
        grown = tuple(slice(s.start - int(lo), s.stop + int(hi)) for s, (lo, hi) in zip(box, room))
        inner = tuple(slice(int(lo), -1 if hi else None) for lo, hi in room)
        filled = binary_fill_holes(lbl_img[grown] == lab, **kwargs)[inner]
        out[box][filled] = lab
    return out


def sample_points(n_samples, mask, prob=None, b=2):
    """Draw `n_samples` pixel positions (with replacement) from a 2D mask, at least `b` pixels from the border, uniformly or weighted by
    `prob` (stardist/utils.py:156-177; numpy's global random state, the same draws as there)."""
    mask = np.asarray(mask)
    if b is not None and b > 0:
        inner = np.zeros_like(mask)
        inner[b:-b, b:-b] = True
    else:
        inner = True
    rows, cols = np.nonzero(mask & inner)
    if prob is not None:
        w = np.asarray(prob)[rows, cols].astype(np.float64)
        w /= np.sum(w)
        pick = np.random.choice(len(rows), n_samples, replace=True, p=w)
    else:
        pick = np.random.choice(len(rows), n_samples, replace=True)
    return np.stack((rows[pick], cols[pick]), axis=-1)


def calculate_extents(lbl, func=np.median):
    """Aggregate (median by default) of the objects' bounding-box sizes per axis, for one 2D / 3D label image, or over a sequence / 4D
    stack of them (stardist/utils.py:180-193).  Label images that are tensors on a HIP device stay there: one sd_label_boxes_device call
    per image, the box table comes to the host and `func` runs over the extents as for host input."""
    from collections.abc import Iterable
    if _is_device_tensor(lbl):
        if lbl.dim() == 4:
            return func(np.stack([calculate_extents(one, func) for one in lbl], axis=0), axis=0)
        if lbl.dim() not in (2, 3):
            raise ValueError("label image should be 2- or 3-dimensional (or pass a list of these)")
        extents = _label_boxes_device(lbl)
        return func(extents, axis=0) if len(extents) else np.zeros(lbl.dim())
    if (isinstance(lbl, np.ndarray) and lbl.ndim == 4) or (not isinstance(lbl, np.ndarray) and isinstance(lbl, Iterable)):
        return func(np.stack([calculate_extents(one, func) for one in lbl], axis=0), axis=0)
    n = lbl.ndim
    if n not in (2, 3):
        raise ValueError("label image should be 2- or 3-dimensional (or pass a list of these)")
    boxes = _object_boxes(lbl)
    if not boxes:
        return np.zeros(n)
    return func(np.array([[s.stop - s.start for s in box] for _, box in boxes]), axis=0)


# ----------------------------------------------------------------------------- measure_labels: the per-object table
# Both routes produce the same "raw" columns -- label (n,), area (n,), bbox (n, 2 nd), csum (n, nd) coordinate sums, all int64, and with
# an image sum, sum2 (n, C) int64 / float64 and min, max (n, C) int64 / the image's float type -- as numpy arrays or as tensors;
# _measure_columns derives the table from them, the one place where centroid, mean and std are computed.
_MEASURE_RAW = ("label", "area", "bbox", "csum", "sum", "sum2", "min", "max")


def _measure_shapes(lbl_shape, img_shape):
    """(number of channels or None without an image, whether the image has a channel axis); raises the ValueErrors of measure_labels"""
    nd = len(lbl_shape)
    if nd not in (2, 3):
        raise ValueError("measure_labels: the label image must be 2D or 3D, got %d axes" % nd)
    if img_shape is None:
        return None, False
    if tuple(img_shape) == tuple(lbl_shape):
        return 1, False
    if len(img_shape) == nd + 1 and tuple(img_shape[:-1]) == tuple(lbl_shape) and img_shape[-1] >= 1:
        return int(img_shape[-1]), True
    raise ValueError("measure_labels: the image's shape %s is neither the label image's %s nor that plus a channel axis"
                     % (tuple(img_shape), tuple(lbl_shape)))


def _measure_pack(raw):
    """the raw columns side by side as one (n, K) int64 array / tensor (floats as the bits of their float64 value): one copy moves it"""
    wide = [raw[key] if raw[key].ndim == 2 else raw[key].reshape(raw[key].shape[0], 1) for key in _MEASURE_RAW if key in raw]
    if type(raw["label"]).__module__.startswith("torch"):
        import torch
        return torch.cat([a.to(torch.float64).contiguous().view(torch.int64) if a.dtype.is_floating_point else a.to(torch.int64)
                          for a in wide], dim=1).contiguous()
    return np.ascontiguousarray(np.concatenate([np.ascontiguousarray(a, np.float64).view(np.int64) if a.dtype.kind == "f"
                                                else a.astype(np.int64) for a in wide], axis=1))


def _measure_unpack(packed, nd, C, sum_dtype, mm_dtype):
    """the raw columns of _measure_pack's array; sum_dtype / mm_dtype: the names of the dtypes of sum, sum2 and of min, max"""
    is_t = type(packed).__module__.startswith("torch")
    widths = [("label", 1, "int64"), ("area", 1, "int64"), ("bbox", 2 * nd, "int64"), ("csum", nd, "int64")]
    if C is not None:
        widths += [("sum", C, sum_dtype), ("sum2", C, sum_dtype), ("min", C, mm_dtype), ("max", C, mm_dtype)]
    raw, at = {}, 0
    for key, w, dt in widths:
        a = packed[:, at:at + w]
        at += w
        if is_t:
            import torch
            a = a.contiguous()
            a = a.view(torch.float64).to(getattr(torch, dt)) if dt.startswith("float") else a
        else:
            a = np.ascontiguousarray(a)
            a = a.view(np.float64).astype(dt) if dt.startswith("float") else a
        raw[key] = a.reshape(-1) if key in ("label", "area") else a
    return raw


def _measure_columns(raw, nd, channel_axis):
    """the table of measure_labels from the raw columns (numpy arrays or tensors): centroid = float64(coordinate sum) / count, mean =
    float64(sum) / count, var = max(0, float64(sum2) / count - mean^2), std = sqrt(var), every operation rounded on its own"""
    is_t = type(raw["label"]).__module__.startswith("torch")
    if is_t:
        import torch
        f64, sqrt, col = (lambda a: a.to(torch.float64)), torch.sqrt, (lambda a: a.contiguous())
    else:
        f64, sqrt, col = (lambda a: a.astype(np.float64)), np.sqrt, np.ascontiguousarray
    out = {"label": raw["label"], "area": raw["area"]}
    for k in range(2 * nd):
        out["bbox-%d" % k] = col(raw["bbox"][:, k])
    count = f64(raw["area"])
    for k in range(nd):
        out["centroid-%d" % k] = f64(raw["csum"][:, k]) / count
    if "sum" in raw:
        with np.errstate(all="ignore"):
            cnt = count[:, None]
            mean = f64(raw["sum"]) / cnt
            var = (f64(raw["sum2"]) / cnt - mean * mean).clip(min=0)
            std = sqrt(var)
        named = (("sum_intensity", raw["sum"]), ("mean_intensity", mean), ("min_intensity", raw["min"]), ("max_intensity", raw["max"]),
                 ("std_intensity", std))
        for name, a in named:
            for c in range(a.shape[1]):
                out[("%s-%d" % (name, c)) if channel_axis else name] = col(a[:, c])
    return out


def _measure_raw_host(lbl, img):
    """the raw columns by numpy over scipy.ndimage.find_objects boxes; img: None or an array of lbl.shape (+ (C,))"""
    if lbl.dtype.kind == "b":
        lbl = lbl.astype(np.uint8)
    if lbl.dtype.kind not in "iu":
        raise ValueError("measure_labels: the label image must have an integer type, got %s" % lbl.dtype)
    nd = lbl.ndim
    top = int(lbl.max()) if lbl.size else 0
    ids = None
    if _ids_need_compaction(top, lbl.size):
        pos = lbl > 0
        ids, inv = np.unique(lbl[pos], return_inverse=True)
        lab = np.zeros(lbl.shape, np.int32)
        lab[pos] = inv.reshape(-1) + 1
    else:
        lab = np.maximum(lbl, 0) if lbl.dtype.kind != "u" else lbl
    boxes = _object_boxes(lab) if lab.size else []
    n = len(boxes)
    raw = {"label": np.array([k for k, _ in boxes], np.int64).reshape(n), "area": np.zeros(n, np.int64),
           "bbox": np.zeros((n, 2 * nd), np.int64), "csum": np.zeros((n, nd), np.int64)}
    if ids is not None:
        raw["label"] = ids.astype(np.int64)[raw["label"] - 1]
    if img is not None:
        C = 1 if img.ndim == nd else img.shape[-1]
        exact = img.dtype.kind in "iub"
        raw["sum"] = np.zeros((n, C), np.int64 if exact else np.float64)
        raw["sum2"] = np.zeros((n, C), np.int64 if exact else np.float64)
        raw["min"] = np.zeros((n, C), np.int64 if exact else img.dtype)
        raw["max"] = np.zeros((n, C), np.int64 if exact else img.dtype)
    with np.errstate(all="ignore"):
        for k, (l, box) in enumerate(boxes):
            mask = lab[box] == l
            where = np.nonzero(mask)
            area = len(where[0])
            raw["area"][k] = area
            raw["bbox"][k] = [s.start for s in box] + [s.stop for s in box]
            raw["csum"][k] = [int(w.sum(dtype=np.int64)) + area * s.start for w, s in zip(where, box)]
            if img is not None:
                v = img[box][mask].reshape(area, C)
                wide = v.astype(np.int64 if exact else np.float64)
                raw["sum"][k] = wide.sum(axis=0)
                raw["sum2"][k] = (wide * wide).sum(axis=0)
                raw["min"][k] = v.min(axis=0)
                raw["max"][k] = v.max(axis=0)
    return raw


def _measure_raw_device(lbl, img, C, device):
    """the raw columns as tensors on the device: sd_label_boxes_device, sd_label_centroid_sums_device and, with an image,
    sd_label_intensity_stats_device, then the rows of the labels present (one scalar, their number, comes to the host)"""
    import ctypes
    import torch
    from .lib import _native as N
    N.require_device()
    lab, top, ids = _device_labels(lbl, device)
    dev, nd = lab.device, lab.dim()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    code = None
    if img is not None:
        img = (img if type(img).__module__.startswith("torch") else torch.as_tensor(np.ascontiguousarray(img))).to(dev).contiguous()
        code = _DEVICE_DTYPE_CODE[str(img.dtype)]
    sum_t, mm_t = (torch.float64, torch.float32) if code == 2 else (torch.int64, torch.int32)
    if lab.numel() == 0 or top <= 0:
        raw = {"label": torch.zeros(0, dtype=torch.int64, device=dev), "area": torch.zeros(0, dtype=torch.int64, device=dev),
               "bbox": torch.zeros((0, 2 * nd), dtype=torch.int64, device=dev), "csum": torch.zeros((0, nd), dtype=torch.int64, device=dev)}
        if img is not None:
            raw.update(sum=torch.zeros((0, C), dtype=sum_t, device=dev), sum2=torch.zeros((0, C), dtype=sum_t, device=dev),
                       min=torch.zeros((0, C), dtype=torch.float32 if code == 2 else torch.int64, device=dev),
                       max=torch.zeros((0, C), dtype=torch.float32 if code == 2 else torch.int64, device=dev))
        return raw
    zyx = _zyx(lab.shape)
    boxes = torch.empty((top + 1, 6), dtype=torch.int32, device=dev)
    sums = torch.empty((top + 1, 4), dtype=torch.int64, device=dev)
    N.dcall(lab, "sd_label_boxes_device", vp(lab), *zyx, top, vp(boxes))
    N.dcall(lab, "sd_label_centroid_sums_device", vp(lab), *zyx, top, vp(sums))
    if img is not None:
        acc = torch.empty((top + 1, C, 2), dtype=sum_t, device=dev)
        mm = torch.empty((top + 1, C, 2), dtype=mm_t, device=dev)
        N.dcall(lab, "sd_label_intensity_stats_device", vp(lab), *zyx, top, vp(boxes), vp(img), code, C,
                vp(acc) if code != 2 else None, vp(acc) if code == 2 else None, vp(mm))
    present = torch.nonzero(sums[:, 0]).reshape(-1)
    s = sums.index_select(0, present)
    b = boxes.index_select(0, present).to(torch.int64)
    if ids is None:
        label = present
    else:
        ids = ids if type(ids).__module__.startswith("torch") else torch.as_tensor(ids.astype(np.int64), device=dev)
        label = ids.to(torch.int64).index_select(0, present)
    raw = {"label": label, "area": s[:, 0].contiguous(), "bbox": b if nd == 3 else b[:, [1, 2, 4, 5]], "csum": s[:, 4 - nd:]}
    if img is not None:
        a, m = acc.index_select(0, present), mm.index_select(0, present)
        raw.update(sum=a[:, :, 0], sum2=a[:, :, 1], min=m[:, :, 0] if code == 2 else m[:, :, 0].to(torch.int64),
                   max=m[:, :, 1] if code == 2 else m[:, :, 1].to(torch.int64))
    return raw


def measure_labels(lbl, img=None, *, device=None, as_tensors=False):
    """Per-object table of a 2D / 3D integer label image (values <= 0 are background) and, optionally, of the image `img` that was
    segmented: shape lbl.shape or lbl.shape + (C,) (channels last).  Returns a dict of 1-D columns, one row per label present,
    ascending by label, named as scikit-image 0.18's regionprops_table names them:

        label                  int64    the label's id
        area                   int64    pixel count
        bbox-0 .. bbox-(2nd-1) int64    starts, then exclusive stops (scipy.ndimage.find_objects)
        centroid-0 .. -(nd-1)  float64  float64(coordinate sum) / count
      with img (with a channel axis every name gets -0 .. -(C-1)):
        sum_intensity          int64 (integer images) / float64
        mean_intensity         float64  float64(sum) / count
        min_intensity, max_intensity    int64 / the image's float type
        std_intensity          float64  population standard deviation: sqrt(max(0, float64(sum of squares) / count - mean^2))

    Arithmetic: integer images are summed (values and squares) in int64, exactly, also beyond 2^53; float images in float64, where
    every square of a float32 is exact.  The derived columns are computed in one place for both routes, every operation rounded on
    its own.  A NaN pixel makes sum, mean, min, max and std of its object and channel NaN, as numpy does; +-inf follow IEEE.  Without
    objects every column is an empty array of its dtype.

    Routing, as fill_label_holes: numpy in without `device` -> the host code (numpy over find_objects boxes).  A tensor on a HIP device
    in -> the device path; numpy in with `device=` -> uploaded and measured there; an image that is elsewhere is moved to the labels'
    device.  The device path takes integer labels and uint8 / uint16 / float32 images (csrc/measure.hip and the box and centroid-sum
    kernels; the inputs are not written): its float64 sums are added in a fixed order without floating-point atomics, so they depend
    on (shape, lbl, img) alone -- the same bits from call to call and from process to process -- and differ from the host's only by the
    order of the additions.  Any other dtype goes through the host code.  Ids beyond int32, or sparse huge ids, are compacted in
    ascending order for the call; `label` reports the originals.  as_tensors=True: the columns are tensors (on the device, for the
    device path: besides what reading the largest label needs, one scalar comes to the host, the number of rows); otherwise numpy
    arrays, which the device path reads back in one copy of the table.  A label image that is not 2D / 3D or an image of another shape
    raises ValueError before anything runs."""
    lbl_t = type(lbl).__module__.startswith("torch")
    img_t = img is not None and type(img).__module__.startswith("torch")
    if not lbl_t:
        lbl = np.asarray(lbl)
    if img is not None and not img_t:
        img = np.asarray(img)
    nd = len(lbl.shape)
    C, channel_axis = _measure_shapes(tuple(lbl.shape), None if img is None else tuple(img.shape))
    on_device = device is not None or (lbl_t and lbl.is_cuda)
    lbl_ok = (str(lbl.dtype) in _DEVICE_LABEL_DTYPES) if lbl_t else (lbl.dtype.kind in "iu")
    img_ok = img is None or (str(img.dtype) if img_t else "torch." + img.dtype.name) in _DEVICE_DTYPE_CODE
    if on_device and lbl_ok and img_ok:
        raw = _measure_raw_device(lbl, img, C, device)
        if as_tensors:
            return _measure_columns(raw, nd, channel_axis)
        sum_dtype, mm_dtype = (str(raw["sum"].dtype)[6:], str(raw["min"].dtype)[6:]) if img is not None else (None, None)
        return _measure_columns(_measure_unpack(to_host(_measure_pack(raw)), nd, C, sum_dtype, mm_dtype), nd, channel_axis)
    if not as_tensors:
        return _measure_columns(_measure_raw_host(lbl.cpu().numpy() if lbl_t else lbl, img.cpu().numpy() if img_t else img), nd, channel_axis)
    # the host table as tensors where the labels are (or on `device`): the packed raw columns make the trip
    import torch
    host_packed = lambda l, i=None: _measure_pack(_measure_raw_host(l, i))
    rest = () if img is None else (img,)
    if lbl_t:
        packed = _via_host(host_packed, lbl, *rest)
        packed = packed if device is None else packed.to(torch.device(device))
    else:
        packed = torch.as_tensor(host_packed(lbl, *[i.cpu().numpy() if img_t else i for i in rest]),
                                 device=torch.device("cpu" if device is None else device))
    sum_dtype = mm_dtype = None
    if img is not None:
        name = str(img.dtype)[6:] if img_t else img.dtype.name
        floating = name.startswith("float") or name.startswith("bfloat")
        sum_dtype, mm_dtype = ("float64", name) if floating else ("int64", "int64")
    return _measure_columns(_measure_unpack(packed, nd, C, sum_dtype, mm_dtype), nd, channel_axis)


# ----------------------------------------------------------------------------- connected components: mask -> label image
# element type codes of sd_label_components_device (a bool mask travels as uint8)
_COMPONENTS_DTYPE_CODE = {"bool": 0, "uint8": 0, "uint16": 1, "int32": 3}


def _backward_offsets(nd, connectivity):
    """the neighbour offsets with at most `connectivity` non-zero coordinates that point backwards in raster order: every edge of the
    pixel graph once"""
    from itertools import product
    return [o for o in product((-1, 0, 1), repeat=nd) if o < (0,) * nd and sum(1 for c in o if c) <= connectivity]


def _label_components_host(img, connectivity, background):
    """(int32 label image, n) of a 2D / 3D numpy array: one edge list per backward offset, scipy's connected_components on the pixel
    graph, ids by first occurrence in raster order"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    a = np.ascontiguousarray(img)
    out = np.zeros(a.shape, np.int32)
    if a.size == 0:
        return out, 0
    if a.size > 2 ** 31 - 1:
        raise ValueError("label_components: more than 2^31 - 1 pixels")
    fg = a != background
    index = np.arange(a.size, dtype=np.int32).reshape(a.shape)
    rows, cols = [], []
    for off in _backward_offsets(a.ndim, connectivity):
        here = tuple(slice(max(0, -d), n - max(0, d)) for d, n in zip(off, a.shape))
        there = tuple(slice(max(0, d), n - max(0, -d)) for d, n in zip(off, a.shape))
        keep = (a[here] == a[there]) & fg[here]
        rows.append(index[here][keep])
        cols.append(index[there][keep])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(a.size, a.size)).tocsr()
    comp = connected_components(graph, directed=False, return_labels=True)[1]
    where = np.flatnonzero(fg.reshape(-1))
    if not len(where):
        return out, 0
    of_pixel = comp[where]
    ids, first = np.unique(of_pixel, return_index=True)                     # first: position of a component's first pixel
    new_id = np.zeros(int(comp.max()) + 1, np.int32)
    new_id[ids[np.argsort(first, kind="stable")]] = np.arange(1, len(ids) + 1, dtype=np.int32)
    out.reshape(-1)[where] = new_id[of_pixel]
    return out, int(len(ids))


def _label_components_device(img, connectivity, background, device):
    """(int32 label tensor, int32 device scalar n) through sd_label_components_device; img a numpy array (uploaded to `device`) or a
    tensor (moved there if it is elsewhere) of one of the dtypes of _COMPONENTS_DTYPE_CODE; nothing comes to the host"""
    import ctypes
    import torch
    from .lib import _native as N
    N.require_device()
    if int(np.prod(img.shape, dtype=np.int64)) > 2 ** 31 - 1:
        raise ValueError("label_components: more than 2^31 - 1 pixels")
    if isinstance(img, np.ndarray):
        a = np.ascontiguousarray(img)
        t = torch.as_tensor(a.view(np.uint8) if a.dtype == np.bool_ else a, device=torch.device("cuda" if device is None else device))
    else:
        t = (img if device is None else img.to(torch.device(device))).contiguous()
        t = t.view(torch.uint8) if t.dtype == torch.bool else t
    out = torch.empty(t.shape, dtype=torch.int32, device=t.device)
    count = torch.zeros(1, dtype=torch.int32, device=t.device)
    if t.numel():
        code = _COMPONENTS_DTYPE_CODE[str(t.dtype).replace("torch.", "")]
        N.dcall(t, "sd_label_components_device", ctypes.c_void_p(t.data_ptr()), code, *_zyx(t.shape), int(connectivity), int(background),
                ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(count.data_ptr()))
    return out, count[0]


def label_components(img, connectivity=None, background=0, *, return_num=False, device=None):
    """Label the connected components of a 2D / 3D image, as skimage.measure.label(img, background=background,
    connectivity=connectivity) does: pixels equal to `background` (None: 0) get 0; two neighbouring pixels belong to one component only if
    their values are equal; `connectivity` = 1 .. ndim is the largest number of coordinates in which neighbours may differ (None: ndim);
    ids 1 .. n are given in raster (C) order of each component's first pixel.  For a boolean mask this is scipy.ndimage.label(mask,
    generate_binary_structure(ndim, connectivity)).  The result is int32, the project's label dtype, on both routes (skimage returns
    int64).  return_num=True: (labels, n) with n a Python int.

    Routing, as fill_label_holes: numpy in without `device` -> the host code (the pixel graph built with numpy, scipy's
    connected_components, ids by first occurrence).  A bool / uint8 / uint16 / int32 tensor on a HIP device in (or `device=` given) -> an
    int32 tensor on that device out, equal to the host result (csrc/label_cc.hip: a tiled union-find whose roots are the components'
    first pixels; the input is not written, the result depends on the input alone); nothing is read back and the stream is not
    synchronised unless return_num=True.  numpy in with `device=` -> uploaded, labelled there, numpy out.  A tensor of another dtype, or
    a background that is no integer, goes through the host code and comes back as a tensor.  An image that is not 2D / 3D, a
    connectivity outside 1 .. ndim or, on the device, more than 2^31 - 1 pixels raise ValueError before anything runs; an empty image
    gives an empty result and n = 0."""
    is_t = type(img).__module__.startswith("torch")
    if not is_t:
        img = np.asarray(img)
    nd = len(img.shape)
    if nd not in (2, 3):
        raise ValueError("label_components: the image must be 2D or 3D, got %d dimensions" % nd)
    if connectivity is None:
        connectivity = nd
    if isinstance(connectivity, (bool, np.bool_)) or not isinstance(connectivity, (int, np.integer)) or not 1 <= connectivity <= nd:
        raise ValueError("Connectivity for %dD images must be in [1, ..., %d]. Got %r." % (nd, nd, connectivity))
    connectivity = int(connectivity)
    background = 0 if background is None else background
    name = str(img.dtype).replace("torch.", "")
    whole = isinstance(background, (int, np.integer, bool, np.bool_)) or (isinstance(background, (float, np.floating))
                                                                           and float(background).is_integer())
    on_device = device is not None or (is_t and img.is_cuda)
    if on_device and name in _COMPONENTS_DTYPE_CODE and whole and abs(int(background)) < 2 ** 63:
        out, count = _label_components_device(img, connectivity, int(background), device)
        if not is_t:
            out = to_host(out)                                              # synchronises: count is there too
        return (out, int(count)) if return_num else out
    if is_t:
        import torch
        n_box = []

        def host(a):
            lab, n = _label_components_host(a, connectivity, background)
            n_box.append(n)
            return lab
        out = _via_host(host, img)
        out = out if device is None else out.to(torch.device(device))
        return (out, n_box[0]) if return_num else out
    out, n = _label_components_host(img, connectivity, background)
    return (out, n) if return_num else out


# ----------------------------------------------------------------------------- nearest-feature transform: expand_labels, distance_transform
# (csrc/edt_feature.hip).  The host routes are scipy's distance_transform_edt; the device routes equal them, ties included.

def _spacing_zyx(spacing, nd, who):
    """one positive finite float per axis from a scalar or a sequence, as (sz, sy, sx) with sz = 1.0 for a 2D image, and the per-axis
    tuple itself"""
    s = np.asarray(1.0 if spacing is None else spacing, dtype=np.float64)
    if s.ndim == 0:
        s = np.full(nd, float(s))
    if s.shape != (nd,):
        raise ValueError("%s: the spacing must be a scalar or one value per axis (%d), got shape %r" % (who, nd, s.shape))
    if not (np.isfinite(s).all() and (s > 0).all()):
        raise ValueError("%s: the spacing must be positive and finite, got %r" % (who, s.tolist()))
    per_axis = tuple(float(v) for v in s)
    return ((1.0,) + per_axis if nd == 2 else per_axis), per_axis


def _check_pixel_count(shape, who):
    if int(np.prod(shape, dtype=np.int64)) > 2 ** 31 - 1:
        raise ValueError("%s: more than 2^31 - 1 pixels" % who)


def _expand_labels_host(lbl, distance, spacing):
    """scikit-image's expand_labels: scipy's nearest labelled pixel of every background pixel, gathered where it is near enough"""
    from scipy.ndimage import distance_transform_edt
    out = np.zeros_like(lbl)
    if not lbl.any():                                                       # scipy's indices are undefined without a feature
        return out
    dist, nearest = distance_transform_edt(lbl == 0, sampling=spacing, return_indices=True)
    near = dist <= distance
    out[near] = lbl[tuple(ax[near] for ax in nearest)]
    return out


def _expand_labels_device(lbl, distance, szyx, device):
    """expand_labels through sd_expand_labels_device; numpy in (uploaded to `device`) -> numpy out, tensor in -> tensor out, of the
    input's dtype and shape; the labels are non-negative; the input is never written"""
    import ctypes
    import torch
    from .lib import _native as N
    N.require_device()
    as_np = isinstance(lbl, np.ndarray)
    lab, _, ids = _device_labels(lbl, device)
    out = torch.empty_like(lab)
    if lab.numel():
        N.dcall(lab, "sd_expand_labels_device", ctypes.c_void_p(lab.data_ptr()), *_zyx(lab.shape), *szyx, float(distance),
                ctypes.c_void_p(out.data_ptr()))
    if as_np:
        res = to_host(out)
        return ids[res] if ids is not None else res.astype(lbl.dtype, copy=False)
    return ids[out.long()] if ids is not None else out.to(lbl.dtype)


def expand_labels(lbl, distance=1, spacing=1, *, device=None):
    """Grow every labelled object of a 2D / 3D label image by up to `distance` without growing into its neighbours, as
    skimage.segmentation.expand_labels(lbl, distance, spacing) does: a background pixel takes the label of the nearest labelled pixel if
    that pixel is at most `distance` away (Euclidean, in units of `spacing`: a scalar or one value per axis), and stays 0 otherwise.
    A pixel equally near to several labels takes the one scipy's distance_transform_edt returns: the nearest pixel with the smallest
    coordinate along the last axis, then along the axis before it.  distance <= 0 returns a copy.

    Routing, as fill_label_holes and label_components: numpy in without `device` -> the host code (scipy's
    distance_transform_edt(lbl == 0, sampling=spacing, return_indices=True) and the gather, as scikit-image composes them).  An integer
    tensor on a HIP device in (or `device=` given) -> a tensor of the same dtype and shape on that device out, equal to the host result
    (csrc/edt_feature.hip: one exact outward scan per pixel and axis, bounded by `distance`; the input is not written).  numpy in with
    `device=` -> uploaded, expanded there, numpy out.  Ids beyond int32, or sparse huge ids, are compacted in ascending order for the
    call and mapped back.  The device route takes non-negative labels: an image with a negative label (a feature like any other, as in
    scikit-image) goes through the host code and comes back in the input's kind; so does a tensor that is no integer tensor.  An image
    that is not 2D / 3D, a spacing that is not positive and finite or, on the device, more than 2^31 - 1 pixels raise ValueError before
    anything runs; an empty image gives an empty result."""
    is_t = type(lbl).__module__.startswith("torch")
    if not is_t:
        lbl = np.asarray(lbl)
    nd = len(lbl.shape)
    if nd not in (2, 3):
        raise ValueError("expand_labels: the label image must be 2D or 3D, got %d dimensions" % nd)
    szyx, per_axis = _spacing_zyx(spacing, nd, "expand_labels")
    distance = float(distance)
    if distance != distance:
        raise ValueError("expand_labels: the distance is not a number")
    size = int(np.prod(lbl.shape, dtype=np.int64))
    if not distance > 0 or size == 0:
        return lbl.clone() if is_t else lbl.copy()
    on_device = device is not None or (is_t and lbl.is_cuda)
    if is_t:
        import torch
        if on_device and str(lbl.dtype) in _DEVICE_LABEL_DTYPES and int(lbl.min()) >= 0:
            _check_pixel_count(lbl.shape, "expand_labels")
            return _expand_labels_device(lbl, distance, szyx, device)
        out = _via_host(_expand_labels_host, lbl, distance, per_axis)
        return out if device is None else out.to(torch.device(device))
    if on_device and lbl.dtype.kind in "iu" and int(lbl.min()) >= 0:
        _check_pixel_count(lbl.shape, "expand_labels")
        return _expand_labels_device(lbl, distance, szyx, device)
    return _expand_labels_host(lbl, distance, per_axis)


def _distance_transform_host(img, per_axis, max_distance, return_distances, return_indices):
    from scipy.ndimage import distance_transform_edt
    zero = img == 0
    if zero.any():
        dist, idx = distance_transform_edt(img, sampling=per_axis, return_indices=True)
        idx = idx.astype(np.int32)
    else:
        dist, idx = np.full(img.shape, np.inf), np.full((img.ndim,) + img.shape, -1, np.int32)
    if max_distance is not None:
        far = dist > max_distance
        dist[far] = np.inf
        idx[:, far] = -1
    return dist if return_distances else None, idx if return_indices else None


def _distance_transform_device(img, szyx, max_distance, return_distances, return_indices, device):
    """(float64 distances or None, (ndim, ...) int32 indices or None) as device tensors, through sd_nearest_feature_device on the
    uint8 mask img != 0 with the zero pixels as the features"""
    import ctypes
    import torch
    from .lib import _native as N
    N.require_device()
    if isinstance(img, np.ndarray):
        t = torch.as_tensor(np.ascontiguousarray(img != 0).view(np.uint8), device=torch.device("cuda" if device is None else device))
    else:
        t = (img if device is None else img.to(torch.device(device)))
        t = (t != 0).to(torch.uint8).contiguous()
    dist = torch.empty(t.shape, dtype=torch.float64, device=t.device) if return_distances else None
    lin = torch.empty(t.shape, dtype=torch.int32, device=t.device) if return_indices else None
    if t.numel():
        N.dcall(t, "sd_nearest_feature_device", ctypes.c_void_p(t.data_ptr()), 0, *_zyx(t.shape), 1, *szyx,
                -1.0 if max_distance is None else float(max_distance),
                ctypes.c_void_p(lin.data_ptr() if return_indices else None), ctypes.c_void_p(dist.data_ptr() if return_distances else None))
    idx = None
    if return_indices:
        none, rest, axes = lin < 0, lin.clamp(min=0), []
        for n in reversed(t.shape):
            axes.append(torch.where(none, lin, rest % n) if n else lin)
            rest = torch.div(rest, max(n, 1), rounding_mode="floor")
        idx = torch.stack(axes[::-1]) if t.numel() else torch.empty((t.dim(),) + tuple(t.shape), dtype=torch.int32, device=t.device)
    return dist, idx


def distance_transform(img, sampling=None, *, max_distance=None, return_distances=True, return_indices=False, device=None):
    """scipy.ndimage.distance_transform_edt(img, sampling, return_distances, return_indices) for a 2D / 3D image: for every non-zero
    pixel the exact Euclidean distance (float64) to the nearest zero pixel, in units of `sampling` (None: 1; a scalar or one value per
    axis), and that pixel's coordinates as an (ndim, ...) int32 array; a zero pixel has distance 0 and its own coordinates.  Among
    equally near zero pixels the indices are scipy's: the smallest coordinate along the last axis, then along the axis before it
    (DESIGN.md section 3n).  Returns the distances, the indices, or (distances, indices), as scipy does.

    Two departures from scipy.  (1) Where no zero pixel exists, or with max_distance given none lies within it, the distance is inf
    and the indices are -1 (scipy leaves an image without a zero pixel undefined and has no bound).  (2) Time: on the device every pixel
    scans outwards along each axis until the axis term alone exceeds its best distance, so an unbounded call costs time proportional
    to the largest distance in the result -- small for images of nuclei, large for a lone zero pixel in a big image.  max_distance
    bounds the scans.

    Routing: numpy in without `device` -> scipy on the host, numpy out.  A tensor on a HIP device in (or `device=` given) ->
    csrc/edt_feature.hip, equal to the host result; tensors on that device out for a tensor, numpy for numpy.  A host tensor without
    `device` -> the host code, host tensors out.  An image that is not 2D / 3D, a sampling that is not positive and finite, a negative
    or NaN max_distance, neither result asked for or, on the device, more than 2^31 - 1 pixels raise ValueError before anything
    runs; an empty image gives empty results."""
    is_t = type(img).__module__.startswith("torch")
    if not is_t:
        img = np.asarray(img)
    nd = len(img.shape)
    if nd not in (2, 3):
        raise ValueError("distance_transform: the image must be 2D or 3D, got %d dimensions" % nd)
    szyx, per_axis = _spacing_zyx(sampling, nd, "distance_transform")
    if max_distance is not None:
        max_distance = float(max_distance)
        if not max_distance >= 0:
            raise ValueError("distance_transform: max_distance must be >= 0 or None")
        if max_distance == np.inf:
            max_distance = None
    if not (return_distances or return_indices):
        raise ValueError("distance_transform: at least one of return_distances / return_indices must be True")
    if device is not None or (is_t and img.is_cuda):
        _check_pixel_count(img.shape, "distance_transform")
        dist, idx = _distance_transform_device(img, szyx, max_distance, return_distances, return_indices, device)
        if not is_t:
            dist, idx = to_host_many([dist, idx])
    else:
        dist, idx = _distance_transform_host(img.numpy() if is_t else img, per_axis, max_distance, return_distances, return_indices)
        if is_t:
            import torch
            dist, idx = (None if a is None else torch.from_numpy(a) for a in (dist, idx))
    return (dist, idx) if return_distances and return_indices else (dist if return_distances else idx)


def mask_to_categorical(y, n_classes, classes, return_cls_dict=False):
    """The multi-channel class map of the integer label array y (stardist/utils.py:318-380): float32 of shape y.shape + (n_classes + 1,),
    the first channel the background.  classes: a dict label id -> class id (0 = background class, 1 ... n_classes = that object class,
    None = ignore the object: -1 in every channel but the background's), or one integer / None for every label.  With return_cls_dict
    also the dict class id -> labels.  Host function: the training step builds the same map on the device (sd_class_targets_device)."""
    from collections import defaultdict
    from .matching import _check_label_array
    _check_label_array(y, "y")
    if not (np.issubdtype(type(n_classes), np.integer) and n_classes >= 1):
        raise ValueError("n_classes is '%s' but should be a positive integer" % (n_classes,))
    y_labels = np.unique(y[y > 0]).tolist()
    if np.issubdtype(type(classes), np.integer) or classes is None:
        classes = dict((k, classes) for k in y_labels)
    elif not isinstance(classes, dict):
        raise ValueError("classes should be dict, single scalar, or None!")
    if not set(y_labels).issubset(set(classes.keys())):
        raise ValueError("all gt labels should be present in class dict provided \ngt_labels found\n%s\nclass dict labels provided\n%s"
                         % (set(y_labels), set(classes.keys())))
    cls_dict = defaultdict(list)
    for k, v in classes.items():
        cls_dict[v].append(k)
    y_mask = np.zeros(y.shape + (n_classes + 1,), np.float32)
    for cls, labels in cls_dict.items():
        if cls is None:
            y_mask[np.isin(y, labels), :] = -1
        elif np.issubdtype(type(cls), np.integer) and 0 <= cls <= n_classes:
            y_mask[np.isin(y, labels), cls] = 1
        else:
            raise ValueError("Wrong class id '%s' (for n_classes=%s)" % (cls, n_classes))
    y_mask[..., 0] = (y == 0)
    return (y_mask, cls_dict) if return_cls_dict else y_mask


_zoom_tables = {}


def nearest_zoom_table(n, g):
    """The rows scipy.ndimage.zoom(a, 1 / g, order=0) reads along an axis of length n, as an int32 array: entry i is the source row of
    output row i, or -1 where scipy reads past the array and fills 0.  Taken from the installed scipy itself (the zoom of 1 ... n), so
    it is what the reference's down-sampling of prob_class gives on this host -- which is not [::g].  Cached per (n, g)."""
    key = (int(n), int(g))
    t = _zoom_tables.get(key)
    if t is None:
        from scipy.ndimage import zoom
        t = (np.rint(zoom(np.arange(1, key[0] + 1, dtype=np.float64), 1.0 / key[1], order=0)) - 1).astype(np.int32)
        t.setflags(write=False)
        _zoom_tables[key] = t
    return t


def optimize_threshold(Y, Yhat, model, nms_thresh, measure="accuracy", iou_threshs=[0.3, 0.5, 0.7], bracket=None, tol=1e-2, maxiter=20, verbose=1):
    """Tune prob_thresh for a fixed nms_thresh so that `measure` of stardist.matching (averaged over iou_threshs) between the label images Y
    and the instances of the predictions Yhat = [(prob, dist), ...] is largest: golden-section search over [max prob / 2, max prob]
    (stardist/utils.py:271-307).  Returns (prob_thresh, value).  Host-side tool: every evaluation is one `_instances_from_prediction` per
    image (NMS + rasteriser natives).  verbose > 1 prints every evaluation; the reference's progress bar is not drawn.  A model on a HIP
    device with the private hook _labels_device (StarDist2D / StarDist3D) is evaluated with the device matching; other objects take the
    host path with the reference's calls."""
    import datetime
    from scipy.optimize import minimize_scalar
    from .matching import matching_dataset
    if not np.isscalar(nms_thresh):
        raise ValueError("nms_thresh must be a scalar")
    iou_threshs = [iou_threshs] if np.isscalar(iou_threshs) else iou_threshs
    if bracket is None:
        top = max([np.max(prob) for prob, dist in Yhat])
        bracket = top / 2, top
    seen = {}
    on_device = callable(getattr(model, "_labels_device", None)) and getattr(model, "device", None) is not None and \
        getattr(model.device, "type", None) == "cuda"
    if on_device:
        # the model renders its label images on its device: the matching runs there too (stardist_amd.matching_sparse, same results as
        # the host's for thresholds > 0), Y uploaded once
        from .matching_sparse import _to_device_int32
        Y_eval = [_to_device_int32(y, "y_true", model.device) for y in Y]

    def negative_score(thr):
        prob_thresh = np.clip(thr, *bracket)
        value = seen.get(prob_thresh)
        if value is None and on_device:
            instances = [model._labels_device(y.shape, *prob_dist, prob_thresh=prob_thresh, nms_thresh=nms_thresh) for y, prob_dist in zip(Y, Yhat)]
            stats = matching_dataset(Y_eval, instances, thresh=iou_threshs, show_progress=False, parallel=False)
            seen[prob_thresh] = value = np.mean([s._asdict()[measure] for s in stats])
        elif value is None:
            instances = [model._instances_from_prediction(y.shape, *prob_dist, prob_thresh=prob_thresh, nms_thresh=nms_thresh)[0] for y, prob_dist in zip(Y, Yhat)]
            stats = matching_dataset(Y, instances, thresh=iou_threshs, show_progress=False, parallel=True)
            seen[prob_thresh] = value = np.mean([s._asdict()[measure] for s in stats])
        if verbose > 1:
            print("%s   thresh: %f   %s: %f" % (datetime.datetime.now().strftime("%H:%M:%S"), prob_thresh, measure, value), flush=True)
        return -value
    opt = minimize_scalar(negative_score, method="golden", bracket=bracket, tol=tol, options={"maxiter": maxiter})
    if verbose > 1:
        print("\n", opt, flush=True)
    return opt.x, -opt.fun
