"""Small host-side helpers mirrored from the reference (stardist/utils.py, csbdeep.utils)."""
from zipfile import ZIP_DEFLATED

import numpy as np

from . import _route as R
from ._route import _DEVICE_DTYPE_CODE, _ids_need_compaction
from .lib import _native as N


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
    out = torch.empty((n_seg, len(qs)), dtype=torch.float32, device=x.device)
    q = (ctypes.c_double * len(qs))(*[float(v) for v in qs])
    N.dcall(x, "sd_percentiles_device", R.ptr(x), _DEVICE_DTYPE_CODE[str(x.dtype)], x.numel() // n_seg, n_seg,
            ctypes.cast(q, ctypes.c_void_p), len(qs), interp, R.ptr(out))
    return out


def _rescale_device(x, mi, ma, n_seg, clip, eps):
    """float32 device tensor (x - mi) / (ma - mi + eps) of the contiguous device tensor x; mi, ma: contiguous float32 device tensors of
    n_seg values"""
    import torch
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    if x.numel():
        N.dcall(x, "sd_normalize_mi_ma_device", R.ptr(x), _DEVICE_DTYPE_CODE[str(x.dtype)], x.numel() // n_seg, n_seg, R.ptr(mi), R.ptr(ma),
                float(np.float32(eps)), int(bool(clip)), R.ptr(out))
    return out


def _bound_device(v, x):
    """a normalisation bound (scalar, numpy array or tensor) as (contiguous float32 device tensor, n_seg), or None if its shape is neither
    one value nor one value per entry of x's last axis"""
    import torch
    if np.isscalar(v):
        return torch.tensor([np.float32(v)], dtype=torch.float32, device=x.device), 1
    if not R.is_device_tensor(v):
        if R.is_torch(v):
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


def normalize_mi_ma(x, mi, ma, clip=False, eps=1e-20, dtype=np.float32):
    """csbdeep.utils.normalize_mi_ma (csbdeep>=0.8.0, caller side of predict_instances).  numpy in -> numpy out.  A tensor on a HIP device
    in -> a float32 tensor on that device out, with the values of the host expression bit for bit: one fused kernel
    (csrc/normalize.hip) for uint8 / uint16 / float32 data with one bound, or one per entry of the last axis; anything else through the
    host expression."""
    if R.is_device_tensor(x):
        if dtype is np.float32 and str(x.dtype) in _DEVICE_DTYPE_CODE and np.isscalar(eps):
            lo, hi = _bound_device(mi, x), _bound_device(ma, x)
            if lo is not None and hi is not None and lo[1] == hi[1] and 1 <= lo[1] <= 64:
                return _rescale_device(x.contiguous(), lo[0], hi[0], lo[1], clip, eps)
        return R.via_host(normalize_mi_ma, x, mi, ma, clip=clip, eps=eps, dtype=dtype)
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
    if R.is_device_tensor(x):
        res = _normalize_device(x, pmin, pmax, axis, clip, eps, dtype)
        if res is not None:
            return res[0]
        return R.via_host(normalize, x, pmin, pmax, axis=axis, clip=clip, eps=eps, dtype=dtype)
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
    if not R.is_torch(x):
        return _scipy_zoom_linear(x, zoom)
    out_shape = _zoom_out_shape(tuple(x.shape), zoom) if (x.is_cuda and str(x.dtype) in _DEVICE_DTYPE_CODE) else None
    if out_shape is None:
        return R.via_host(_scipy_zoom_linear, x, zoom)
    import ctypes
    import torch
    x = x.contiguous()
    i0, w0, w1 = _zoom_tables_on(x.device, x.shape, out_shape)
    out = torch.empty(out_shape, dtype=x.dtype, device=x.device)
    shapes = (ctypes.c_int * len(out_shape))(*x.shape), (ctypes.c_int * len(out_shape))(*out_shape)
    N.dcall(x, "sd_zoom_linear_device", R.ptr(x), R.ptr(out), _DEVICE_DTYPE_CODE[str(x.dtype)], len(out_shape),
            ctypes.cast(shapes[0], ctypes.c_void_p), ctypes.cast(shapes[1], ctypes.c_void_p), R.ptr(i0), R.ptr(w0), R.ptr(w1))
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
        if R.is_device_tensor(x):
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
        mi, ma = (v.cpu().numpy() if R.is_torch(v) else v for v in (self.mi, self.ma))
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
    import warnings
    import torch
    N.require_device()
    as_np = not R.is_torch(lbl_img)
    # label ids: the kernel keeps one table entry per id up to the largest, in int32.  Ids beyond int32, or sparse huge ids (hash-like
    # labels), are first compacted to 1..n -- the result depends on which pixels share a label, not on the ids
    if as_np:
        a = np.ascontiguousarray(lbl_img)
        if a.size and _ids_need_compaction(int(a.max()), a.size):
            u, inv = np.unique(a, return_inverse=True)
            a = inv.reshape(a.shape).astype(np.int64) + (0 if (len(u) and u[0] == 0) else 1)
            if len(u) and u[0] < 0:
                raise ValueError("edt_prob: negative labels")
        lab = torch.from_numpy(a.astype(np.int32, copy=False)).cuda()
    else:
        t = lbl_img
        if t.numel() and _ids_need_compaction(int(t.max()), t.numel()):
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
    out = torch.empty(lab.shape, dtype=torch.float32, device=lab.device)
    N.dcall(lab, "sd_edt_prob_device", R.ptr(lab), *R.zyx(lab.shape), *((1.0,) + samp if nd == 2 else samp), max(hi, 0), R.ptr(out))
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


# the label-image functions with a host and a device route live in stardist_amd.label_ops; their public names stay importable from here
from .label_ops import (clear_border, find_boundaries, remove_small_objects, select_labels,  # noqa: E402, F401
                        calculate_extents, distance_transform, expand_labels, fill_label_holes, label_components,
                        label_contacts, measure_labels, point_neighbors)
from .spots import gaussian_filter, difference_of_gaussians, peak_local_max, detect_spots  # noqa: E402, F401
from .rank_filters import (minimum_filter, maximum_filter, median_filter, rank_filter, percentile_filter,  # noqa: E402, F401
                           grey_opening, grey_closing, white_tophat, black_tophat)
