"""What the functions with a host route and a device route share (stardist_amd.label_ops, the relabel functions of stardist_amd.geometry,
normalisation and zoom in stardist_amd.utils): what an input is, where a call runs, how an input gets to the device and how a result comes
back like the input.  DESIGN.md section 3p states the rule and the functions' exceptions."""
import math
from types import SimpleNamespace

import numpy as np

from .lib import _native as N

is_torch = N.is_torch
ptr = N.tptr

# element type codes of sd_percentiles_device / sd_normalize_mi_ma_device / sd_zoom_linear_device / sd_label_intensity_stats_device
_DEVICE_DTYPE_CODE = {"torch.uint8": 0, "torch.uint16": 1, "torch.float32": 2}
_DEVICE_LABEL_DTYPES = ("torch.uint8", "torch.int8", "torch.int16", "torch.int32", "torch.int64")


def is_device_tensor(x):
    return is_torch(x) and hasattr(x, "is_cuda") and x.is_cuda


def classify(x, device=None):
    """(x, whether x is a tensor, whether the call runs on the device): anything that is no tensor (a list) becomes a numpy array; the
    call runs on the device for a tensor that lives there and for any input with `device=`"""
    is_t = is_torch(x)
    if not is_t:
        x = np.asarray(x)
    return x, is_t, device is not None or (is_t and x.is_cuda)


def dtype_name(x):
    """the name of x's dtype, the same for an array and a tensor: "int64", "float32" """
    return str(x.dtype).replace("torch.", "")


def _tensor_sqrt(a):
    """the correctly rounded square root of a tensor: torch's on the device; numpy's for a host tensor, where torch's goes through a
    vector maths library that on some CPUs is an ulp off, so that host tensors and numpy arrays give the same bits"""
    import torch
    return torch.sqrt(a) if a.is_cuda else torch.from_numpy(np.sqrt(a.contiguous().numpy()))


_NUMPY_OPS = SimpleNamespace(
    xp=np, is_torch=False, int64=np.dtype("int64"), float64=np.dtype("float64"), astype=lambda a, name: a.astype(name),
    f64=lambda a: np.asarray(a).astype(np.float64), i64=lambda a: np.asarray(a).astype(np.int64),
    col=np.ascontiguousarray, sqrt=np.sqrt, atan2=np.arctan2, cat=lambda arrays, axis=0: np.concatenate(arrays, axis=axis),
    searchsorted=np.searchsorted, zeros_i64=lambda n: np.zeros(n, np.int64), add_at=lambda out, at, v: np.add.at(out, at, v),
    stable_argsort=lambda k: np.argsort(k, kind="stable"), bincount=lambda at, n: np.bincount(at, minlength=n).astype(np.int64),
    clip_max=lambda a, top: np.minimum(a, top))


def _torch_ops(dev):
    import torch
    as_kind = lambda dtype: lambda a: a.to(dev, dtype) if torch.is_tensor(a) else torch.as_tensor(a, dtype=dtype, device=dev)
    return SimpleNamespace(
        xp=torch, is_torch=True, int64=torch.int64, float64=torch.float64, astype=lambda a, name: a.to(getattr(torch, name)),
        f64=as_kind(torch.float64), i64=as_kind(torch.int64),
        col=lambda a: a.contiguous(), sqrt=_tensor_sqrt, atan2=torch.atan2, cat=lambda tensors, axis=0: torch.cat(tensors, dim=axis),
        searchsorted=torch.searchsorted, zeros_i64=lambda n: torch.zeros(n, dtype=torch.int64, device=dev),
        add_at=lambda out, at, v: out.index_add_(0, at, v), stable_argsort=lambda k: torch.sort(k, stable=True)[1],
        bincount=lambda at, n: torch.bincount(at, minlength=n), clip_max=lambda a, top: a.clamp(max=top))


_TORCH_OPS = {}                                                             # per device, made once


def ops(x):
    """The operations that the table functions apply to numpy arrays and to tensors alike, for arrays of x's kind (tensors: on x's
    device).  The routes agree to the bit because each name is one numpy call and the one torch call that computes the same:
    xp (the module, for where / abs / maximum / minimum / ones_like), int64 and float64 (the dtypes), astype(a, name), f64(a) and
    i64(a) (of an array or a sequence), col(a) (contiguous), sqrt (_tensor_sqrt), atan2, cat(arrays, axis), searchsorted, zeros_i64(n), add_at(out, at, v) (in
    place, duplicates add up), stable_argsort, bincount(at, n) (int64, n long), clip_max(a, top)."""
    if not is_torch(x):
        return _NUMPY_OPS
    o = _TORCH_OPS.get(x.device)
    if o is None:
        o = _TORCH_OPS[x.device] = _torch_ops(x.device)
    return o


def table_exit(cols, as_tensors, x=None, device=None):
    """A route's finished columns as the caller asked for them (exception 4): numpy arrays whatever the input's
    kind, tensors with as_tensors.  The device route's tensors become numpy arrays with one stream synchronisation for all of them
    (utils.to_host_many); the host route's arrays become tensors on `device` if given, else where the input x lives if it is a
    tensor, else on the CPU; in every other case the columns pass through.  A None among the columns stays None."""
    cols = list(cols)
    from_device_route = any(is_torch(c) for c in cols)
    if from_device_route and not as_tensors:
        from .utils import to_host_many
        return to_host_many(cols)
    if as_tensors and not from_device_route:
        import torch
        where = torch.device(device) if device is not None else (x.device if is_torch(x) else torch.device("cpu"))
        return [None if c is None else torch.as_tensor(np.ascontiguousarray(c), device=where) for c in cols]
    return cols


def opt_ptr(t):
    """ptr(t), or a null pointer for an optional output that is not asked for"""
    return None if t is None else ptr(t)


def to_device_tensor(x, device=None):
    """the contiguous tensor of x on the device: a numpy array is uploaded to `device` (None: the current one), a tensor is moved there
    if `device` names another place; a bool image travels as uint8 (the same memory)"""
    import torch
    if isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        return torch.as_tensor(a.view(np.uint8) if a.dtype == np.bool_ else a, device=torch.device("cuda" if device is None else device))
    t = (x if device is None else x.to(torch.device(device))).contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def via_host(fn, x, *args, to=None, **kwargs):
    """the host function on a tensor (dtypes and arguments the kernels do not cover): same values, a tensor out, where x lives or on `to`"""
    import torch
    args = [a.cpu().numpy() if is_torch(a) else a for a in args]
    out = torch.as_tensor(np.ascontiguousarray(fn(x.cpu().numpy(), *args, **kwargs)), device=x.device)
    return out if to is None else out.to(torch.device(to))


def like_input(out, x, ids=None):
    """the int32 device tensor `out` as what a caller who passed x expects: a numpy array (one pinned copy, one synchronisation) for a
    numpy array, a tensor where `out` lives for a tensor; of x's dtype, the labels mapped back through _device_labels' ids"""
    if isinstance(x, np.ndarray):
        from .utils import to_host
        res = to_host(out)
        return ids[res] if ids is not None else res.astype(x.dtype, copy=False)
    return ids[out.long()] if ids is not None else out.to(x.dtype)


def original_labels(labels, ids):
    """the ids the image had for the labels in the int64 device tensor `labels`, as an int64 tensor there (ids: as _device_labels
    returns them; None: the labels are the image's own)"""
    import torch
    if ids is None:
        return labels
    ids = ids if is_torch(ids) else torch.as_tensor(ids.astype(np.int64), device=labels.device)
    return ids.to(torch.int64).index_select(0, labels)


def zyx(shape):
    return ((1,) + tuple(shape)) if len(shape) == 2 else tuple(shape)


def spacing_zyx(spacing, nd, who):
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


def check_pixel_count(shape, who):
    if math.prod(shape) > 2 ** 31 - 1:
        raise ValueError("%s: more than 2^31 - 1 pixels" % who)


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
        return to_device_tensor(lab, device), max(top, 0), ids
    t = to_device_tensor(lbl, device)
    top = int(t.max()) if t.numel() else 0
    if _ids_need_compaction(top, t.numel()):
        pos = t > 0
        u, inv = torch.unique(t[pos], return_inverse=True)
        lab = torch.zeros(t.shape, dtype=torch.int32, device=t.device)
        lab[pos] = (inv + 1).to(torch.int32)
        return lab, int(u.numel()), torch.cat([torch.zeros(1, dtype=t.dtype, device=t.device), u])
    return t.clamp(min=0).to(torch.int32).contiguous(), max(top, 0), None


def label_tables(lab, top, boxes=False, sums=False):
    """(boxes, sums) of a contiguous int32 2D / 3D label tensor on the device whose objects are the labels 1 .. top, each None unless
    asked for: the (top + 1, 6) int32 table of sd_label_boxes_device (starts z y x, then exclusive stops z y x; a label
    that is absent has no stop beyond its start) and the (top + 1, 4) int64 table of sd_label_centroid_sums_device (the pixel count,
    then the z, y, x coordinate sums).  The one driver of the two kernels."""
    import torch
    b = s = None
    if boxes:
        b = torch.empty((top + 1, 6), dtype=torch.int32, device=lab.device)
        N.dcall(lab, "sd_label_boxes_device", ptr(lab), *zyx(lab.shape), top, ptr(b))
    if sums:
        s = torch.empty((top + 1, 4), dtype=torch.int64, device=lab.device)
        N.dcall(lab, "sd_label_centroid_sums_device", ptr(lab), *zyx(lab.shape), top, ptr(s))
    return b, s
