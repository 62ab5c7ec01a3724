"""Functions of label images with a host route (numpy + scipy, like the reference's) and a device route (hand-written HIP):
fill_label_holes, calculate_extents, measure_labels, label_components, expand_labels, distance_transform, find_boundaries, clear_border,
remove_small_objects, select_labels, label_contacts -- and point_neighbors, which takes the objects' centroids.  stardist_amd.utils
re-exports the public names.  Which route a call takes and what comes back is one rule, DESIGN.md section 3p, and its code is stardist_amd._route;
a `_X_device` half here allocates its outputs and calls its kernels."""
import numpy as np

from . import _route as R
from ._route import _DEVICE_DTYPE_CODE, _DEVICE_LABEL_DTYPES, _ids_need_compaction
from .lib import _native as N


def _object_boxes(lbl_img):
    """[(label id, bounding-box slices)] of the labels present, ascending (scipy.ndimage.find_objects: entry i - 1 belongs to label i)"""
    from scipy.ndimage import find_objects
    return [(i, sl) for i, sl in enumerate(find_objects(lbl_img), 1) if sl is not None]


# ----------------------------------------------------------------------------- fill_label_holes, calculate_extents
# (stardist/__init__.py:13 exports them; csrc/fill_holes.hip)

def _fill_label_holes_device(lbl_img, device=None):
    """fill_label_holes through sd_fill_label_holes_device; numpy in (uploaded to `device`) -> numpy out, tensor in -> tensor out, of the
    input's dtype and shape; the input is never written"""
    import torch
    N.require_device()
    if lbl_img.ndim not in (2, 3):
        raise ValueError("fill_label_holes: a label image on the device must be 2D or 3D")
    lab, top, ids = R._device_labels(lbl_img, device)
    out = torch.empty_like(lab)
    if lab.numel():
        Z, Y, X = R.zyx(lab.shape)
        if lab.dim() == 3 and Z == 1:
            # one plane given as a volume: along z every pixel lies on the box's outer layer, so nothing is a hole (the host function
            # says the same); the library takes Z = 1 for a 2D image, so the plane goes in as the volume (Y, 1, X) -- the same memory
            Z, Y = Y, 1
        N.dcall(lab, "sd_fill_label_holes_device", R.ptr(lab), Z, Y, X, top, R.ptr(out))
    res = R.like_input(out, lbl_img, ids)
    return res if isinstance(lbl_img, np.ndarray) else res.to(lbl_img.device)         # section 3p, exception 1


def _label_boxes_device(t):
    """(n present, ndim) int64 numpy array of the bounding-box sizes of the labels of a 2D / 3D device tensor, by ascending label
    (sd_label_boxes_device; only the box table comes to the host)"""
    import torch
    from .utils import to_host
    N.require_device()
    nd = t.dim()
    if t.numel() == 0:
        return np.zeros((0, nd), np.int64)
    if str(t.dtype) not in _DEVICE_LABEL_DTYPES:
        t = t.to(torch.int64)
    lab, top, _ = R._device_labels(t)
    b = to_host(R.label_tables(lab, top, boxes=True)[0]).astype(np.int64)
    b = b[b[:, 5] > b[:, 2]]
    return (b[:, 3:] - b[:, :3])[:, 3 - nd:]


def fill_label_holes(lbl_img, *, device=None, **kwargs):
    """Fill the holes of every labelled object (stardist/utils.py:137-153): per object, `binary_fill_holes` of its mask on its bounding
    box grown by one pixel on every side that is not an image border -- a cavity that reaches the image border stays open, as there.
    **kwargs go to scipy.ndimage.binary_fill_holes.

    Routing: DESIGN.md section 3p; the device route takes 2D / 3D integer images and equals the host result (csrc/fill_holes.hip:
    bounding boxes in one pass, then per object two bit planes and a flood from the box's outer layer; the input is not written).  Its
    own: the kernels implement the default structure, so with any **kwargs a tensor goes through the host function and comes back as a
    tensor, and a numpy array takes the host code; a tensor's result lives where the tensor lives, whatever `device=` says (exceptions
    1 and 2 there).  Ids beyond int32, or sparse huge ids, are compacted in ascending order for the call and mapped back."""
    if R.is_torch(lbl_img):
        on_device = lbl_img.is_cuda or device is not None
        if kwargs or not on_device or str(lbl_img.dtype) not in _DEVICE_LABEL_DTYPES:
            return R.via_host(fill_label_holes, lbl_img, **kwargs)
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


def calculate_extents(lbl, func=np.median):
    """Aggregate (median by default) of the objects' bounding-box sizes per axis, for one 2D / 3D label image, or over a sequence / 4D
    stack of them (stardist/utils.py:180-193).  Label images that are tensors on a HIP device stay there: one sd_label_boxes_device call
    per image, the box table comes to the host and `func` runs over the extents as for host input.  There is no `device=` (DESIGN.md
    section 3p, exception 3)."""
    from collections.abc import Iterable
    if R.is_device_tensor(lbl):
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
# Both routes produce the same "raw" columns, as numpy arrays or as tensors: _measure_schema states their keys, widths and dtypes, once,
# for the host half's allocations, the device half's empty table and the packed form in which a table travels (_measure_pack,
# _measure_unpack).  _measure_columns derives the table from them, the one place where centroid, mean and std are computed.  csum holds
# the coordinate sums; m2 the second-order sums of the box-local coordinates in the order zz, zy, zx, yy, yx, xx and, for a 2D image,
# contour = [n_1, n_r2, n_h, h_1 .. h_15], the contour-pixel classes and the 2 x 2 configuration histogram (csrc/measure_shape.h), from
# which _shape_columns derives the shape columns; hull = [convex_area, F2] (csrc/measure_hull.h), from which
# _hull_columns derives the hull columns.
# With percentiles both routes add pct (n, C, n_q): float64 for integer images, else the image's float type.  It is no part of the packed
# table: it travels as an array of its own.  _MAX_PERCENTILES is csrc/measure_rank.h's MR_MAX_Q.
_MAX_PERCENTILES = 8
_M2_INDEX = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}
_CONTOUR_WIDTH = 18
# the counter a border pixel with a / d border neighbours along the axes / the diagonals counts into (-1: none): n_1, n_r2, n_h
_CONTOUR_CLASS = np.full((5, 5), -1, np.int8)
_CONTOUR_CLASS[2:4, 0:3] = 0
_CONTOUR_CLASS[0, 2] = _CONTOUR_CLASS[1, 3] = 1
_CONTOUR_CLASS[1, 1:3] = 2
# skimage.measure.perimeter_crofton(., 4)'s coefficient of every 2 x 2 configuration, written as scikit-image writes them
_CROFTON = [float(w) for w in (0, np.pi / 4 * (1 + 1 / (np.sqrt(2))), np.pi / (4 * np.sqrt(2)), np.pi / (2 * np.sqrt(2)), 0,
                                np.pi / 4 * (1 + 1 / (np.sqrt(2))), 0, np.pi / (4 * np.sqrt(2)), np.pi / 4, np.pi / 2,
                                np.pi / (4 * np.sqrt(2)), np.pi / (4 * np.sqrt(2)), np.pi / 4, np.pi / 2, 0, 0)]
_SQRT2 = float(np.sqrt(2))
_JACOBI_SWEEPS = 6
_HULL_MAX_EXTENT = 2 ** 30                                                   # csrc/measure_hull.h's MH_MAX_EXTENT


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


def _measure_schema(nd, C, mm_dtype, shape=False, hull=False):
    """[(key, width, dtype name)] of the raw columns, in their order: a column is (n, width), or (n,) where the width is None.  C: the
    number of channels, None without an image; mm_dtype: the name of the dtype of min and max -- the image's for a float image, for
    which sum and sum2 are float64, else int64 like everything else"""
    cols = [("label", None, "int64"), ("area", None, "int64"), ("bbox", 2 * nd, "int64"), ("csum", nd, "int64")]
    if C is not None:
        sum_dtype = "float64" if "float" in mm_dtype else "int64"
        cols += [("sum", C, sum_dtype), ("sum2", C, sum_dtype), ("min", C, mm_dtype), ("max", C, mm_dtype)]
    if shape:
        cols += [("m2", 6, "int64")] + ([("contour", _CONTOUR_WIDTH, "int64")] if nd == 2 else [])
    if hull:
        cols += [("hull", 2, "int64")]
    return cols


def _as_bits(o, a):
    """int64 as it is, a float array / tensor as the bits of its float64 value (o: R.ops of a)"""
    return o.col(o.f64(a)).view(o.int64) if "float" in str(a.dtype) else o.i64(a)


def _from_bits(o, a, dtype):
    return o.astype(o.col(a).view(o.float64), dtype) if "float" in dtype else o.col(a)


def _measure_pack(raw, schema):
    """the raw columns side by side as one (n, K) int64 array / tensor (_as_bits): one copy moves it"""
    o = R.ops(raw["label"])
    return o.col(o.cat([_as_bits(o, raw[key] if w else raw[key].reshape(-1, 1)) for key, w, _ in schema], 1))


def _measure_unpack(packed, schema):
    """the raw columns of _measure_pack's array"""
    o, raw, at = R.ops(packed), {}, 0
    for key, w, dtype in schema:
        a = _from_bits(o, packed[:, at:at + (w or 1)], dtype)
        at += w or 1
        raw[key] = a.reshape(-1) if w is None else a
    return raw


def _measure_columns(raw, nd, channel_axis, qs=None):
    """the table of measure_labels from the raw columns (numpy arrays or tensors): centroid = float64(coordinate sum) / count, mean =
    float64(sum) / count, var = max(0, float64(sum2) / count - mean^2), std = sqrt(var), every operation rounded on its own; qs: the
    percentiles of raw["pct"] (n, C, len(qs)), whose columns come after the intensity columns"""
    o = R.ops(raw["label"])
    f64, sqrt, col = o.f64, o.sqrt, o.col
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
    if qs:
        for j, q in enumerate(qs):
            name = "p%g_intensity" % q
            if ("%s-0" % name if channel_axis else name) in out:            # a duplicate q: the column is there already
                continue
            for c in range(raw["pct"].shape[1]):
                out[("%s-%d" % (name, c)) if channel_axis else name] = col(raw["pct"][:, c, j])
    if "m2" in raw:
        _shape_columns(out, raw, nd)
    if "hull" in raw:
        _hull_columns(out, raw)
    return out


def _jacobi_eigvals(T, o):
    """eigenvalues of the symmetric matrices T[i][j] (arrays / tensors of one length), unsorted: _JACOBI_SWEEPS cyclic Jacobi sweeps of
    + - * / sqrt, comparisons and selects, the same code for numpy and torch (o: their R.ops).  A zero off-diagonal element is left
    alone; an angle whose square would overflow takes its limit t = 1 / (2 theta)."""
    xp, sqrt = o.xp, o.sqrt
    n = len(T)
    T = [list(row) for row in T]
    for _ in range(_JACOBI_SWEEPS):
        for p in range(n):
            for q in range(p + 1, n):
                apq, one = T[p][q], xp.ones_like(T[p][q])
                zero = apq == 0
                theta = (T[q][q] - T[p][p]) / xp.where(zero, one, 2.0 * apq)
                big = xp.abs(theta) > 1e150
                th = xp.where(big, one, theta)
                t = xp.where(th < 0, -one, one) / (xp.abs(th) + sqrt(th * th + 1.0))
                t = xp.where(big, (0.5 * one) / xp.where(big, theta, one), t)
                t = xp.where(zero, 0.0 * one, t)
                c = one / sqrt(t * t + 1.0)
                s = t * c
                T[p][p], T[q][q] = T[p][p] - t * apq, T[q][q] + t * apq
                T[p][q] = T[q][p] = 0.0 * one
                for r in range(n):
                    if r not in (p, q):
                        arp, arq = T[r][p], T[r][q]
                        T[r][p] = T[p][r] = c * arp - s * arq
                        T[r][q] = T[q][r] = s * arp + c * arq
    return [T[d][d] for d in range(n)]


def _shape_columns(out, raw, nd):
    """adds the shape columns to the table `out` from the raw columns (numpy arrays or tensors), DESIGN.md section 3q: every operation
    is rounded on its own, in the order written there; only orientation (atan2) and the 3D equivalent_diameter (pow) call a maths
    library, everything else is + - * / sqrt, comparisons and selects and so has the same bits on every route"""
    o = R.ops(raw["label"])
    xp, f64, col, atan2, sqrt = o.xp, o.f64, o.col, o.atan2, o.sqrt
    with np.errstate(all="ignore"):
        area = raw["area"]
        A = f64(area)
        start, stop = raw["bbox"][:, :nd], raw["bbox"][:, nd:]
        s = [f64(raw["csum"][:, d] - area * start[:, d]) for d in range(nd)]
        m2 = lambda i, j: f64(raw["m2"][:, _M2_INDEX[(i + 3 - nd, j + 3 - nd)]])
        mu = {(i, j): m2(i, j) - s[i] * s[j] / A for i in range(nd) for j in range(i, nd)}
        tr = mu[(0, 0)]
        for d in range(1, nd):
            tr = tr + mu[(d, d)]
        T = [[((tr - mu[(i, i)]) / A) if i == j else (-mu[(min(i, j), max(i, j))] / A) for j in range(nd)] for i in range(nd)]
        lam = [xp.where(l > 0, l, 0.0 * l) for l in _jacobi_eigvals(T, o)]
        # descending by a sorting network of maxima and minima
        for i, j in (((0, 1),) if nd == 2 else ((0, 1), (1, 2), (0, 1))):
            lam[i], lam[j] = xp.maximum(lam[i], lam[j]), xp.minimum(lam[i], lam[j])
        box = stop[:, 0] - start[:, 0]
        for d in range(1, nd):
            box = box * (stop[:, d] - start[:, d])
        # (every division is array by array: torch divides a device tensor by a Python number by multiplying with its reciprocal)
        one = xp.ones_like(A)
        out["equivalent_diameter"] = sqrt(f64(4 * area) / (np.pi * one)) if nd == 2 else (f64(6 * area) / (np.pi * one)) ** (1.0 / 3.0)
        out["extent"] = A / f64(box)
        for i in range(nd):
            for j in range(nd):
                out["inertia_tensor-%d-%d" % (i, j)] = col(T[i][j])
        for k in range(nd):
            out["inertia_tensor_eigvals-%d" % k] = col(lam[k])
        out["major_axis_length"] = 4.0 * sqrt(lam[0])
        out["minor_axis_length"] = 4.0 * sqrt(lam[-1])
        if nd == 2:
            degenerate = lam[0] == 0
            out["eccentricity"] = xp.where(degenerate, 0.0 * one, sqrt(1.0 - lam[1] / xp.where(degenerate, one, lam[0])))
            a, b, c = T[0][0], T[0][1], T[1][1]
            out["orientation"] = xp.where(a - c == 0, xp.where(b < 0, (np.pi / 4) * one, (-np.pi / 4) * one), 0.5 * atan2(-2.0 * b, c - a))
            n = f64(raw["contour"])
            out["perimeter"] = n[:, 0] + n[:, 1] * _SQRT2 + n[:, 2] * ((1 + _SQRT2) / 2)
            crofton = n[:, 3] * _CROFTON[1]
            for k in range(2, 16):
                crofton = crofton + n[:, 2 + k] * _CROFTON[k]
            out["perimeter_crofton"] = crofton
            h = raw["contour"]
            out["euler_number"] = col(h[:, 2 + 8] - h[:, 2 + 6] - h[:, 2 + 14])
    return out


def _hull_columns(out, raw):
    """adds the hull columns to the table `out` from the raw columns (numpy arrays or tensors), DESIGN.md section 3u: convex_area as it
    is, solidity = float64(area) / float64(convex_area), feret_diameter_max = sqrt(float64(F2) / 4), every operation rounded on its own"""
    o = R.ops(raw["label"])
    f64, col, sqrt = o.f64, o.col, o.sqrt
    convex = col(raw["hull"][:, 0])
    f2 = f64(raw["hull"][:, 1])
    out["convex_area"] = convex
    out["solidity"] = f64(raw["area"]) / f64(convex)
    out["feret_diameter_max"] = sqrt(f2 / 4.0)                              # (a power of two: exact also as a product with 0.25)
    return out


def _hull_chain(points, side):
    """the left (side < 0) or right chain of the hull of `points` [(y, x)], ascending in y: csrc/measure_hull.h's chain_step"""
    st = []
    for p in points:
        while len(st) >= 2:
            a, b = st[-2], st[-1]
            c = (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
            if (c > 0) if side < 0 else (c < 0):
                break
            st.pop()
        st.append(p)
    return st


def _hull_chains(first, last):
    """(left chain, right chain) of the hull of the diamond points of a row table -- first[j] .. last[j] the columns of row j, first >
    last for a row without a pixel -- in doubled coordinates with row 0 at y = 0: level k = 0 .. 2 h lies at y = k - 1"""
    h = len(first)
    left, right = [], []
    for k in range(2 * h + 1):
        j = k >> 1
        if k & 1:
            if first[j] <= last[j]:
                left.append((k - 1, 2 * first[j] - 1))
                right.append((k - 1, 2 * last[j] + 1))
        else:
            rows = [r for r in (j - 1, j) if 0 <= r < h and first[r] <= last[r]]
            if rows:
                left.append((k - 1, 2 * min(first[r] for r in rows)))
                right.append((k - 1, 2 * max(last[r] for r in rows)))
    return _hull_chain(left, -1), _hull_chain(right, 1)


def _hull_chain_at(st, ys, y):
    """the chain's x at the height y as (numerator, denominator > 0); None outside the chain's heights"""
    from bisect import bisect_right
    if not st or y < ys[0] or y > ys[-1]:
        return None
    i = bisect_right(ys, y)                                                 # st[i - 1]: the last vertex at or above y
    a = st[i - 1]
    if a[0] == y:
        return a[1], 1
    b = st[i]
    den = b[0] - a[0]
    return a[1] * den + (b[1] - a[1]) * (y - a[0]), den


def _hull_of_rows(first, last):
    """(convex_area, F2) of the object with the row table first, last (lists of Python integers): the definition of DESIGN.md section
    3u in Python integers, stage by stage as csrc/measure_hull.h"""
    h = len(first)
    left, right = _hull_chains(first, last)
    ly, ry = [p[0] for p in left], [p[0] for p in right]
    cfirst, clast, area = [], [], 0
    for j in range(h):
        lo, hi = _hull_chain_at(left, ly, 2 * j), _hull_chain_at(right, ry, 2 * j)
        a, b = 1, 0
        if lo is not None and hi is not None:
            a, b = -((-lo[0]) // (2 * lo[1])), hi[0] // (2 * hi[1])          # ceil(xl / 2), floor(xr / 2)
            if a > b:
                a, b = 1, 0
        cfirst.append(a)
        clast.append(b)
        area += b - a + 1
    left, right = _hull_chains(cfirst, clast)
    v = left + right
    if len(v) <= 48:
        f2 = max([(p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 for i, p in enumerate(v) for q in v[i + 1:]] or [0])
    else:
        vy, vx = np.array([p[0] for p in v], np.int64), np.array([p[1] for p in v], np.int64)
        f2 = max(int(((vy[i + 1:] - vy[i]) ** 2 + (vx[i + 1:] - vx[i]) ** 2).max()) for i in range(len(v) - 1))
    return area, f2


def _hull_raw_host(lab, boxes):
    """hull (n, 2) int64 = [convex_area, F2] of the objects `boxes` [(label, slices)] of the 2D non-negative integer image lab"""
    out = np.zeros((len(boxes), 2), np.int64)
    for k, (l, box) in enumerate(boxes):
        mask = lab[box] == l
        w = mask.shape[1]
        has = mask.any(axis=1)
        first = np.where(has, mask.argmax(axis=1), 1)
        last = np.where(has, w - 1 - mask[:, ::-1].argmax(axis=1), 0)
        out[k] = _hull_of_rows(first.tolist(), last.tolist())
    return out


_NEIGHBOR_NAMES = ("neighbors", "contact_objects", "contact_background")      # the columns of measure_labels(neighbors=), after all others


def _shape_raw_host(lab, rows, starts):
    """(m2 (n, 6), contour (n, 18) or None for a volume) of the labels `rows` (ascending, all that are present) of the non-negative
    integer image lab, starts (n, nd) their boxes' starts: the definitions of csrc/measure_shape.h by numpy on the whole image"""
    nd, n = lab.ndim, len(rows)
    m2 = np.zeros((n, 6), np.int64)
    contour = np.zeros((n, _CONTOUR_WIDTH), np.int64) if nd == 2 else None
    if n == 0:
        return m2, contour
    row_of = np.zeros(int(rows[-1]) + 1, np.int64)
    row_of[rows] = np.arange(n)
    where = np.nonzero(lab)
    r = row_of[lab[where]]
    u = [w.astype(np.int64) - starts[r, d] for d, w in enumerate(where)]
    for i in range(nd):
        for j in range(i, nd):
            np.add.at(m2[:, _M2_INDEX[(i + 3 - nd, j + 3 - nd)]], r, u[i] * u[j])
    if nd == 3:
        return m2, None
    Y, X = lab.shape
    count = lambda labels, field: np.bincount(row_of[labels] * _CONTOUR_WIDTH + field, minlength=n * _CONTOUR_WIDTH).reshape(n, _CONTOUR_WIDTH)
    # border pixels, one pixel beyond the image too (where there are none): a pixel of l with a 4-neighbour that is not l
    P = np.pad(lab, 2)
    c = P[1:-1, 1:-1]
    B = (c > 0) & ((P[:-2, 1:-1] != c) | (P[2:, 1:-1] != c) | (P[1:-1, :-2] != c) | (P[1:-1, 2:] != c))
    near = lambda dy, dx: ((P[2 + dy:2 + dy + Y, 2 + dx:2 + dx + X] == lab) & B[1 + dy:1 + dy + Y, 1 + dx:1 + dx + X]).astype(np.uint8)
    a = near(-1, 0) + near(1, 0) + near(0, -1) + near(0, 1)
    d = near(-1, -1) + near(-1, 1) + near(1, -1) + near(1, 1)
    cls = _CONTOUR_CLASS[a, d]
    sel = B[1:-1, 1:-1] & (cls >= 0)
    contour += count(lab[sel], cls[sel].astype(np.int64))
    # 2 x 2 windows at i in [0, Y], j in [0, X]: bit 1 L(i, j), bit 2 L(i-1, j), bit 4 L(i, j-1), bit 8 L(i-1, j-1); every label of
    # a window is counted at its first pixel in bit order
    Q = np.pad(lab, 1)
    w = [Q[1:, 1:], Q[:-1, 1:], Q[1:, :-1], Q[:-1, :-1]]
    for k in range(4):
        lead = w[k] > 0
        for m in range(k):
            lead &= w[m] != w[k]
        code = sum((w[m] == w[k]).astype(np.uint8) << m for m in range(4))
        contour += count(w[k][lead], 2 + code[lead].astype(np.int64))
    return m2, contour


def _percentile_list(percentiles, has_img):
    """the percentiles of measure_labels as a tuple of Python floats (None for None); raises its ValueErrors"""
    if percentiles is None:
        return None
    try:
        qs = tuple(float(q) for q in percentiles)
    except TypeError:
        raise ValueError("measure_labels: percentiles must be None or a sequence of real numbers, got %r" % (percentiles,))
    if not 1 <= len(qs) <= _MAX_PERCENTILES:
        raise ValueError("measure_labels: percentiles takes 1 to %d values, got %d" % (_MAX_PERCENTILES, len(qs)))
    if not all(np.isfinite(q) and 0.0 <= q <= 100.0 for q in qs):
        raise ValueError("measure_labels: percentiles must be finite and in the range [0, 100], got %r" % (qs,))
    if not has_img:
        raise ValueError("measure_labels: percentiles needs the image `img`")
    return qs


def _measure_raw_host(lbl, img, shape=False, percentiles=None, hull=False):
    """the raw columns by numpy over scipy.ndimage.find_objects boxes; img: None or an array of lbl.shape (+ (C,)); shape: with m2 and,
    for a 2D image, contour (_shape_raw_host); hull: with hull (_hull_raw_host); percentiles: a tuple of Python floats, with pct (n, C,
    len(percentiles)) = np.percentile(values of the object in the channel, q), one q at a time"""
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
    C = None if img is None else 1 if img.ndim == nd else img.shape[-1]
    exact = img is not None and img.dtype.kind in "iub"
    raw = {key: np.zeros((n,) if w is None else (n, w), dtype)              # (m2, contour and hull come whole from their functions)
           for key, w, dtype in _measure_schema(nd, C, None if img is None else "int64" if exact else img.dtype.name)}
    raw["label"] = np.array([k for k, _ in boxes], np.int64).reshape(n)
    if ids is not None:
        raw["label"] = ids.astype(np.int64)[raw["label"] - 1]
    if img is not None:
        if percentiles:
            if img.dtype.kind == "b":
                img = img.astype(np.uint8)
            # integer images: float64; float32: float32 (an older numpy interpolates in float64, rounded here); else numpy's type
            pct_dtype = (np.float64 if exact else np.float32 if img.dtype == np.float32
                         else np.asarray(np.percentile(np.zeros(1, img.dtype), 50.0)).dtype)
            raw["pct"] = np.zeros((n, C, len(percentiles)), pct_dtype)
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
                if percentiles:
                    for c in range(C):
                        for j, q in enumerate(percentiles):
                            raw["pct"][k, c, j] = np.percentile(v[:, c], q)
    if shape:
        m2, contour = _shape_raw_host(lab, np.array([k for k, _ in boxes], np.int64), raw["bbox"][:, :nd])
        raw["m2"] = m2
        if contour is not None:
            raw["contour"] = contour
    if hull:
        raw["hull"] = _hull_raw_host(lab, boxes)
    return raw


def _measure_raw_device(lbl, img, C, device, shape=False, percentiles=None, hull=False):
    """the raw columns as tensors on the device: sd_label_boxes_device, sd_label_centroid_sums_device, with an image
    sd_label_intensity_stats_device, with percentiles sd_label_percentiles_device and with shape sd_label_moment_sums_device and (2D)
    sd_label_contour_counts_device, with hull sd_label_hull_device (which reads two scalars back to size its row table), then the rows
    of the labels present (one scalar, their number, comes to the host)"""
    import torch
    N.require_device()
    lab, top, ids = R._device_labels(lbl, device)
    dev, nd = lab.device, lab.dim()
    code = None
    if img is not None:
        img = R.to_device_tensor(img, dev)                                  # an image that is elsewhere is moved to the labels' device
        code = _DEVICE_DTYPE_CODE[str(img.dtype)]
    sum_t, mm_t = (torch.float64, torch.float32) if code == 2 else (torch.int64, torch.int32)
    pct_t = torch.float32 if code == 2 else torch.float64
    if lab.numel() == 0 or top <= 0:
        schema = _measure_schema(nd, C, "float32" if code == 2 else "int64", shape, hull)
        raw = {key: torch.zeros((0,) if w is None else (0, w), dtype=getattr(torch, dtype), device=dev) for key, w, dtype in schema}
        if percentiles:
            raw["pct"] = torch.zeros((0, C, len(percentiles)), dtype=pct_t, device=dev)
        return raw
    boxes, sums = R.label_tables(lab, top, boxes=True, sums=True)
    if img is not None:
        acc = torch.empty((top + 1, C, 2), dtype=sum_t, device=dev)
        mm = torch.empty((top + 1, C, 2), dtype=mm_t, device=dev)
        N.dcall(lab, "sd_label_intensity_stats_device", R.ptr(lab), *R.zyx(lab.shape), top, R.ptr(boxes), R.ptr(img), code, C,
                R.ptr(acc) if code != 2 else None, R.ptr(acc) if code == 2 else None, R.ptr(mm))
        if percentiles:
            import ctypes
            from .utils import _interp_mode
            pct = torch.empty((top + 1, C, len(percentiles)), dtype=torch.float64, device=dev)
            q = (ctypes.c_double * len(percentiles))(*percentiles)
            N.dcall(lab, "sd_label_percentiles_device", R.ptr(lab), *R.zyx(lab.shape), top, R.ptr(boxes), R.ptr(img), code, C,
                    ctypes.cast(q, ctypes.c_void_p), len(percentiles), _interp_mode(img, percentiles[0]), R.ptr(pct))
    present = torch.nonzero(sums[:, 0]).reshape(-1)
    s = sums.index_select(0, present)
    b = boxes.index_select(0, present).to(torch.int64)
    raw = {"label": R.original_labels(present, ids), "area": s[:, 0].contiguous(), "bbox": b if nd == 3 else b[:, [1, 2, 4, 5]], "csum": s[:, 4 - nd:]}
    if img is not None:
        a, m = acc.index_select(0, present), mm.index_select(0, present)
        raw.update(sum=a[:, :, 0], sum2=a[:, :, 1], min=m[:, :, 0] if code == 2 else m[:, :, 0].to(torch.int64),
                   max=m[:, :, 1] if code == 2 else m[:, :, 1].to(torch.int64))
        if percentiles:
            raw["pct"] = pct.index_select(0, present).to(pct_t)             # a float32 result came widened to double: narrowed back
    if shape:
        m2 = torch.empty((top + 1, 6), dtype=torch.int64, device=dev)
        N.dcall(lab, "sd_label_moment_sums_device", R.ptr(lab), *R.zyx(lab.shape), top, R.ptr(boxes), R.ptr(m2))
        raw["m2"] = m2.index_select(0, present)
        if nd == 2:
            counts = torch.empty((top + 1, _CONTOUR_WIDTH), dtype=torch.int64, device=dev)
            N.dcall(lab, "sd_label_contour_counts_device", R.ptr(lab), *lab.shape, top, R.ptr(counts))
            raw["contour"] = counts.index_select(0, present)
    if hull:
        table = torch.empty((top + 1, 2), dtype=torch.int64, device=dev)
        N.dcall(lab, "sd_label_hull_device", R.ptr(lab), *lab.shape, top, R.ptr(boxes), R.ptr(table))
        raw["hull"] = table.index_select(0, present)
    return raw


def _proximity_args(nearest, within, spacing, nd):
    """(k, radius, r2, per-axis spacing) of measure_labels' nearest=, within= and spacing=, checked; spacing without the two is refused"""
    if nearest is None and within is None:
        if not (np.ndim(spacing) == 0 and not isinstance(spacing, (str, bytes)) and spacing == 1):
            raise ValueError("measure_labels: spacing applies to nearest= and within= only; give one of them")
        return None, None, None, None
    k = radius = r2 = None
    if nearest is not None:
        k = _point_neighbors_args(nearest, None, False, "measure_labels: nearest")[0]
    if within is not None:
        _, radius, r2 = _point_neighbors_args(None, within, False, "measure_labels: within")
    return k, radius, r2, R.spacing_zyx(spacing, nd, "measure_labels")[1]


def _proximity_names(k, radius):
    names = [n % j for j in range(k or 0) for n in ("nearest_label-%d", "nearest_distance-%d")]
    return names + (["neighbors_within"] if radius is not None else [])


def _proximity_columns(label, csum, area, k, radius, r2, per_axis):
    """the columns of _proximity_names from the objects' labels, coordinate sums and pixel counts (numpy arrays, or tensors on the
    device): point_neighbors over the centroids float64(sum) / count times the spacing, the points their own queries; an index becomes
    the label of that row, 0 where there is none"""
    o = R.ops(label)
    P = o.col(o.f64(csum) / o.f64(area)[:, None] * o.f64(per_axis))
    cols = []
    if k is not None:
        idx, d2 = _point_neighbors_device(P, None, 0, k, None) if o.is_torch else _nearest_host(P, P, True, k, None)
        lab = o.xp.where(idx >= 0, label[idx.clip(min=0)] if len(label) else idx, 0 * idx)
        dist = o.sqrt(d2)
        for j in range(k):
            cols += [o.col(lab[:, j]), o.col(dist[:, j])]
    if radius is not None:
        cols.append(_point_neighbors_device(P, None, 1, None, r2) if o.is_torch else _within_host(P, P, True, radius, r2, True)[0])
    return cols


def _spot_coords(spots, nd):
    """measure_labels' spots= as an (n, nd) integer array or tensor, checked"""
    if not R.is_torch(spots):
        spots = np.asarray(spots)
        if spots.size == 0 and spots.ndim == 2 and spots.shape[1] == nd:
            spots = spots.astype(np.int64)
    integer = (not spots.dtype.is_floating_point and str(spots.dtype) != "torch.bool") if R.is_torch(spots) else spots.dtype.kind in "iu"
    if len(spots.shape) != 2 or int(spots.shape[1]) != nd or not integer:
        raise ValueError("measure_labels: spots must be (n, %d) integer coordinates, got shape %r of %s" % (nd, tuple(spots.shape), spots.dtype))
    return spots


def _spot_counts(label, lbl, coords):
    """the spot_count column: for every row of the label column `label` (ascending ids) the number of rows of `coords` whose pixel of
    the label image `lbl` carries that id -- gather, search in the label column, bincount; numpy arrays, or tensors on one device"""
    o = R.ops(label)
    c = o.i64(coords)
    if len(c) and bool(((c < 0) | (c >= o.i64([int(n) for n in lbl.shape]))).any()):
        raise ValueError("measure_labels: a coordinate of spots lies outside the image")
    if R.dtype_name(lbl) == "uint16" and o.is_torch:                        # (torch does not index a uint16 tensor)
        lbl = o.astype(lbl, "int32")
    ids = o.i64(lbl[tuple(c.T)])
    if not len(label):
        return o.zeros_i64(0)
    at = o.clip_max(o.searchsorted(label, ids), len(label) - 1)
    hit = (ids > 0) & (label[at] == ids)
    return o.bincount(at[hit], len(label))


def measure_labels(lbl, img=None, *, shape=False, hull=False, percentiles=None, neighbors=None, nearest=None, within=None, spacing=1,
                   spots=None, device=None, as_tensors=False):
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
      with percentiles=(q, ...), after the intensity columns, in the order given (a q given twice gives one column):
        p<q>_intensity         float64 (integer images) / the image's float type; <q> as "%g" writes it: p50_intensity, p99.8_intensity
      with shape=True, after the columns above (pixel units; float64 but for euler_number, int64):
        equivalent_diameter    sqrt(4 area / pi); 3D: (6 area / pi) ** (1 / 3)
        extent                 area / volume of the bounding box
        inertia_tensor-i-j     all nd^2 entries, from the second-order sums of the box-local coordinates
        inertia_tensor_eigvals-k   descending, clipped at 0 (six cyclic Jacobi sweeps)
        major_axis_length, minor_axis_length   4 sqrt(largest / smallest eigenvalue)
      and for a 2D image:
        eccentricity           sqrt(1 - l_1 / l_0), 0 where l_0 = 0
        orientation            0.5 atan2(-2 b, c - a) of the tensor [[a, b], [b, c]]; where a - c == 0: pi / 4 for b < 0, else -pi / 4
        perimeter              skimage.measure.perimeter(mask, 4)
        perimeter_crofton      skimage.measure.perimeter_crofton(mask, 4)
        euler_number           skimage.measure.euler_number(mask, connectivity=2)
      with hull=True (2D images only; it does not need shape), after the columns above:
        convex_area            int64    pixels of the convex image, counted over the object's box (pixels of other labels count)
        solidity               float64  float64(area) / float64(convex_area)
        feret_diameter_max     float64  sqrt(float64(F2) / 4), F2 the largest squared distance between two contour points, doubled
      with neighbors=c (a connectivity, 1 .. ndim), after all columns above (int64; from label_contacts(lbl, c, background=True)):
        neighbors              the number of other objects the object is in contact with
        contact_objects        its contacts with other objects, summed
        contact_background     its contacts with the background, value 0
      A negative label raises ValueError with neighbors=, as in label_contacts.
      with nearest=k (1 .. 64), after all columns above, for j = 0 .. k - 1 (the k nearest other objects by centroid, in the order
      (squared distance, row) of point_neighbors, whose definition they follow):
        nearest_label-j        int64    the label of the j-th nearest other object, 0 where there is none
        nearest_distance-j     float64  the distance between the two centroids, inf where there is none
      with within=r (finite, >= 0), after those:
        neighbors_within       int64    the number of other objects whose centroid lies within r of the object's
      spacing (a positive scalar or one value per axis, default 1) scales the centroids for these two keywords only -- the centroid-*
      columns stay in pixels -- and raises ValueError without them.  The two are point_neighbors(centroids, k, spacing=spacing) and
      point_neighbors(centroids, radius=r, spacing=spacing, count_only=True) over the table's own centroid columns; on the device
      route the centroids stay on the device (the read-backs of point_neighbors' device route apply: the box of the points, once per
      keyword).
      with spots=coords ((n, ndim) integer coordinates, numpy or tensor: peak_local_max's), after every column above:
        spot_count             int64    the number of rows of coords whose pixel carries the object's label
      Rows on the background count for nobody, a coordinate given twice counts twice; a coordinate outside the image raises
      ValueError.  On the device route the column is made there by tensor operations (gather, search, bincount), one flag comes to
      the host for that check.

    The shape columns are scikit-image 0.18's regionprops_table columns of these names, computed from integer tables per object
    (second-order coordinate sums, three counts of contour-pixel classes, a histogram of 2 x 2 pixel configurations: DESIGN.md section
    3q), on which the routes agree exactly.  One deviation, on purpose: where a - c == 0 scikit-image 0.18.3 returns -pi / 4 for b < 0 and
    pi / 4 otherwise, which is 90 degrees from the limit of its own general formula; this function returns the limit.  A call with
    shape=True whose pixel count times the square of the largest extent reaches 2^63 raises ValueError before anything runs.

    The hull columns are scikit-image 0.18's regionprops_table columns of these names, stated in integers: in
    doubled coordinates pixel (r, c) has the diamond points (2 r +- 1, 2 c), (2 r, 2 c +- 1); the convex image holds the pixels of the
    object's box whose centre (2 r, 2 c) lies in the convex hull of the object's diamond points or on its boundary (cross products in
    int64); F2 is the largest squared distance between two diamond points of the convex image's pixels, which are the extreme points of
    skimage.measure.find_contours(convex image, 0.5).  Both routes produce the two integers convex_area and F2 per object (the host
    route in Python integers over the find_objects boxes, the device route by csrc/measure_hull.hip) and agree on them exactly; they
    equal scikit-image 0.18.3 bit for bit on tests/golden/hull_reference.npz.  hull=True on a 3D label image raises ValueError before
    anything runs: scikit-image's 3D hull goes through Qhull with a floating tolerance, so voxels on facets cannot be matched (README
    limit 3); so does an extent of 2^30 or more (doubled coordinates are int32).  On the device the call costs, besides the read-backs
    named under Routing, one synchronisation that brings two scalars to the host, which size the table of object rows.

    Arithmetic: integer images are summed (values and squares) in int64, exactly, also beyond 2^53; float images in float64, where
    every square of a float32 is exact.  The derived columns are computed in one place for both routes, every operation rounded on
    its own.  A NaN pixel makes sum, mean, min, max and std of its object and channel NaN, as numpy does; +-inf follow IEEE.  Without
    objects every column is an empty array of its dtype.

    Percentiles: `percentiles` is None or 1 to 8 finite real numbers in [0, 100] (Python or numpy scalars; each is taken as float(q))
    and needs `img`; anything else raises ValueError before anything runs.  With v the object's values in a channel, the column holds
    np.percentile(v, float(q)) (method 'linear'), q one at a time -- the host route calls exactly that, the device route
    (csrc/measure_rank.hip) finds the two order statistics exactly and interpolates as numpy does, so the two agree
    bit for bit: float64 for integer images; for float32 images float32, interpolated in float32 under numpy >= 2.0 and in float64
    rounded at the end under an older numpy.  A NaN among an object's values of a channel makes its percentiles of that channel NaN,
    and only those; +-inf follow numpy's interpolation ([1, inf] at q = 0 is NaN); the sign of a zero result is not pinned (numpy does
    not order -0.0 against +0.0).  Other float types take the host route and numpy's result type.

    Routing: DESIGN.md section 3p, by the label image; an image that is elsewhere is moved to the labels' device.  The device route
    takes integer labels and uint8 / uint16 / float32 images (csrc/measure.hip and the box and centroid-sum kernels; the inputs are not
    written): its float64 sums are added in a fixed order without floating-point atomics, so they depend on (shape, lbl, img) alone --
    the same bits from call to call and from process to process -- and differ from the host's only by the order of the additions.  Any
    other dtype goes through the host code.  Ids beyond int32, or sparse huge ids, are compacted in ascending order for the call;
    `label` reports the originals.  Its own (exception 4 there, R.table_exit): the columns are numpy arrays whatever the input's kind, which
    the device route reads back with one synchronisation, whatever the keywords; as_tensors=True makes them tensors, on the device for the
    device route (besides what reading the largest label needs, one scalar comes to the host, the number of rows), else where the labels
    are or on `device`.
    A label image that is not 2D / 3D or an image of another shape raises ValueError before anything runs."""
    lbl, lbl_t, on_device = R.classify(lbl, device)
    img_t = img is not None and R.is_torch(img)
    if img is not None and not img_t:
        img = np.asarray(img)
    nd = len(lbl.shape)
    C, channel_axis = _measure_shapes(tuple(lbl.shape), None if img is None else tuple(img.shape))
    shape = bool(shape)
    if shape and lbl.shape and int(np.prod([int(n) for n in lbl.shape], dtype=object)) * max(int(n) for n in lbl.shape) ** 2 >= 2 ** 63:
        raise ValueError("measure_labels: shape=True needs (number of pixels) x (largest extent)^2 below 2^63, got shape %s" % (tuple(lbl.shape),))
    hull = bool(hull)
    if hull and nd != 2:
        raise ValueError("measure_labels: hull=True takes a 2D label image (scikit-image's 3D hull is Qhull's, with a floating tolerance "
                         "that integers cannot restate), got %d axes" % nd)
    if hull and max(int(n) for n in lbl.shape) >= _HULL_MAX_EXTENT:
        raise ValueError("measure_labels: hull=True needs extents below 2^30, got shape %s" % (tuple(lbl.shape),))
    qs = _percentile_list(percentiles, img is not None)
    if neighbors is not None:
        neighbors = _contacts_connectivity(neighbors, nd, "measure_labels: neighbors")
    near_k, near_r, near_r2, near_spacing = _proximity_args(nearest, within, spacing, nd)
    near_names = _proximity_names(near_k, near_r)
    if spots is not None:
        spots = _spot_coords(spots, nd)
    # without shape / percentiles / hull the two halves are called as before
    more = {key: value for key, value in (("shape", shape), ("percentiles", qs), ("hull", hull)) if value}
    lbl_ok = (str(lbl.dtype) in _DEVICE_LABEL_DTYPES) if lbl_t else (lbl.dtype.kind in "iu")
    img_ok = img is None or (str(img.dtype) if img_t else "torch." + img.dtype.name) in _DEVICE_DTYPE_CODE
    if on_device and lbl_ok and img_ok:
        raw = _measure_raw_device(lbl, img, C, device, **more)
        contacts = None if neighbors is None else _label_contacts_device(lbl, neighbors, True, device)    # the edge table, there
        if spots is not None:
            image, spots = (R.to_device_tensor(x, raw["label"].device) for x in (lbl, spots))
    else:
        image = lbl.cpu().numpy() if lbl_t else lbl
        raw = _measure_raw_host(image, img.cpu().numpy() if img_t else img, **more)
        contacts = None if neighbors is None else _label_contacts_host(image, neighbors, True)
        spots = spots.cpu().numpy() if R.is_torch(spots) else spots
    # the optional column families, in the raw columns' kind and in the table's order
    extras = [] if contacts is None else list(zip(_NEIGHBOR_NAMES, _neighbor_columns(raw["label"], *contacts)))
    if near_names:
        extras += zip(near_names, _proximity_columns(raw["label"], raw["csum"], raw["area"], near_k, near_r, near_r2, near_spacing))
    if spots is not None:
        extras.append(("spot_count", _spot_counts(raw["label"], image, spots)))
    if R.is_torch(raw["label"]) != bool(as_tensors):
        # the table changes its kind (R.table_exit): the packed raw columns, pct and one block of all extra columns make the trip
        o = R.ops(raw["label"])
        schema = _measure_schema(nd, C, None if img is None else R.dtype_name(raw["min"]), shape, hull)
        block = o.cat([_as_bits(o, c).reshape(1, -1) for _, c in extras]) if extras else None
        packed, pct, block = R.table_exit([_measure_pack(raw, schema), raw.get("pct"), block], as_tensors, lbl, device)
        raw = _measure_unpack(packed, schema)
        if qs:
            raw["pct"] = pct
        extras = [(name, _from_bits(R.ops(block), block[j], R.dtype_name(c))) for j, (name, c) in enumerate(extras)]
    out = _measure_columns(raw, nd, channel_axis, qs)
    out.update(extras)
    return out


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
    R.check_pixel_count(a.shape, "label_components")
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
    import torch
    N.require_device()
    R.check_pixel_count(img.shape, "label_components")
    t = R.to_device_tensor(img, device)
    out = torch.empty(t.shape, dtype=torch.int32, device=t.device)
    count = torch.zeros(1, dtype=torch.int32, device=t.device)
    if t.numel():
        code = _COMPONENTS_DTYPE_CODE[str(t.dtype).replace("torch.", "")]
        N.dcall(t, "sd_label_components_device", R.ptr(t), code, *R.zyx(t.shape), int(connectivity), int(background), R.ptr(out),
                R.ptr(count))
    return out, count[0]


def label_components(img, connectivity=None, background=0, *, return_num=False, device=None):
    """Label the connected components of a 2D / 3D image, as skimage.measure.label(img, background=background,
    connectivity=connectivity) does: pixels equal to `background` (None: 0) get 0; two neighbouring pixels belong to one component only if
    their values are equal; `connectivity` = 1 .. ndim is the largest number of coordinates in which neighbours may differ (None: ndim);
    ids 1 .. n are given in raster (C) order of each component's first pixel.  For a boolean mask this is scipy.ndimage.label(mask,
    generate_binary_structure(ndim, connectivity)).  The result is int32, the project's label dtype, on both routes (skimage returns
    int64).  return_num=True: (labels, n) with n a Python int.

    Routing: DESIGN.md section 3p; the host code builds the pixel graph with numpy and runs scipy's connected_components, ids by first
    occurrence.  The device route takes bool / uint8 / uint16 / int32 images and a background that is an integer, and equals the host
    result (csrc/label_cc.hip: a tiled union-find whose roots are the components' first pixels; the input is not written, the result
    depends on the input alone).  Its own (exception 5 there): for a tensor nothing is read back and the stream is not synchronised
    unless return_num=True.  An image that is not 2D / 3D, a connectivity outside 1 .. ndim or, on the device, more than 2^31 - 1
    pixels raise ValueError before anything runs; an empty image gives an empty result and n = 0."""
    img, is_t, on_device = R.classify(img, device)
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
    if on_device and name in _COMPONENTS_DTYPE_CODE and whole and abs(int(background)) < 2 ** 63:
        out, count = _label_components_device(img, connectivity, int(background), device)
        if not is_t:
            from .utils import to_host
            out = to_host(out)                                              # synchronises: count is there too
        return (out, int(count)) if return_num else out
    if is_t:
        n_box = []

        def host(a):
            lab, n = _label_components_host(a, connectivity, background)
            n_box.append(n)
            return lab
        out = R.via_host(host, img, to=device)
        return (out, n_box[0]) if return_num else out
    out, n = _label_components_host(img, connectivity, background)
    return (out, n) if return_num else out


# ----------------------------------------------------------------------------- nearest-feature transform: expand_labels, distance_transform
# (csrc/edt_feature.hip).  The host routes are scipy's distance_transform_edt; the device routes equal them, ties included.

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
    import torch
    N.require_device()
    lab, _, ids = R._device_labels(lbl, device)
    out = torch.empty_like(lab)
    if lab.numel():
        N.dcall(lab, "sd_expand_labels_device", R.ptr(lab), *R.zyx(lab.shape), *szyx, float(distance), R.ptr(out))
    return R.like_input(out, lbl, ids)


def expand_labels(lbl, distance=1, spacing=1, *, device=None):
    """Grow every labelled object of a 2D / 3D label image by up to `distance` without growing into its neighbours, as
    skimage.segmentation.expand_labels(lbl, distance, spacing) does: a background pixel takes the label of the nearest labelled pixel if
    that pixel is at most `distance` away (Euclidean, in units of `spacing`: a scalar or one value per axis), and stays 0 otherwise.
    A pixel equally near to several labels takes the one scipy's distance_transform_edt returns: the nearest pixel with the smallest
    coordinate along the last axis, then along the axis before it.  distance <= 0 returns a copy.

    Routing: DESIGN.md section 3p; the host code is scipy's distance_transform_edt(lbl == 0, sampling=spacing, return_indices=True) and
    the gather, as scikit-image composes them.  The device route takes integer images and equals the host result (csrc/edt_feature.hip:
    one exact outward scan per pixel and axis, bounded by `distance`; the input is not written).  Ids beyond int32, or sparse huge ids,
    are compacted in ascending order for the call and mapped back.  Its own (exception 6 there): the device route takes non-negative
    labels, so an image with a negative label (a feature like any other, as in scikit-image) goes through the host code and comes back
    in the input's kind.  An image that is not 2D / 3D, a spacing that is not positive and finite or, on the device, more than
    2^31 - 1 pixels raise ValueError before anything runs; an empty image gives an empty result."""
    lbl, is_t, on_device = R.classify(lbl, device)
    nd = len(lbl.shape)
    if nd not in (2, 3):
        raise ValueError("expand_labels: the label image must be 2D or 3D, got %d dimensions" % nd)
    szyx, per_axis = R.spacing_zyx(spacing, nd, "expand_labels")
    distance = float(distance)
    if distance != distance:
        raise ValueError("expand_labels: the distance is not a number")
    size = int(np.prod(lbl.shape, dtype=np.int64))
    if not distance > 0 or size == 0:
        return lbl.clone() if is_t else lbl.copy()
    integer = (str(lbl.dtype) in _DEVICE_LABEL_DTYPES) if is_t else (lbl.dtype.kind in "iu")
    if on_device and integer and int(lbl.min()) >= 0:
        R.check_pixel_count(lbl.shape, "expand_labels")
        return _expand_labels_device(lbl, distance, szyx, device)
    if is_t:
        return R.via_host(_expand_labels_host, lbl, distance, per_axis, to=device)
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
    import torch
    N.require_device()
    if isinstance(img, np.ndarray):
        t = R.to_device_tensor(img != 0, device)                            # the mask of a numpy image is taken before the upload
    else:
        t = (R.to_device_tensor(img, device) != 0).to(torch.uint8)
    dist = torch.empty(t.shape, dtype=torch.float64, device=t.device) if return_distances else None
    lin = torch.empty(t.shape, dtype=torch.int32, device=t.device) if return_indices else None
    if t.numel():
        N.dcall(t, "sd_nearest_feature_device", R.ptr(t), 0, *R.zyx(t.shape), 1, *szyx,
                -1.0 if max_distance is None else float(max_distance), R.opt_ptr(lin), R.opt_ptr(dist))
    idx = None
    if return_indices:
        # the kernel's linear index, split into one coordinate per axis; -1 stays -1
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

    Routing: DESIGN.md section 3p; the host code is scipy's, the device route (csrc/edt_feature.hip) equals it.  Its own (exception 7
    there): every dtype takes the device route, the results have their own dtypes whatever the input's, and a host tensor without
    `device=` is read in place (`.numpy()`), its results are host tensors.  An image that is not 2D / 3D, a sampling that is not
    positive and finite, a negative or NaN max_distance, neither result asked for or, on the device, more than 2^31 - 1 pixels raise
    ValueError before anything runs; an empty image gives empty results."""
    img, is_t, on_device = R.classify(img, device)
    nd = len(img.shape)
    if nd not in (2, 3):
        raise ValueError("distance_transform: the image must be 2D or 3D, got %d dimensions" % nd)
    szyx, per_axis = R.spacing_zyx(sampling, nd, "distance_transform")
    if max_distance is not None:
        max_distance = float(max_distance)
        if not max_distance >= 0:
            raise ValueError("distance_transform: max_distance must be >= 0 or None")
        if max_distance == np.inf:
            max_distance = None
    if not (return_distances or return_indices):
        raise ValueError("distance_transform: at least one of return_distances / return_indices must be True")
    if on_device:
        R.check_pixel_count(img.shape, "distance_transform")
        dist, idx = _distance_transform_device(img, szyx, max_distance, return_distances, return_indices, device)
        if not is_t:
            from .utils import to_host_many
            dist, idx = to_host_many([dist, idx])
    else:
        dist, idx = _distance_transform_host(img.numpy() if is_t else img, per_axis, max_distance, return_distances, return_indices)
        if is_t:
            import torch
            dist, idx = (None if a is None else torch.from_numpy(a) for a in (dist, idx))
    return (dist, idx) if return_distances and return_indices else (dist if return_distances else idx)


# ----------------------------------------------------------------------------- label clean-up: find_boundaries, clear_border,
# remove_small_objects, select_labels (csrc/label_edit.hip).  The first three are scikit-image 0.18's functions
# of these names without `in_place`; their host routes are numpy and scipy, the device routes equal them.
_BOUNDARY_MODES = {"thick": 0, "inner": 1, "outer": 2}
_INT32_MIN, _INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _whole_number(v):
    """the int a scalar argument stands for, or None where it is no whole number below 2^63 in magnitude"""
    if isinstance(v, (bool, np.bool_, int, np.integer)):
        v = int(v)
    elif isinstance(v, (float, np.floating)) and float(v).is_integer():
        v = int(v)
    else:
        return None
    return v if abs(v) < 2 ** 63 else None


def _int32_values_device(x, device):
    """the contiguous int32 device tensor with the values of x as they are (negative ones too), or None where x's dtype or values do
    not fit: x a numpy array (uploaded to `device`) or a tensor (moved there if it is elsewhere) of a bool or integer dtype.  int64
    values are checked first: a tensor's smallest and largest value come to the host in one copy."""
    import torch
    if isinstance(x, np.ndarray):
        if x.dtype.kind not in "iub" or x.dtype == np.uint64:
            return None
        if x.dtype.itemsize >= 4 and x.dtype != np.int32 and x.size and (int(x.min()) < _INT32_MIN or int(x.max()) > _INT32_MAX):
            return None
        return R.to_device_tensor(x.astype(np.int32, copy=False), device)
    if str(x.dtype) not in _DEVICE_LABEL_DTYPES + ("torch.bool",):
        return None
    t = R.to_device_tensor(x, device)
    if t.dtype == torch.int64 and t.numel():
        lo, hi = torch.stack([t.min(), t.max()]).tolist()
        if lo < _INT32_MIN or hi > _INT32_MAX:
            return None
    return t.to(torch.int32).contiguous()


def _dtype_max(x):
    """the largest value of the integer dtype of the array / tensor x (a bool image counts as uint8), or None for another dtype"""
    name = str(x.dtype).replace("torch.", "")
    if name == "bool":
        return 255
    try:
        return int(np.iinfo(np.dtype(name)).max)
    except (TypeError, ValueError):
        return None


def _distinct_count_exceeds_two(stack):
    """per position, whether the values stack[:, ...] hold more than two different ones"""
    s = np.sort(stack, axis=0)
    return (s[1:] != s[:-1]).sum(axis=0) > 1


def _find_boundaries_subpixel_host(a):
    """scikit-image's mode 'subpixel': the image on a grid of twice the resolution (2 n - 1 per axis), the pixels at the even positions,
    every other position an edge cell holding the dtype's largest value; an edge cell is a boundary where its 3^nd window of the grid,
    padded with 0, holds more than two different values"""
    from itertools import product
    nd = a.ndim
    grid = np.full([max(2 * s - 1, 0) for s in a.shape], np.iinfo(a.dtype).max, a.dtype)
    even = (slice(None, None, 2),) * nd
    grid[even] = a
    edge = np.ones(grid.shape, bool)
    edge[even] = False
    if grid.size == 0:
        return np.zeros(grid.shape, bool)
    padded = np.pad(grid, 1, mode="constant", constant_values=0)
    windows = np.stack([padded[tuple(slice(1 + d, 1 + d + n) for d, n in zip(off, grid.shape))] for off in product((-1, 0, 1), repeat=nd)])
    return _distinct_count_exceeds_two(windows) & edge


def _find_boundaries_host(a, connectivity, mode, background):
    """scikit-image 0.18's find_boundaries by scipy.ndimage.grey_dilation / grey_erosion, composed as there"""
    from scipy import ndimage as ndi
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    if mode == "subpixel":
        return _find_boundaries_subpixel_host(a)
    if a.size == 0:
        return np.zeros(a.shape, bool)
    top = np.iinfo(a.dtype).max
    if a.dtype.itemsize == 8:
        # scipy's filters compute in float64, which holds neither every 64-bit id nor the dtype's largest value (scikit-image's result
        # for such an image depends on how the platform converts 2^63 back).  The rules only compare values, so they are applied to the
        # values' ranks, which float64 holds
        values, ranks = np.unique(a, return_inverse=True)
        at = np.searchsorted(values, background) if values[0] <= background <= values[-1] else 0
        background = int(at) if values[at] == background else -1
        a, top = ranks.reshape(a.shape).astype(np.int64), len(values)
    near = ndi.generate_binary_structure(a.ndim, connectivity)
    out = ndi.grey_dilation(a, footprint=near) != ndi.grey_erosion(a, footprint=near)
    if mode == "inner":
        out &= a != background
    elif mode == "outer":
        is_bg = a == background
        window = ndi.generate_binary_structure(a.ndim, a.ndim)
        raised = a.copy()
        raised[is_bg] = top
        adjacent = (ndi.grey_dilation(a, footprint=window) != ndi.grey_erosion(raised, footprint=window)) & ~is_bg
        out &= is_bg | adjacent
    return out


def _find_boundaries_device(lab, connectivity, mode, background, sentinel):
    """the uint8 boundary image of the int32 device tensor lab (2D / 3D) through sd_find_boundaries_device"""
    import torch
    out = torch.empty(lab.shape, dtype=torch.uint8, device=lab.device)
    if lab.numel():
        N.dcall(lab, "sd_find_boundaries_device", R.ptr(lab), *R.zyx(lab.shape), int(connectivity), _BOUNDARY_MODES[mode], int(background),
                int(sentinel), R.ptr(out))
    return out


def find_boundaries(label_img, connectivity=1, mode="thick", background=0, *, device=None):
    """The boundaries between the labelled regions of an image as a bool image, as skimage.segmentation.find_boundaries(label_img,
    connectivity, mode, background) of scikit-image 0.18 gives them.  With N_c(p) the neighbours of p inside the image whose offsets have
    at most c = `connectivity` (1 .. ndim) non-zero coordinates:

        thick     p has a neighbour in N_c(p) with another value
        inner     thick, and p is not background
        outer     thick, and p is background or the largest value in p's full 3^ndim window differs from the window's smallest value
                  after every background pixel was raised to the dtype's largest value: an object pixel next to another object
        subpixel  the boundaries on a grid of 2 n - 1 positions per axis

    A bool image is taken as uint8.  DESIGN.md section 3r states the rules and how they follow from scikit-image's morphology.

    Routing: DESIGN.md section 3p; the host code is scipy.ndimage.grey_dilation / grey_erosion.  The device route takes 2D / 3D bool and
    integer images whose values fit int32 and a background that is a whole number, and equals the host result (csrc/label_edit.hip: a
    tile of labels with a halo of 1 in local memory, one read of the labels, one byte written per pixel; the input is not written).
    Nothing is read back but, for an int64 tensor, its smallest and largest value in one copy.  mode="subpixel" takes the host route on
    every input, like an image of another rank, of a float dtype or with values beyond int32, and comes back in the input's kind.  A
    connectivity outside 1 .. ndim, an unknown mode or, on the device, more than 2^31 - 1 pixels raise ValueError before anything
    runs."""
    label_img, is_t, on_device = R.classify(label_img, device)
    nd = len(label_img.shape)
    if isinstance(connectivity, (bool, np.bool_)) or not isinstance(connectivity, (int, np.integer)) or not 1 <= connectivity <= max(nd, 1):
        raise ValueError("find_boundaries: connectivity for %dD images must be in [1, ..., %d], got %r" % (nd, nd, connectivity))
    if mode not in _BOUNDARY_MODES and mode != "subpixel":
        raise ValueError("find_boundaries: mode must be 'thick', 'inner', 'outer' or 'subpixel', got %r" % (mode,))
    connectivity = int(connectivity)
    bg, sentinel = _whole_number(background), _dtype_max(label_img)
    if on_device and mode != "subpixel" and nd in (2, 3) and bg is not None and sentinel is not None and sentinel < 2 ** 63:
        R.check_pixel_count(label_img.shape, "find_boundaries")
        N.require_device()
        lab = _int32_values_device(label_img, device)
        if lab is not None:
            out = _find_boundaries_device(lab, connectivity, mode, bg, sentinel)
            if is_t:
                import torch
                return out.to(torch.bool)
            from .utils import to_host
            return to_host(out).astype(np.bool_)
    if is_t:
        return R.via_host(_find_boundaries_host, label_img, connectivity, mode, background, to=device)
    return _find_boundaries_host(label_img, connectivity, mode, background)


def _border_band(shape, ext):
    """bool image: the pixels within ext of an edge along any axis"""
    band = np.zeros(shape, bool)
    for d in range(len(shape)):
        at = [slice(None)] * len(shape)
        at[d] = slice(ext)
        band[tuple(at)] = True
        at[d] = slice(-ext, None)
        band[tuple(at)] = True
    return band


def _clear_border_host(a, buffer_size, bgval, mask):
    outside = _border_band(a.shape, buffer_size + 1) if mask is None else ~mask
    out = a.copy()
    if a.size == 0:
        return out
    comp = _label_components_host(a, a.ndim, 0)[0]
    hit = np.zeros(int(comp.max()) + 1, bool)
    hit[comp[outside]] = True
    out[hit[comp]] = bgval
    return out


def _clear_border_device(val, nd, buffer_size, bgval, mask):
    """clear_border of the int32 device tensor val (2D / 3D): sd_label_components_device under full connectivity, then
    sd_label_border_flags_device and sd_label_clear_flagged_device; mask: None or a uint8 device tensor of val's shape"""
    import torch
    out = torch.empty_like(val)
    if val.numel():
        comp, _ = _label_components_device(val, nd, 0, None)
        n, n_flags = val.numel(), val.numel() + 1                               # no more components than pixels, and the background
        flags = torch.empty(n_flags, dtype=torch.uint8, device=val.device)
        N.dcall(val, "sd_label_border_flags_device", R.ptr(comp), *R.zyx(val.shape), nd, int(buffer_size), R.opt_ptr(mask), n_flags, R.ptr(flags))
        N.dcall(val, "sd_label_clear_flagged_device", R.ptr(val), R.ptr(comp), R.ptr(flags), n_flags, n, int(bgval), R.ptr(out))
    return out


def clear_border(labels, buffer_size=0, bgval=0, mask=None, *, device=None):
    """Clear the objects connected to the image border, as skimage.segmentation.clear_border(labels, buffer_size, bgval, mask=mask) of
    scikit-image 0.18 does (there is no `in_place`: the input is never written).  It works on connected components, not on ids: the
    components are those of label_components(labels, background=0) -- equal values joined under full connectivity -- and a component is
    cleared, its pixels set to `bgval`, when one of its pixels lies within buffer_size + 1 of an image edge along any axis; with a bool
    `mask` of the image's shape, when one of its pixels lies where the mask is False (buffer_size is then ignored).  Of an id with two
    components only the one at the border goes.  scikit-image's quirk is kept: the background counts as component 0, so if any
    background pixel lies in the band (or outside the mask) every background pixel becomes `bgval`, which shows with bgval != 0.

    Routing: DESIGN.md section 3p, by `labels`; a mask that is elsewhere is moved to the labels' place.  The host code is numpy on the
    project's label_components host route.  The device route takes 2D / 3D bool and integer images whose values fit int32 and a bgval
    that is a whole number of the image's dtype, and equals the host result (csrc/label_cc.hip, then csrc/label_edit.hip: only the
    band's pixels are visited for the flags, or the mask in one pass; one more pass clears).  Nothing is read back but, for an int64
    tensor, its smallest and largest value in one copy.  Everything else goes through the host code and comes back in the input's kind.
    Errors, scikit-image's: ValueError for a buffer_size >= an extent without a mask, AssertionError for a mask of another shape,
    TypeError for a mask that is not bool; and ValueError for a negative buffer_size or, on the device, more than 2^31 - 1 pixels."""
    labels, is_t, on_device = R.classify(labels, device)
    nd = len(labels.shape)
    buffer_size = int(buffer_size)
    if buffer_size < 0:
        raise ValueError("clear_border: buffer_size must be >= 0")
    if mask is None and any(buffer_size >= s for s in labels.shape):
        raise ValueError("buffer size may not be greater than image size")
    mask_t = mask is not None and R.is_torch(mask)
    if mask is not None:
        if not mask_t:
            mask = np.asarray(mask)
        if tuple(mask.shape) != tuple(labels.shape):
            raise AssertionError("image and mask should have the same shape but are %s and %s" % (tuple(labels.shape), tuple(mask.shape)))
        if str(mask.dtype).replace("torch.", "") != "bool":
            raise TypeError("mask should be of type bool.")
    fill, top = _whole_number(bgval), _dtype_max(labels)
    name = str(labels.dtype).replace("torch.", "")
    fits = fill is not None and top is not None and (name == "bool" or (0 if name.startswith("u") else -top - 1) <= fill <= top) \
        and _INT32_MIN <= fill <= _INT32_MAX
    if on_device and nd in (2, 3) and fits:
        R.check_pixel_count(labels.shape, "clear_border")
        N.require_device()
        val = _int32_values_device(labels, device)
        if val is not None:
            m = None if mask is None else R.to_device_tensor(mask, val.device)
            return R.like_input(_clear_border_device(val, nd, buffer_size, fill, m), labels)
    host_mask = None if mask is None else (mask.cpu().numpy() if mask_t else mask)
    if is_t:
        return R.via_host(_clear_border_host, labels, buffer_size, bgval, host_mask, to=device)
    return _clear_border_host(labels, buffer_size, bgval, host_mask)


_NEGATIVE_LABELS = ("Negative value labels are not supported. Try relabeling the input with `scipy.ndimage.label` or "
                    "`skimage.morphology.label`.")


def _remove_small_objects_host(a, min_size, connectivity):
    out = a.copy()
    if min_size == 0 or a.size == 0:
        return out
    if a.dtype == np.bool_:
        from scipy import ndimage as ndi
        keys = ndi.label(a, ndi.generate_binary_structure(a.ndim, connectivity))[0]
    else:
        keys = a
        if a.dtype.kind == "i" and int(a.min()) < 0:
            raise ValueError(_NEGATIVE_LABELS)
    if int(keys.max()) <= 4 * keys.size + 1024:
        sizes = np.bincount(keys.reshape(-1))
        if len(sizes) == 2 and a.dtype != np.bool_:
            import warnings
            warnings.warn("Only one label was provided to `remove_small_objects`. Did you mean to use a boolean array?")
        out[(sizes < min_size)[keys]] = 0
    else:                                                                   # sparse huge ids: the same counts without the table
        ids, inv, sizes = np.unique(keys, return_inverse=True, return_counts=True)
        out[(sizes < min_size)[inv.reshape(keys.shape)]] = 0
    return out


def _clear_small_device(val, key, top, min_size):
    """val with the pixels cleared whose key (1 .. top; val itself or a component image) has fewer than min_size pixels: the count column
    of sd_label_centroid_sums_device, then sd_label_clear_flagged_device"""
    import torch
    sizes = R.label_tables(key, top, sums=True)[1][:, 0]
    flags = (sizes < min_size).to(torch.uint8).contiguous()
    out = torch.empty_like(val)
    N.dcall(val, "sd_label_clear_flagged_device", R.ptr(val), R.ptr(key), R.ptr(flags), top + 1, val.numel(), 0, R.ptr(out))
    return out


def remove_small_objects(ar, min_size=64, connectivity=1, *, device=None):
    """Remove the objects smaller than `min_size` pixels, as skimage.morphology.remove_small_objects(ar, min_size, connectivity) of
    scikit-image 0.18 does (there is no `in_place`: the input is never written).  An integer image is taken per id, not per component:
    an id whose pixels, wherever they lie, number fewer than min_size becomes 0, and `connectivity` plays no part; a negative value
    raises ValueError.  A bool image is taken per connected component of scipy.ndimage.label(ar, generate_binary_structure(ndim,
    connectivity)), and bool comes back.  min_size = 0 returns a copy.

    Routing: DESIGN.md section 3p; the host code is np.bincount, and it alone keeps scikit-image's warning about an image with one label.
    The device route takes 2D / 3D bool and integer images and equals the host result: for an integer image the pixel counts of
    sd_label_centroid_sums_device, for a mask label_components and the counts of its components, then one pass that clears
    (csrc/label_edit.hip).  Ids beyond int32, or sparse huge ids, are compacted in ascending order for the call and mapped back.  Read
    back: the largest value (as for every label function) and, for a tensor, the smallest, to refuse negative values; for a mask the
    number of components instead.  An image that is neither bool nor integer or, on the device, more than 2^31 - 1 pixels raise
    ValueError before anything runs; so does, for a mask only, a connectivity outside 1 .. ndim (scipy would clamp it; one rule for both
    routes, as label_components has it)."""
    ar, is_t, on_device = R.classify(ar, device)
    nd = len(ar.shape)
    name = str(ar.dtype).replace("torch.", "")
    if name != "bool" and not (name.startswith("int") or name.startswith("uint")):
        raise ValueError("Only bool or integer image types are supported. Got %s." % name)
    if name != "bool":
        connectivity = 1                                                    # an integer image is taken per id: no part in it
    elif isinstance(connectivity, (bool, np.bool_)) or not isinstance(connectivity, (int, np.integer)) or not 1 <= connectivity <= max(nd, 1):
        raise ValueError("remove_small_objects: connectivity for %dD masks must be in [1, ..., %d], got %r" % (nd, nd, connectivity))
    size = int(np.prod(ar.shape, dtype=np.int64))
    if min_size == 0 or size == 0:
        return ar.clone() if is_t else ar.copy()
    if on_device and nd in (2, 3) and (name == "bool" or not is_t or str(ar.dtype) in _DEVICE_LABEL_DTYPES) and name != "uint64":
        import torch
        R.check_pixel_count(ar.shape, "remove_small_objects")
        if name.startswith("int") and not is_t and int(ar.min()) < 0:
            raise ValueError(_NEGATIVE_LABELS)
        N.require_device()
        if name == "bool":
            comp, count = _label_components_device(ar, int(connectivity), 0, device)
            n = int(count)
            if n == 0:
                return ar.clone() if is_t else ar.copy()
            mask = R.to_device_tensor(ar, comp.device).to(torch.int32)
            return R.like_input(_clear_small_device(mask, comp, n, min_size), ar)
        if name.startswith("int") and is_t and int(ar.min()) < 0:
            raise ValueError(_NEGATIVE_LABELS)
        lab, top, ids = R._device_labels(ar, device)
        if top == 0:
            return ar.clone() if is_t else ar.copy()
        return R.like_input(_clear_small_device(lab, lab, top, min_size), ar, ids)
    if is_t:
        return R.via_host(_remove_small_objects_host, ar, min_size, int(connectivity), to=device)
    return _remove_small_objects_host(ar, min_size, int(connectivity))


def _wanted_ids_host(labels):
    """the ids of `labels` (an array, a tensor, a sequence or one id) as a 1-D numpy array of an integer dtype"""
    w = labels.detach().cpu().numpy() if R.is_torch(labels) else np.asarray(labels)
    w = w.reshape(-1)
    if w.size == 0:
        return np.zeros(0, np.int64)
    if w.dtype.kind == "b":
        w = w.astype(np.uint8)
    if w.dtype.kind not in "iu":
        raise ValueError("select_labels: the ids must be integers, got %s" % w.dtype)
    return w


def _select_labels_host(a, wanted, invert, relabel):
    keep = np.isin(a, wanted)
    keep = (~keep if invert else keep) & (a > 0)
    out = np.where(keep, a, 0).astype(a.dtype)
    if relabel:
        inv = np.unique(out[keep], return_inverse=True)[1]
        out[keep] = (inv.reshape(-1) + 1).astype(a.dtype)
    return out


def _select_labels_device(lbl, labels, invert, relabel, device):
    """select_labels through sd_relabel_stack_device with one frame: a table over the ids 1 .. top whose entry is the id itself (or its
    rank among the ids kept and present, with relabel) where the id is kept, else 0; built on the device, nothing is read back"""
    import ctypes
    import torch
    lab, top, ids = R._device_labels(lbl, device)
    dev = lab.device
    if lab.numel() == 0 or top == 0:
        return R.like_input(torch.zeros_like(lab), lbl)
    if R.is_torch(labels):
        if labels.dtype.is_floating_point or labels.dtype.is_complex:
            raise ValueError("select_labels: the ids must be integers, got %s" % labels.dtype)
        w = labels.detach().reshape(-1).to(dev).to(torch.int64)
    else:
        w = _wanted_ids_host(labels)
        w = torch.as_tensor(w[(w > 0) & (w <= 2 ** 63 - 1)].astype(np.int64), device=dev)
    if ids is not None:                                                     # compacted: an original id -> its place among the ids
        ids_t = (ids if R.is_torch(ids) else torch.as_tensor(ids.astype(np.int64), device=dev)).to(torch.int64)
        at = torch.searchsorted(ids_t, w).clamp(max=top)
        w = torch.where(ids_t[at] == w, at, torch.zeros_like(at))
    else:
        w = torch.where((w > 0) & (w <= top), w, torch.zeros_like(w))
    keep = torch.zeros(top + 1, dtype=torch.bool, device=dev)
    keep[w] = True
    if invert:
        keep = ~keep
    keep[0] = False
    if relabel:
        keep &= R.label_tables(lab, top, sums=True)[1][:, 0] > 0
        new = torch.cumsum(keep, 0) * keep
    else:
        new = torch.arange(top + 1, device=dev) * keep
    table_ids = torch.arange(1, top + 1, dtype=torch.int32, device=dev)
    table_new = new[1:].to(torch.int32).contiguous()
    out = torch.empty_like(lab)
    N.dcall(lab, "sd_relabel_stack_device", R.ptr(lab), 1, ctypes.c_longlong(lab.numel()), R.ptr(table_ids), R.ptr(table_new),
            (ctypes.c_longlong * 2)(0, top), (ctypes.c_int32 * 1)(top), R.ptr(out))
    return R.like_input(out, lbl, None if relabel else ids)


def select_labels(lbl, labels, *, invert=False, relabel=False, device=None):
    """Keep the objects of the label image `lbl` whose ids are in `labels`; every other pixel becomes 0.  `labels`: an array, a tensor
    or a sequence of ids, for example table["label"][table["area"] > 50] of measure_labels(as_tensors=True); ids that the image does
    not hold, and ids <= 0, select nothing (values <= 0 are background and come out as 0).  invert=True keeps the other objects
    instead.  relabel=True renumbers what is kept to 1 .. n in ascending order of the ids.  The project's own function: with
    measure_labels it is the filter between "labels" and "measure".

    Routing: DESIGN.md section 3p, by `lbl`; the host code is np.isin.  The device route takes integer images of any rank and equals
    the host result: a table over the ids, built on the device from `labels` wherever they live, applied by sd_relabel_stack_device
    (csrc/relabel.hip) with one frame -- no kernel of its own; with relabel the ids present come from sd_label_centroid_sums_device
    (2D / 3D images; another rank takes the host code).  Ids beyond int32, or sparse huge ids, are compacted in ascending order for
    the call and mapped back.  Nothing is read back beyond the largest id.  An image or ids that are not integers raise ValueError."""
    lbl, is_t, on_device = R.classify(lbl, device)
    name = str(lbl.dtype).replace("torch.", "")
    if not (name.startswith("int") or name.startswith("uint")):
        raise ValueError("select_labels: the label image must have an integer type, got %s" % name)
    invert, relabel = bool(invert), bool(relabel)
    kernel_dtype = (str(lbl.dtype) in _DEVICE_LABEL_DTYPES) if is_t else name != "uint64"
    if on_device and kernel_dtype and (not relabel or len(lbl.shape) in (2, 3)):
        R.check_pixel_count(lbl.shape, "select_labels")
        N.require_device()
        return _select_labels_device(lbl, labels, invert, relabel, device)
    wanted = _wanted_ids_host(labels)
    if is_t:
        return R.via_host(_select_labels_host, lbl, wanted, invert, relabel, to=device)
    return _select_labels_host(lbl, wanted, invert, relabel)


# ----------------------------------------------------------------------------- label contacts: which objects touch, and by how much
# (csrc/label_contacts.hip).  Both routes produce the plain table -- label_a < label_b and contacts, int64, ascending
# by (label_a, label_b), original ids -- as numpy arrays or as tensors; _symmetric_contacts and _neighbor_columns derive everything else
# from it with the same integer operations on either kind.

def _forward_offsets(nd, connectivity):
    """the offsets of generate_binary_structure(nd, connectivity) that are lexicographically positive: every unordered pair of
    neighbouring pixels once (2 / 4 of them in 2D, 3 / 9 / 13 in 3D)"""
    from itertools import product
    return [o for o in product((-1, 0, 1), repeat=nd) if o > (0,) * nd and sum(1 for c in o if c) <= connectivity]


def _contacts_connectivity(connectivity, nd, who):
    if isinstance(connectivity, (bool, np.bool_)) or not isinstance(connectivity, (int, np.integer)) or not 1 <= connectivity <= nd:
        raise ValueError("%s: connectivity for %dD images must be in [1, ..., %d], got %r" % (who, nd, nd, connectivity))
    return int(connectivity)


def _label_contacts_host(lbl, connectivity, background):
    """(label_a, label_b, contacts) of a 2D / 3D numpy array of a bool or integer dtype: per forward offset two shifted slices, a != b,
    the pairs as keys min << 32 | max and np.unique(..., return_counts=True), then a merge over the offsets"""
    if lbl.dtype.kind == "b":
        lbl = lbl.astype(np.uint8)
    if lbl.size and lbl.dtype.kind == "i" and int(lbl.min()) < 0:
        raise ValueError(_NEGATIVE_LABELS)
    top = int(lbl.max()) if lbl.size else 0
    ids = None
    lab = lbl
    if _ids_need_compaction(top, lbl.size):
        pos = lbl > 0
        ids, inv = np.unique(lbl[pos], return_inverse=True)
        lab = np.zeros(lbl.shape, np.int64)
        lab[pos] = inv.reshape(-1) + 1
        ids = np.concatenate([np.zeros(1, np.int64), ids.astype(np.int64)])
    keys, counts = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for off in _forward_offsets(lab.ndim, connectivity):
        here = tuple(slice(max(0, -d), n - max(0, d)) for d, n in zip(off, lab.shape))
        there = tuple(slice(max(0, d), n - max(0, -d)) for d, n in zip(off, lab.shape))
        a, b = lab[here], lab[there]
        keep = a != b
        if not background:
            keep &= (a != 0) & (b != 0)
        a, b = a[keep].astype(np.int64), b[keep].astype(np.int64)
        k, c = np.unique((np.minimum(a, b) << 32) | np.maximum(a, b), return_counts=True)
        keys.append(k)
        counts.append(c.astype(np.int64))
    key, inv = np.unique(np.concatenate(keys), return_inverse=True)
    total = np.zeros(len(key), np.int64)
    np.add.at(total, inv.reshape(-1), np.concatenate(counts))
    a, b = key >> 32, key & 0xFFFFFFFF
    return (a, b, total) if ids is None else (ids[a], ids[b], total)


def _label_contacts_device(lbl, connectivity, background, device=None, runs=None):
    """(label_a, label_b, contacts) as int64 tensors on the device through sd_label_contacts_device; lbl a numpy array (uploaded to
    `device`) or a tensor of an integer dtype.  Two scalars come to the host besides what reading the largest label needs: the number
    of runs and the number of rows.  runs: a list that receives the number of runs the kernel appended"""
    import ctypes
    import torch
    N.require_device()
    if lbl.dtype.is_signed if R.is_torch(lbl) else lbl.dtype.kind == "i":
        if (lbl.numel() if R.is_torch(lbl) else lbl.size) and int(lbl.min()) < 0:
            raise ValueError(_NEGATIVE_LABELS)
    lab, top, ids = R._device_labels(lbl, device)
    dev = lab.device
    if lab.numel() == 0 or top <= 0:
        if runs is not None:
            runs.append(0)
        return tuple(torch.zeros(0, dtype=torch.int64, device=dev) for _ in range(3))
    count, n_runs, mm = ctypes.c_longlong(0), ctypes.c_longlong(0), (ctypes.c_int32 * 2)()
    cap = max(1024, lab.numel() // 64)        # a first guess; a table that is larger takes a second call with the real count
    while True:
        keys = torch.empty(cap, dtype=torch.int64, device=dev)
        counts = torch.empty(cap, dtype=torch.int64, device=dev)
        N.dcall(lab, "sd_label_contacts_device", R.ptr(lab), lab.dim(), *R.zyx(lab.shape), int(connectivity), int(bool(background)),
                ctypes.c_longlong(cap), R.ptr(keys), R.ptr(counts), ctypes.byref(count), mm, ctypes.byref(n_runs))
        if count.value <= cap:
            break
        cap = count.value
    if runs is not None:
        runs.append(n_runs.value)
    m = count.value
    keys, counts = keys[:m].clone(), counts[:m].clone()                     # the first guess's buffers go back to the allocator
    return R.original_labels(keys >> 32, ids), R.original_labels(keys & 0xFFFFFFFF, ids), counts


def _symmetric_contacts(a, b, contacts, present):
    """the plain table listed both ways, sorted by (label_a, label_b), and the CSR offsets of the labels `present` (ascending, > 0):
    the rows of present[i] are offsets[i] : offsets[i + 1]; the rows of label_a = 0 come before offsets[0]"""
    o = R.ops(a)
    sa, sb, sc = o.cat([a, b]), o.cat([b, a]), o.cat([contacts, contacts])
    # two stable sorts, by label_b and then by label_a: no key of two ids has to fit 64 bits
    order = o.stable_argsort(sb)
    order = order[o.stable_argsort(sa[order])]
    sa, sb, sc = sa[order], sb[order], sc[order]
    offsets = o.zeros_i64(len(present) + 1)
    offsets[:len(present)] = o.searchsorted(sa, present)
    offsets[len(present):] = len(sa)
    return sa, sb, sc, offsets


def _neighbor_columns(label, a, b, contacts):
    """(neighbors, contact_objects, contact_background) of the objects `label` (ascending, all > 0) from the plain contact table with
    the background's pairs: the number of rows an object shares with another object, the contacts of those rows, and the contacts of
    its row with 0"""
    o = R.ops(label)
    searchsorted, add_at = o.searchsorted, o.add_at
    n = len(label)
    neighbors, objects, bg = o.zeros_i64(n), o.zeros_i64(n), o.zeros_i64(n)
    if len(a):
        with_bg = a == 0
        both = ~with_bg
        ia, ib, c = searchsorted(label, a[both]), searchsorted(label, b[both]), contacts[both]
        one = c * 0 + 1
        for at in (ia, ib):
            add_at(neighbors, at, one)
            add_at(objects, at, c)
        add_at(bg, searchsorted(label, b[with_bg]), contacts[with_bg])
    return neighbors, objects, bg


def _labels_present(lbl, on_device, device):
    """the labels > 0 of the image, ascending, int64: a tensor on the device for the device route, else a numpy array"""
    if on_device:
        import torch
        lab, top, ids = R._device_labels(lbl, device)
        if lab.numel() == 0 or top <= 0:
            return torch.zeros(0, dtype=torch.int64, device=lab.device)
        sums = R.label_tables(lab, top, sums=True)[1]
        return R.original_labels(torch.nonzero(sums[:, 0]).reshape(-1), ids)
    u = np.unique(lbl)
    return u[u > 0].astype(np.int64)


def label_contacts(lbl, connectivity=1, *, background=False, symmetric=False, device=None, as_tensors=False):
    """Which objects of a 2D / 3D integer label image touch, and over how many pixel pairs: the region adjacency graph with its edge
    weights (scikit-image's future.graph.RAG has the edges, CLIJ's touch matrix the same relation).  With `connectivity` c in 1 .. ndim,
    the forward offsets are the offsets of scipy.ndimage.generate_binary_structure(ndim, c) that are lexicographically positive (2 / 4
    in 2D, 3 / 9 / 13 in 3D), and a contact is a pixel pair (p, p + o), o a forward offset, both inside the image, with
    lbl[p] != lbl[p + o].  The image edge is no contact.  Returns a dict of int64 columns, one row per unordered pair of values that has
    a contact:

        label_a, label_b   the pair, label_a < label_b; rows ascend by (label_a, label_b)
        contacts           its number of contacts

    Value 0 is the background: its pairs (0, b) are listed only with background=True.  symmetric=True lists every row both ways,
    (a, b) and (b, a), sorted by (label_a, label_b), so that the neighbours of one object are a contiguous slice, and adds

        offsets            CSR offsets over the labels > 0 present in the image, ascending -- the rows of measure_labels: the neighbours
                           of the i-th label are the rows offsets[i] : offsets[i + 1]; with background=True the rows with
                           label_a = 0 come first, before offsets[0]

    Objects "within a gap of d pixels" of each other are label_contacts(expand_labels(lbl, d / 2)); there is no distance argument.
    The objects near an object by centroid, with their distances, are point_neighbors'.

    Routing: DESIGN.md section 3p, like measure_labels (exception 4 there, R.table_exit): the columns are numpy arrays whatever the
    input's kind, which the device route reads back with one synchronisation; as_tensors=True makes them tensors, on the device for the
    device route, else where the labels are or on `device`.  The host code is numpy: per forward offset two shifted slices and
    np.unique.  The device route
    takes bool and integer images and equals the host result exactly (csrc/label_contacts.hip: a tile of labels with a halo of 1 in
    local memory, runs of equal pairs combined within a wave, a radix sort and a reduce-by-key; integers only, the same bits from call
    to call; the input is not written).  Ids beyond int32, or sparse huge ids, are compacted in ascending order for the call and mapped
    back.  A negative label, an image that is not 2D / 3D or not of a bool or integer dtype, or a connectivity outside 1 .. ndim
    raise ValueError."""
    lbl, is_t, on_device = R.classify(lbl, device)
    nd = len(lbl.shape)
    if nd not in (2, 3):
        raise ValueError("label_contacts: the label image must be 2D or 3D, got %d dimensions" % nd)
    connectivity = _contacts_connectivity(connectivity, nd, "label_contacts")
    name = str(lbl.dtype).replace("torch.", "")
    if name != "bool" and not (name.startswith("int") or name.startswith("uint")):
        raise ValueError("label_contacts: the label image must have a bool or integer type, got %s" % name)
    background, symmetric = bool(background), bool(symmetric)
    taken = on_device and ((str(lbl.dtype) in _DEVICE_LABEL_DTYPES + ("torch.bool",)) if is_t else True)
    if taken:
        cols = _label_contacts_device(lbl, connectivity, background, device)
    else:
        host = lbl.cpu().numpy() if is_t else lbl
        cols = _label_contacts_host(host, connectivity, background)
    names = ("label_a", "label_b", "contacts")
    if symmetric:
        present = _labels_present(lbl if taken else (host.astype(np.uint8) if host.dtype.kind == "b" else host), taken, device)
        cols = _symmetric_contacts(*cols, present)
        names += ("offsets",)
    return dict(zip(names, R.table_exit(cols, as_tensors, lbl, device)))


# ----------------------------------------------------------------------------- point neighbours: the nearest points, the points within a radius
# (csrc/point_neighbors.hip).  Both routes work on scaled float64 coordinates and produce squared distances by the
# one definition: d2 = ((q0 - p0)^2 + (q1 - p1)^2) + (q2 - p2)^2, every operation rounded, candidates ordered by (d2, index).

_POINT_NEIGHBORS_MAX_K = 64                                                 # csrc/point_neighbors.h's PN_MAX_K
_POINT_NEIGHBORS_MAX_COORD = 2.0 ** 500                                     # PN_MAX_COORD
_POINT_NEIGHBORS_SLACK = 2.0 ** -40                                         # by how much a k-d tree's own distances may differ from d2's
_POINT_NEIGHBORS_WORKERS = 1                                                # threads of the host route's tree queries (tools/time_point_neighbors.py tries 16)


def _points_as_float64(x, what, nd=None):
    """the (n, nd) float64 array / tensor of the points x (numpy, tensor or nested lists; integer, float32 or float64)"""
    if R.is_torch(x):
        import torch
        name = str(x.dtype).replace("torch.", "")
        ok = name in ("float32", "float64", "uint8", "int8", "int16", "int32", "int64")
        p = x.to(torch.float64) if ok else x
    else:
        x = np.asarray(x)
        if x.size == 0 and x.dtype.kind not in "iuf":
            x = x.astype(np.float64)
        ok = x.dtype.kind in "iu" or x.dtype in (np.float32, np.float64)
        p = x.astype(np.float64) if ok else x
    if not ok:
        raise ValueError("point_neighbors: the %s must be integer, float32 or float64, got %s" % (what, x.dtype))
    if len(p.shape) != 2 or p.shape[1] not in (2, 3) or (nd is not None and p.shape[1] != nd):
        raise ValueError("point_neighbors: the %s must have the shape (n, %s), got %s" % (what, nd or "2 or 3", tuple(p.shape)))
    if p.shape[0] >= 2 ** 31:
        raise ValueError("point_neighbors: 2^31 or more %s" % what)
    return p


def _scaled_points(p, per_axis, what):
    """p * spacing, rounded once per coordinate; ValueError for a coordinate that is not finite or reaches 2^500 in magnitude"""
    if R.is_torch(p):
        import torch
        s = p * torch.as_tensor(per_axis, dtype=torch.float64, device=p.device)
        fine = p.numel() == 0 or bool((torch.isfinite(p).all() & (s.abs() < _POINT_NEIGHBORS_MAX_COORD).all()))
    else:
        with np.errstate(all="ignore"):
            s = p * np.asarray(per_axis, np.float64)
            fine = bool(np.isfinite(p).all() and (np.abs(s) < _POINT_NEIGHBORS_MAX_COORD).all())
    if not fine:
        raise ValueError("point_neighbors: the %s must be finite and below 2^500 in magnitude (after the spacing)" % what)
    return s


def _squared_distances(q, p):
    """d2 of the definition between q (..., nd) and p (..., nd), numpy"""
    d = q - p
    s = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    return s + d[..., 2] * d[..., 2] if d.shape[-1] == 3 else s


def _nearest_host(P, Q, own, k, r2):
    """(indices (m, k) int64, d2 (m, k) float64) of the definition; the k-d tree supplies candidates only: K = min(n, k + 9) per row, a
    row is accepted when K >= n or when its k-th recomputed d2 is below (1 - 2^-40) times its largest recomputed d2 (then nothing the
    tree left out can reach the first k), and K doubles for the rows left.  own: the points are their own queries"""
    from scipy.spatial import cKDTree
    n, m = len(P), len(Q)
    out_i, out_d = np.full((m, k), -1, np.int64), np.full((m, k), np.inf)
    if n == 0 or m == 0:
        return out_i, out_d
    tree = cKDTree(P)
    rows, K = np.arange(m), min(n, k + 9)
    while len(rows):
        idx = np.asarray(tree.query(Q[rows], k=K, workers=_POINT_NEIGHBORS_WORKERS)[1], np.int64).reshape(len(rows), K)
        d2 = _squared_distances(Q[rows][:, None, :], P[idx])
        largest = d2.max(axis=1)
        if own:
            d2 = np.where(idx == rows[:, None], np.inf, d2)                 # a point is not its own neighbour; its slot sorts last
        order = np.lexsort((idx, d2), axis=1)[:, :k]                        # by (d2, index)
        best_d, best_i = np.take_along_axis(d2, order, axis=1), np.take_along_axis(idx, order, axis=1)
        if K >= n:
            done = np.ones(len(rows), bool)
        elif best_d.shape[1] < k:
            done = np.zeros(len(rows), bool)
        else:
            done = best_d[:, k - 1] < (1.0 - _POINT_NEIGHBORS_SLACK) * largest
        w = best_d.shape[1]
        got_d, got_i = best_d[done], best_i[done]
        keep = np.isfinite(got_d) if r2 is None else (got_d <= r2)          # inf: the own slot; the rest of a row is beyond r2 too
        out_d[rows[done], :w] = np.where(keep, got_d, np.inf)
        out_i[rows[done], :w] = np.where(keep, got_i, -1)
        rows, K = rows[~done], min(n, 2 * K)
    return out_i, out_d


def _within_host(P, Q, own, radius, r2, count_only):
    """(counts (m,), indices, d2) of the points within the radius, the rows ascending by index (indices and d2 None with count_only):
    the tree's ball of radius * (1 + 2^-40) supplies the candidates, d2 <= r2 decides"""
    from scipy.spatial import cKDTree
    n, m = len(P), len(Q)
    if n == 0 or m == 0:
        return np.zeros(m, np.int64), None if count_only else np.zeros(0, np.int64), None if count_only else np.zeros(0)
    lists = cKDTree(P).query_ball_point(Q, radius * (1.0 + _POINT_NEIGHBORS_SLACK), workers=_POINT_NEIGHBORS_WORKERS)
    lens = np.fromiter((len(l) for l in lists), np.int64, m)
    idx = np.fromiter((i for l in lists for i in l), np.int64, int(lens.sum()))
    row = np.repeat(np.arange(m), lens)
    d2 = _squared_distances(Q[row], P[idx])
    keep = d2 <= r2
    if own:
        keep &= idx != row
    row, idx, d2 = row[keep], idx[keep], d2[keep]
    counts = np.bincount(row, minlength=m).astype(np.int64)
    if count_only:
        return counts, None, None
    order = np.lexsort((idx, row))
    return counts, idx[order], d2[order]


def _point_neighbors_device(P, Q, mode, k, r2, cell_size=0.0, cell=None):
    """sd_point_neighbors_device on the contiguous float64 device tensors P (n, nd) and Q (m, nd) or None (the points are their own
    queries): mode 0 -> (indices (m, k), d2 (m, k)); mode 1 -> counts (m,); mode 2 -> (offsets (m + 1,), indices, d2), for which the
    total comes to the host to size the lists.  cell: a list that receives the cell edge the library used"""
    import ctypes
    import torch
    N.require_device()
    dev, n, nd = P.device, int(P.shape[0]), int(P.shape[1])
    m = n if Q is None else int(Q.shape[0])
    total, used = ctypes.c_longlong(0), ctypes.c_double(0.0)
    i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    fixed = (R.ptr(P), ctypes.c_longlong(n), None if Q is None else R.ptr(Q), ctypes.c_longlong(m), nd, int(mode), int(k or 0),
             int(r2 is not None), ctypes.c_double(0.0 if r2 is None else r2), ctypes.c_double(cell_size))
    tail = (ctypes.byref(total), ctypes.byref(used))
    if m == 0:                                    # no query: an empty tensor has no address to tell it from "no queries"
        out = (i64(0, k), f64(0, k)) if mode == 0 else i64(0) if mode == 1 else (torch.zeros(1, dtype=torch.int64, device=dev), i64(0), f64(0))
    elif mode == 0:
        idx, d2 = i64(m, k), f64(m, k)
        N.dcall(P, "sd_point_neighbors_device", *fixed, ctypes.c_longlong(0), R.ptr(idx), R.ptr(d2), None, *tail)
        out = idx, d2
    elif mode == 1:
        out = i64(m)
        N.dcall(P, "sd_point_neighbors_device", *fixed, ctypes.c_longlong(0), None, None, R.ptr(out), *tail)
    else:
        offsets = i64(m + 1)
        cap = max(1024, 32 * m)                   # a first guess; longer lists take a second call with the real total
        while True:
            idx, d2 = i64(cap), f64(cap)
            N.dcall(P, "sd_point_neighbors_device", *fixed, ctypes.c_longlong(cap), R.ptr(idx), R.ptr(d2), R.ptr(offsets), *tail)
            if total.value <= cap:
                break
            cap = total.value
        out = offsets, idx[:total.value].clone(), d2[:total.value].clone()
    if cell is not None:
        cell.append(used.value)
    return out


def _point_neighbors_args(k, radius, count_only, who="point_neighbors"):
    if k is None and radius is None:
        raise ValueError("%s: give k, radius or both" % who)
    if k is not None:
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= k <= _POINT_NEIGHBORS_MAX_K:
            raise ValueError("%s: k must be an integer in 1 .. %d, got %r" % (who, _POINT_NEIGHBORS_MAX_K, k))
        k = int(k)
    r2 = None
    if radius is not None:
        if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, float, np.integer, np.floating)) \
                or not np.isfinite(radius) or radius < 0:
            raise ValueError("%s: the radius must be a finite number >= 0, got %r" % (who, radius))
        radius = float(radius)
        with np.errstate(over="ignore"):
            r2 = float(np.float64(radius) * np.float64(radius))
    if count_only and radius is None:
        raise ValueError("%s: count_only needs a radius" % who)
    if count_only and k is not None:
        raise ValueError("%s: count_only counts the points within a radius; it takes no k" % who)
    return k, radius, r2


def point_neighbors(points, k=None, radius=None, *, queries=None, spacing=1, count_only=False, device=None, as_tensors=False):
    """The nearest points of every query, and the points within a radius of it: the k-nearest / radius graph over object centroids
    (CellProfiler's MeasureObjectNeighbors reports FirstClosestDistance, SecondClosestDistance and NumberOfNeighbors within a distance
    from it), or the nearest nucleus of every spot with a second point set.

    points: (n, nd), nd 2 or 3, a numpy array, a tensor or nested lists of an integer, float32 or float64 type, converted to float64
    (exactly, but for integers beyond 2^53) -- the stacked centroid-* columns of measure_labels, or details["points"].  queries: (m, nd)
    or None; with None the points are their own queries and point i is never a neighbour of query i -- only index i is left out, other
    points at the same place count, at distance 0.  spacing: a positive finite scalar or nd values.  At least one of k (1 .. 64) and
    radius (finite, >= 0) is needed.

    The definition, which both routes follow bit for bit.  A coordinate is scaled once, p[a] = fl(x[a] * spacing[a]).
    d2(q, p) = ((q0 - p0)^2 + (q1 - p1)^2) + (q2 - p2)^2, left to right (two terms for nd = 2), every operation rounded in float64, no
    fused multiply-add.  The candidates of a query are ordered by (d2, index).  "Within the radius" means d2 <= fl(radius * radius).
    A distance is sqrt(d2), correctly rounded.

    Returns a dict:
        with k            indices (m, k) int64 and distances (m, k) float64: the first k candidates of every query in that order --
                          with a radius as well, only those within it; -1 and inf where there are fewer
        radius alone      offsets (m + 1,) int64, and indices, distances (offsets[-1],): the points within the radius of query i are
                          the rows offsets[i] : offsets[i + 1], ascending by index
        count_only=True   counts (m,) int64, the lengths of those rows; the lists are not made

    Routing: DESIGN.md section 3p, like label_contacts: numpy or host input without device= runs the host code, a tensor on a HIP
    device or device= the kernels; the columns leave as measure_labels' do (exception 4 there, R.table_exit): numpy arrays, which the
    device route reads back with one synchronisation, unless as_tensors=True, which makes them tensors -- on the device for the device
    route, else where the points are or on `device`.  The
    host code asks scipy.spatial.cKDTree for candidates only (a few more than k, doubled while ties or near-ties reach the last of
    them; the ball of radius * (1 + 2^-40)) and recomputes d2, the order and the radius test by the definition.  The device route
    (csrc/point_neighbors.hip) sorts the points into a uniform grid of about two points per cell and walks the
    rings of cells around every query, one lane per query, until a bound that is safe under rounding says nothing nearer is left; no
    atomics, so the same bits from call to call.  It brings the points' box to the host once (a synchronisation), the total length
    for the radius lists once more, and for tensors one flag per point set that says the coordinates are fine.  Its time grows with
    the fullest cells: a single far outlier stretches the box and can put all other points into one cell, which is correct but
    quadratic, and a query far from all points walks up to every cell once.

    ValueError before anything runs: points that are not (n, 2) or (n, 3) or queries of another width, another dtype, a coordinate
    that is not finite, |coordinate * spacing| >= 2^500, n or m >= 2^31, k outside 1 .. 64, a radius that is negative or not finite,
    neither k nor radius, count_only without a radius or with k, a spacing that is not positive and finite."""
    if not R.is_torch(points):
        points = np.asarray(points)
    if queries is not None and not R.is_torch(queries):
        queries = np.asarray(queries)
    is_t = R.is_torch(points)
    on_device = device is not None or (is_t and points.is_cuda) or (queries is not None and R.is_device_tensor(queries))
    count_only = bool(count_only)
    k, radius, r2 = _point_neighbors_args(k, radius, count_only)
    P = _points_as_float64(points, "points")
    nd = int(P.shape[1])
    Q = None if queries is None else _points_as_float64(queries, "queries", nd)
    per_axis = R.spacing_zyx(spacing, nd, "point_neighbors")[1]
    own = Q is None
    P = _scaled_points(P, per_axis, "points")
    if not own:
        Q = _scaled_points(Q, per_axis, "queries")
    names = ("counts",) if count_only else ("indices", "distances") if k is not None else ("offsets", "indices", "distances")
    if on_device:
        import torch
        N.require_device()
        where = None
        for t in (points, queries):
            if where is None and R.is_device_tensor(t):
                where = t.device
        where = torch.device(device) if device is not None else where
        P = R.to_device_tensor(P, where)
        Q = None if own else R.to_device_tensor(Q, P.device)
        if count_only:
            cols = [_point_neighbors_device(P, Q, 1, None, r2)]
        elif k is not None:
            idx, d2 = _point_neighbors_device(P, Q, 0, k, r2)
            cols = [idx, R.ops(d2).sqrt(d2)]
        else:
            offsets, idx, d2 = _point_neighbors_device(P, Q, 2, None, r2)
            cols = [offsets, idx, R.ops(d2).sqrt(d2)]
        return dict(zip(names, R.table_exit(cols, as_tensors)))
    hP = P.cpu().numpy() if is_t else P
    hQ = hP if own else (Q.cpu().numpy() if R.is_torch(Q) else Q)
    if count_only:
        cols = [_within_host(hP, hQ, own, radius, r2, True)[0]]
    elif k is not None:
        idx, d2 = _nearest_host(hP, hQ, own, k, r2)
        cols = [idx, np.sqrt(d2)]
    else:
        counts, idx, d2 = _within_host(hP, hQ, own, radius, r2, False)
        cols = [np.concatenate([np.zeros(1, np.int64), np.cumsum(counts, dtype=np.int64)]), idx, np.sqrt(d2)]
    return dict(zip(names, R.table_exit(cols, as_tensors, points)))
