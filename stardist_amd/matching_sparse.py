"""Detection metrics from the SPARSE overlap of two label images: the device path of stardist_amd.matching.matching.

The host path (matching.py:109-230 as stardist_amd.matching states it) builds a dense (n_true + 1) x (n_pred + 1) overlap matrix, a dense
score matrix and a dense linear_sum_assignment.  Only pairs of objects that share pixels matter, so here:

1. the overlap list -- every pair (t, p) != (0, 0) that occurs, with its pixel count, ascending by (t, p) -- comes from the HIP kernel
   sd_label_overlap_device (csrc/overlap.hip) for device tensors, or from `sparse_overlap` (numpy, the same list) on the host;
2. areas, scores and the assignment are finished on the host from that list (`matching_from_overlap`) with the host path's arithmetic:
   integer numerators and denominators divided in float64 and stored as float32 (_safe_divide), the same assignment cost
   -(s >= thr) - s / (2 n_matched), solved per connected component of the graph of pairs with a positive score (pairs of score 0 cost
   0 for thr > 0, so the dense optimum decomposes), and the matched-score sum built as the host builds it (float32 scores of the ok
   pairs in ascending true-id order, np.sum).

Exactness: every integer field equals the host path's; every float field is bit-identical for thresh > 0; for thresh <= 0 (None) the
float fields agree to 1e-6 relative (the host's sum then includes zero-score filler pairs whose places only the dense assignment fixes).
Exact score ties between two optimal assignments are outside this statement (either optimum is correct; the two paths may pick
different ones).  report_matches=True needs those filler pairs too: the sparse scores are expanded to the dense matrix and the host's
code runs on it, up to DENSE_LIMIT matrix entries.
"""
import threading

import numpy as np

from . import matching as M
from .lib import _native as N

# report_matches=True expands the score matrix: n_true * n_pred above this raises (float32 scores plus the float64 cost: ~12 bytes each)
DENSE_LIMIT = 1 << 28
_native_lock = threading.Lock()          # the native workspace arena serves one call at a time (matching_dataset(parallel=True))


def sparse_overlap(y_true, y_pred):
    """numpy mirror of sd_label_overlap_device: (t, p, count) int64 arrays of every pair (t, p) != (0, 0) of labels that share pixels,
    ascending by (t, p), original ids.  Labels must be non-negative and below 2**31."""
    t = np.asarray(y_true).ravel().astype(np.int64)
    p = np.asarray(y_pred).ravel().astype(np.int64)
    keys, counts = np.unique((t << 32) | p, return_counts=True)
    if len(keys) and keys[0] == 0:
        keys, counts = keys[1:], counts[1:]
    return keys >> 32, keys & 0xFFFFFFFF, counts.astype(np.int64)


def label_overlap_device(y_true, y_pred):
    """sd_label_overlap_device on two int32 device tensors of the same number of elements: ((t, p, count) as in sparse_overlap, numpy int64;
    (min, max) of y_true; (min, max) of y_pred).  The list is empty when a minimum is negative."""
    import ctypes
    import torch
    assert y_true.dtype == torch.int32 and y_pred.dtype == torch.int32 and y_true.device == y_pred.device
    a, b = y_true.contiguous().reshape(-1), y_pred.contiguous().reshape(-1)
    n = a.numel()
    assert b.numel() == n
    count, mm = ctypes.c_longlong(0), (ctypes.c_int32 * 4)()
    cap = max(1024, n // 16)              # pairs are rarely smaller than 16 pixels on average; else a second call with the real count
    with _native_lock:
        while True:
            keys = torch.empty(cap, dtype=torch.int64, device=a.device)
            counts = torch.empty(cap, dtype=torch.int64, device=a.device)
            N.dcall(a, "sd_label_overlap_device", N.tptr(a), N.tptr(b), ctypes.c_longlong(n), ctypes.c_longlong(cap), N.tptr(keys),
                    N.tptr(counts), ctypes.byref(count), mm)
            if count.value <= cap:
                break
            cap = count.value
        m = count.value
        keys, counts = keys[:m].cpu().numpy(), counts[:m].cpu().numpy()
    return (keys >> 32, keys & 0xFFFFFFFF, counts), (mm[0], mm[1]), (mm[2], mm[3])


def _components(ti, pi, n_true, n_pred):
    """connected component of every pair of the bipartite graph (true ranks ti, predicted ranks pi)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    g = coo_matrix((np.ones(len(ti), np.int8), (ti, n_true + pi)), shape=(n_true + n_pred,) * 2)
    _, comp = connected_components(g, directed=False)
    return comp[ti]


def matching_from_overlap(t, p, counts, n_pixels, thresh=0.5, criterion="iou", report_matches=False):
    """Matching namedtuple(s) of stardist_amd.matching.matching from the sparse overlap list (t, p, counts) of two label images with
    n_pixels pixels each (the list as sparse_overlap / label_overlap_device return it).  thresh: scalar or sequence, None = 0.
    Exactness as stated in the module docstring."""
    from collections import namedtuple
    from scipy.optimize import linear_sum_assignment
    if criterion not in M.matching_criteria:
        raise ValueError("Matching criterion '%s' not supported." % criterion)
    if thresh is None:
        thresh = 0
    thresh = float(thresh) if np.isscalar(thresh) else [float(x) for x in thresh]
    t, p, counts = (np.asarray(x, np.int64) for x in (t, p, counts))
    ids_t, ids_p = np.unique(t[t > 0]), np.unique(p[p > 0])
    n_true, n_pred = len(ids_t), len(ids_p)
    rt = np.searchsorted(ids_t, t) + (t > 0)            # relabelled ids: 0 stays 0, the others 1 ... n in ascending order
    rp = np.searchsorted(ids_p, p) + (p > 0)
    if report_matches:
        if n_true * n_pred > DENSE_LIMIT:
            raise ValueError("report_matches=True needs the dense %d x %d score matrix (more than %d entries); call matching without it"
                             % (n_true, n_pred, DENSE_LIMIT))
        overlap = np.zeros((n_true + 1, n_pred + 1), np.uint)
        overlap[rt, rp] = counts
        overlap[0, 0] = n_pixels - int(counts.sum())
        back_true = np.concatenate([[0], ids_t])
        back_pred = np.concatenate([[0], ids_p])
        return M._matching_dense(overlap, back_true, back_pred, thresh, criterion, report_matches)
    # areas: row sums include column 0, column sums include row 0
    area_t = np.bincount(rt, weights=counts, minlength=n_true + 1).astype(np.int64)
    area_p = np.bincount(rp, weights=counts, minlength=n_pred + 1).astype(np.int64)
    inner = (rt > 0) & (rp > 0)
    ti, pi, c = rt[inner] - 1, rp[inner] - 1, counts[inner]            # ascending by (true id, predicted id)
    den = {"iou": area_t[ti + 1] + area_p[pi + 1] - c, "iot": area_t[ti + 1], "iop": area_p[pi + 1]}[criterion]
    s = M._safe_divide(c, den)                                          # float32 of the float64 quotient, every entry > 0
    n_matched = min(n_true, n_pred)
    comp = order = starts = None

    def assign(thr):
        """flags of the pairs an optimal assignment takes (the positive-score part of it)"""
        nonlocal comp, order, starts
        if criterion == "iou" and thr > 0.5:
            return s >= thr                                             # ok pairs are disjoint: all of them are taken
        if len(s) == 0:
            return np.zeros(0, bool)
        if comp is None:
            comp = _components(ti, pi, n_true, n_pred)
            order = np.argsort(comp, kind="stable")
            starts = np.flatnonzero(np.r_[True, comp[order][1:] != comp[order][:-1], True])
        take = np.zeros(len(s), bool)
        size = np.diff(starts)
        take[order[starts[:-1][size == 1]]] = True                      # 1 x 1 components: their positive-score pair is taken
        for k in np.flatnonzero(size > 1):
            e = order[starts[k]:starts[k + 1]]
            ut, it = np.unique(ti[e], return_inverse=True)
            up, ip = np.unique(pi[e], return_inverse=True)
            sub = np.zeros((len(ut), len(up)), np.float32)
            sub[it, ip] = s[e]
            r, q = linear_sum_assignment(-(sub >= thr).astype(float) - sub / (2 * n_matched))
            hit = np.zeros_like(sub, bool)
            hit[r, q] = True
            take[e] = hit[it, ip]
        return take

    def at(thr):
        tp, total = 0, 0.0
        if n_matched > 0:
            take = assign(thr)
            if thr > 0:
                ok = take & (s >= thr)
                tp = int(np.count_nonzero(ok))
                total = np.sum(s[ok])                                   # ascending true id, as the host's scores[ti, pi][ok]
            else:
                # every pair of the dense assignment is ok: n_matched of them, the rows not matched here take score-0 fillers
                tp = n_matched
                row = np.zeros(n_true, np.float32)
                row[ti[take]] = s[take]
                if n_true <= n_pred:
                    total = np.sum(row)                                 # the host sums exactly this array
                else:
                    matched = np.zeros(n_true, bool)
                    matched[ti[take]] = True
                    sel = np.flatnonzero(matched)
                    fill = np.flatnonzero(~matched)[:n_matched - len(sel)]
                    total = np.sum(row[np.sort(np.r_[sel, fill])])
        vals = M._matching_vals(criterion, thr, tp, total, n_true, n_pred)
        return namedtuple("Matching", vals.keys())(*vals.values())
    return at(thresh) if np.isscalar(thresh) else tuple(at(x) for x in thresh)


def _is_int_dtype(y):
    if N.is_torch(y):
        return not (y.dtype.is_floating_point or y.dtype.is_complex) and str(y.dtype) != "torch.bool"
    return M.is_array_of_integers(y)


def _label_err(name):
    return ValueError("%s must be an array of non-negative integers." % name)


def _minimum(y):
    import torch
    return int(y.min()) if not N.is_torch(y) else int(y.to(torch.int64).min())


def _to_device_int32(y, name, dev):
    """int32 copy (or view) of the label image y on dev; ids outside int32 raise"""
    import torch
    if N.is_torch(y):
        if y.dtype in (torch.int64, torch.uint32, torch.uint64):
            y64 = y.to(torch.int64)
            lo, hi = (int(v) for v in torch.aminmax(y64))
            if lo < 0:
                raise _label_err(name)
            if hi > 2 ** 31 - 1:
                raise ValueError("%s: label ids above 2**31 - 1 are not supported on the device" % name)
        return y.to(device=dev, dtype=torch.int32).contiguous()
    y = np.asarray(y)
    if y.dtype.itemsize > 4 or y.dtype == np.uint32:
        lo, hi = int(y.min()), int(y.max())
        if lo < 0:
            raise _label_err(name)
        if hi > 2 ** 31 - 1:
            raise ValueError("%s: label ids above 2**31 - 1 are not supported on the device" % name)
    return torch.from_numpy(np.ascontiguousarray(y, dtype=np.int32)).to(dev)


def matching_device(y_true, y_pred, thresh=0.5, criterion="iou", report_matches=False, device=None):
    """stardist_amd.matching.matching on a HIP device: torch tensors or numpy arrays of any integer dtype (ids below 2**31), uploaded to
    `device` (default: the device of a device tensor among the inputs); same errors and messages as the host path, one overlap for all
    thresholds.  Exactness as stated in the module docstring."""
    import torch
    if device is None:
        device = next(y.device for y in (y_true, y_pred) if M._on_device(y))
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("device must be a HIP device, not %s" % device)
    N.require_device()
    for y, name in ((y_true, "y_true"), (y_pred, "y_pred")):
        if not _is_int_dtype(y):
            raise _label_err(name)
    shape_t, shape_p = tuple(y_true.shape), tuple(y_pred.shape)
    n = int(np.prod(shape_t))
    if shape_t != shape_p or n == 0:
        # the host path's order: negative labels of y_true, of y_pred, then the shapes; empty images go the host's way
        for y, name in ((y_true, "y_true"), (y_pred, "y_pred")):
            if len(y) and _minimum(y) < 0:
                raise _label_err(name)
        if shape_t != shape_p:
            raise ValueError("y_true (%s) and y_pred (%s) have different shapes" % (shape_t, shape_p))
        host = lambda y: y.cpu().numpy() if N.is_torch(y) else np.asarray(y)
        return M.matching(host(y_true), host(y_pred), thresh=thresh, criterion=criterion, report_matches=report_matches)
    a = _to_device_int32(y_true, "y_true", device)
    b = _to_device_int32(y_pred, "y_pred", device)
    (t, p, c), mm_t, mm_p = label_overlap_device(a, b)
    if mm_t[0] < 0:
        raise _label_err("y_true")
    if mm_p[0] < 0:
        raise _label_err("y_pred")
    if criterion not in M.matching_criteria:
        raise ValueError("Matching criterion '%s' not supported." % criterion)
    return matching_from_overlap(t, p, c, n, thresh=thresh, criterion=criterion, report_matches=report_matches)
