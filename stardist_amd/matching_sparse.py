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


class _ScoredPairs:
    """the pairs of two objects (both ids > 0) of a sparse overlap list with their scores, and the optimal assignment among them: what
    matching_from_overlap and matched_pairs_from_overlap share.  ids_t / ids_p: the ids present, ascending; rt / rp: the relabelled ids of
    the list's entries (0 stays 0, the others 1 ... n); ti / pi / s: true rank, predicted rank and float32 score of every pair of two
    objects, ascending by (true id, predicted id)."""

    def __init__(self, t, p, counts, criterion):
        if criterion not in M.matching_criteria:
            raise ValueError("Matching criterion '%s' not supported." % criterion)
        self.criterion = criterion
        t, p, counts = (np.asarray(x, np.int64) for x in (t, p, counts))
        self.counts = counts
        self.ids_t, self.ids_p = np.unique(t[t > 0]), np.unique(p[p > 0])
        self.n_true, self.n_pred = len(self.ids_t), len(self.ids_p)
        self.n_matched = min(self.n_true, self.n_pred)
        self.rt = np.searchsorted(self.ids_t, t) + (t > 0)            # relabelled ids: 0 stays 0, the others 1 ... n in ascending order
        self.rp = np.searchsorted(self.ids_p, p) + (p > 0)
        self._scored = False
        self._comp = None

    def score(self):
        if self._scored:
            return
        rt, rp, counts, n_true, n_pred = self.rt, self.rp, self.counts, self.n_true, self.n_pred
        # areas: row sums include column 0, column sums include row 0
        area_t = np.bincount(rt, weights=counts, minlength=n_true + 1).astype(np.int64)
        area_p = np.bincount(rp, weights=counts, minlength=n_pred + 1).astype(np.int64)
        inner = (rt > 0) & (rp > 0)
        ti, pi, c = rt[inner] - 1, rp[inner] - 1, counts[inner]            # ascending by (true id, predicted id)
        den = {"iou": area_t[ti + 1] + area_p[pi + 1] - c, "iot": area_t[ti + 1], "iop": area_p[pi + 1]}[self.criterion]
        self.ti, self.pi = ti, pi
        self.s = M._safe_divide(c, den)                                     # float32 of the float64 quotient, every entry > 0
        self._scored = True

    def assign(self, thr):
        """flags of the pairs an optimal assignment takes (the positive-score part of it)"""
        from scipy.optimize import linear_sum_assignment
        self.score()
        s, ti, pi = self.s, self.ti, self.pi
        if self.criterion == "iou" and thr > 0.5:
            return s >= thr                                             # ok pairs are disjoint: all of them are taken
        if len(s) == 0:
            return np.zeros(0, bool)
        if self._comp is None:
            comp = _components(ti, pi, self.n_true, self.n_pred)
            order = np.argsort(comp, kind="stable")
            starts = np.flatnonzero(np.r_[True, comp[order][1:] != comp[order][:-1], True])
            self._comp = (order, starts)
        order, starts = self._comp
        take = np.zeros(len(s), bool)
        size = np.diff(starts)
        take[order[starts[:-1][size == 1]]] = True                      # 1 x 1 components: their positive-score pair is taken
        for k in np.flatnonzero(size > 1):
            e = order[starts[k]:starts[k + 1]]
            ut, it = np.unique(ti[e], return_inverse=True)
            up, ip = np.unique(pi[e], return_inverse=True)
            sub = np.zeros((len(ut), len(up)), np.float32)
            sub[it, ip] = s[e]
            r, q = linear_sum_assignment(-(sub >= thr).astype(float) - sub / (2 * self.n_matched))
            hit = np.zeros_like(sub, bool)
            hit[r, q] = True
            take[e] = hit[it, ip]
        return take


def matching_from_overlap(t, p, counts, n_pixels, thresh=0.5, criterion="iou", report_matches=False):
    """Matching namedtuple(s) of stardist_amd.matching.matching from the sparse overlap list (t, p, counts) of two label images with
    n_pixels pixels each (the list as sparse_overlap / label_overlap_device return it).  thresh: scalar or sequence, None = 0.
    Exactness as stated in the module docstring."""
    from collections import namedtuple
    if thresh is None:
        thresh = 0
    sp = _ScoredPairs(t, p, counts, criterion)
    thresh = float(thresh) if np.isscalar(thresh) else [float(x) for x in thresh]
    n_true, n_pred, n_matched = sp.n_true, sp.n_pred, sp.n_matched
    if report_matches:
        if n_true * n_pred > DENSE_LIMIT:
            raise ValueError("report_matches=True needs the dense %d x %d score matrix (more than %d entries); call matching without it"
                             % (n_true, n_pred, DENSE_LIMIT))
        overlap = np.zeros((n_true + 1, n_pred + 1), np.uint)
        overlap[sp.rt, sp.rp] = sp.counts
        overlap[0, 0] = n_pixels - int(sp.counts.sum())
        back_true = np.concatenate([[0], sp.ids_t])
        back_pred = np.concatenate([[0], sp.ids_p])
        return M._matching_dense(overlap, back_true, back_pred, thresh, criterion, report_matches)
    sp.score()
    s, ti = sp.s, sp.ti

    def at(thr):
        tp, total = 0, 0.0
        if n_matched > 0:
            take = sp.assign(thr)
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


def matched_pairs_from_overlap(t, p, counts, thresh, criterion="iou"):
    """(true ids, predicted ids) of the true positives of matching(y_true, y_pred, thresh, criterion) -- the pairs its report_matches
    output marks in matched_tps -- from the sparse overlap list, ascending by true id; thresh: one number > 0 (for thresh <= 0 the dense
    assignment's filler pairs count as matches, and only the dense path defines them).  Same scores and per-component assignment as
    matching_from_overlap."""
    thr = float(thresh)
    if not thr > 0:
        raise ValueError("matched_pairs_from_overlap needs thresh > 0")
    sp = _ScoredPairs(t, p, counts, criterion)
    sp.score()
    ok = sp.assign(thr) & (sp.s >= thr)
    return sp.ids_t[sp.ti[ok]], sp.ids_p[sp.pi[ok]]


def group_tables_from_overlaps(lists, ids_first_max, thresh, criterion="iou"):
    """The id maps of stardist_amd.matching.group_matching_labels from the sparse overlap lists of the RAW consecutive frames
    (lists[k] = sparse_overlap(ys[k], ys[k + 1])): K tables (raw ids ascending, new ids), int64.  Grouping renames the ids of a frame one
    to one, so frame k + 1 matches the grouped frame k as it matches the raw one; the maps compose: frame 0 keeps its ids, an id of
    frame k + 1 takes the new id of its partner in frame k, or -- in ascending order of the ids without a partner -- the next free id,
    the first one being ids_first_max + 1 (ids_first_max = max(ys[0])).  thresh > 0."""
    t0 = np.asarray(lists[0][0], np.int64)
    ids = np.unique(t0[t0 > 0])
    tables = [(ids, ids.copy())]
    next_id = int(ids_first_max) + 1
    for t, p, c in lists:
        prev_ids, prev_new = tables[-1]
        mt, mp = matched_pairs_from_overlap(t, p, c, thresh, criterion)
        p = np.asarray(p, np.int64)
        ids = np.unique(p[p > 0])
        new = np.zeros(len(ids), np.int64)
        has = np.zeros(len(ids), bool)
        at = np.searchsorted(ids, mp)
        has[at] = True
        new[at] = prev_new[np.searchsorted(prev_ids, mt)]
        fresh = int(np.count_nonzero(~has))
        if next_id + fresh > 2 ** 31:
            raise ValueError("the grouped labels need ids above 2**31 - 1")
        new[~has] = next_id + np.arange(fresh)
        next_id += fresh
        tables.append((ids, new))
    return tables


def lookup_tables(ys, tables):
    """numpy mirror of sd_relabel_stack_device: int32 stack with out[k] = new id of ys[k] by tables[k] (0 stays 0)"""
    out = np.zeros((len(ys),) + tuple(ys[0].shape), np.int32)
    for k, (ids, new) in enumerate(tables):
        y = np.asarray(ys[k]).astype(np.int64)
        if len(ids):
            at = np.minimum(np.searchsorted(ids, y), len(ids) - 1)
            out[k] = np.where((ids[at] == y) & (y > 0), new[at], 0)
    return out


def _is_int_dtype(y):
    if N.is_torch(y):
        return not (y.dtype.is_floating_point or y.dtype.is_complex) and str(y.dtype) != "torch.bool"
    return M.is_array_of_integers(y)


def _label_err(name):
    return ValueError("%s must be an array of non-negative integers." % name)


def _minimum(y):
    import torch
    return int(y.min()) if not N.is_torch(y) else int(y.to(torch.int64).min())


def _int32_range_error(lo, hi, name):
    if lo < 0:
        return _label_err(name)
    if hi > 2 ** 31 - 1:
        return ValueError("%s: label ids above 2**31 - 1 are not supported on the device" % name)


def _wide(y):
    """can the dtype of y hold ids outside int32?"""
    import torch
    if N.is_torch(y):
        return y.dtype in (torch.int64, torch.uint32, torch.uint64)
    return y.dtype.itemsize > 4 or y.dtype == np.uint32


def _to_device_int32(y, name, dev):
    """int32 copy (or view) of the label image y on dev; ids outside int32 raise"""
    import torch
    if N.is_torch(y):
        if _wide(y):
            err = _int32_range_error(*(int(v) for v in torch.aminmax(y.to(torch.int64))), name)
            if err:
                raise err
        return y.to(device=dev, dtype=torch.int32).contiguous()
    y = np.asarray(y)
    if _wide(y):
        err = _int32_range_error(int(y.min()), int(y.max()), name)
        if err:
            raise err
    return torch.from_numpy(np.ascontiguousarray(y, dtype=np.int32)).to(dev)


def _stack_to_device_int32(frames, name, dev):
    """int32 device stack of frames of one shape; ids outside int32 raise.  numpy frames are checked on the host; wide device frames are
    stacked first and checked together: one read-back however many frames there are"""
    import torch
    wide = [N.is_torch(y) and _wide(y) for y in frames]
    if not any(wide):
        return torch.stack([_to_device_int32(y, name, dev) for y in frames])
    parts = [y.to(device=dev, dtype=torch.int64) if w else _to_device_int32(y, name, dev).to(torch.int64) for y, w in zip(frames, wide)]
    return _to_device_int32(torch.stack(parts), name, dev)


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


def _overlap_stack_call(a):
    """sd_label_overlap_stack_device on an int32 device stack (K, n): (keys, counts) device tensors cut to the real count, the K list
    offsets and the (K, 2) {min, max} of the frames, numpy"""
    import ctypes
    import torch
    K, n = a.shape
    count, offs, mm = ctypes.c_longlong(0), (ctypes.c_longlong * K)(), (ctypes.c_int32 * (2 * K))()
    cap = max(1024, (K - 1) * n // 16)    # pairs are rarely smaller than 16 pixels on average; else a second call with the real count
    with _native_lock:
        while True:
            keys = torch.empty(cap, dtype=torch.int64, device=a.device)
            counts = torch.empty(cap, dtype=torch.int64, device=a.device)
            N.dcall(a, "sd_label_overlap_stack_device", N.tptr(a), K, ctypes.c_longlong(n), ctypes.c_longlong(cap), N.tptr(keys),
                    N.tptr(counts), offs, ctypes.byref(count), mm)
            if count.value <= cap:
                break
            cap = count.value
    m = count.value
    return keys[:m], counts[:m], np.array(offs[:], np.int64), np.array(mm[:], np.int32).reshape(K, 2)


def _split_lists(keys, counts, offs):
    """the K - 1 lists (t, p, count) of the concatenated keys / counts (numpy) of a stack call"""
    return [(keys[lo:hi] >> 32, keys[lo:hi] & 0xFFFFFFFF, counts[lo:hi]) for lo, hi in zip(offs[:-1], offs[1:])]


def label_overlap_stack_device(ys):
    """sd_label_overlap_stack_device on an int32 device stack (K, ...), K >= 2, in one native call: ([sparse_overlap(ys[k], ys[k + 1]) for
    k < K - 1] as numpy int64 triples, the (K, 2) array of {min, max} per frame).  The lists are empty when a minimum is negative."""
    import torch
    assert ys.dtype == torch.int32 and ys.is_cuda and ys.shape[0] >= 2
    keys, counts, offs, mm = _overlap_stack_call(ys.contiguous().reshape(ys.shape[0], -1))
    return _split_lists(keys.cpu().numpy(), counts.cpu().numpy(), offs), mm


def relabel_stack_device(ys, tables, maxima=None):
    """sd_relabel_stack_device: the int32 device stack ys (K, ...) relabelled by tables[k] = (raw ids ascending, new ids) -- as lookup_tables
    does on the host -- in one native call; maxima: the largest id of every frame where known (else the tables' last ids)"""
    import ctypes
    import torch
    K = ys.shape[0]
    assert ys.dtype == torch.int32 and ys.is_cuda and len(tables) == K
    a = ys.contiguous().reshape(K, -1)
    offs = np.concatenate([[0], np.cumsum([len(ids) for ids, _ in tables])]).astype(np.int64)
    if maxima is None:
        maxima = [int(ids[-1]) if len(ids) else 0 for ids, _ in tables]
    both = np.stack([np.concatenate([np.asarray(ids, np.int64) for ids, _ in tables]), np.concatenate([np.asarray(new, np.int64) for _, new in tables])])
    assert both.size == 0 or (0 <= both.min() and both.max() <= 2 ** 31 - 1)
    dev = torch.from_numpy(both.astype(np.int32)).to(a.device)          # one upload for ids and new ids
    out = torch.empty_like(a)
    h_offs, h_max = (ctypes.c_longlong * (K + 1))(*offs.tolist()), (ctypes.c_int32 * K)(*[int(v) for v in maxima])
    with _native_lock:
        N.dcall(a, "sd_relabel_stack_device", N.tptr(a), K, ctypes.c_longlong(a.shape[1]), N.tptr(dev[0]), N.tptr(dev[1]), h_offs, h_max,
                N.tptr(out))
    return out.reshape(ys.shape)


def group_matching_labels_device(ys, thresh=1e-10, criterion="iou", device=None):
    """stardist_amd.matching.group_matching_labels on a HIP device.  ys: a stack (torch tensor or numpy array) or a sequence of label
    images of any integer dtype (ids below 2**31), uploaded to `device` (default: the device of a device tensor among the inputs).  One
    overlap call for all consecutive pairs of the raw frames, the id maps composed on the host from the sparse lists
    (group_tables_from_overlaps), one relabel call.  Returns the int32 stack: a device tensor if an input lives on a device, numpy
    otherwise; the inputs stay untouched.  Same errors, in the same order, as the host function (a `device` that is no HIP device is
    reported after the label-type and the shape checks).  Equal to the host function wherever no
    two optimal assignments tie exactly (module docstring).  thresh <= 0 (None) counts the dense assignment's filler pairs as matches,
    which only the dense path defines: the stack is then downloaded, grouped by the host function and uploaded again."""
    import torch
    if len(ys) <= 1:
        raise ValueError("'ys' must have 2 or more entries")
    single = N.is_torch(ys) or isinstance(ys, np.ndarray)
    frames = [ys] if single else list(ys)
    on_device = [y for y in frames if M._on_device(y)]
    device = torch.device(device if device is not None else on_device[0].device if on_device else "cpu")
    if not all((N.is_torch(y) or isinstance(y, np.ndarray)) and _is_int_dtype(y) for y in frames):
        raise _label_err("ys")
    shape = tuple(frames[0].shape)
    same_shape = all(tuple(y.shape) == shape for y in frames)
    n = int(np.prod(shape))
    host = lambda y: y.cpu().numpy() if N.is_torch(y) else np.asarray(y)
    host_call = lambda: M.group_matching_labels(host(ys) if single else [host(y) for y in frames], thresh=thresh, criterion=criterion)
    back = (lambda g: torch.from_numpy(g).to(device)) if on_device else (lambda g: g)
    wrong_shape = (single and ys.ndim <= 1) or not same_shape or n == 0
    # the host's own checks, in its order (labels, then dimensions / shapes), before the one check it does not have
    grouped = host_call() if wrong_shape else None
    if device.type != "cuda":
        raise ValueError("device must be a HIP device, not %s" % device)
    if wrong_shape:
        return back(grouped)                                            # empty frames: nothing to do on the device
    N.require_device()
    if thresh is None or not float(thresh) > 0:
        return back(host_call())                                        # the host's dense matching for thresh <= 0
    a = _to_device_int32(ys, "ys", device) if single else _stack_to_device_int32(frames, "ys", device)
    lists, mm = label_overlap_stack_device(a)
    if mm[:, 0].min() < 0:
        raise _label_err("ys")
    tables = group_tables_from_overlaps(lists, mm[0, 1], thresh, criterion)
    out = relabel_stack_device(a, tables, mm[:, 1])
    return out if on_device else out.cpu().numpy()
