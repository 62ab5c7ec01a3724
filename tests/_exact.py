"""Helpers shared by the exact-comparison tests (test_gpu_training_scale.py, test_gpu_conv_exact.py, test_gpu_glue.py and the CPU tests
that stand in for a native): nothing here needs a GPU."""
import contextlib

import numpy as np


@contextlib.contextmanager
def nan_empty():
    """torch.empty / empty_like give NaN-filled floating tensors: a buffer the package allocates and a kernel leaves unwritten then
    shows up in its result"""
    import torch
    empty, empty_like = torch.empty, torch.empty_like

    def fill(t):
        return t.fill_(float("nan")) if t.is_floating_point() else t
    torch.empty = lambda *a, **k: fill(empty(*a, **k))
    torch.empty_like = lambda *a, **k: fill(empty_like(*a, **k))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = empty, empty_like


def select_numpy(prob, dist, prob_thresh, bs):
    """the contract of the selection native (sd_select_candidates_device, csrc/select.hip) as numpy: strict threshold (a NaN is never
    selected), a border of (lo, hi) grid steps per axis excluded, np.where order, max(1e-3, dist).  prob (*shape), dist (*shape, R) or
    None -> (prob (n,), dist (n, R) or None, points (n, ndim) int64)"""
    p = np.asarray(prob)
    with np.errstate(invalid="ignore"):
        mask = p > np.float32(prob_thresh)
    inner = np.zeros_like(mask)
    inner[tuple(slice(lo if lo > 0 else None, -hi if hi > 0 else None) for lo, hi in bs)] = True
    mask &= inner
    pts = np.stack(np.nonzero(mask), 1).astype(np.int64)
    return p[mask], (None if dist is None else np.maximum(np.float32(1e-3), np.asarray(dist)[mask])), pts
