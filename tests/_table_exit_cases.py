"""Cases for the table functions' shared exit (stardist_amd._route.table_exit): measure_labels with every keyword at once, label_contacts
and point_neighbors, shared by tests/golden/make_measure_table_golden.py (which records the host route's tables of the commit before
the exit was shared), tests/test_cpu_table_exit.py and tests/test_gpu_table_exit.py.  `call(name)` gives (function name, arguments,
keywords); `run(name, **more)` calls it; `host(name)` is the host route's table, computed once and read-only."""
import hashlib
import os

import numpy as np

import _hull_cases as H
import _measure_cases as M
import _shape_cases as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "measure_table_parent.npz")
LIBM = S.LIBM
_calls, _host = {}, {}


def libm_close(a, b):
    """the project's rule for the columns that call atan2 / pow (tests/test_gpu_measure_shape.py): 1e-14 of max(|a|, |b|, 1)"""
    return bool((np.abs(a - b) <= 1e-14 * np.maximum(np.maximum(np.abs(a), np.abs(b)), 1)).all())


def _every_keyword(lbl, hull=True):
    nd = lbl.ndim
    return dict(shape=True, hull=hull, percentiles=(50, 99.8), neighbors=2, nearest=3, within=9.0, spacing=(2, 0.5) if nd == 2 else (2, 0.5, 1.5),
                spots=np.argwhere(lbl > 0)[::7] if (lbl > 0).any() else np.argwhere(lbl == 0)[::7])


def _build():
    lbl, img = M.case("2d_u8_rgb")
    lbl = np.maximum(lbl, 0)                                                # neighbors= refuses the case's negative label
    _calls["measure_2d"] = ("measure_labels", (lbl, img), _every_keyword(lbl))
    lbl3, img3 = M.case("3d_u8")
    _calls["measure_3d"] = ("measure_labels", (lbl3, img3), _every_keyword(lbl3, hull=False))
    lbl_f, img_f = M.case("2d_f32_random")                                  # float sums: compared through M.check_float_columns
    _calls["measure_2d_f32"] = ("measure_labels", (np.maximum(lbl_f, 0), img_f), _every_keyword(np.maximum(lbl_f, 0)))
    none = np.zeros((0, 5), np.int32)
    _calls["measure_no_pixels"] = ("measure_labels", (none, np.zeros((0, 5), np.uint8)), _every_keyword(none))
    bg = np.zeros((11, 13), np.int32)
    _calls["measure_background"] = ("measure_labels", (bg, np.random.default_rng(5201).integers(0, 256, bg.shape, dtype=np.uint8)),
                                    _every_keyword(bg))
    _calls["contacts"] = ("label_contacts", (lbl, 2), dict(symmetric=True, background=True))
    pts = np.random.default_rng(5202).uniform(0, 40, (61, 3))
    pts[7] = pts[3]                                                         # two points at one place
    _calls["points_k"] = ("point_neighbors", (pts,), dict(k=3, spacing=(1, 0.5, 2)))
    _calls["points_radius"] = ("point_neighbors", (pts,), dict(radius=9.0, spacing=(1, 0.5, 2)))
    _calls["points_count"] = ("point_neighbors", (pts,), dict(radius=9.0, spacing=(1, 0.5, 2), count_only=True))


GOLDEN_NAMES = ("measure_2d", "measure_3d", "measure_no_pixels", "measure_background", "contacts", "points_k", "points_radius", "points_count")
MEASURE_GPU = ("measure_2d", "measure_3d")
# the derived columns (_measure_columns, _shape_columns with its Jacobi sweeps, _hull_columns) on the raw tables of these cases
DERIVED = tuple(("shape", n) for n in S.SMALL) + tuple(("hull", n) for n in H.SMALL)


def derived(kind, name):
    return S.host(name) if kind == "shape" else H.host(name)


def digests(table):
    """(columns that are not LIBM, 32) uint8: the SHA-256 of every such column's name, dtype and bytes, in the table's order"""
    rows = [hashlib.sha256(("%s %s " % (k, v.dtype)).encode() + np.ascontiguousarray(v).tobytes()).digest() for k, v in table.items() if k not in LIBM]
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), 32)


def call(name):
    if not _calls:
        _build()
    return _calls[name]


def run(name, convert=None, **more):
    """the case's call; convert: applied to every array argument and to spots (to make them tensors)"""
    from stardist_amd import utils
    fn, args, kw = call(name)
    if convert is not None:
        args = tuple(convert(a) if isinstance(a, np.ndarray) else a for a in args)
        kw = {k: convert(v) if k == "spots" else v for k, v in kw.items()}
    return getattr(utils, fn)(*args, **kw, **more)


def host(name):
    got = _host.get(name)
    if got is None:
        got = _host[name] = run(name)
        for v in got.values():
            v.setflags(write=False)
    return got


def same_table(got, want, libm=()):
    """keys, order, dtypes and bytes; the columns `libm` by libm_close.  got may hold tensors"""
    assert list(got) == list(want)
    for k in want:
        g = got[k] if isinstance(got[k], np.ndarray) else got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, k
        if k in libm:
            assert libm_close(g, want[k]), k
        else:
            assert g.tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
