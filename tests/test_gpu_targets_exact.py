"""GPU: the training targets (csrc/edt.hip, csrc/star_dist.hip and their drivers) compared EXACTLY -- with ==, no tolerance anywhere -- with
the plain numpy references of _target_cases.py, which stand alone (no scipy, no compiled reference; test_cpu_target_cases.py proves them
against both).  Every case of EDT2D / EDT3D / SD2D / SD3D / BATCH2D / BATCH3D goes through the public route (utils.edt_prob with a numpy
array and with a device tensor, geom2d.star_dist / geom3d.star_dist3D with mode="hip", targets.stardist_targets, training.targets_device /
training3d.targets_device3d, TrainData2D / TrainData3D.batch_device) where that route accepts its arguments (star_dist refuses
n_rays < 3 and grids that are no power of two: those cases are raw only), and through the raw entry points (N.dcall).  Every output buffer
starts as NaN (torch.empty is patched while the package allocates, raw calls write into torch.full(nan)): an element that no thread writes
fails.  Each driver case runs twice with other batches in between: the arena and the 3D `full` buffer are reused."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import _target_cases as T
from _exact import nan_empty

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _same(got, want, lbl=None, tag=""):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.dtype == np.float32, (tag, got.dtype)
    assert not np.isnan(got).any() and np.array_equal(got, want), "%s: %s" % (tag, T.describe(got, want, lbl))


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def _raw_edt(lab, aniso):
    """sd_edt_prob_device on an int32 label image (a constant one padded with background first, as the driver does)"""
    from stardist_amd.lib import _native as N
    lab = np.ascontiguousarray(lab, np.int32)
    nd = lab.ndim
    const = lab.min() == lab.max() and lab.flat[0] > 0
    if const:
        lab = np.pad(lab, ((1, 1),) * nd)
    samp = (1.0,) * nd if aniso is None else tuple(float(a) for a in aniso)
    Z, Y, X = ((1,) + lab.shape) if nd == 2 else lab.shape
    sz, sy, sx = ((1.0,) + samp) if nd == 2 else samp
    d_lab = torch.from_numpy(lab).to(DEV)
    out = torch.full(lab.shape, float("nan"), dtype=torch.float32, device=DEV)
    N.dcall(d_lab, "sd_edt_prob_device", _p(d_lab), Z, Y, X, sz, sy, sx, max(int(lab.max()), 0), _p(out))
    return out[(slice(1, -1),) * nd] if const else out


@pytest.mark.parametrize("id", T.ids(T.EDT2D + T.EDT3D))
def test_edt_prob_equals_box_reference(id):
    from stardist_amd import utils
    c = T.BY_ID[id]
    lab, want = T.labels(id), T.edt_want(id)
    sel = (lambda a: a) if "ids" not in c else (lambda a: np.where(np.isin(lab, c["ids"]), a.cpu().numpy() if torch.is_tensor(a) else a, np.float32(0)))
    with nan_empty():
        got_np = _quiet(utils.edt_prob, lab, anisotropy=c["aniso"])
        got_t = _quiet(utils.edt_prob, torch.from_numpy(lab).to(DEV), anisotropy=c["aniso"])
    assert got_t.is_cuda and not torch.isnan(got_t).any() and not np.isnan(got_np).any()
    _same(sel(got_np), want, lab, id + " numpy in")
    _same(sel(got_t), want, lab, id + " tensor in")
    raw = _raw_edt(lab, c["aniso"])
    assert not torch.isnan(raw).any()
    _same(sel(raw), want, lab, id + " raw")
    assert (got_np[lab == 0] == 0).all()


@pytest.mark.parametrize("id", T.ids(T.SD2D))
def test_star_dist2d_equals_float32_restatement(id):
    from stardist_amd.geometry.geom2d import star_dist
    from stardist_amd.lib import _native as N
    c = T.BY_ID[id]
    lab, want = T.labels(id), T.sd_want(id)
    R, (gy, gx) = c["n_rays"], c["grid"]
    sub = lab[::gy, ::gx]
    u16 = torch.from_numpy(T._as_u16(lab).view(np.int16).copy()).to(DEV).view(torch.uint16)
    dst = torch.full(want.shape, float("nan"), dtype=torch.float32, device=DEV)
    N.dcall(u16, "sd_star_dist2d_device", _p(u16), lab.shape[0], lab.shape[1], R, gy, gx, _p(dst))
    _same(dst, want, sub, id + " raw")
    if c["public"]:
        _same(star_dist(lab, R, grid=c["grid"], mode="hip"), want, sub, id + " numpy in")
        with nan_empty():
            got = star_dist(torch.from_numpy(lab).to(DEV), R, grid=c["grid"], mode="hip")
        assert got.is_cuda
        _same(got, want, sub, id + " tensor in")


@pytest.mark.parametrize("id", T.ids(T.SD3D))
def test_star_dist3d_equals_float32_restatement(id):
    from stardist_amd.geometry.geom3d import star_dist3D
    from stardist_amd.lib import _native as N
    c = T.BY_ID[id]
    lab, want, rays = T.labels(id), T.sd_want(id), c["rays"]()
    gz, gy, gx = c["grid"]
    sub = lab[::gz, ::gy, ::gx]
    u16 = torch.from_numpy(T._as_u16(lab).view(np.int16).copy()).to(DEV).view(torch.uint16)
    rz, ry, rx = (torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(DEV) for v in np.asarray(rays.vertices).T)
    dst = torch.full(want.shape, float("nan"), dtype=torch.float32, device=DEV)
    N.dcall(u16, "sd_star_dist3d_device", _p(u16), *lab.shape, _p(rz), _p(ry), _p(rx), len(rays), gz, gy, gx, _p(dst))
    _same(dst, want, sub, id + " raw")
    _same(star_dist3D(lab, rays, grid=c["grid"], mode="hip"), want, sub, id + " numpy in")
    with nan_empty():
        got = star_dist3D(torch.from_numpy(lab).to(DEV), rays, grid=c["grid"], mode="hip")
    _same(got, want, sub, id + " tensor in")


def _drive(c):
    from stardist_amd.training import targets_device
    from stardist_amd.training3d import targets_device3d
    Y = T.labels(c["id"])
    with nan_empty():
        if "n_rays" in c:
            return _quiet(targets_device, Y, c["n_rays"], c["grid"], DEV)
        return _quiet(targets_device3d, Y, c["rays"](), c["grid"], c["aniso"], DEV)


@pytest.mark.parametrize("id", T.ids(T.BATCH2D + T.BATCH3D))
def test_batch_targets_equal_generator_reference(id):
    """targets_device / targets_device3d twice with another batch of the same list in between, then stardist_targets (the host route)"""
    from stardist_amd.targets import stardist_targets
    c = T.BY_ID[id]
    L = T.BATCH2D if "n_rays" in c else T.BATCH3D
    other = L[(L.index(c) + 1) % len(L)]
    wp, wd = T.batch_want(id)
    for turn in range(2):
        prob, dtm = _drive(c)
        _same(dtm, wd, None, "%s dist_true_mask, run %d" % (id, turn))
        _same(prob, wp, None, "%s prob_true, run %d" % (id, turn))
        po, do = _drive(other)
        assert not torch.isnan(po).any() and not torch.isnan(do).any()
    Y = T.labels(id)
    with nan_empty():
        if "n_rays" in c:
            p, d = _quiet(stardist_targets, Y, n_rays=c["n_rays"], grid=c["grid"])
        else:
            p, d = _quiet(stardist_targets, Y, rays=c["rays"](), grid=c["grid"], anisotropy=c["aniso"])
    _same(d, wd, None, id + " stardist_targets dist_and_mask")
    _same(p[..., 0], wp, None, id + " stardist_targets prob")


def test_stardist_targets_border_crop():
    """b=: the generators' border crop (model2d.py:71, 77-78): prob from the cropped, sub-sampled labels; dist computed on the whole image
    without the grid, then cropped and sub-sampled.  3D: the transform of the whole volume, cropped and sub-sampled (model3d.py:86)"""
    from stardist_amd.targets import stardist_targets
    Y = T.labels("b2-negon-g24")
    b, grid = (slice(3, -5), slice(2, -2)), (2, 4)
    ss = tuple(slice(0, None, g) for g in grid)
    with nan_empty():
        p, d = stardist_targets(Y, n_rays=8, grid=grid, b=b)
    neg = np.stack([y[b][ss] < 0 for y in Y])
    assert neg.any()
    Y0 = [np.maximum(y, 0) for y in Y]
    wp = np.stack([T.edt_prob_box(y[b][ss]) for y in Y0])
    wd = np.stack([T.star_dist2d_np(y, 8)[b][ss] for y in Y0])
    _same(d[..., :-1], wd, None, "2D dist")
    _same(d[..., -1], wp, None, "2D mask")
    _same(p[..., 0], np.where(neg, np.float32(-1), wp), None, "2D prob")
    c = T.BY_ID["b3-negoff-g122"]
    Y, rays, b = T.labels(c["id"]), c["rays"](), (slice(1, -1), slice(2, -3), slice(4, None))
    ss = tuple(slice(0, None, g) for g in c["grid"])
    with nan_empty():
        p, d = _quiet(stardist_targets, Y, rays=rays, grid=c["grid"], anisotropy=c["aniso"], b=b)
    assert not any((y[b][ss] < 0).any() for y in Y)
    wp = np.stack([_quiet(T.edt_prob_box, y, c["aniso"])[b][ss] for y in Y])
    wd = np.stack([T.star_dist3d_np(y, rays.vertices)[b][ss] for y in Y])
    _same(d[..., :-1], wd, None, "3D dist")
    _same(d[..., -1], wp, None, "3D mask")
    _same(p[..., 0], wp, None, "3D prob")


def test_train_data_batches_on_a_seeded_draw():
    """TrainData2D / TrainData3D.batch_device: the targets of the patches that the same seed draws"""
    from stardist_amd.training import TrainData2D
    from stardist_amd.training3d import TrainData3D
    Ys = [T.ellipses((150, 170), 12, s, rfrac=0.2) for s in (71, 72, 73)]
    Ys[1][40:90:3, 30:120:5] = -1
    Xs = [np.zeros(y.shape, np.float32) for y in Ys]
    for turn in range(2):
        a, b = (TrainData2D(Xs, Ys, 3, 16, 8, patch_size=(96, 112), grid=(2, 2)) for _ in range(2))
        np.random.seed(5 + turn)
        _, Y = a.sample(1)
        np.random.seed(5 + turn)
        with nan_empty():
            x, prob, dtm = b.batch_device(1, DEV)
        wp, wd = T.targets_ref(Y, (2, 2), n_rays=16)
        _same(prob, wp, None, "2D prob_true")
        _same(dtm, wd, None, "2D dist_true_mask")
    rays = T.golden_spiral(12)
    Ys = [T.ellipses((20, 40, 44), 8, s, rfrac=0.25, rmin=2.0) for s in (81, 82)]
    Xs = [np.zeros(y.shape, np.float32) for y in Ys]
    for turn in range(2):
        a, b = (TrainData3D(Xs, Ys, 2, rays, 8, patch_size=(12, 24, 32), grid=(1, 2, 2), anisotropy=(1.9, 1.1, 0.7)) for _ in range(2))
        np.random.seed(9 + turn)
        _, Y = a.sample(0)
        np.random.seed(9 + turn)
        with nan_empty():
            x, prob, dtm = b.batch_device(0, DEV)
        wp, wd = T.targets_ref(Y, (1, 2, 2), rays=rays, anisotropy=(1.9, 1.1, 0.7))
        _same(prob, wp, None, "3D prob_true")
        _same(dtm, wd, None, "3D dist_true_mask")
