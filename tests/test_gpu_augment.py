"""GPU: the augmentation kernel (csrc/augment.hip) against the host route of stardist_amd.augment on every case of
tests/_augment_cases.py -- each operation alone and the full chain on six small shapes and one batch of the training size, both modes
of Warp, coordinates exactly on the edges, several periods away, elastic fields, images with inf / NaN, labels with negative and huge
ids, sigma = 0 -- then the training data: batch_device through the device route against the host route, and whole train() runs with
identical histories.  Every comparison is ==, NaN matching NaN by position."""
import ctypes

import numpy as np
import pytest

import _augment_cases as C
from stardist_amd import augment as A

pytestmark = pytest.mark.gpu

CHAIN = [A.FlipRot90, lambda: A.Warp(elastic_grid=4, elastic_amount=1.5), A.IntensityScaleShift, A.AdditiveNoise]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def upload(torch, a):
    return torch.as_tensor(np.array(a, order="C"), device="cuda")           # a writable copy: the cases are read-only


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_apply_device_equals_apply_host(torch, name):
    x, y, params = C.case(name)
    wx, wy = C.reference(name)
    dx, dy = upload(torch, x), upload(torch, y)
    gx, gy = A.Compose.apply_device(dx, dy, params)
    gx2, gy2 = A.Compose.apply_device(dx, dy, params)
    assert gx.dtype == torch.float32 and gy.dtype == torch.int32 and gx.shape == dx.shape and gy.shape == dy.shape
    assert gx.data_ptr() != dx.data_ptr() and gy.data_ptr() != dy.data_ptr()
    hx, hy = gx.cpu().numpy(), gy.cpu().numpy()
    for b in range(len(params)):
        assert C.same(hx[b], wx[b]), (name, b)
        assert C.same(hy[b], wy[b]), (name, b)
    # the same bits from call to call, the inputs untouched
    assert hx.tobytes() == gx2.cpu().numpy().tobytes() and torch.equal(gy, gy2)
    assert dx.cpu().numpy().tobytes() == x.tobytes() and dy.cpu().numpy().tobytes() == y.tobytes()


def test_entry_point_with_the_tables_of_the_host_harness(torch):
    """sd_augment_batch_device itself, on the table and the displacement field the CPU test gives the host build of the header"""
    from stardist_amd.lib import _native as N
    for name in ("33x33-chain-constant-hard", "3x8x8-chain-reflect"):
        x, y, params = C.case(name)
        flags, tab, disp = C.packed(name)
        dx, dy, dd = upload(torch, x), upload(torch, y), upload(torch, disp)
        d_tab = upload(torch, tab.view(np.uint8))
        ox, oy = torch.full_like(dx, -7), torch.full_like(dy, -7)
        shape = (ctypes.c_int * 3)(*x.shape[1:])
        N.dcall(dx, "sd_augment_batch_device", N.tptr(dx), N.tptr(dy), x.shape[0], x.ndim - 1, ctypes.cast(shape, ctypes.c_void_p), flags,
                ctypes.c_void_p(tab.ctypes.data), N.tptr(d_tab), N.tptr(dd), disp.shape[1], N.tptr(ox), N.tptr(oy))
        wx, wy = C.reference(name)
        assert C.same(ox.cpu().numpy(), wx) and C.same(oy.cpu().numpy(), wy)


def test_entry_point_refuses_bad_arguments(torch):
    from stardist_amd.lib import _native as N
    x, y, params = C.case("5x7-flip")
    flags, tab, _ = C.packed("5x7-flip")
    dx, dy = upload(torch, x), upload(torch, y)
    d_tab = upload(torch, tab.view(np.uint8))
    ox, oy = torch.full_like(dx, -7), torch.full_like(dy, -7)

    def run(tab=tab, B=3, nd=2, shape=(5, 7, 0), flags=flags, out=ox, n_disp=0):
        h_shape = (ctypes.c_int * 3)(*shape)
        N.dcall(dx, "sd_augment_batch_device", N.tptr(dx), N.tptr(dy), B, nd, ctypes.cast(h_shape, ctypes.c_void_p), flags,
                ctypes.c_void_p(tab.ctypes.data), N.tptr(d_tab), None, n_disp, N.tptr(out), N.tptr(oy))

    for field, value in (("base", 35), ("base", -1), ("step", 8), ("comp", 0)):
        bad = tab.copy()
        bad[field][1] = value
        with pytest.raises(N.NativeError):
            run(tab=bad)
    for kw in (dict(B=0), dict(nd=4), dict(flags=16), dict(out=dx), dict(shape=(5, 0, 0)), dict(n_disp=2)):
        with pytest.raises(N.NativeError):
            run(**kw)
    torch.cuda.synchronize()
    assert bool((ox == -7).all()) and bool((oy == -7).all())                # nothing was launched
    run()
    assert C.same(ox.cpu().numpy(), C.reference("5x7-flip")[0])


def test_apply_device_refuses_what_it_cannot_take(torch):
    x, y, params = C.case("5x7-flip")
    dx, dy = upload(torch, x), upload(torch, y)
    with pytest.raises(ValueError):
        A.Compose.apply_device(dx, dy, params[:2])
    with pytest.raises(ValueError):
        A.Compose.apply_device(dx, dy.long(), params)
    with pytest.raises(ValueError):
        A.Compose.apply_device(dx.cpu(), dy.cpu(), params)
    with pytest.raises(ValueError):
        A.Compose.apply_device(dx, dy, [params[0], params[1], {"noise": {"sigma": 0, "key": (0, 0)}}])


# ---- training data -------------------------------------------------------------------------------------------------------------------------
def _blobs(shape, seed, dtype=np.int32):
    """a label image of boxes with ids 1 ..., and a noisy image of it"""
    rng = np.random.RandomState(seed)
    y = np.zeros(shape, dtype)
    for k in range(1, 9):
        lo = [rng.randint(0, n - 2) for n in shape]
        y[tuple(slice(a, a + rng.randint(2, max(3, n // 3))) for a, n in zip(lo, shape))] = k
    return (y > 0).astype(np.float32) + rng.uniform(0, 0.5, shape).astype(np.float32), y


def _data(nd, aug, Y_of=None, classes=False, n=3, exact=False):
    """exact: images of the patch size, so that a patch is the whole image"""
    from stardist_amd.training import TrainData2D
    from stardist_amd.training3d import TrainData3D
    shape = ((32, 32) if exact else (44, 40)) if nd == 2 else ((8, 16, 16) if exact else (12, 24, 20))
    X, Y = zip(*[_blobs(shape, s) for s in range(n)])
    if Y_of is not None:
        Y = [Y_of(y, k) for k, y in enumerate(Y)]
    kw = dict(n_classes=2, classes=[{k: 1 + k % 2 for k in range(1, 12)}, 1, None][:n]) if classes else {}
    if nd == 2:
        return TrainData2D(X, Y, batch_size=2, n_rays=8, length=8, patch_size=(32, 32), grid=(2, 2), augmenter=aug, **kw)
    from stardist_amd.rays3d import Rays_GoldenSpiral
    return TrainData3D(X, Y, batch_size=2, rays=Rays_GoldenSpiral(8), length=8, patch_size=(8, 16, 16), grid=(1, 2, 2), augmenter=aug, **kw)


def _both_routes(torch, nd, aug, steps=3, **kw):
    """the batches of the device route and of the host route (the same object behind a plain callable), from one seed"""
    dev = torch.device("cuda:0")
    device, host = _data(nd, aug, **kw), _data(nd, lambda x, y: aug(x, y), **kw)
    assert device.augments_on(dev) and not host.augments_on(dev)
    np.random.seed(21)
    got = [device.batch_device(i, dev) for i in range(steps)]
    state = np.random.get_state()
    np.random.seed(21)
    want = [host.batch_device(i, dev) for i in range(steps)]
    assert np.array_equal(state[1], np.random.get_state()[1]) and state[2] == np.random.get_state()[2]
    return got, want


def _assert_same_batches(torch, got, want, n_out):
    for g, w in zip(got, want):
        assert len(g) == len(w) == n_out
        for a, b in zip(g, w):
            assert a.dtype == b.dtype and a.shape == b.shape and a.is_contiguous() == b.is_contiguous()
            assert C.same(a.cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize("classes", [False, True], ids=["single", "classes"])
@pytest.mark.parametrize("nd", [2, 3])
def test_batch_device_full_chain(torch, nd, classes):
    aug = A.Compose([f() for f in CHAIN])
    negative = lambda y, k: np.where(y == 3, -1, y)
    got, want = _both_routes(torch, nd, aug, Y_of=negative, classes=classes)
    _assert_same_batches(torch, got, want, 4 if classes else 3)
    assert any(bool((g[1] == -1).any()) for g in got)
    none = _data(nd, None, Y_of=negative, classes=classes)
    np.random.seed(21)
    assert not torch.equal(none.batch_device(0, torch.device("cuda:0"))[0], got[0][0])


@pytest.mark.parametrize("nd", [2, 3])
def test_batch_device_labels_that_a_flip_moves_onto_the_grid(torch, nd):
    """negative labels at odd positions only: off the grid (2, 2) in the raw patch (no clip, no mask), on it after a flip of an even
    extent; decided from the augmented labels"""
    def odd_negative(y, k):
        y = y.copy()
        y[..., 1::2, 1::2] = np.where(y[..., 1::2, 1::2] > 0, -1, y[..., 1::2, 1::2])
        return y
    got, want = _both_routes(torch, nd, A.Compose([A.FlipRot90()]), steps=6, Y_of=odd_negative, classes=True, exact=True)
    _assert_same_batches(torch, got, want, 4)
    with_mask = [bool((g[1] == -1).any()) for g in got]
    assert any(with_mask) and not all(with_mask)


@pytest.mark.parametrize("nd", [2, 3])
def test_batch_device_constant_patch_turned_mixed_by_a_warp(torch, nd):
    """a patch of one positive id (the special case of edt_prob) into which a constant-mode warp brings zeros"""
    aug = A.Compose([A.Warp(scale=(0.5, 0.7), mode="constant")])
    got, want = _both_routes(torch, nd, aug, Y_of=lambda y, k: np.full_like(y, 5))
    _assert_same_batches(torch, got, want, 3)
    for g in got:
        prob = g[1].cpu().numpy()
        assert (prob == 0).any() and (prob > 0).any()
    # without the warp every patch is the constant one: no background anywhere
    plain = _data(nd, None, Y_of=lambda y, k: np.full_like(y, 5))
    np.random.seed(21)
    assert bool((plain.batch_device(0, torch.device("cuda:0"))[1] > 0).all())


def test_batch_device_wide_label_types(torch):
    """int64 labels go through the int32 range check on the host: the values of the host route, or its error"""
    aug = A.Compose([A.FlipRot90()])
    got, want = _both_routes(torch, 2, aug, steps=1, Y_of=lambda y, k: y.astype(np.int64))
    _assert_same_batches(torch, got, want, 3)
    huge = _data(2, aug, Y_of=lambda y, k: np.where(y > 0, y.astype(np.int64) + 2 ** 31, 0))
    np.random.seed(1)
    with pytest.raises(ValueError):
        for i in range(4):
            huge.batch_device(i, torch.device("cuda:0"))


# ---- whole training runs -------------------------------------------------------------------------------------------------------------------
def _train(nd, aug):
    import torch
    from stardist_amd.models import Config2D, Config3D, StarDist2D, StarDist3D
    dev = torch.device("cuda:0")
    if nd == 2:
        X, Y = zip(*[_blobs((48, 48), s, np.uint16) for s in range(3)])
        cfg = Config2D(n_rays=8, grid=(2, 2), unet_n_depth=1, train_patch_size=(32, 32), train_batch_size=2)
        model = StarDist2D(cfg, basedir=None, device=dev, seed=0)
    else:
        X, Y = zip(*[_blobs((12, 24, 24), s, np.uint16) for s in range(3)])
        cfg = Config3D(backbone="unet", n_rays=8, grid=(1, 2, 2), unet_n_depth=1, train_patch_size=(8, 16, 16), train_batch_size=2)
        model = StarDist3D(cfg, basedir=None, device=dev, seed=0)
    hist = model.train(list(X), list(Y), validation_data=(list(X[:1]), list(Y[:1])), augmenter=aug, seed=5, epochs=2, steps_per_epoch=2)
    return dict(hist), [p.detach().cpu().numpy().copy() for p in model.net.parameters()]


@pytest.mark.parametrize("nd", [2, 3])
def test_train_history_is_the_same_on_both_routes(nd):
    aug = A.Compose([f() for f in CHAIN])
    h_dev, w_dev = _train(nd, aug)
    h_host, w_host = _train(nd, lambda x, y: aug(x, y))
    assert set(h_dev) == set(h_host) and len(h_dev["loss"]) == 2
    for k in h_dev:
        assert h_dev[k] == h_host[k], k
    assert all(np.isfinite(v) for v in h_dev["loss"] + h_dev["val_loss"])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(w_dev, w_host))
    h_none, _ = _train(nd, None)
    assert h_none["loss"] != h_dev["loss"]
