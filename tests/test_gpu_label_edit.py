"""GPU: stardist_amd.utils.find_boundaries, clear_border, remove_small_objects and select_labels on the device (csrc/label_edit.hip, and
csrc/label_cc.hip, csrc/relabel.hip, csrc/relabel_star.hip behind them) against the host routes: the three entry points on shapes one
more and one less than the tile extents and smaller than a tile, find_boundaries on all 3^9 3 x 3 windows of three values and on a volume
of touching balls, every case of tests/_label_edit_cases.py through the public functions with numpy in (device=) -> numpy out and
tensor in -> tensor out, the same bits from call to call, the inputs untouched, and the entry points' argument checks.  Nothing here
needs a tolerance."""
import ctypes
import warnings

import numpy as np
import pytest

import _label_edit_cases as C

pytestmark = pytest.mark.gpu

MODE_CODE = {"thick": 0, "inner": 1, "outer": 2}


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def U():
    from stardist_amd import utils
    return utils


def zyx(shape):
    return ((1,) + tuple(shape)) if len(shape) == 2 else tuple(shape)


def upload(torch, a):
    return torch.as_tensor(np.array(a, order="C"), device="cuda")           # a writable copy: the cases are read-only


def boundaries_entry(torch, t, connectivity, mode, background, sentinel=2 ** 31 - 1):
    from stardist_amd.lib import _native as N
    out = torch.full(t.shape, 7, dtype=torch.uint8, device=t.device)
    N.dcall(t, "sd_find_boundaries_device", N.tptr(t), *zyx(t.shape), connectivity, MODE_CODE[mode], background, sentinel, N.tptr(out))
    return out


@pytest.mark.parametrize("nd", (2, 3))
def test_find_boundaries_entry_point_around_the_tile_extents(torch, nd):
    for shape in C.tile_shapes(nd):
        for k, kind in enumerate(C.KINDS):
            img = C.tiled(kind, shape)
            t = upload(torch, img)
            keep = t.clone()
            for c in range(1, nd + 1):
                for mode in C.MODES:
                    want = U().find_boundaries(img, c, mode, k % 2)
                    got = boundaries_entry(torch, t, c, mode, k % 2)
                    again = boundaries_entry(torch, t, c, mode, k % 2)
                    assert torch.equal(got, again), (shape, kind, c, mode)                        # the same bits from call to call
                    assert np.array_equal(got.cpu().numpy(), want.astype(np.uint8)), (shape, kind, c, mode)
            assert torch.equal(t, keep)                                     # the input is not written
            if kind == "noise" and min(shape) > 2:
                assert U().find_boundaries(img, 1).mean() > 0.9
            if kind == "constant":
                assert not U().find_boundaries(img, nd).any()
    if nd == 2:                                                             # Z = 1 with connectivity 3: the rule for connectivity 2
        img = C.tiled("stripes", C.tile_shapes(2)[2])
        assert np.array_equal(boundaries_entry(torch, upload(torch, img), 3, "outer", 0).cpu().numpy(), U().find_boundaries(img, 2, "outer").astype(np.uint8))


def test_find_boundaries_more_tiles_than_blocks(torch):
    """a column of 2^25 + 40 pixels is 2^20 + 2 tiles, more than the grid's cap: blocks take a second tile"""
    n = 2 ** 25 + 40
    assert (n - 1) // C.TY + 1 > 2 ** 20
    a = ((np.arange(n) // 5) % 3).astype(np.int32).reshape(n, 1)
    a[-C.TY - 3:] = 7                                                       # the last two tiles differ from the pattern
    t = upload(torch, a)
    for mode, background in (("thick", 0), ("outer", 1)):
        got = boundaries_entry(torch, t, 1, mode, background).cpu().numpy()
        assert np.array_equal(got, U().find_boundaries(a, 1, mode, background).astype(np.uint8)), mode


def test_find_boundaries_all_3x3_windows(torch):
    w = C.windows_image()
    t = upload(torch, w)
    for c in (1, 2):
        for mode in C.MODES:
            for background in (0, 1):
                got = U().find_boundaries(t, c, mode, background)
                assert got.dtype == torch.bool and got.device == t.device
                assert np.array_equal(got.cpu().numpy(), U().find_boundaries(w, c, mode, background)), (c, mode, background)


def test_find_boundaries_touching_balls(torch):
    vol = C.balls()
    assert vol.shape == (9, 35, 67) and (U().find_boundaries(vol, 1, "inner") & U().find_boundaries(vol, 1, "outer") & (vol > 0)).sum() > 100
    for a in (vol, vol[4:5], vol[4]):                                       # the volume, one slice as a stack, that slice as an image
        t = upload(torch, a)
        for c in range(1, a.ndim + 1):
            for mode in C.MODES:
                got = U().find_boundaries(t, c, mode)
                assert np.array_equal(got.cpu().numpy(), U().find_boundaries(a, c, mode)), (a.shape, c, mode)
    assert np.array_equal(U().find_boundaries(upload(torch, vol[4:5]), 3, "outer").cpu().numpy()[0],
                          U().find_boundaries(upload(torch, vol[4]), 2, "outer").cpu().numpy())


@pytest.mark.parametrize("name", sorted(C.FB))
def test_find_boundaries_public_function(torch, name):
    img = C.FB[name]
    for c, mode, background in C.fb_params(img):
        want = U().find_boundaries(img, c, mode, background)
        got = U().find_boundaries(img, c, mode, background, device="cuda")
        assert isinstance(got, np.ndarray) and got.dtype == np.bool_ and np.array_equal(got, want), (name, c, mode, background)
        t = upload(torch, img)
        out = U().find_boundaries(t, c, mode, background)
        assert isinstance(out, torch.Tensor) and out.dtype == torch.bool and out.device == t.device
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(t.cpu().numpy(), img), (name, c, mode, background)
    sub = U().find_boundaries(upload(torch, img), mode="subpixel")          # the host code, a device tensor out
    assert sub.is_cuda and np.array_equal(sub.cpu().numpy(), U().find_boundaries(img, mode="subpixel"))


@pytest.mark.parametrize("name", sorted(C.CB))
def test_clear_border(torch, name):
    img, kw = C.CB[name]
    want = U().clear_border(img, **kw)
    got = U().clear_border(img, device="cuda", **kw)
    assert isinstance(got, np.ndarray) and got.dtype == img.dtype and np.array_equal(got, want), name
    t = upload(torch, img)
    tkw = {k: (upload(torch, v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    out = U().clear_border(t, **tkw)
    again = U().clear_border(t, **tkw)
    assert isinstance(out, torch.Tensor) and out.dtype == t.dtype and out.device == t.device and torch.equal(out, again)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(t.cpu().numpy(), img), name
    if "mask" in kw:                                                        # a mask that lives elsewhere is moved to the labels
        assert np.array_equal(U().clear_border(t, **kw).cpu().numpy(), want)


def test_clear_border_entry_points_on_a_band_of_every_width(torch):
    """the band kernel against numpy for every buffer_size of a small volume and image, keys = pixel indices: every band pixel's flag
    is set and no other"""
    from stardist_amd.lib import _native as N
    for shape in ((5, 6, 7), (9, 70), (1, 5, 6)):
        n = int(np.prod(shape))
        key = torch.arange(1, n + 1, dtype=torch.int32, device="cuda").reshape(shape)
        for b in range(0, max(shape)):
            flags = torch.full((n + 1,), 9, dtype=torch.uint8, device="cuda")
            N.dcall(key, "sd_label_border_flags_device", N.tptr(key), *zyx(shape), len(shape), b, None, n + 1, N.tptr(flags))
            band = np.zeros(shape, bool)
            for d, s in enumerate(shape):
                idx = np.arange(s).reshape([-1 if k == d else 1 for k in range(len(shape))])
                band |= (idx < b + 1) | (idx >= s - b - 1)
            assert np.array_equal(flags.cpu().numpy()[1:].reshape(shape).astype(bool), band) and int(flags[0]) == 0, (shape, b)


@pytest.mark.parametrize("name", sorted(C.RS))
def test_remove_small_objects(torch, name):
    img, kw = C.RS[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = U().remove_small_objects(img, **kw)
    got = U().remove_small_objects(img, device="cuda", **kw)
    assert isinstance(got, np.ndarray) and got.dtype == img.dtype and np.array_equal(got, want), name
    t = upload(torch, img)
    out = U().remove_small_objects(t, **kw)
    again = U().remove_small_objects(t, **kw)
    assert isinstance(out, torch.Tensor) and out.dtype == t.dtype and out.device == t.device and torch.equal(out, again)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(t.cpu().numpy(), img), name


def test_remove_small_objects_refuses_negative_values_of_a_tensor(torch):
    with pytest.raises(ValueError, match="Negative value labels"):
        U().remove_small_objects(torch.tensor([[1, -1], [2, 2]], dtype=torch.int32, device="cuda"), 2)


@pytest.mark.parametrize("name", sorted(C.SL))
def test_select_labels(torch, name):
    lbl, wanted, kw = C.SL[name]
    want = U().select_labels(lbl, wanted, **kw)
    got = U().select_labels(lbl, wanted, device="cuda", **kw)
    assert isinstance(got, np.ndarray) and got.dtype == lbl.dtype and np.array_equal(got, want), name
    t = upload(torch, lbl)
    for ids in (wanted, upload(torch, wanted), wanted.tolist()):            # the ids wherever they live
        out = U().select_labels(t, ids, **kw)
        assert isinstance(out, torch.Tensor) and out.dtype == t.dtype and out.device == t.device
        assert np.array_equal(out.cpu().numpy(), want), name
    assert np.array_equal(t.cpu().numpy(), lbl)


def test_select_labels_filters_by_a_device_table(torch):
    from stardist_amd.utils import measure_labels
    lbl = C.SL["some"][0]
    t = upload(torch, lbl)
    table = measure_labels(t, as_tensors=True)
    ids = table["label"][table["area"] > 50]
    assert ids.is_cuda
    out = U().select_labels(t, ids, relabel=True)
    host_table = measure_labels(lbl)
    assert np.array_equal(out.cpu().numpy(), U().select_labels(lbl, host_table["label"][host_table["area"] > 50], relabel=True))


def test_chain_clear_remove_outline(torch):
    """labels -> clear_border -> remove_small_objects -> find_boundaries on device tensors equals the host chain"""
    lbl = C.CB["blobs"][0]
    host = U().remove_small_objects(U().clear_border(lbl), 20)
    dev = U().remove_small_objects(U().clear_border(upload(torch, lbl)), 20)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), host) and 0 < (host > 0).sum() < (lbl > 0).sum()
    assert np.array_equal(U().find_boundaries(dev, mode="inner").cpu().numpy(), U().find_boundaries(host, mode="inner"))


def test_entry_point_argument_checks(torch):
    from stardist_amd.lib import _native as N
    L = N.lib()
    t = torch.ones((4, 4), dtype=torch.int32, device="cuda")
    o8 = torch.zeros((4, 4), dtype=torch.uint8, device="cuda")
    o32 = torch.zeros((4, 4), dtype=torch.int32, device="cuda")
    flags = torch.zeros(17, dtype=torch.uint8, device="cuda")
    p, P8, P32, F = N.tptr(t), N.tptr(o8), N.tptr(o32), N.tptr(flags)
    fb, bf, cf = L.sd_find_boundaries_device, L.sd_label_border_flags_device, L.sd_label_clear_flagged_device
    assert fb(p, 1, 4, 4, 1, 0, 0, 255, P8, None) == 0 and bf(p, 1, 4, 4, 2, 0, None, 17, F, None) == 0
    assert cf(p, p, F, 17, 16, 5, P32, None) == 0
    torch.cuda.synchronize()
    assert not o8.any() and flags.cpu().tolist() == [0, 1] + [0] * 15 and bool((o32 == 5).all())
    for args in ((None, 1, 4, 4, 1, 0, 0, 255, P8), (p, 1, 4, 4, 1, 0, 0, 255, None), (p, 0, 4, 4, 1, 0, 0, 255, P8), (p, 1, 4, -4, 1, 0, 0, 255, P8),
                 (p, 1, 4, 4, 0, 0, 0, 255, P8), (p, 1, 4, 4, 4, 0, 0, 255, P8), (p, 1, 4, 4, 1, 3, 0, 255, P8), (p, 1, 4, 4, 1, -1, 0, 255, P8),
                 (p, 1, 4, 4, 1, 0, 0, 255, p), (p, 2, 2 ** 15, 2 ** 15, 1, 0, 0, 255, P8)):
        assert fb(*args, None) == -1 and L.sd_last_error().startswith(b"sd_find_boundaries"), args
    for args in ((None, 1, 4, 4, 2, 0, None, 17, F), (p, 1, 4, 4, 2, 0, None, 17, None), (p, 1, 0, 4, 2, 0, None, 17, F), (p, 1, 4, 4, 2, 0, None, 0, F),
                 (p, 1, 4, 4, 4, 0, None, 17, F), (p, 2, 4, 2, 2, 0, None, 17, F), (p, 1, 4, 4, 2, -1, None, 17, F), (p, 1, 4, 4, 2, 0, F, 17, F),
                 (p, 1, 4, 4, 2, 0, None, 17, p), (p, 2, 2 ** 15, 2 ** 15, 3, 0, None, 17, F)):
        assert bf(*args, None) == -1 and L.sd_last_error().startswith(b"sd_label_border_flags"), args
    for args in ((None, p, F, 17, 16, 0, P32), (p, None, F, 17, 16, 0, P32), (p, p, None, 17, 16, 0, P32), (p, p, F, 17, 16, 0, None),
                 (p, p, F, 0, 16, 0, P32), (p, p, F, 17, 0, 0, P32), (p, p, F, 17, 16, 0, p), (p, p, F, 17, 2 ** 31, 0, P32)):
        assert cf(*args, None) == -1 and L.sd_last_error().startswith(b"sd_label_clear_flagged"), args
    torch.cuda.synchronize()
    assert not o8.any() and bool((o32 == 5).all()) and bool((t == 1).all())  # nothing was launched
    for fn, arg in ((U().find_boundaries, ()), (U().clear_border, ()), (U().remove_small_objects, (1,)), (U().select_labels, ([1],))):
        with pytest.raises(ValueError, match="2\\^31"):                     # refused before anything is allocated
            fn(torch.zeros(1, dtype=torch.uint8, device="cuda").expand(2, 2 ** 15, 2 ** 15), *arg)
