"""GPU: stardist_amd.utils.label_components on device input (csrc/label_cc.hip) against the host route, on the cases of
tests/_label_cc_cases.py in every input dtype and connectivity, through the C entry point, tensor in -> tensor out and numpy in with
device= -> numpy out: the labels exactly, the count, the input untouched, the same bits from call to call; a call on a side stream
between dependent work; a 4096^2 mask at the percolation threshold against scipy.ndimage.label; and the chain label_components ->
fill_label_holes -> measure_labels on device tensors against the host chain.  Nothing here needs a tolerance."""
import ctypes

import numpy as np
import pytest

import _label_cc_cases as C

pytestmark = pytest.mark.gpu

DTYPE_CODE = {"bool": 0, "uint8": 0, "uint16": 1, "int32": 3}
NOT_EMPTY = [n for n in C.NAMES if n not in C.EMPTY]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def label(*a, **kw):
    from stardist_amd.utils import label_components
    return label_components(*a, **kw)


def zyx(shape):
    return ((1,) + tuple(shape)) if len(shape) == 2 else tuple(shape)


def upload(torch, a):
    a = np.array(a, order="C")                                              # a writable copy: the cases are read-only
    return torch.as_tensor(a.view(np.uint8) if a.dtype == np.bool_ else a, device="cuda")


def entry(torch, t, connectivity, background):
    """(labels, count) tensors of one call of sd_label_components_device on the contiguous device tensor t"""
    from stardist_amd.lib import _native as N
    out = torch.full(t.shape, -5, dtype=torch.int32, device=t.device)
    n = torch.full((1,), -5, dtype=torch.int32, device=t.device)
    N.dcall(t, "sd_label_components_device", N.tptr(t), DTYPE_CODE[str(t.dtype)[6:]], *zyx(t.shape), connectivity, background, N.tptr(out), N.tptr(n))
    return out, n


@pytest.mark.parametrize("name", NOT_EMPTY)
def test_entry_point(torch, name):
    img, background = C.case(name)
    for dt in C.dtypes(name):
        t = upload(torch, img.astype(dt))
        keep = t.clone()
        for c in C.connectivities(name):
            want, n = C.host(name, c)
            got, m = entry(torch, t, c, background)
            again, m2 = entry(torch, t, c, background)
            assert torch.equal(got, again) and torch.equal(m, m2), (name, dt, c)                  # the same bits from call to call
            assert int(m) == n == int(got.max()) and np.array_equal(got.cpu().numpy(), want), (name, dt, c)
        assert torch.equal(t, keep), (name, dt)                             # the input is not written
    if img.ndim == 2:                                                       # Z = 1 with the 3D offsets: the rule for connectivity 2
        got, m = entry(torch, upload(torch, img), 3, background)
        assert int(m) == C.host(name, 2)[1] and np.array_equal(got.cpu().numpy(), C.host(name, 2)[0])


@pytest.mark.parametrize("name", C.NAMES)
def test_tensor_in_tensor_out(torch, name):
    img, background = C.case(name)
    for dt in C.dtypes(name):
        t = torch.as_tensor(np.ascontiguousarray(img.astype(dt)), device="cuda")                 # a bool mask stays a bool tensor
        keep = t.clone()
        for c in C.connectivities(name):
            want, n = C.host(name, c)
            got = label(t, c, background)
            assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == torch.int32 and got.shape == t.shape
            assert np.array_equal(got.cpu().numpy(), want), (name, dt, c)
            again, m = label(t, c, background, return_num=True)
            assert type(m) is int and m == n and torch.equal(again, got), (name, dt, c)
        assert torch.equal(t, keep)
    default = label(torch.as_tensor(img.copy(), device="cuda"), background=background)
    assert np.array_equal(default.cpu().numpy(), C.host(name, img.ndim)[0])                      # connectivity None: ndim


@pytest.mark.parametrize("name", C.NAMES)
def test_numpy_in_with_device_numpy_out(torch, name):
    img, background = C.case(name)
    for dt in C.dtypes(name):
        a = img.astype(dt)
        for c in C.connectivities(name):
            want, n = C.host(name, c)
            got, m = label(a, c, background, return_num=True, device="cuda")
            assert isinstance(got, np.ndarray) and got.dtype == np.int32 and m == n and np.array_equal(got, want), (name, dt, c)
        assert np.array_equal(a, img.astype(dt))


def test_other_dtypes_and_views_go_the_right_way(torch):
    img, _ = C.case("blocks_u8")
    want = C.host("blocks_u8", 2)[0]
    for dt in (torch.int64, torch.float32, torch.int16):                    # through the host code, a device tensor out
        got = label(torch.as_tensor(img.astype(np.int16), device="cuda").to(dt))
        assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    wide = torch.as_tensor(np.ascontiguousarray(np.repeat(img, 2, axis=1)), device="cuda")
    assert np.array_equal(label(wide[:, ::2]).cpu().numpy(), want)          # a strided view is made contiguous
    moved = label(torch.from_numpy(img.copy()), device="cuda")              # a host tensor with device=
    assert moved.is_cuda and np.array_equal(moved.cpu().numpy(), want)


def test_entry_point_argument_checks(torch):
    from stardist_amd.lib import _native as N
    t = torch.ones((4, 4), dtype=torch.uint8, device="cuda")
    out = torch.zeros((4, 4), dtype=torch.int32, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    fn = N.lib().sd_label_components_device
    assert fn(N.tptr(t), 0, 1, 4, 4, 1, 0, N.tptr(out), N.tptr(n), None) == 0
    torch.cuda.synchronize()
    assert int(n) == 1 and bool((out == 1).all())
    for args in ((None, 0, 1, 4, 4, 1, 0, N.tptr(out), N.tptr(n)), (N.tptr(t), 0, 1, 4, 4, 1, 0, None, N.tptr(n)),
                 (N.tptr(t), 0, 1, 4, 4, 1, 0, N.tptr(out), None), (N.tptr(t), 2, 1, 4, 4, 1, 0, N.tptr(out), N.tptr(n)),
                 (N.tptr(t), 0, 0, 4, 4, 1, 0, N.tptr(out), N.tptr(n)), (N.tptr(t), 0, 1, 4, -4, 1, 0, N.tptr(out), N.tptr(n)),
                 (N.tptr(t), 0, 1, 4, 4, 0, 0, N.tptr(out), N.tptr(n)), (N.tptr(t), 0, 1, 4, 4, 4, 0, N.tptr(out), N.tptr(n)),
                 (N.tptr(t), 0, 2, 2 ** 15, 2 ** 15, 1, 0, N.tptr(out), N.tptr(n))):
        assert fn(*args, None) == -1 and N.lib().sd_last_error().startswith(b"sd_label_components"), args
    with pytest.raises(ValueError, match="2\\^31"):                         # refused before anything is allocated
        label(torch.zeros(1, dtype=torch.uint8, device="cuda").expand(2, 2 ** 15, 2 ** 15))


def test_side_stream_between_dependent_work(torch):
    """the mask is made on a side stream right before the call and the labels are consumed right after it, with no synchronisation in
    between: the call's launches are ordered on the stream it was made on"""
    rng = np.random.RandomState(4)
    noise = torch.as_tensor(rng.random_sample((1024, 1536)).astype(np.float32), device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        mask = (noise * 2.0) < 1.18                                         # density 0.59
        lab = label(mask, 1)
        sizes = torch.bincount(lab.reshape(-1))
        top = lab.max()
    side.synchronize()
    want, n = label(mask.cpu().numpy(), 1, return_num=True)
    assert int(top) == n and np.array_equal(lab.cpu().numpy(), want) and np.array_equal(sizes.cpu().numpy(), np.bincount(want.reshape(-1)))


def test_4096_square_at_the_percolation_threshold_equals_scipy(torch):
    from scipy import ndimage
    mask = np.random.RandomState(59).random_sample((4096, 4096)) < 0.59
    want, n = ndimage.label(mask)
    got, m = label(torch.as_tensor(mask, device="cuda"), 1, return_num=True)
    assert m == n and np.array_equal(got.cpu().numpy(), want)
    # just below the threshold (0.5927) nothing spans the image yet, but the largest component covers hundreds of tiles
    assert np.bincount(want.reshape(-1))[1:].max() > 2 ** 18 and n > 100000


def test_chain_with_fill_label_holes_and_measure_labels(torch):
    from stardist_amd.utils import fill_label_holes, measure_labels
    img, _ = C.case("blocks_u8")
    mask = (img != 0) & ~C.random_mask(img.shape, 0.03, 21)                 # objects with pin holes
    host_lab = fill_label_holes(label(mask, 1))
    host_table = measure_labels(host_lab, img)
    assert (host_lab != label(mask, 1)).sum() > 20                          # holes were filled
    t = torch.as_tensor(mask, device="cuda")
    lab = fill_label_holes(label(t, 1))
    table = measure_labels(lab, torch.as_tensor(img.copy(), device="cuda"), as_tensors=True)
    assert lab.is_cuda and lab.dtype == torch.int32 and np.array_equal(lab.cpu().numpy(), host_lab)
    assert list(table) == list(host_table)
    for k, v in table.items():
        assert v.is_cuda and np.array_equal(v.cpu().numpy(), host_table[k]), k
