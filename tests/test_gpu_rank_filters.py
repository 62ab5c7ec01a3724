"""GPU: the device routes of stardist_amd.rank_filters (csrc/rank_filter.hip) against the host route, which
tests/test_cpu_rank_filters.py holds against scipy.ndimage and a brute-force statement of the definition: every case with == and equal
NaN positions, "the input is not written", "the same bits in a second call", numpy in and numpy out, the caps, the LDS tiers of both
kernels, the compositions, an image past 2^31 elements, and the entry points' argument checks."""
import ctypes

import numpy as np
import pytest

import _rank_filter_cases as C

pytestmark = pytest.mark.gpu

CASES = C.cases()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def U():
    from stardist_amd import utils
    return utils


def device_call(torch, fn, img, **kw):
    """the public function on a device tensor, twice: the input is not written, the second call gives the first one's bits"""
    raw = lambda x: x.contiguous().view(torch.uint8)
    t = torch.as_tensor(img, device="cuda")
    keep = t.clone()
    a = getattr(U(), fn)(t, **kw)
    b = getattr(U(), fn)(t, **kw)
    assert a.is_cuda and a.dtype == t.dtype and a.shape == t.shape and a.is_contiguous()
    assert torch.equal(raw(t), raw(keep)) and torch.equal(raw(a), raw(b))
    return a.cpu().numpy()


@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_host_route(torch, name):
    fn, img, kw = CASES[name]
    want = getattr(U(), fn)(img, **kw)
    assert C.same(device_call(torch, fn, img, **kw), want)
    assert C.same(getattr(U(), fn)(img, device="cuda", **kw), want)          # numpy in, numpy out


def test_many_workgroups(torch):
    for dtype in (np.uint16, np.float32):
        img = C.noise((512, 515), dtype, 50)
        for fn, kw in (("median_filter", dict(size=5)), ("minimum_filter", dict(size=(15, 14), mode="mirror")),
                       ("white_tophat", dict(size=15)), ("percentile_filter", dict(percentile=80, footprint=C.disc(3), mode="nearest"))):
            assert C.same(device_call(torch, fn, img, **kw), getattr(U(), fn)(img, **kw))
    vol = C.noise((33, 70, 130), np.uint8, 51)
    assert C.same(device_call(torch, "median_filter", vol, size=3), U().median_filter(vol, 3))
    assert C.same(device_call(torch, "black_tophat", vol, size=(3, 4, 5)), U().black_tophat(vol, (3, 4, 5)))


# ----------------------------------------------------------------------------- caps and tiers

def host_code_only(monkeypatch):
    from stardist_amd import rank_filters
    monkeypatch.setattr(rank_filters, "_device_plan", lambda *a, **k: pytest.fail("device path taken"))


@pytest.mark.parametrize("size", ((1, 1025), (1025, 1), (1, 1026), (1026, 3), (1, 2000)), ids=str)
def test_window_length_cap(torch, monkeypatch, size):
    from stardist_amd import rank_filters as RF
    assert RF.MAX_WINDOW == 1025
    if max(size) > RF.MAX_WINDOW:
        host_code_only(monkeypatch)                                         # beyond the cap: the host code, a device tensor back
    for dtype in (np.uint16, np.float32):
        img = C.noise((6, 40), dtype, 60)
        for fn in ("minimum_filter", "grey_closing"):
            assert C.same(device_call(torch, fn, img, size=size), getattr(U(), fn)(img, size=size))
    sparse = np.zeros(size, bool)                                           # a footprint as long: the footprint kernel's cap is the same
    sparse[0, 0] = sparse[-1, -1] = sparse[size[0] // 2, size[1] // 3] = True
    img = C.noise((6, 40), np.uint8, 61)
    assert C.same(device_call(torch, "median_filter", img, footprint=sparse, mode="mirror"), U().median_filter(img, footprint=sparse, mode="mirror"))


@pytest.mark.parametrize("count", (4096, 4097, 4160), ids=str)
def test_footprint_element_cap(torch, monkeypatch, count):
    from stardist_amd import rank_filters as RF
    assert RF.MAX_FOOTPRINT == 4096
    if count > RF.MAX_FOOTPRINT:
        host_code_only(monkeypatch)
    fp = np.ones((65, 64), bool)
    fp[0, :] = False
    fp[0, :count - 4096] = True
    assert fp.sum() == count
    img = C.noise((20, 70), np.uint16, 62)
    assert C.same(device_call(torch, "median_filter", img, footprint=fp), U().median_filter(img, footprint=fp))
    box = {4096: (64, 64), 4097: (17, 241), 4160: (64, 65)}[count]          # a box under a rank: the same cap on its elements
    assert box[0] * box[1] == count
    assert C.same(device_call(torch, "rank_filter", img, rank=-3, size=box), U().rank_filter(img, -3, size=box))
    monkeypatch.undo()                                                      # a box's extremes have no element cap: the kernels again
    assert C.same(device_call(torch, "maximum_filter", img, size=box), U().maximum_filter(img, size=box))


@pytest.mark.parametrize("dtype,top", ((np.uint8, 737), (np.uint16, 353), (np.float32, 161)), ids=str)
def test_box_pass_at_and_past_the_lds_tier(torch, dtype, top):
    from stardist_amd import rank_filters as RF
    assert RF.box_window_in_lds(dtype, top, False) and not RF.box_window_in_lds(dtype, top + 1, False)
    img, vol = C.noise((67, 131), dtype, 63), C.noise((5, 70, 33), dtype, 64)
    for size in (top, top + 1):
        for mode in ("reflect", "constant"):
            kw = dict(mode=mode, cval=C.a_cval(dtype))
            assert C.same(device_call(torch, "minimum_filter", img, size=(size, 3), **kw), U().minimum_filter(img, (size, 3), **kw))
            assert C.same(device_call(torch, "maximum_filter", vol, size=(2, size, 1), **kw), U().maximum_filter(vol, (2, size, 1), **kw))
    nan = C.nan_images()["nan2d"]
    assert C.same(device_call(torch, "white_tophat", nan, size=(162, 2)), U().white_tophat(nan, (162, 2)))


@pytest.mark.parametrize("dtype,nd,at,past", ((np.float32, 2, (81, 65), (82, 65)), (np.uint16, 3, (13, 13, 33), (13, 14, 33)),
                                              (np.uint8, 2, (177, 193), (178, 193))), ids=str)
def test_footprint_kernel_at_and_past_the_lds_tier(torch, dtype, nd, at, past):
    from stardist_amd import rank_filters as RF
    assert RF.footprint_window_in_lds(nd, dtype, at) and not RF.footprint_window_in_lds(nd, dtype, past)
    img = C.noise((67, 131) if nd == 2 else (5, 70, 33), dtype, 65)
    for extent in (at, past):
        fp = np.random.RandomState(66).rand(*extent) > 0.995
        fp[(0,) * nd] = fp[(-1,) * nd] = True
        for fn, kw in (("median_filter", dict(mode="mirror")), ("minimum_filter", dict(mode="constant", cval=C.a_cval(dtype))),
                       ("rank_filter", dict(rank=3))):
            assert C.same(device_call(torch, fn, img, footprint=fp, **kw), getattr(U(), fn)(img, footprint=fp, **kw))
    if dtype == np.float32:
        nan = C.nan_images()["nan2d"]
        assert C.same(device_call(torch, "median_filter", nan, footprint=fp), U().median_filter(nan, footprint=fp))


# ----------------------------------------------------------------------------- compositions

@pytest.mark.parametrize("dtype", (np.uint8, np.uint16, np.float32, np.bool_), ids=str)
def test_fused_tophat_equals_the_separate_steps(torch, dtype):
    img = C.noise((130, 200), dtype, 70)
    t = torch.as_tensor(img, device="cuda")
    for kw in (dict(size=15), dict(size=(4, 7), mode="constant", cval=C.a_cval(dtype)), dict(footprint=C.disc(3))):
        opening, closing = U().grey_opening(t, **kw).cpu().numpy(), U().grey_closing(t, **kw).cpu().numpy()
        white, black = U().white_tophat(t, **kw).cpu().numpy(), U().black_tophat(t, **kw).cpu().numpy()
        if dtype == np.bool_:
            assert C.same(white, img ^ opening) and C.same(black, closing ^ img)
        else:
            assert C.same(white, img - opening) and C.same(black, closing - img)
        assert C.same(white, U().white_tophat(img, **kw)) and C.same(black, U().black_tophat(img, **kw))


def test_tophat_then_detect_spots_stays_on_the_device(torch):
    import _spots_cases as S
    img, _ = S.scene((256, 256), np.uint16, seed=2, spots=60)
    img = (img + np.linspace(0, 400, 256)[None, :]).astype(np.uint16)       # an uneven background
    kw = dict(min_distance=2, threshold_rel=0.2, return_table=True)
    want = U().detect_spots(U().white_tophat(img, size=15), 1.5, **kw)
    assert len(want["coords"]) > 20
    t = torch.as_tensor(img, device="cuda")
    flat = U().white_tophat(U().median_filter(t, 3), size=15)
    assert flat.is_cuda and flat.dtype == torch.uint16
    got = U().detect_spots(U().white_tophat(t, size=15), 1.5, **kw)
    assert list(got) == list(want) and all(got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]) for k in want)
    chain = U().detect_spots(flat, 1.5, **kw)
    host = U().detect_spots(U().white_tophat(U().median_filter(img, 3), size=15), 1.5, **kw)
    assert all(np.array_equal(chain[k], host[k]) for k in host)


# ----------------------------------------------------------------------------- past 2^31 elements

BIG = (32800, 65600)          # 2 151 680 000 pixels: element offsets pass 2^31


def test_offsets_past_2_to_31(torch):
    import scipy.ndimage as ndi
    g = torch.Generator(device="cuda").manual_seed(5)
    t = torch.randint(0, 256, BIG, dtype=torch.uint8, device="cuda", generator=g)
    middle = 2 ** 31 // BIG[1]                                              # the row that holds element 2^31
    rows = 24
    bands = ((0, rows), (middle - rows // 2, middle + rows // 2), (BIG[0] - rows, BIG[0]))
    for fn, ref in (("minimum_filter", ndi.minimum_filter), ("median_filter", ndi.median_filter)):
        out = getattr(U(), fn)(t, size=3)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == BIG
        for lo, hi in bands:
            a, b = max(lo - 1, 0), min(hi + 1, BIG[0])                      # the band with its halo of one row; an image edge keeps its own rule
            want = ref(t[a:b].cpu().numpy(), size=3)[lo - a:(lo - a) + (hi - lo)]
            assert np.array_equal(out[lo:hi].cpu().numpy(), want), (fn, lo)
        del out
        torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- the entry points refuse bad arguments before any launch

def test_entry_points_check_their_arguments(torch):
    from stardist_amd.lib import _native as N
    lib = N.lib()
    t = torch.zeros((4, 5), dtype=torch.float32, device="cuda")
    ref, out, work = torch.zeros_like(t), torch.full_like(t, 7.0), torch.full_like(t, 7.0)
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    ints = lambda *v: N.ptr(np.asarray(v, np.int32))
    s = N.current_stream()
    good = (p(t), 2, 2, 1, 4, 5)

    def box(image=good, size=(1, 3, 3), origin=(0, 0, 0), mode=0, cval=0.0, fuse=0, r=None, o=out, w=work):
        return lib.sd_minmax_box_device(*image, None if size is None else ints(*size), None if origin is None else ints(*origin), 0, mode, cval,
                                        fuse, p(r), p(o), p(w), s)

    def rank(image=good, extent=(1, 3, 3), origin=(0, 0, 0), offsets=((0, 0, 0), (0, 1, 1), (0, 2, 2)), count=3, k=1, mode=0, cval=0.0, o=out):
        return lib.sd_rank_filter_device(*image, None if extent is None else ints(*extent), None if origin is None else ints(*origin),
                                         None if offsets is None else N.ptr(np.asarray(offsets, np.int32)), count, k, mode, cval, p(o), s)

    assert box() == 0 and rank() == 0
    torch.cuda.synchronize()
    assert (out == 0).all()
    out.fill_(7.0)
    work.fill_(7.0)
    for image in ((None, 2, 2, 1, 4, 5), (p(t), 3, 2, 1, 4, 5), (p(t), -1, 2, 1, 4, 5), (p(t), 2, 1, 1, 4, 5), (p(t), 2, 4, 1, 4, 5),
                  (p(t), 2, 2, 1, 0, 5), (p(t), 2, 2, 2, 4, 5), (p(t), 2, 3, 1, 4, -5), (p(t), 2, 2, 1, 2 ** 20, 2 ** 12)):
        assert box(image=image) == -1 and rank(image=image) == -1 and "sd_" in lib.sd_last_error().decode()
    for kw in (dict(size=None), dict(origin=None), dict(o=None), dict(size=(1, 0, 3)), dict(size=(1, 3, 1026)), dict(size=(2, 3, 3)),
               dict(origin=(0, 2, 0)), dict(origin=(0, 0, -2)), dict(mode=4), dict(mode=-1), dict(cval=float("nan")), dict(cval=0.1),
               dict(fuse=4), dict(fuse=-1), dict(fuse=3, r=ref), dict(fuse=1), dict(w=None), dict(o=t), dict(w=t), dict(o=work),
               dict(fuse=1, r=out)):
        assert box(**kw) == -1, kw
    for kw in (dict(extent=None), dict(origin=None), dict(offsets=None), dict(o=None), dict(o=t), dict(count=0), dict(count=4097), dict(k=3),
               dict(k=-1), dict(offsets=((0, 0, 0), (0, 3, 1), (0, 2, 2))), dict(offsets=((0, 0, 0), (1, 1, 1), (0, 2, 2))),
               dict(offsets=((0, 0, 0), (0, 1, -1), (0, 2, 2))), dict(extent=(1, 3, 1026)), dict(origin=(0, -2, 0)), dict(mode=7),
               dict(cval=float("nan"))):
        assert rank(**kw) == -1, kw
    u8 = torch.zeros((4, 5), dtype=torch.uint8, device="cuda")
    o8, w8 = torch.full_like(u8, 7), torch.full_like(u8, 7)
    for cval in (-1.0, 256.0, 0.5, float("inf")):
        assert lib.sd_minmax_box_device(p(u8), 0, 2, 1, 4, 5, ints(1, 3, 3), ints(0, 0, 0), 0, 3, cval, 0, None, p(o8), p(w8), s) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (work == 7.0).all() and (o8 == 7).all()   # nothing ran
