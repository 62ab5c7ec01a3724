"""GPU: the device routes of stardist_amd.spots (csrc/spots.hip) against the host route, which tests/test_cpu_spots.py holds against
scipy, a brute-force statement of the definition and scikit-image: gaussian_filter and difference_of_gaussians bit for bit (NaN
positions equal, every other bit equal), peak_local_max with its table, detect_spots and measure_labels(spots=) with ==, "the input is
not written", "the same bits in a second call", images past 2^31 pixels, and the entry points' argument checks."""
import ctypes

import numpy as np
import pytest

import _spots_cases as C

pytestmark = pytest.mark.gpu

GAUSS = C.gauss_cases()
PEAKS = C.peak_cases()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def U():
    from stardist_amd import utils
    return utils


def same_floats(got, want):
    """bit for bit, but for the payload and sign of a NaN"""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(np.where(nan, 0, got.view(np.uint32)), np.where(nan, 0, want.view(np.uint32)))


def device_gauss(torch, img, sigma, **kw):
    """gaussian_filter on the device, twice: the input is not written, the second call gives the first one's bits"""
    t = torch.as_tensor(img, device="cuda")
    keep = t.clone()
    a = U().gaussian_filter(t, sigma, **kw)
    b = U().gaussian_filter(t, sigma, **kw)
    assert a.is_cuda and a.dtype == torch.float32 and torch.equal(t.view(torch.uint8), keep.view(torch.uint8))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    return a.cpu().numpy()


@pytest.mark.parametrize("case", GAUSS, ids=[c[0] for c in GAUSS])
def test_gaussian_equals_host_route(torch, case):
    _, img, sigma, truncate = case
    want = U().gaussian_filter(img, sigma, truncate=truncate)
    assert same_floats(device_gauss(torch, img, sigma, truncate=truncate), want)
    got = U().gaussian_filter(img, sigma, truncate=truncate, device="cuda")  # numpy in, numpy out
    assert isinstance(got, np.ndarray) and same_floats(got, want)


@pytest.mark.parametrize("sigma", (20.0, 20.2, (20.2, 1.0), 127.9), ids=str)
def test_gaussian_at_and_past_the_lds_tier(torch, sigma):
    from stardist_amd import spots
    radius = int(4.0 * np.max(sigma) + 0.5)
    assert radius == {20.0: spots.GAUSSIAN_LDS_RADIUS, 20.2: spots.GAUSSIAN_LDS_RADIUS + 1, 127.9: spots.GAUSSIAN_MAX_RADIUS}.get(sigma, 81)
    for shape in ((67, 131), (5, 70, 33)):
        img = C.noise(shape, np.float32, 3)
        s = sigma if np.isscalar(sigma) or len(shape) == 2 else sigma + (0.7,)
        assert same_floats(device_gauss(torch, img, s), U().gaussian_filter(img, s))


def test_gaussian_beyond_the_radius_cap_takes_the_host_code(torch):
    img = C.noise((6, 40), np.float32, 4)
    got = U().gaussian_filter(torch.as_tensor(img, device="cuda"), 128.2)
    assert got.is_cuda and same_floats(got.cpu().numpy(), U().gaussian_filter(img, 128.2))


@pytest.mark.parametrize("dtype", (np.uint8, np.uint16))
def test_gaussian_integer_images_at_their_maxima(torch, dtype):
    img = np.full((33, 70), np.iinfo(dtype).max, dtype)
    img[::5, ::7] = 0
    assert same_floats(device_gauss(torch, img, (1.0, 2.5)), U().gaussian_filter(img, (1.0, 2.5)))


@pytest.mark.parametrize("name", ("inf_nan", "denormals", "huge"))
def test_gaussian_special_floats(torch, name):
    img = C.special_float_images()[name]
    want = U().gaussian_filter(img, (1.0, 2.5))
    assert same_floats(device_gauss(torch, img, (1.0, 2.5)), want)
    assert name != "inf_nan" or (np.isnan(want).sum() > 20 and np.isinf(want).sum() > 20)
    low, high = U().gaussian_filter(img, 1.0), U().gaussian_filter(img, 1.6)
    dog = U().difference_of_gaussians(torch.as_tensor(img, device="cuda"), 1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        assert dog.is_cuda and same_floats(dog.cpu().numpy(), low - high)


def test_gaussian_many_workgroups_and_difference(torch):
    img = C.noise((1024, 1024), np.float32, 8)
    assert same_floats(device_gauss(torch, img, 2.0), U().gaussian_filter(img, 2.0))
    want = U().difference_of_gaussians(img, 2.0)
    assert np.array_equal(want, U().gaussian_filter(img, 2.0) - U().gaussian_filter(img, 3.2))
    assert same_floats(U().difference_of_gaussians(torch.as_tensor(img, device="cuda"), 2.0).cpu().numpy(), want)
    assert same_floats(U().difference_of_gaussians(img, 2.0, (3.0, 4.0), device="cuda"), U().difference_of_gaussians(img, 2.0, (3.0, 4.0)))


BIG = (32800, 65600)          # 2 151 680 000 pixels: element offsets pass 2^31


def test_gaussian_offsets_past_2_to_31(torch):
    import scipy.ndimage as ndi
    g = torch.Generator(device="cuda").manual_seed(5)
    t = torch.randint(0, 256, BIG, dtype=torch.uint8, device="cuda", generator=g)
    out = U().gaussian_filter(t, (1.5, 1.5))
    r, rows = 6, 48
    head, tail = t[:rows + r].cpu().numpy(), t[-(rows + r):].cpu().numpy()
    got_head, got_tail = out[:rows].cpu().numpy(), out[-rows:].cpu().numpy()
    del out, t
    torch.cuda.empty_cache()
    # a slab with r rows of context: rows farther than r from the cut have the image's own neighbours, the axis-1 pass is row by row
    assert same_floats(got_head, ndi.gaussian_filter(head, (1.5, 1.5), output=np.float32)[:rows])
    assert same_floats(got_tail, ndi.gaussian_filter(tail, (1.5, 1.5), output=np.float32)[r:])


# ----------------------------------------------------------------------------- peaks

def same_table(got, want):
    return list(got) == list(want) == ["coords", "values", "labels"] and all(
        isinstance(got[n], np.ndarray) and got[n].dtype == want[n].dtype and got[n].shape == want[n].shape and got[n].tobytes() == want[n].tobytes()
        for n in want)


def device_peaks(torch, img, **kw):
    """peak_local_max's table on the device, twice: inputs not written, the same bits again"""
    kw = dict(kw)
    t = torch.as_tensor(img, device="cuda")
    keep = t.clone()
    lab = keep_lab = None
    if kw.get("labels") is not None:
        lab = kw["labels"] = torch.as_tensor(kw["labels"], device="cuda")
        keep_lab = lab.clone()
    a = U().peak_local_max(t, return_table=True, as_tensors=True, **kw)
    b = U().peak_local_max(t, return_table=True, as_tensors=True, **kw)
    assert torch.equal(t.view(torch.uint8), keep.view(torch.uint8)) and (lab is None or torch.equal(lab, keep_lab))
    assert all(v.is_cuda and torch.equal(v.view(torch.uint8), b[n].view(torch.uint8)) for n, v in a.items())
    return {n: v.cpu().numpy() for n, v in a.items()}


@pytest.mark.parametrize("name", sorted(PEAKS))
def test_peaks_equal_host_route(torch, name):
    img, kw = PEAKS[name]
    want = U().peak_local_max(img, return_table=True, **kw)
    assert same_table(device_peaks(torch, img, **kw), want)
    got = U().peak_local_max(img, device="cuda", **kw)                      # numpy in, coordinates out
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want["coords"])


def test_peak_cases_are_what_they_say():
    from stardist_amd import spots
    run = lambda name: U().peak_local_max(PEAKS[name][0], device="cuda", **PEAKS[name][1]).tolist()
    assert run("constant") == [] and run("constant_low_threshold") == [[0, 0]]
    assert run("ramp") == [] and run("ramp_no_border") == [[17, 66]] and run("all_nan") == [] and run("border_half") == []
    assert run("value_equals_threshold") == [[5, 5]] and run("signed_zeros") == [[4, 10], [7, 63]]
    assert run("labels_touching") == [[10, 31], [10, 30]] and run("num_peaks_0") == []
    for d in (1, 2, 5):
        for where in ("inside", "x_edge", "y_edge", "corner", "anti", "z_edge", "zy"):
            assert len(run("pair_d%d_gap%d_%s" % (d, d, where))) == 1 and len(run("pair_d%d_gap%d_%s" % (d, d + 1, where))) == 2
    assert spots.peak_window_in_lds(2, (36, 36)) and not spots.peak_window_in_lds(2, (37, 37))
    assert len(run("lds_tier_last")) > 0 and len(run("lds_tier_beyond")) > 0


def test_peaks_of_a_large_tie_free_image_in_order(torch):
    img = C.tie_free((1024, 1024), 30, smooth=0)
    want = U().peak_local_max(img, return_table=True)
    assert 90000 < len(want["coords"]) and (np.diff(want["values"]) < 0).all()
    assert same_table(device_peaks(torch, img), want)
    cut = U().peak_local_max(torch.as_tensor(img, device="cuda"), num_peaks=5000)
    assert np.array_equal(cut, want["coords"][:5000])
    many = device_peaks(torch, img, min_distance=0, threshold_abs=1.0, exclude_border=False)       # more peaks than the first guess holds
    assert len(many["coords"]) == img.size - 1 and same_table(many, U().peak_local_max(img, 0, 1.0, exclude_border=False, return_table=True))


def test_peaks_of_heavily_tied_noise(torch):
    img = C.noise((1024, 1024), np.uint8, 31)
    assert same_table(device_peaks(torch, img), U().peak_local_max(img, return_table=True))
    lab = (np.arange(1024)[:, None] // 100 * 11 + np.arange(1024)[None, :] // 100).astype(np.int32)
    kw = dict(min_distance=2, labels=lab, num_peaks_per_label=40)
    assert same_table(device_peaks(torch, img, **kw), U().peak_local_max(img, return_table=True, **kw))


def test_peaks_past_2_to_31_pixels(torch):
    t = torch.zeros(BIG, dtype=torch.uint8, device="cuda")
    planted = [(0, 3, 9), (1, 65599, 7), (2, 100, 200), (20000, 30000, 5), (32797, 65597, 8), (32799, 65599, 6), (32799, 0, 4), (32798, 65598, 8)]
    for y, x, v in planted:
        t[y, x] = v
    got = U().peak_local_max(t, 1, threshold_abs=0, exclude_border=False, return_table=True)
    # (32797, 65597) and (32798, 65598) tie within each other's window: the lower index stays; (32799, 65599) loses to its neighbour
    assert got["coords"].tolist() == [[2, 100], [0, 3], [32797, 65597], [1, 65599], [20000, 30000], [32799, 0]]
    assert got["values"].tolist() == [200, 9, 8, 7, 5, 4] and got["values"].dtype == np.uint8 and not got["labels"].any()
    assert U().peak_local_max(t, 1, threshold_abs=0).tolist() == [[2, 100], [32797, 65597], [20000, 30000]]     # the default border of 1


# ----------------------------------------------------------------------------- the composition, and measure_labels(spots=)

@pytest.mark.parametrize("shape,dtype", (((256, 256), np.uint16), ((16, 64, 64), np.float32)))
def test_detect_spots_and_spot_counts(torch, shape, dtype):
    img, lab = C.scene(shape, dtype, seed=len(shape), spots=60 if len(shape) == 2 else 200)
    kw = dict(min_distance=2, threshold_rel=0.2)
    want = U().detect_spots(img, 1.5, return_table=True, **kw)
    assert len(want["coords"]) > 20
    assert np.array_equal(want["coords"], U().peak_local_max(U().difference_of_gaussians(img, 1.5, 1.5 * 1.6), **kw))
    t = torch.as_tensor(img, device="cuda")
    got = U().detect_spots(t, 1.5, return_table=True, as_tensors=True, **kw)
    assert all(v.is_cuda for v in got.values()) and same_table({n: v.cpu().numpy() for n, v in got.items()}, want)
    assert np.array_equal(U().detect_spots(img, 1.5, device="cuda", **kw), want["coords"])
    with_labels = U().detect_spots(t, 1.5, labels=torch.as_tensor(lab, device="cuda"), num_peaks_per_label=2, return_table=True, **kw)
    assert same_table(with_labels, U().detect_spots(img, 1.5, labels=lab, num_peaks_per_label=2, return_table=True, **kw))
    # spots per object
    table = U().measure_labels(lab, spots=want["coords"])
    assert table["spot_count"].sum() > 5 and table["spot_count"].sum() == (lab[tuple(want["coords"].T)] > 0).sum()
    dev = U().measure_labels(torch.as_tensor(lab, device="cuda"), spots=got["coords"])
    assert list(dev) == list(table) and all(dev[k].dtype == table[k].dtype and np.array_equal(dev[k], table[k]) for k in table)
    dev = U().measure_labels(lab, spots=want["coords"], device="cuda", as_tensors=True)
    assert dev["spot_count"].is_cuda and dev["spot_count"].dtype == torch.int64 and np.array_equal(dev["spot_count"].cpu().numpy(), table["spot_count"])
    outside = want["coords"].copy()
    outside[0, -1] = shape[-1]
    with pytest.raises(ValueError, match="outside"):
        U().measure_labels(torch.as_tensor(lab, device="cuda"), spots=outside)


# ----------------------------------------------------------------------------- the entry points refuse bad arguments before any launch

def test_entry_points_check_their_arguments(torch):
    from stardist_amd.lib import _native as N
    lib = N.lib()
    t = torch.zeros((4, 5), dtype=torch.float32, device="cuda")
    out, work = torch.full_like(t, 7.0), torch.full_like(t, 7.0)
    w = torch.ones(3, dtype=torch.float64, device="cuda")
    keys = torch.full((64,), 7, dtype=torch.int64, device="cuda")
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    radius, far = np.asarray([-1, 1, -1], np.int32), np.asarray([-1, 513, -1], np.int32)
    dist, border, count = np.asarray([0, 1, 1], np.int32), np.zeros(3, np.int64), np.zeros(2, np.int64)
    s = N.current_stream()
    good = (p(t), 2, 2, 1, 4, 5)
    assert lib.sd_gaussian_filter_device(*good, N.ptr(radius), p(w), p(out), p(work), s) == 0
    for image in ((None, 2, 2, 1, 4, 5), (p(t), 3, 2, 1, 4, 5), (p(t), -1, 2, 1, 4, 5), (p(t), 2, 1, 1, 4, 5), (p(t), 2, 4, 1, 4, 5),
                  (p(t), 2, 2, 1, 0, 5), (p(t), 2, 2, 2, 4, 5), (p(t), 2, 3, 1, 4, -5), (p(t), 2, 2, 1, 2 ** 20, 2 ** 12)):
        out.fill_(7.0)
        assert lib.sd_gaussian_filter_device(*image, N.ptr(radius), p(w), p(out), p(work), s) == -1
        assert lib.sd_peak_local_max_device(*image, None, N.ptr(dist), N.ptr(border), 0, 0.0, 0, 0.0, -1, -1, 64, p(keys), N.ptr(count), s) == -1
        assert lib.sd_peaks_emit_device(*image, None, p(keys), 1, p(keys), p(out), p(keys), s) == -1
        assert "sd_" in lib.sd_last_error().decode()
    assert lib.sd_gaussian_filter_device(*good, N.ptr(far), p(w), p(out), p(work), s) == -1
    assert lib.sd_gaussian_filter_device(*good, None, p(w), p(out), p(work), s) == -1
    assert lib.sd_gaussian_filter_device(*good, N.ptr(radius), None, p(out), p(work), s) == -1
    assert lib.sd_gaussian_filter_device(*good, N.ptr(radius), p(w), None, p(work), s) == -1
    assert lib.sd_gaussian_filter_device(*good, N.ptr(np.asarray([-1, 1, 1], np.int32)), p(w), p(out), None, s) == -1
    peaks = lambda d=dist, b=border, a=0.0, k=keys, c=count, cap=64: lib.sd_peak_local_max_device(
        *good, None, None if d is None else N.ptr(d), None if b is None else N.ptr(b), 1, a, 0, 0.0, -1, -1, cap, None if k is None else p(k),
        None if c is None else N.ptr(c), s)
    assert peaks() == 0 and count.tolist() == [0, 0]
    assert peaks(d=None) == -1 and peaks(b=None) == -1 and peaks(k=None) == -1 and peaks(c=None) == -1 and peaks(cap=-1) == -1
    assert peaks(d=np.asarray([0, -1, 1], np.int32)) == -1 and peaks(d=np.asarray([0, 1, 2 ** 20 + 1], np.int32)) == -1
    assert peaks(b=np.asarray([0, -1, 0], np.int64)) == -1 and peaks(a=float("nan")) == -1
    assert lib.sd_peaks_emit_device(*good, None, None, 1, p(keys), p(out), p(keys), s) == -1
    assert lib.sd_peaks_emit_device(*good, None, p(keys), -1, p(keys), p(out), p(keys), s) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (keys == 7).all()                         # nothing ran
