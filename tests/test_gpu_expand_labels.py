"""GPU: the nearest-feature transform (csrc/edt_feature.hip) against the references of tests/_expand_cases.py -- the brute-force
statement of the definition for the small cases, scipy's distance_transform_edt for the large ones.  Both C entry points on every
non-empty case, distance and spacing, outputs poisoned beforehand, the input untouched, the same bits from call to call, with and
without each optional output; stardist_amd.utils.expand_labels tensor in -> tensor out and numpy in with device= -> numpy out in
every dtype; a call on a side stream between dependent work; a 1500 x 2100 image and a 40 x 200 x 300 volume against scikit-image's
composition on scipy; the chain label_components -> expand_labels -> measure_labels against the host chain; distance_transform on the
device against scipy, bounded and unbounded.  Nothing here needs a tolerance."""
import numpy as np
import pytest

import _expand_cases as C

pytestmark = pytest.mark.gpu

DTYPE_CODE = {"uint8": 0, "uint16": 1, "int32": 3}


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def expand(*a, **kw):
    from stardist_amd.utils import expand_labels
    return expand_labels(*a, **kw)


def transform(*a, **kw):
    from stardist_amd.utils import distance_transform
    return distance_transform(*a, **kw)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def zyx(shape):
    return ((1,) + tuple(shape)) if len(shape) == 2 else tuple(shape)


def szyx(spacing):
    return ((1.0,) + tuple(spacing)) if len(spacing) == 2 else tuple(spacing)


def upload(torch, a):
    return torch.as_tensor(np.array(a, order="C"), device="cuda")           # a writable copy: the cases are read-only


def narrow(torch, name):
    """the case as a device tensor of a dtype sd_nearest_feature_device takes (uint16 travels as the int16 of the same bits)"""
    a = C.case(name) if C.case(name).dtype.name in DTYPE_CODE else C.as_int32(C.case(name))
    return upload(torch, a.view(np.int16) if a.dtype == np.uint16 else a), DTYPE_CODE[a.dtype.name]


def nearest_entry(torch, t, code, spacing, max_distance=-1.0, feature_is_zero=0, want_index=True, want_dist=True):
    from stardist_amd.lib import _native as N
    index = torch.full(t.shape, -7, dtype=torch.int32, device=t.device)
    dist = torch.full(t.shape, -7.0, dtype=torch.float64, device=t.device)
    N.dcall(t, "sd_nearest_feature_device", N.tptr(t), code, *zyx(t.shape), feature_is_zero, *szyx(spacing), float(max_distance),
            N.tptr(index) if want_index else None, N.tptr(dist) if want_dist else None)
    return index, dist


def expand_entry(torch, t, spacing, distance):
    from stardist_amd.lib import _native as N
    out = torch.full(t.shape, -7, dtype=torch.int32, device=t.device)
    N.dcall(t, "sd_expand_labels_device", N.tptr(t), *zyx(t.shape), *szyx(spacing), float(distance), N.tptr(out))
    return out


@pytest.mark.parametrize("name", C.NAMES)
def test_expand_entry_point(torch, name):
    a = C.as_int32(C.case(name))
    t = upload(torch, a)
    keep = t.clone()
    for spacing in C.spacings(name):
        index, dist = C.reference(name, spacing)
        for distance in C.distances(name):
            got = expand_entry(torch, t, spacing, distance)
            assert torch.equal(got, expand_entry(torch, t, spacing, distance)), (name, spacing, distance)      # the same bits again
            assert same_bits(got.cpu().numpy(), C.expanded(a, index, dist, distance)), (name, spacing, distance)
    assert torch.equal(t, keep)                                             # the input is not written


@pytest.mark.parametrize("name", C.NAMES)
def test_nearest_feature_entry_point(torch, name):
    t, code = narrow(torch, name)
    keep = t.clone()
    for spacing in C.spacings(name):
        index, dist = C.reference(name, spacing)
        got_index, got_dist = nearest_entry(torch, t, code, spacing)
        again_index, again_dist = nearest_entry(torch, t, code, spacing, np.inf)               # inf: no bound either
        assert torch.equal(got_index, again_index) and torch.equal(got_dist, again_dist), (name, spacing)
        assert same_bits(got_index.cpu().numpy(), index) and same_bits(got_dist.cpu().numpy(), dist), (name, spacing)
        for distance in C.distances(name):
            b_index, b_dist = nearest_entry(torch, t, code, spacing, distance)
            w_index, w_dist = C.bounded(index, dist, distance)
            assert same_bits(b_index.cpu().numpy(), w_index) and same_bits(b_dist.cpu().numpy(), w_dist), (name, spacing, distance)
    spacing = C.spacings(name)[2]
    index, dist = C.reference(name, spacing)
    only_index, untouched = nearest_entry(torch, t, code, spacing, want_dist=False)
    assert same_bits(only_index.cpu().numpy(), index) and bool((untouched == -7.0).all())
    untouched, only_dist = nearest_entry(torch, t, code, spacing, want_index=False)
    assert same_bits(only_dist.cpu().numpy(), dist) and bool((untouched == -7).all())
    z_index, z_dist = nearest_entry(torch, t, code, spacing, feature_is_zero=1)                # the background as the features
    want = C.brute(C.case(name), spacing, True) if name in C.SMALL else C.scipy_reference(C.case(name), spacing, True)
    assert same_bits(z_index.cpu().numpy(), want[0]) and same_bits(z_dist.cpu().numpy(), want[1])
    assert torch.equal(t, keep)


def test_entry_point_argument_checks(torch):
    from stardist_amd.lib import _native as N
    t = torch.ones((4, 4), dtype=torch.int32, device="cuda")
    out = torch.zeros((4, 4), dtype=torch.int32, device="cuda")
    dist = torch.zeros((4, 4), dtype=torch.float64, device="cuda")
    near, grow = N.lib().sd_nearest_feature_device, N.lib().sd_expand_labels_device
    one = (1.0, 1.0, 1.0)
    assert near(N.tptr(t), 3, 1, 4, 4, 0, *one, -1.0, N.tptr(out), N.tptr(dist), None) == 0
    assert grow(N.tptr(t), 1, 4, 4, *one, 0.0, N.tptr(out), None) == 0
    torch.cuda.synchronize()
    assert bool((out == 1).all()) and bool((dist == 0).all())
    for args in ((None, 3, 1, 4, 4, 0, *one, -1.0), (N.tptr(t), 2, 1, 4, 4, 0, *one, -1.0), (N.tptr(t), 3, 0, 4, 4, 0, *one, -1.0),
                 (N.tptr(t), 3, 1, 4, -4, 0, *one, -1.0), (N.tptr(t), 3, 1, 4, 4, 2, *one, -1.0), (N.tptr(t), 3, 1, 4, 4, 0, 1.0, 0.0, 1.0, -1.0),
                 (N.tptr(t), 3, 1, 4, 4, 0, 1.0, 1.0, np.nan, -1.0), (N.tptr(t), 3, 1, 4, 4, 0, np.inf, 1.0, 1.0, -1.0),
                 (N.tptr(t), 3, 1, 4, 4, 0, *one, np.nan), (N.tptr(t), 3, 2, 2 ** 15, 2 ** 15, 0, *one, -1.0)):
        assert near(*args, N.tptr(out), N.tptr(dist), None) == -1 and N.lib().sd_last_error().startswith(b"sd_nearest_feature"), args
    for args in ((None, 1, 4, 4, *one, 1.0, N.tptr(out)), (N.tptr(t), 1, 4, 4, *one, 1.0, None), (N.tptr(t), 1, 4, 4, *one, 1.0, N.tptr(t)),
                 (N.tptr(t), 1, 4, 4, *one, -1.0, N.tptr(out)), (N.tptr(t), 1, 4, 4, *one, np.nan, N.tptr(out)),
                 (N.tptr(t), 1, 0, 4, *one, 1.0, N.tptr(out)), (N.tptr(t), 1, 4, 4, 1.0, -1.0, 1.0, 1.0, N.tptr(out)),
                 (N.tptr(t), 2, 2 ** 15, 2 ** 15, *one, 1.0, N.tptr(out))):
        assert grow(*args, None) == -1 and N.lib().sd_last_error().startswith(b"sd_expand_labels"), args
    with pytest.raises(ValueError, match="2\\^31"):                         # refused before anything is allocated
        expand(torch.zeros(1, dtype=torch.uint8, device="cuda").expand(2, 2 ** 15, 2 ** 15), 2)
    with pytest.raises(ValueError, match="2\\^31"):
        transform(torch.zeros(1, dtype=torch.uint8, device="cuda").expand(2, 2 ** 15, 2 ** 15))


@pytest.mark.parametrize("name", C.NAMES)
def test_python_routes(torch, name):
    a = C.case(name)
    cut = lambda x, dt: x.astype(dt) if np.dtype(dt).itemsize >= a.dtype.itemsize else (x % 251).astype(dt)      # narrower: other labels
    for dt in ("uint8", "uint16", "int32", "int64"):
        b = cut(a, dt)
        for spacing, distance in zip(C.spacings(name), (3.0, C.SQRT2, 6.5)):
            want = expand(b, distance, spacing)                             # the host route (== the reference: the CPU tests)
            got = expand(b, distance, spacing, device="cuda")
            assert isinstance(got, np.ndarray) and same_bits(got, want), (name, dt, spacing)
            if dt != "uint16":                                              # torch has no arithmetic on uint16: a tensor of it is no label image
                t = upload(torch, b)
                keep = t.clone()
                got = expand(t, distance, spacing)
                assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == t.dtype and got.shape == t.shape
                assert same_bits(got.cpu().numpy(), want) and torch.equal(t, keep), (name, dt, spacing)
    t = upload(torch, C.as_int32(a))
    assert torch.equal(expand(t), expand(t, 1, 1)) and torch.equal(expand(t, 0), t) and expand(t, 0) is not t


def test_python_routes_empty_negative_and_views(torch):
    for shape in C.EMPTY_SHAPES:
        for dt in (torch.uint8, torch.int32, torch.int64):
            e = expand(torch.zeros(shape, dtype=dt, device="cuda"), 2)
            assert e.is_cuda and e.dtype == dt and tuple(e.shape) == shape
        assert expand(np.zeros(shape, np.uint16), 2, device="cuda").shape == shape
        d, i = transform(torch.zeros(shape, dtype=torch.uint8, device="cuda"), return_indices=True)
        assert d.is_cuda and d.dtype == torch.float64 and tuple(d.shape) == shape and i.dtype == torch.int32 and tuple(i.shape) == (len(shape),) + shape
    a = C.case("discs")
    want = expand(a, 3, (1.3, 0.7))
    wide = upload(torch, np.repeat(a, 2, axis=1))
    assert same_bits(expand(wide[:, ::2], 3, (1.3, 0.7)).cpu().numpy(), want)                  # a strided view is made contiguous
    moved = expand(torch.from_numpy(a.copy()), 3, (1.3, 0.7), device="cuda")                   # a host tensor with device=
    assert moved.is_cuda and same_bits(moved.cpu().numpy(), want)
    neg = np.where(a == 2, -2, a).astype(np.int32)                          # a negative label: the host code, a device tensor out
    got = expand(upload(torch, neg), 3)
    assert got.is_cuda and got.dtype == torch.int32 and same_bits(got.cpu().numpy(), expand(neg, 3)) and bool((got == -2).any())
    f = expand(upload(torch, a.astype(np.float32)), 3)                      # no integer tensor: the host code
    assert f.is_cuda and f.dtype == torch.float32 and np.array_equal(f.cpu().numpy(), expand(a, 3))


def test_side_stream_between_dependent_work(torch):
    """the label image is made on a side stream right before the call and the result is consumed right after it, with no
    synchronisation in between: the call's launches are ordered on the stream it was made on"""
    a = C.discs((700, 900), 500, 4, 9, 31)
    half = upload(torch, a // 2 + (a % 2) * 1000)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        lbl = half * 2 - (half >= 1000).to(torch.int32) * 1999              # == a, computed right before the call
        grown = expand(lbl, 5)
        sizes = torch.bincount(grown.reshape(-1))
    side.synchronize()
    want = expand(a, 5)
    assert np.array_equal(lbl.cpu().numpy(), a) and same_bits(grown.cpu().numpy(), want)
    assert np.array_equal(sizes.cpu().numpy(), np.bincount(want.reshape(-1)))


def test_nuclei_image_1500_by_2100_equals_scipy_composition(torch):
    a = C.discs((1500, 2100), 6000, 4, 10, 32)
    want = expand(a, 5)
    got = expand(upload(torch, a), 5)
    assert same_bits(got.cpu().numpy(), want) and (want != 0).sum() > 1.3 * (a != 0).sum() and len(np.unique(a)) > 4000


def test_volume_40_by_200_by_300_equals_scipy_composition(torch):
    a = C.discs((40, 200, 300), 1500, 3, 7, 33)
    want = expand(a, 3, (2, 1, 1))
    got = expand(upload(torch, a), 3, (2, 1, 1))
    assert same_bits(got.cpu().numpy(), want) and (want != 0).sum() > 1.3 * (a != 0).sum() and len(np.unique(a)) > 1000


def test_chain_with_label_components_and_measure_labels(torch):
    from stardist_amd.utils import label_components, measure_labels
    a = C.case("discs_big")
    mask = a != 0
    img = (np.random.RandomState(34).random_sample(a.shape) * 255).astype(np.uint8)
    host_lab = expand(label_components(mask, 1), 4)
    host_table = measure_labels(host_lab, img)
    assert (host_lab != 0).sum() > 1.2 * mask.sum()
    lab = expand(label_components(torch.as_tensor(mask, device="cuda"), 1), 4)
    table = measure_labels(lab, upload(torch, img), as_tensors=True)
    assert lab.is_cuda and lab.dtype == torch.int32 and same_bits(lab.cpu().numpy(), host_lab)
    assert list(table) == list(host_table)
    for k, v in table.items():
        assert v.is_cuda and np.array_equal(v.cpu().numpy(), host_table[k]), k


@pytest.mark.parametrize("name", ("discs", "lattice", "balls", "lattice3d", "no_feature", "all_labelled", "one_column", "discs_u16", "discs_big",
                                  "balls_big"))
def test_distance_transform_on_the_device_equals_scipy(torch, name):
    a = C.case(name)
    for img in (a, a == 0):                                                 # distances inside the objects; distances to the objects
        for spacing in C.spacings(name):
            want, want_idx = transform(img, spacing, return_indices=True)    # the host route: scipy (the CPU tests)
            dist, idx = transform(img, spacing, return_indices=True, device="cuda")
            assert isinstance(dist, np.ndarray) and same_bits(dist, want) and same_bits(idx, want_idx), (name, spacing)
            if img.dtype != np.uint16:
                t = upload(torch, img)
                dist, idx = transform(t, spacing, return_indices=True)
                assert dist.device == t.device and idx.device == t.device and dist.dtype == torch.float64 and idx.dtype == torch.int32
                assert same_bits(dist.cpu().numpy(), want) and same_bits(idx.cpu().numpy(), want_idx), (name, spacing)
                assert same_bits(transform(t, spacing).cpu().numpy(), want)
                assert same_bits(transform(t, spacing, return_distances=False, return_indices=True).cpu().numpy(), want_idx)
            for bound in (0.0, C.SQRT2, 3.0, 1e9):
                want_b, want_idx_b = transform(img, spacing, max_distance=bound, return_indices=True)
                dist, idx = transform(img, spacing, max_distance=bound, return_indices=True, device="cuda")
                assert same_bits(dist, want_b) and same_bits(idx, want_idx_b), (name, spacing, bound)
