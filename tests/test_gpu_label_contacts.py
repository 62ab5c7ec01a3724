"""GPU: sd_label_contacts_device and the device routes of stardist_amd.utils.label_contacts and measure_labels(neighbors=) against the
host route (which tests/test_cpu_label_contacts.py holds against a brute-force statement of the definition) and against closed forms:
around the tile extents, on trivial images, with ids that fill 62 bits of key, with no lane combined and with whole waves combined,
with more tiles than blocks, past 2^31 elements, and through the public functions.  All comparisons are exact."""
import ctypes

import numpy as np
import pytest

import _label_contacts_cases as C

pytestmark = pytest.mark.gpu

NEIGHBOR_NAMES = ("neighbors", "contact_objects", "contact_background")


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


def entry(torch, t, connectivity, background, cap=None, nd=None, buffers=True):
    """sd_label_contacts_device on the int32 device tensor t: (label_a, label_b, contacts as numpy arrays of the rows written, the
    number of rows, the number of runs, (min, max), the key and count buffers)"""
    from stardist_amd.lib import _native as N
    cap = max(64, t.numel() * 13) if cap is None else cap
    keys = torch.full((cap,), -7, dtype=torch.int64, device=t.device)
    counts = torch.full((cap,), -7, dtype=torch.int64, device=t.device)
    count, runs, mm = ctypes.c_longlong(-1), ctypes.c_longlong(-1), (ctypes.c_int32 * 2)(-5, -5)
    N.dcall(t, "sd_label_contacts_device", N.tptr(t), t.dim() if nd is None else nd, *zyx(t.shape), connectivity, int(background),
            ctypes.c_longlong(cap), N.tptr(keys) if buffers else None, N.tptr(counts) if buffers else None, ctypes.byref(count), mm,
            ctypes.byref(runs))
    m = min(count.value, cap)
    k, c = keys[:m].cpu().numpy(), counts[:m].cpu().numpy()
    return (k >> 32, k & 0xFFFFFFFF, c), count.value, runs.value, (mm[0], mm[1]), (keys, counts)


def host_table(a, connectivity, background):
    t = U().label_contacts(a, connectivity, background=background)
    return t["label_a"], t["label_b"], t["contacts"]


def same(got, want):
    return all(g.dtype == np.int64 and np.array_equal(g, w) for g, w in zip(got, want))


def pair_count(shape, connectivity):
    """the number of pixel pairs (p, p + o) inside an image over the forward offsets o"""
    return sum(int(np.prod([n - abs(d) for n, d in zip(shape, o)])) for o in C.forward_offsets(len(shape), connectivity))


@pytest.mark.parametrize("nd", (2, 3))
def test_entry_point_around_the_tile_extents(torch, nd):
    """extent - 1, the extent and + 1 on every axis, every connectivity, with and without the background: blocks whose contacts straddle
    the tile faces, edges and corners, noise, and single pixels at the image's far edges (the diagonal offsets there would read the
    clamped halo cells)"""
    for shape in C.tile_shapes(nd):
        for kind in C.KINDS:
            img = C.tiled(kind, shape)
            t = upload(torch, img)
            keep = t.clone()
            for c in range(1, nd + 1):
                with_bg = entry(torch, t, c, True)
                without = entry(torch, t, c, False)
                assert same(with_bg[0], host_table(img, c, True)), (shape, kind, c)
                assert same(without[0], host_table(img, c, False)), (shape, kind, c)
                again = entry(torch, t, c, True)
                assert all(torch.equal(x, y) for x, y in zip(with_bg[4], again[4])) and again[1:4] == with_bg[1:4]      # the same bits
                objects = with_bg[0][0] > 0                                 # the background only adds its rows
                assert same([v[objects] for v in with_bg[0]], without[0])
                assert with_bg[3] == (int(img.min()), int(img.max())) and with_bg[1] == len(with_bg[0][0])
                assert 0 < with_bg[2] <= with_bg[0][2].sum()
            assert torch.equal(t, keep)                                     # the input is not written
    if nd == 2:                                                             # a plane given as a volume: connectivity 3 is 2 there
        img = C.tiled("noise", C.tile_shapes(2)[-1])
        got = entry(torch, upload(torch, img[None]), 3, True)
        assert same(got[0], host_table(img, 2, True)) and same(got[0], host_table(img[None], 3, True))


def test_trivial_images(torch):
    for a in (np.array([[5]], np.int32), np.array([[4, 4, 4, 4, 4, 4, 4]], np.int32), np.zeros((37, 70), np.int32), np.full((37, 70), 3, np.int32),
              np.full((5, 9, 66), 2, np.int32)):
        for c in range(1, a.ndim + 1):
            table, count, runs, mm, _ = entry(torch, upload(torch, a), c, True)
            assert count == 0 and runs == 0 and len(table[0]) == 0 and mm == (int(a.min()), int(a.max()))
    row = np.array([[1, 1, 0, 2, 2, 3, 0, 0, 3]], np.int32)
    assert same(entry(torch, upload(torch, row), 2, True)[0], host_table(row, 2, True))
    assert [v.tolist() for v in entry(torch, upload(torch, row), 1, False)[0]] == [[2], [3], [1]]
    for shape in ((0, 5), (5, 0), (0, 3, 4), (2, 0, 4)):                    # n <= 0: no error, no row
        table, count, runs, mm, _ = entry(torch, torch.zeros(shape, dtype=torch.int32, device="cuda"), 1, True)
        assert count == 0 and runs == 0 and mm == (0, 0)
    neg = np.array([[1, -2, 3]], np.int32)                                  # a negative label: nothing is computed, the caller raises
    table, count, runs, mm, _ = entry(torch, upload(torch, neg), 1, True)
    assert count == 0 and mm == (-2, 3)


def test_wide_ids_fill_62_bits_of_key(torch):
    top = 2 ** 31 - 1
    small = C.SMALL["wide_ids"].astype(np.int32)
    a = np.zeros((C.TY + 5, C.TX + 9), np.int32)
    a[::3], a[1::3], a[2::3] = 1, 2 ** 30, top                              # three ids in contact over two tiles each way
    a[:, C.TX - 1:C.TX + 1] = top
    for img in (small, a):
        for c in (1, 2):
            got = entry(torch, upload(torch, img), c, False)
            assert same(got[0], host_table(img, c, False)) and got[3][1] == top
            assert got[0][0].tolist() == [1, 1, 2 ** 30] and got[0][1].tolist() == [2 ** 30, top, top]


@pytest.mark.parametrize("shape", ((37, 70), (5, 9, 66)))
def test_no_lane_is_combined_where_every_pixel_has_its_own_id(torch, shape):
    a = np.arange(1, int(np.prod(shape)) + 1, dtype=np.int32).reshape(shape)
    for c in range(1, a.ndim + 1):
        table, count, runs, _, _ = entry(torch, upload(torch, a), c, False)
        n = pair_count(shape, c)
        assert runs == table[2].sum() == n == count and (table[2] == 1).all()
        assert same(table, host_table(a, c, False))


def test_whole_waves_are_combined_along_horizontal_stripes(torch):
    Y, X = C.TY + 8, 4 * C.TX + 44                                          # stripes 300 pixels wide, one row high, over five tiles
    assert X >= 256
    a = np.repeat(np.arange(1, Y + 1, dtype=np.int32)[:, None], X, axis=1)
    for c, per_pair in ((1, X), (2, X + 2 * (X - 1))):
        table, count, runs, _, _ = entry(torch, upload(torch, a), c, False)
        assert count == Y - 1 and table[0].tolist() == list(range(1, Y)) and table[1].tolist() == list(range(2, Y + 1))
        assert (table[2] == per_pair).all()                                 # the closed form
        assert runs < table[2].sum() and runs * 16 <= table[2].sum()        # a wave's 64 lanes went into one run, mostly
    # borders that cross the wave and tile boundaries at odd positions: staggered steps, two rows high
    y, x = np.indices((2 * C.TY + 3, 3 * C.TX + 7))
    b = (1 + ((x + 3 * (y // 2)) // 37 + 5 * (y // 2)) % 23).astype(np.int32)
    for c in (1, 2):
        for background in (False, True):
            table, count, runs, _, _ = entry(torch, upload(torch, b), c, background)
            assert same(table, host_table(b, c, background)) and runs < table[2].sum()


def test_more_tiles_than_blocks(torch):
    """three rows of 2^19 + 70 pixels are 8194 tiles, more than the grid's 8192 blocks: blocks take a second tile"""
    X = 8192 * C.TX + 70
    a = (1 + (np.arange(X) // 7) % 5).astype(np.int32)[None, :].repeat(3, axis=0)
    a[1] = np.roll(a[1], 3)
    a[:, -C.TX - 5:] = 9                                                    # the last two tiles differ from the pattern
    a[2, -3:] = 8
    t = upload(torch, a)
    for c in (1, 2):
        assert same(entry(torch, t, c, True, cap=4096)[0], host_table(a, c, True))


def test_touching_balls(torch):
    vol = C.balls()
    for a in (vol, vol[5:6], vol[5]):                                       # the volume, one slice as a stack, that slice as an image
        t = upload(torch, a)
        for c in range(1, a.ndim + 1):
            got = entry(torch, t, c, True)
            assert same(got[0], host_table(a, c, True)), (a.shape, c)
    assert entry(torch, upload(torch, vol), 1, False)[0][0].tolist() == [1, 2, 3, 4]


def test_past_2_to_the_31_elements(torch):
    Y, X = 2 ** 15 + 1, 2 ** 16                                             # 2^31 + 2^16 elements, 2^20 + 1024 tiles
    free = torch.cuda.mem_get_info()[0]
    if free < 12e9:
        pytest.skip("needs 12 GB of free device memory, the device reports %.1f GB" % (free / 1e9))
    crop = np.zeros((8, 256), np.int32)                                     # the image's last rows and columns; zero elsewhere
    crop[-3:, -40:-20], crop[-3:, -20:], crop[-5:-3, -30:-10], crop[-1, -1], crop[-2, -2] = 1, 2, 3, 4, 5
    t = torch.zeros((Y, X), dtype=torch.int32, device="cuda")
    t[-8:, -256:] = upload(torch, crop)
    for c in (1, 2):
        got = entry(torch, t, c, True, cap=1024)
        assert same(got[0], host_table(crop, c, True)) and got[3] == (0, 5)
    del t
    torch.cuda.empty_cache()


def test_entry_point_argument_checks(torch):
    from stardist_amd.lib import _native as N
    a = C.SMALL["blobs_2d"].astype(np.int32)
    t = upload(torch, a)
    for nd, shape, c in ((1, (1, 24, 31), 1), (4, (1, 24, 31), 1), (2, (2, 12, 31), 1), (2, (1, 24, 31), 0), (2, (1, 24, 31), 3),
                         (3, (1, 24, 31), 4), (3, (1, 24, 31), -1)):
        keys = torch.empty(64, dtype=torch.int64, device="cuda")
        count, mm = ctypes.c_longlong(0), (ctypes.c_int32 * 2)()
        with pytest.raises(N.NativeError, match="ndim|connectivity"):
            N.dcall(t, "sd_label_contacts_device", N.tptr(t), nd, *shape, c, 1, ctypes.c_longlong(64), N.tptr(keys), N.tptr(keys),
                    ctypes.byref(count), mm, None)
    mm = (ctypes.c_int32 * 2)()
    with pytest.raises(N.NativeError, match="h_count"):
        N.dcall(t, "sd_label_contacts_device", N.tptr(t), 2, 1, 24, 31, 1, 1, ctypes.c_longlong(0), None, None, None, mm, None)
    with pytest.raises(N.NativeError, match="capacity"):
        entry(torch, t, 1, True, cap=8, buffers=False)
    want = host_table(a, 2, True)
    m = len(want[0])
    assert m > 8
    table, count, runs, _, (keys, counts) = entry(torch, t, 2, True, cap=5)  # a capacity below the table: the first rows, the full size
    assert count == m and same(table, [w[:5] for w in want]) and len(keys) == 5
    table, count, runs, _, (keys, counts) = entry(torch, t, 2, True, cap=m + 3)
    assert count == m and same(table, want) and keys[m:].tolist() == [-7] * 3 and counts[m:].tolist() == [-7] * 3
    assert entry(torch, t, 2, True, cap=0, buffers=False)[1] == m           # a pure count query


@pytest.mark.parametrize("name", sorted(C.SMALL))
def test_public_function_in_all_keyword_combinations(torch, name):
    a = C.SMALL[name]
    for c in range(1, a.ndim + 1):
        for background in (False, True):
            for symmetric in (False, True):
                want = U().label_contacts(a, c, background=background, symmetric=symmetric)
                got = U().label_contacts(a, c, background=background, symmetric=symmetric, device="cuda")
                assert list(got) == list(want)
                assert all(isinstance(got[k], np.ndarray) and got[k].dtype == np.int64 and np.array_equal(got[k], want[k]) for k in want)
                if name == "huge_ids" or c > 1:
                    continue
                for x in (upload(torch, a), torch.as_tensor(np.array(a))):  # a device tensor; a host tensor with device=
                    kw = {} if x.is_cuda else {"device": "cuda"}
                    got = U().label_contacts(x, c, background=background, symmetric=symmetric, **kw)
                    assert all(isinstance(got[k], np.ndarray) and np.array_equal(got[k], want[k]) for k in want)
                    got = U().label_contacts(x, c, background=background, symmetric=symmetric, as_tensors=True, **kw)
                    assert list(got) == list(want)
                    assert all(got[k].is_cuda and got[k].dtype == torch.int64 and np.array_equal(got[k].cpu().numpy(), want[k]) for k in want)


def test_public_function_errors(torch):
    with pytest.raises(ValueError, match="Negative"):
        U().label_contacts(upload(torch, np.array([[1, -2]], np.int32)))
    with pytest.raises(ValueError, match="Negative"):
        U().label_contacts(np.array([[1, -2]], np.int64), device="cuda")
    with pytest.raises(ValueError, match="connectivity"):
        U().label_contacts(upload(torch, np.zeros((3, 3), np.int32)), 3)
    empty = U().label_contacts(torch.zeros((0, 4), dtype=torch.int32, device="cuda"), symmetric=True, as_tensors=True)
    assert [len(v) for v in empty.values()] == [0, 0, 0, 1] and all(v.is_cuda for v in empty.values())


@pytest.mark.parametrize("name", ("blobs_2d", "blobs_3d", "noise_3d", "all_background", "huge_ids", "ring"))
def test_measure_labels_neighbors(torch, name):
    a = C.SMALL[name]
    img = np.random.RandomState(3).randint(0, 250, a.shape).astype(np.uint8)
    for c in range(1, a.ndim + 1):
        want = U().measure_labels(a, neighbors=c)
        for got in (U().measure_labels(a, neighbors=c, device="cuda"), U().measure_labels(upload(torch, a), neighbors=c)):
            assert list(got) == list(want)
            assert all(isinstance(got[k], np.ndarray) and got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]) for k in want)
        got = U().measure_labels(upload(torch, a), neighbors=c, as_tensors=True)
        assert list(got) == list(want) and all(got[k].is_cuda and np.array_equal(got[k].cpu().numpy(), want[k]) for k in want)
    # together with the other keywords: the neighbour columns come last and are the same
    alone = U().measure_labels(a, neighbors=1)
    plain = U().measure_labels(upload(torch, a), upload(torch, img), shape=True, percentiles=(25, 50))
    full = U().measure_labels(upload(torch, a), upload(torch, img), shape=True, percentiles=(25, 50), neighbors=1)
    assert list(full) == list(plain) + list(NEIGHBOR_NAMES)
    assert all(np.array_equal(full[k], plain[k], equal_nan=full[k].dtype.kind == "f") for k in plain)
    assert all(np.array_equal(full[k], alone[k]) for k in NEIGHBOR_NAMES)


def test_expand_labels_then_label_contacts_on_nuclei(torch):
    nuclei = C._blobs((90, 130), 24, 11)
    t = upload(torch, nuclei)
    grown_host = U().expand_labels(nuclei, 3)
    grown = U().expand_labels(t, 3)
    assert np.array_equal(grown.cpu().numpy(), grown_host)
    for c in (1, 2):
        want = U().label_contacts(grown_host, c, symmetric=True)
        got = U().label_contacts(grown, c, symmetric=True, as_tensors=True)
        assert all(np.array_equal(got[k].cpu().numpy(), want[k]) for k in want)
        assert len(want["contacts"]) > len(U().label_contacts(nuclei, c, symmetric=True)["contacts"])      # the gaps closed
