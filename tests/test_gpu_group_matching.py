"""GPU: group_matching_labels on the device.  sd_label_overlap_stack_device (csrc/overlap.hip) returns, in one call, exactly the numpy
overlap list of every consecutive pair of frames (order included, identical from call to call); sd_relabel_stack_device
(csrc/relabel.hip) equals the numpy table lookup in its dense-table and its sorted-search form and writes every element;
group_matching_labels on device tensors equals the host function on the scenes of tests/_group_cases.py and, on the 8 x 2048^2 scene of
tools/time_group_matching.py, the host composition of sparse_overlap lists; the number of native calls does not grow with the frames."""
import numpy as np
import pytest

import _group_cases as G

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda:0")


def _up(y):
    import torch
    return torch.from_numpy(np.ascontiguousarray(y)).to(_dev())


def _check_stack(ys):
    """the stack call against sparse_overlap pair by pair, and against itself"""
    from stardist_amd import matching_sparse as S
    ys = np.ascontiguousarray(ys, dtype=np.int32)
    lists, mm = S.label_overlap_stack_device(_up(ys))
    assert len(lists) == len(ys) - 1
    for k, (t, p, c) in enumerate(lists):
        rt, rp, rc = S.sparse_overlap(ys[k], ys[k + 1])
        assert t.dtype == p.dtype == c.dtype == np.int64
        assert np.array_equal(t, rt) and np.array_equal(p, rp) and np.array_equal(c, rc), k
    assert np.array_equal(mm, [[int(y.min()), int(y.max())] for y in ys])
    again, mm2 = S.label_overlap_stack_device(_up(ys))
    assert np.array_equal(mm, mm2) and all(np.array_equal(x, y) for a, b in zip(lists, again) for x, y in zip(a, b))
    return lists


@pytest.mark.parametrize("case", ["k2_odd", "k3_unaligned", "k9", "zero_frame", "all_zero", "huge_ids", "wide_ids_k9", "tiny"])
def test_stack_overlap_equals_numpy(case):
    if case == "k2_odd":                                               # n = 97 * 211: not a multiple of 4 (nor of 256)
        ys = G.moving(1, shape=(97, 211), n=60, frames=2)
    elif case == "k3_unaligned":                                       # n a multiple of 4, not of 256
        ys = G.moving(2, shape=(90, 102), n=50, frames=3)
    elif case == "k9":
        ys = G.moving(3, shape=(256, 320), n=200, frames=9)
    elif case == "zero_frame":
        ys = G.moving(4, shape=(64, 128), n=30, frames=4)
        ys[2] = np.zeros_like(ys[2])
    elif case == "all_zero":
        ys = np.zeros((3, 33, 57), np.int32)
    elif case == "huge_ids":                                           # 31 bits per id: two bits are left for the pair index
        ys = G.moving(5, shape=(120, 130), n=80, frames=3)
        ys = [np.where(y > 0, 2 ** 31 - 1 - (k + 1) * (y.astype(np.int64) - 1), 0).astype(np.int32) for k, y in enumerate(ys)]
        assert max(int(y.max()) for y in ys) == 2 ** 31 - 1
    elif case == "wide_ids_k9":                                        # 8 pairs at 31 bits per id: the pairs are worked off in groups
        ys = G.moving(6, shape=(60, 100), n=40, frames=9)
        ys = [np.where(y > 0, 2 ** 31 - 1 - y.astype(np.int64), 0).astype(np.int32) for y in ys]
    else:
        ys = [np.array([[0, 1, 1], [2, 0, 3]], np.int32), np.array([[1, 1, 0], [2, 2, 0]], np.int32), np.array([[7, 7, 7], [0, 0, 2]], np.int32)]
    _check_stack(np.stack(ys))


def test_stack_overlap_capacity_and_negative_labels(monkeypatch):
    """a first call whose capacity is too small is repeated once with the count it returned; a negative label leaves the lists empty and
    shows in the frame's minimum"""
    from stardist_amd import matching_sparse as S
    from stardist_amd.lib import _native as N
    base = np.arange(128 * 128, dtype=np.int32).reshape(128, 128) // 2 + 1                       # two-pixel objects: about n pairs per frame pair
    ys = np.stack([np.roll(base, k, axis=1) for k in range(4)])
    calls = []
    orig = N.dcall
    monkeypatch.setattr(N, "dcall", lambda t, name, *a: (calls.append(name), orig(t, name, *a))[1])
    lists = _check_stack(ys)
    assert sum(len(t) for t, _, _ in lists) > max(1024, 3 * 128 * 128 // 16)
    assert calls == ["sd_label_overlap_stack_device"] * 4              # two calls per list, for the two lists _check_stack takes
    neg = ys.copy()
    neg[2, 5, 5] = -4
    lists, mm = S.label_overlap_stack_device(_up(neg))
    assert all(len(t) == 0 for t, _, _ in lists) and mm[2, 0] == -4


@pytest.mark.parametrize("case", ["dense", "search", "mixed_odd"])
def test_stack_relabel_equals_numpy_lookup(case, monkeypatch):
    import torch
    from stardist_amd import matching_sparse as S
    rng = np.random.RandomState(5)
    if case == "dense":
        ys = np.stack(G.moving(8, shape=(96, 128), n=60, frames=4))
    elif case == "search":                                             # sparse ids up to 2**31 - 1: no dense table
        ys = np.stack(G.moving(9, shape=(96, 128), n=60, frames=3)).astype(np.int64)
        ys = np.where(ys > 0, 2 ** 31 - 1 - 5000 * (ys - 1), 0)
        assert ys.max() == 2 ** 31 - 1
    else:                                                              # n odd (scalar loads and stores), one frame dense, one searched, one empty
        ys = np.stack(G.moving(10, shape=(97, 211), n=60, frames=3)).astype(np.int64)
        ys[1] = np.where(ys[1] > 0, 2 ** 30 + 977 * ys[1], 0)
        ys[2] = 0
    tables = []
    for y in ys:
        ids = np.unique(y[y > 0])
        tables.append((ids, rng.permutation(2 ** 31 - 1 - np.arange(len(ids)) * 3) if case == "search" else rng.permutation(len(ids)) + 1 + 10 * len(tables)))
    want = S.lookup_tables(ys, tables)
    a = _up(ys.astype(np.int32))
    # the output buffer starts as a sentinel: an element the kernel does not write shows
    monkeypatch.setattr(torch, "empty_like", lambda t, **kw: torch.full_like(t, -77, **kw))
    got = S.relabel_stack_device(a, tables)
    assert got.dtype == torch.int32 and got.device == a.device and got.shape == a.shape
    assert np.array_equal(got.cpu().numpy(), want)
    # an id missing from its table becomes 0, like in the lookup
    short = [(ids[1:], new[1:]) for ids, new in tables]
    assert np.array_equal(S.relabel_stack_device(a, short, [int(y.max()) for y in ys]).cpu().numpy(), S.lookup_tables(ys, short))


SCENES = G.scenes()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_device_grouping_equals_host_function(name):
    import torch
    from stardist_amd import matching as M
    ys = SCENES[name]
    single = isinstance(ys, np.ndarray)
    small = all(np.asarray(y).max() <= 2 ** 31 - 1 for y in ys)
    assert small
    dys = _up(ys) if single else [_up(y.astype(np.int32) if y.dtype == np.uint16 else y) for y in ys]     # torch has no arithmetic on uint16
    before = dys.clone() if single else [y.clone() for y in dys]
    for crit in G.CRITERIA:
        for thr in G.THRESHS:
            h = M.group_matching_labels(ys, thresh=thr, criterion=crit)
            d = M.group_matching_labels(dys, thresh=thr, criterion=crit)
            assert N_is_device_int32(d) and tuple(d.shape) == h.shape
            assert np.array_equal(d.cpu().numpy(), h), (name, crit, thr)
    e = M.group_matching_labels(ys, device=_dev())
    assert isinstance(e, np.ndarray) and e.dtype == np.int32 and np.array_equal(e, M.group_matching_labels(ys))
    after = [dys] if single else dys
    assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip([before] if single else before, after))


def N_is_device_int32(d):
    import torch
    return isinstance(d, torch.Tensor) and d.dtype == torch.int32 and d.device == _dev()


def test_device_grouping_thresh_none_and_mixed_inputs():
    """thresh <= 0 (None) goes through the host function and still returns where the inputs live; one device tensor among numpy frames
    is enough for the device path"""
    from stardist_amd import matching as M
    ys = SCENES["moving1"]
    for thr in (None, 0):
        d = M.group_matching_labels([_up(y) for y in ys], thresh=thr)
        assert N_is_device_int32(d) and np.array_equal(d.cpu().numpy(), M.group_matching_labels(ys, thresh=thr))
    d = M.group_matching_labels([_up(ys[0])] + ys[1:])
    assert N_is_device_int32(d) and np.array_equal(d.cpu().numpy(), M.group_matching_labels(ys))
    with pytest.raises(ValueError, match="not supported"):
        M.group_matching_labels([_up(y) for y in ys], criterion="dice")


def test_device_grouping_errors_equal_host():
    from stardist_amd import matching as M
    from test_cpu_group_matching import error_cases
    y = G.discs((40, 50), 10, 3)
    neg = y.copy()
    neg[0, 0] = -1
    for ys in error_cases(y, neg, device_free=False):
        with pytest.raises(ValueError) as host:
            M.group_matching_labels(ys)
        with pytest.raises(ValueError) as dev:
            M.group_matching_labels(ys, device=_dev())
        assert str(dev.value) == str(host.value)
        if isinstance(ys, np.ndarray) or all(isinstance(v, np.ndarray) for v in ys):
            with pytest.raises(ValueError) as dev:
                M.group_matching_labels(_up(ys) if isinstance(ys, np.ndarray) else [_up(v) for v in ys])
            assert str(dev.value) == str(host.value)
    with pytest.raises(ValueError, match="2\\*\\*31"):
        M.group_matching_labels(_up(np.stack([y, y]).astype(np.int64) + 2 ** 31))


def test_timing_scene_equals_host_composition():
    """8 x 2048^2, 12 756 lattice discs per frame: the device result equals the composition of sparse_overlap lists (independent of both
    kernels), and the first two frames equal the dense host function"""
    from stardist_amd import matching as M
    ys = G.lattice_stack()
    assert ys.shape == (8, 2048, 2048) and len(np.unique(ys[0])) - 1 == 12756
    d = M.group_matching_labels(_up(ys))
    assert N_is_device_int32(d)
    d = d.cpu().numpy()
    assert np.array_equal(d, G.compose(ys, 1e-10, "iou"))
    assert np.array_equal(d[:2], M.group_matching_labels(ys[:2]))
    assert len(np.unique(d)) - 1 < 12756 + 7 * 12756 // 2                # most objects keep their id through the stack


def test_native_calls_do_not_grow_with_frames(monkeypatch):
    """two native calls whatever the number of frames (small ids: one group of pairs), and no host synchronisation per frame: the stack
    goes through N.dcall twice"""
    from stardist_amd import matching as M
    from stardist_amd.lib import _native as N
    calls = []
    orig = N.dcall
    monkeypatch.setattr(N, "dcall", lambda t, name, *a: (calls.append(name), orig(t, name, *a))[1])
    counts = {}
    for K in (3, 9):
        ys = _up(np.stack(G.moving(12, shape=(128, 160), n=40, frames=K)))
        del calls[:]
        M.group_matching_labels(ys)
        counts[K] = list(calls)
    assert counts[3] == counts[9] == ["sd_label_overlap_stack_device", "sd_relabel_stack_device"]


def test_int64_frame_lists_are_range_checked_once(monkeypatch):
    """a list of int64 device frames: the check that the ids fit int32 reads back once for the stack, not once per frame, and the
    result equals the host function's"""
    import torch
    from stardist_amd import matching as M
    reads = []
    orig = torch.aminmax
    monkeypatch.setattr(torch, "aminmax", lambda *a, **k: (reads.append(1), orig(*a, **k))[1])
    for K in (3, 9):
        ys = G.moving(12, shape=(128, 160), n=40, frames=K)
        del reads[:]
        d = M.group_matching_labels([_up(y.astype(np.int64)) for y in ys])
        assert len(reads) == 1, (K, len(reads))
        assert N_is_device_int32(d) and np.array_equal(d.cpu().numpy(), M.group_matching_labels(ys))
    with pytest.raises(ValueError, match="2\\*\\*31"):
        M.group_matching_labels([_up(ys[0].astype(np.int64)), _up(ys[1].astype(np.int64) + 2 ** 31)])
