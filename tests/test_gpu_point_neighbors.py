"""GPU: sd_point_neighbors_device and the device routes of stardist_amd.utils.point_neighbors and measure_labels(nearest=, within=)
against the host route (which tests/test_cpu_point_neighbors.py holds against an O(n m) statement of the definition): every case of
tests/_point_neighbors_cases.py in every result form, with the automatic cell size and with cell sizes that put points on cell faces, a
set that needs more workgroups than are resident at once, the same bits from call to call, and the entry point's argument checks.  All
comparisons are exact."""
import ctypes

import numpy as np
import pytest

import _label_contacts_cases as LC
import _point_neighbors_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def U():
    from stardist_amd import utils
    return utils


def upload(torch, a):
    return torch.as_tensor(np.array(a, np.float64, order="C"), device="cuda")


def entry(torch, P, Q, k, radius, count_only, cell_size=0.0, cell=None):
    """sd_point_neighbors_device through its one driver, on scaled float64 arrays: the result dict with squared distances under "d2\""""
    from stardist_amd.label_ops import _point_neighbors_device
    r2 = None if radius is None else float(np.float64(radius) * np.float64(radius))
    tP, tQ = upload(torch, P), None if Q is None else upload(torch, Q)
    keep = tP.clone()
    if count_only:
        out = {"counts": _point_neighbors_device(tP, tQ, 1, None, r2, cell_size, cell)}
    elif k is not None:
        out = dict(zip(("indices", "d2"), _point_neighbors_device(tP, tQ, 0, k, r2, cell_size, cell)))
    else:
        out = dict(zip(("offsets", "indices", "d2"), _point_neighbors_device(tP, tQ, 2, None, r2, cell_size, cell)))
    assert torch.equal(tP, keep)                                            # the input is not written
    return {n: v.cpu().numpy() for n, v in out.items()}


def same(got, want, names=None):
    names = names or list(got)
    return all(got[n].dtype == want[n].dtype and got[n].shape == want[n].shape and got[n].tobytes() == want[n].tobytes() for n in names)


@pytest.fixture(scope="module")
def host_results():
    """the host route on every case and call, once"""
    out = {}
    for call in C.calls():
        name, k, radius, count_only = call
        c = C.CASES[name]
        out[call] = U().point_neighbors(c["points"], k, radius, queries=c["queries"], spacing=c["spacing"], count_only=count_only)
    return out


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_entry_point_equals_host_route_for_every_cell_size(torch, host_results, name):
    c = C.CASES[name]
    P = C.scaled(c["points"], c["spacing"])
    Q = None if c["queries"] is None else C.scaled(c["queries"], c["spacing"])
    for k, radius, count_only in c["calls"]:
        want = host_results[(name, k, radius, count_only)]
        for cell_size in (0.0,) + c["cell_sizes"]:
            used = []
            got = entry(torch, P, Q, k, radius, count_only, cell_size, used)
            if "d2" in got:
                got["distances"] = np.sqrt(got.pop("d2"))
            assert list(got) == list(want) and same(got, want), (k, radius, count_only, cell_size)
            assert (used[0] == cell_size if cell_size else used[0] > 0) or len(P) == 0 or (Q is not None and len(Q) == 0)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_public_function_equals_host_route(torch, host_results, name):
    c = C.CASES[name]
    kw = dict(queries=c["queries"], spacing=c["spacing"])
    for k, radius, count_only in c["calls"]:
        want = host_results[(name, k, radius, count_only)]
        got = U().point_neighbors(c["points"], k, radius, count_only=count_only, device="cuda", **kw)
        assert list(got) == list(want) and all(isinstance(v, np.ndarray) for v in got.values()) and same(got, want), (k, radius, count_only)
    k, radius, count_only = c["calls"][0]
    want = host_results[(name, k, radius, count_only)]
    tkw = dict(queries=None if c["queries"] is None else upload(torch, c["queries"]), spacing=c["spacing"], count_only=count_only)
    got = U().point_neighbors(upload(torch, c["points"]), k, radius, **tkw)                       # device tensors in, numpy out
    assert list(got) == list(want) and all(isinstance(v, np.ndarray) for v in got.values()) and same(got, want)
    got = U().point_neighbors(upload(torch, c["points"]), k, radius, as_tensors=True, **tkw)      # and tensors out, on the device
    assert list(got) == list(want) and all(v.is_cuda for v in got.values())
    assert same({n: v.cpu().numpy() for n, v in got.items()}, want)


def test_more_workgroups_than_are_resident(torch):
    """70 000 points are 1094 workgroups of 64 lanes; k = 8, the radius lists and the counts against the host route, and the same bits
    from a second call"""
    pts = np.random.RandomState(5).rand(70000, 2) * 2048
    radius = 19.5                                                           # about 20 neighbours
    for k, r, count_only in ((8, None, False), (None, radius, False), (None, radius, True), (8, radius / 2, False)):
        want = U().point_neighbors(pts, k, r, count_only=count_only)
        got = U().point_neighbors(pts, k, r, count_only=count_only, device="cuda")
        again = U().point_neighbors(upload(torch, pts), k, r, count_only=count_only)
        assert list(got) == list(want) and same(got, want) and same(again, got)
    counts = U().point_neighbors(pts, radius=radius, count_only=True)["counts"]
    assert 15 < counts.mean() < 25


def test_same_bits_from_call_to_call(torch):
    c = C.CASES["five_fold"]
    P = C.scaled(c["points"], 1)
    for k, radius, count_only in ((8, None, False), (None, 1.5, False), (None, 1.5, True)):
        first = entry(torch, P, None, k, radius, count_only)
        for _ in range(3):
            assert same(entry(torch, P, None, k, radius, count_only), first)


@pytest.mark.parametrize("name", ("blobs_2d", "blobs_3d", "noise_3d", "one_label", "all_background", "huge_ids"))
def test_measure_labels_nearest_and_within(torch, name):
    a = LC.SMALL[name]
    spacing = (2.0, 0.7, 0.7)[3 - a.ndim:]
    t = torch.as_tensor(np.array(a, order="C"), device="cuda")
    for kw in (dict(nearest=3), dict(within=6.5, spacing=spacing), dict(nearest=2, within=9, spacing=spacing, neighbors=1)):
        want = U().measure_labels(a, **kw)
        for got in (U().measure_labels(a, device="cuda", **kw), U().measure_labels(t, **kw)):
            assert list(got) == list(want)
            assert all(isinstance(got[n], np.ndarray) and got[n].dtype == want[n].dtype and got[n].tobytes() == want[n].tobytes() for n in want)
        got = U().measure_labels(t, as_tensors=True, **kw)
        assert list(got) == list(want) and all(got[n].is_cuda and got[n].cpu().numpy().tobytes() == want[n].tobytes() for n in want)
    plain = U().measure_labels(t)                                           # without the keywords: the table it was
    assert list(plain) == [n for n in U().measure_labels(a, nearest=1) if not n.startswith("nearest")]


def test_entry_point_argument_checks(torch):
    from stardist_amd.lib import _native as N
    P = upload(torch, np.random.RandomState(1).rand(50, 2))
    idx = torch.full((50 * 4,), -7, dtype=torch.int64, device="cuda")
    d2 = torch.full((50 * 4,), -7.0, dtype=torch.float64, device="cuda")
    off = torch.full((51,), -7, dtype=torch.int64, device="cuda")
    total, used = ctypes.c_longlong(-1), ctypes.c_double(-1)

    def call(points=P, n=50, queries=None, m=50, nd=2, mode=0, k=4, use_radius=0, r2=0.0, cell=0.0, cap=0, indices=idx, dists=d2, offsets=off,
             h_total=total):
        N.dcall(P, "sd_point_neighbors_device", None if points is None else N.tptr(points), ctypes.c_longlong(n),
                None if queries is None else N.tptr(queries), ctypes.c_longlong(m), nd, mode, k, use_radius, ctypes.c_double(r2),
                ctypes.c_double(cell), ctypes.c_longlong(cap), None if indices is None else N.tptr(indices),
                None if dists is None else N.tptr(dists), None if offsets is None else N.tptr(offsets),
                None if h_total is None else ctypes.byref(h_total), ctypes.byref(used))

    for bad, what in ((dict(nd=1), "coordinates"), (dict(nd=4), "coordinates"), (dict(mode=3), "mode"), (dict(mode=-1), "mode"),
                      (dict(k=0), "k outside"), (dict(k=65), "k outside"), (dict(n=-1, m=-1), "n and m"), (dict(n=2 ** 31 - 1, m=2 ** 31 - 1), "n and m"),
                      (dict(m=49), "without queries"), (dict(mode=1), "need a radius"), (dict(mode=2), "need a radius"),
                      (dict(use_radius=1, r2=-1.0), "squared radius"), (dict(use_radius=1, r2=float("nan")), "squared radius"),
                      (dict(cell=-1.0), "cell size"), (dict(cell=float("inf")), "cell size"), (dict(cell=1e-200), "cell size"),
                      (dict(cell=float("nan")), "cell size"), (dict(cell=1e-9), "cells"), (dict(cap=-1), "capacity"),
                      (dict(indices=None), "null output"), (dict(dists=None), "null output"), (dict(mode=1, use_radius=1, offsets=None), "null output"),
                      (dict(mode=2, use_radius=1, h_total=None), "null output"), (dict(mode=2, use_radius=1, cap=10, indices=None), "null output"),
                      (dict(points=None), "null points")):
        with pytest.raises(N.NativeError, match=what):
            call(**bad)
    assert idx.eq(-7).all() and d2.eq(-7).all() and off.eq(-7).all()          # nothing was written
    for value in (float("nan"), float("inf"), 2.0 ** 500):                  # the library checks the points it is given
        broken = P.clone()
        broken[17, 1] = value
        with pytest.raises(N.NativeError, match="not finite"):
            call(points=broken)
    # the list protocol: a pure size query, a capacity that is too small (nothing is written), one with room to spare
    want = U().point_neighbors(P.cpu().numpy(), radius=0.2)
    call(mode=2, use_radius=1, r2=0.2 * 0.2, cap=0, indices=None, dists=None)
    assert total.value == len(want["indices"]) > 50 and off.cpu().numpy().tolist() == want["offsets"].tolist()
    big = torch.full((total.value + 5,), -7, dtype=torch.int64, device="cuda")
    bigd = torch.full((total.value + 5,), -7.0, dtype=torch.float64, device="cuda")
    call(mode=2, use_radius=1, r2=0.2 * 0.2, cap=total.value - 1, indices=big, dists=bigd)
    assert big.eq(-7).all() and total.value == len(want["indices"])
    call(mode=2, use_radius=1, r2=0.2 * 0.2, cap=total.value + 5, indices=big, dists=bigd)
    assert big[:total.value].cpu().numpy().tolist() == want["indices"].tolist() and big[total.value:].eq(-7).all() and bigd[total.value:].eq(-7).all()
    assert np.sqrt(bigd[:total.value].cpu().numpy()).tobytes() == want["distances"].tobytes()
    call(mode=0, k=4, cell=0.125)
    assert used.value == 0.125 and idx.reshape(50, 4).cpu().numpy().tolist() == U().point_neighbors(P.cpu().numpy(), 4)["indices"].tolist()


def test_public_function_errors_on_device_input(torch):
    for points, kw in C.ERRORS:
        if points.dtype.kind == "c":
            continue
        with pytest.raises(ValueError, match="point_neighbors"):
            U().point_neighbors(torch.as_tensor(points, device="cuda"), **kw)
    empty = U().point_neighbors(torch.zeros((0, 3), dtype=torch.float64, device="cuda"), radius=1.0, as_tensors=True)
    assert [len(v) for v in empty.values()] == [1, 0, 0] and all(v.is_cuda for v in empty.values())
