"""CPU: the one exit of the table functions (stardist_amd._route.table_exit), the one numpy / torch shim (_route.ops) and the one
raw-column schema (label_ops._measure_schema).  The host route's tables against the bytes of the commit before them
(tests/golden/measure_table_parent.npz); the device route's assembly with its halves replaced by fakes that return the host halves'
results as CPU tensors -- byte for byte the host route's table, through exactly one read-back call; every operation of the shim on an
array and on a CPU tensor of the same values; the schema through pack and unpack.  Cases: tests/_table_exit_cases.py."""
import itertools
import math

import numpy as np
import pytest

import _hull_cases as H
import _measure_cases as M
import _shape_cases as S
import _table_exit_cases as T
from test_cpu_measure_hull import combos


@pytest.fixture(scope="module")
def golden():
    return np.load(T.GOLDEN)


# ----------------------------------------------------------------------------- pinned against the parent

@pytest.mark.parametrize("name", T.GOLDEN_NAMES)
def test_host_tables_are_the_parent_s(golden, name):
    """key order, dtypes and bytes; orientation and the 3D equivalent_diameter by libm_close (another machine's libm may differ by an ulp)"""
    want = {k.split("/", 2)[2]: golden[k] for k in sorted(k for k in golden.files if k.startswith(name + "/"))}
    assert len(want) >= 1
    nd3 = name == "measure_3d"
    T.same_table(T.host(name), want, libm=("orientation",) + (("equivalent_diameter",) if nd3 else ()))


@pytest.mark.parametrize("kind,name", T.DERIVED)
def test_derived_columns_are_the_parent_s_on_arrays_and_on_host_tensors(golden, kind, name):
    """_measure_columns, _shape_columns (with _jacobi_eigvals) and _hull_columns on the cases' raw tables: every column that is + - * /
    sqrt of the integers has the parent's digest, computed on arrays and computed on CPU tensors; the libm columns by libm_close"""
    import torch
    from stardist_amd.label_ops import _measure_columns
    want = T.derived(kind, name)
    assert np.array_equal(T.digests(want), golden["derived/%s/%s" % (kind, name)])
    raw = S.raw(name) if kind == "shape" else None
    if raw is not None:
        on_tensors = _measure_columns({k: torch.from_numpy(v.copy()) for k, v in raw.items()}, S.case(name).ndim, False)
    else:
        from stardist_amd.utils import measure_labels
        on_tensors = measure_labels(torch.from_numpy(H.case(name).copy()), hull=True, as_tensors=True)
    assert all(isinstance(v, torch.Tensor) for v in on_tensors.values())
    on_tensors = {k: v.numpy() for k, v in on_tensors.items()}
    assert np.array_equal(T.digests(on_tensors), golden["derived/%s/%s" % (kind, name)])
    for key in T.LIBM:
        if key in want:
            assert T.libm_close(want[key], golden["derived/%s/%s/%s" % (kind, name, key)]), key
            assert T.libm_close(on_tensors[key], golden["derived/%s/%s/%s" % (kind, name, key)]), key


# ----------------------------------------------------------------------------- the device route's assembly, with faked halves

class Fakes:
    """the device halves replaced by the host halves, their results as CPU tensors; utils.to_host / to_host_many counted"""

    def __init__(self, monkeypatch):
        import torch
        from stardist_amd import label_ops, utils
        self.reads = []
        tensors = lambda cols: tuple(None if c is None else torch.from_numpy(np.ascontiguousarray(c)) for c in cols)
        array = lambda x: x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        raw_host, contacts_host = label_ops._measure_raw_host, label_ops._label_contacts_host
        nearest_host, within_host = label_ops._nearest_host, label_ops._within_host

        def measure(lbl, img, C, device, **more):
            raw = raw_host(array(lbl), None if img is None else array(img), **more)
            return dict(zip(raw, tensors(raw.values())))

        def contacts(lbl, connectivity, background, device=None, runs=None):
            return tensors(contacts_host(array(lbl), connectivity, background))

        def neighbors(P, Q, mode, k, r2, cell_size=0.0, cell=None):
            P = P.numpy()
            Q, own = (P, True) if Q is None else (Q.numpy(), False)
            if mode == 0:
                return tensors(nearest_host(P, Q, own, k, r2))
            counts, idx, d2 = within_host(P, Q, own, math.sqrt(r2), r2, mode == 1)
            return tensors([counts])[0] if mode == 1 else tensors([np.concatenate([np.zeros(1, np.int64), np.cumsum(counts)]), idx, d2])

        def counted(name):
            real = getattr(utils, name)
            return lambda *a: self.reads.append(name) or real(*a)

        monkeypatch.setattr(label_ops, "_measure_raw_device", measure)
        monkeypatch.setattr(label_ops, "_label_contacts_device", contacts)
        monkeypatch.setattr(label_ops, "_point_neighbors_device", neighbors)
        monkeypatch.setattr(label_ops, "_labels_present", lambda lbl, on_device, device: (
            torch.from_numpy(np.unique(array(lbl)[array(lbl) > 0]).astype(np.int64)) if on_device else np.unique(lbl[lbl > 0]).astype(np.int64)))
        monkeypatch.setattr(label_ops.N, "require_device", lambda: None)
        monkeypatch.setattr(utils, "to_host", counted("to_host"))
        monkeypatch.setattr(utils, "to_host_many", counted("to_host_many"))

    def take(self):
        reads, self.reads[:] = list(self.reads), []
        return reads


def every_combination():
    for lbl, img, kw in combos():
        spots = np.argwhere(lbl > 0)[::7]
        for nearest, within, with_spots in itertools.product((None, 3), (None, 9.0), (False, True)):
            more = dict(kw, hull=bool(kw["shape"]) != (nearest is None), nearest=nearest, within=within)      # hull on in half of them
            if nearest is not None or within is not None:
                more["spacing"] = (2, 0.5)
            if with_spots:
                more["spots"] = spots
            yield lbl, img, more


def test_device_route_assembles_the_host_route_s_table_through_one_read_back(monkeypatch):
    """for every combination of image / shape / percentiles / neighbors / nearest / within / spots, with the device halves faked:
    numpy out equals the host route byte for byte, in keys, order and dtypes, through exactly one to_host_many and no to_host;
    as_tensors=True reads nothing back, returns tensors only and equals the host route but for the libm columns (libm_close)"""
    import torch
    from stardist_amd.utils import measure_labels
    fakes = Fakes(monkeypatch)
    widest = 0
    for lbl, img, kw in every_combination():
        want = measure_labels(lbl, img, **kw)
        assert fakes.take() == [], kw
        got = measure_labels(lbl, img, device="cuda", **kw)
        assert fakes.take() == ["to_host_many"], kw
        assert all(isinstance(v, np.ndarray) for v in got.values())
        T.same_table(got, want)
        got = measure_labels(lbl, img, device="cuda", as_tensors=True, **kw)
        assert fakes.take() == [], kw
        assert all(isinstance(v, torch.Tensor) for v in got.values())
        T.same_table(got, want, libm=T.LIBM)
        widest = max(widest, len(got))
    assert widest == 58                                                     # every column family at once


def test_host_route_as_tensors_equals_the_arrays(monkeypatch):
    import torch
    fakes = Fakes(monkeypatch)
    for name in T.GOLDEN_NAMES:
        convert = torch.from_numpy if name.startswith("points") else None  # point_neighbors puts them where the points are
        got = T.run(name, convert=(lambda a: convert(a.copy())) if convert else None, as_tensors=True)
        assert fakes.take() == []
        assert all(isinstance(v, torch.Tensor) and v.device.type == "cpu" for v in got.values())
        T.same_table(got, T.host(name), libm=T.LIBM)


def test_label_contacts_and_point_neighbors_read_back_at_most_once(monkeypatch):
    import torch
    from stardist_amd import label_ops
    fakes = Fakes(monkeypatch)
    monkeypatch.setattr(label_ops.R, "to_device_tensor", lambda x, device=None: torch.as_tensor(np.ascontiguousarray(x)))      # point_neighbors' upload
    for name in ("contacts", "points_k", "points_radius", "points_count"):
        got = T.run(name, device="cuda")
        assert len(fakes.take()) <= 1, name
        assert all(isinstance(v, np.ndarray) for v in got.values())
        T.same_table(got, T.host(name))
        got = T.run(name, device="cuda", as_tensors=True)
        assert fakes.take() == [] and all(isinstance(v, torch.Tensor) for v in got.values())
        T.same_table(got, T.host(name))


def test_table_exit_rule():
    """rule 4 of DESIGN.md section 3p on its own: what passes through, what moves, and where to"""
    import torch
    from stardist_amd import _route as R
    a, t = np.arange(3), torch.arange(3)
    assert R.table_exit([a, None], False)[0] is a and R.table_exit([t, None], True)[0] is t
    back = R.table_exit([t, None, t[::2]], False)
    assert isinstance(back[0], np.ndarray) and back[1] is None and back[2].tolist() == [0, 2]
    for x, device, want in ((None, None, "cpu"), (a, None, "cpu"), (t, None, "cpu"), (a, "cpu", "cpu"), (t, "meta", "meta")):
        out = R.table_exit([a[::2], None], True, x, device)
        assert isinstance(out[0], torch.Tensor) and out[0].device.type == want and out[1] is None


# ----------------------------------------------------------------------------- the shim

def both(x):
    import torch
    return x, torch.from_numpy(x.copy())


def same(a, t):
    import torch
    assert isinstance(a, np.ndarray) and isinstance(t, torch.Tensor)
    n = t.numpy()
    return a.dtype == n.dtype and a.shape == n.shape and a.tobytes() == np.ascontiguousarray(n).tobytes()


def test_every_operation_of_the_shim_gives_the_same_bytes_on_arrays_and_tensors():
    import torch
    from stardist_amd import _route as R
    rng = np.random.default_rng(5301)
    f, ft = both(np.concatenate([[0.0, -0.0, 5e-324, 2.2250738585072014e-308, np.inf, np.nan, 2.0, 1e300], rng.uniform(0, 1e6, 200)]))
    g, gt = both(rng.standard_normal(len(f)))
    i, it = both(np.concatenate([[2 ** 53 + 1, -(2 ** 53) - 1, 2 ** 62 + 3, 2 ** 63 - 1, -(2 ** 63), 0], rng.integers(-50, 50, 60)]).astype(np.int64))
    o, ot = R.ops(f), R.ops(ft)
    assert o is R.ops(i) and not o.is_torch and ot.is_torch and o.xp is np and ot.xp is torch
    assert set(vars(o)) == set(vars(ot))
    with np.errstate(all="ignore"):
        assert same(o.sqrt(f), ot.sqrt(ft))                                 # 0, a subnormal, inf and NaN among them
        assert same(o.atan2(f[6:], g[6:]), ot.atan2(ft[6:], gt[6:])) or T.libm_close(o.atan2(f[6:], g[6:]), ot.atan2(ft[6:], gt[6:]).numpy())
    assert same(o.f64(i), ot.f64(it)) and o.f64(i)[0] == 2.0 ** 53         # beyond 2^53: rounded, the same way
    assert same(o.f64((2, 0.5)), ot.f64((2, 0.5))) and same(o.i64([3, 4]), ot.i64([3, 4]))
    assert same(o.i64(i.astype(np.int32, casting="unsafe")), ot.i64(it.to(torch.int32)))
    assert same(o.astype(i[5:], "int32"), ot.astype(it[5:], "int32")) and o.int64 == np.int64 and ot.float64 is torch.float64
    assert same(o.col(f[::3]), ot.col(ft[::3])) and o.col(f[::3]).flags.c_contiguous and ot.col(ft[::3]).is_contiguous()
    assert same(o.cat([i, i[:4]]), ot.cat([it, it[:4]]))
    assert same(o.cat([i.reshape(-1, 1), i.reshape(-1, 1)], 1), ot.cat([it.reshape(-1, 1), it.reshape(-1, 1)], 1))
    keys, keyst = both(np.array([3, 3, 5, 9, 9, 9, 12], np.int64))
    probe, probet = both(np.array([0, 3, 4, 9, 12, 13], np.int64))
    assert same(o.searchsorted(keys, probe), ot.searchsorted(keyst, probet))
    assert same(o.zeros_i64(4), ot.zeros_i64(4))
    at, att = both(np.array([1, 1, 3, 1, 0, 3], np.int64))                  # duplicate indices add up
    out, outt = o.zeros_i64(5), ot.zeros_i64(5)
    o.add_at(out, at, i[:6] // 4)
    ot.add_at(outt, att, torch.div(it[:6], 4, rounding_mode="floor"))
    assert same(out, outt) and out[1] == (i[[0, 1, 3]] // 4).sum()
    ties, tiest = both(rng.integers(0, 4, 300))                             # ties keep their order
    assert same(o.stable_argsort(ties), ot.stable_argsort(tiest))
    assert same(o.bincount(at, 6), ot.bincount(att, 6)) and same(o.bincount(at[:0], 3), ot.bincount(att[:0], 3))
    assert same(o.clip_max(i, 7), ot.clip_max(it, 7))
    assert same(o.xp.where(i > 0, i, 0 * i), ot.xp.where(it > 0, it, 0 * it)) and same(o.xp.abs(g), ot.xp.abs(gt))
    assert same(o.xp.maximum(f[6:], g[6:]), ot.xp.maximum(ft[6:], gt[6:])) and same(o.xp.minimum(f[6:], g[6:]), ot.xp.minimum(ft[6:], gt[6:]))
    assert same(o.xp.ones_like(f), ot.xp.ones_like(ft))


# ----------------------------------------------------------------------------- the schema

SCHEMAS = [(nd, C, kind, shape, hull) for nd in (2, 3) for C in (None, 1, 3) for kind in ("uint8", "float32")
           for shape in (False, True) for hull in (False, True) if not (hull and nd == 3) and not (C is None and kind == "float32")]


@pytest.mark.parametrize("nd,C,kind,shape,hull", SCHEMAS)
def test_schema_holds_for_both_halves_and_through_the_packed_form(monkeypatch, nd, C, kind, shape, hull):
    """the host half's output has the schema's keys, shapes and dtypes and comes back from _measure_unpack(_measure_pack(.)) with the same
    bytes, as arrays and as tensors; the device half's empty table has the keys and dtypes of a non-empty one"""
    import torch
    from stardist_amd import label_ops
    lbl = S.case("small_2d" if nd == 2 else "small_3d")
    img = None if C is None else (np.random.default_rng(5401).uniform(-3, 300, lbl.shape + (() if C == 1 else (C,))).astype(kind))
    more = dict(shape=shape, hull=hull)
    raw = label_ops._measure_raw_host(lbl, img, **more)
    schema = label_ops._measure_schema(nd, C, None if img is None else ("int64" if kind == "uint8" else kind), **more)
    n = len(raw["label"])
    assert n > 3 and [(k, v.shape, v.dtype.name) for k, v in raw.items()] == [(k, (n,) if w is None else (n, w), d) for k, w, d in schema]
    for kind_of in (lambda a: a, lambda a: torch.from_numpy(a.copy())):
        packed = label_ops._measure_pack({k: kind_of(v) for k, v in raw.items()}, schema)
        assert tuple(packed.shape) == (n, sum(w or 1 for _, w, _ in schema)) and "int64" in str(packed.dtype)
        back = label_ops._measure_unpack(packed, schema)
        assert list(back) == list(raw) and type(back["label"]) is type(kind_of(raw["label"]))
        for k, v in raw.items():
            b = np.asarray(back[k])
            assert b.dtype == v.dtype and b.shape == v.shape and b.tobytes() == v.tobytes(), k
    # the device half's empty table (its kernels are not reached): an image without a label
    monkeypatch.setattr(label_ops.N, "require_device", lambda: None)
    monkeypatch.setattr(label_ops.R, "to_device_tensor", lambda x, device=None: torch.as_tensor(np.ascontiguousarray(x)))
    monkeypatch.setattr(label_ops.R, "_device_labels", lambda x, device=None: (torch.as_tensor(np.ascontiguousarray(x)), 0, None))
    empty = label_ops._measure_raw_device(np.zeros_like(lbl), img, C, None, **more)
    assert [(k, tuple(v.shape), str(v.dtype)[6:]) for k, v in empty.items()] == [(k, (0,) if w is None else (0, w), d) for k, w, d in schema]
    fakes = Fakes(monkeypatch)
    table = label_ops.measure_labels(lbl, img, device="cuda", **more)
    monkeypatch.setattr(label_ops, "_measure_raw_device", lambda *a, **k: empty)
    none = label_ops.measure_labels(np.zeros_like(lbl), img, device="cuda", **more)
    assert fakes.take() == ["to_host_many"] * 2
    assert [(k, v.dtype) for k, v in none.items()] == [(k, v.dtype) for k, v in table.items()] and all(v.shape == (0,) for v in none.values())
