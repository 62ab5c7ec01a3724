"""CPU: the references and the case lists of the exact target tests (_target_cases.py), proven without a GPU.

  * edt_prob_box == oracle.port.edt_prob on the small cases, and its face-neighbour search == the search over every non-object pixel;
  * edt_prob_box == the reference's own _edt_prob_scipy (stardist/utils.py:98-125, taken from the reference file at run time, on scipy) on
    EVERY EDT case, the 2048^2 one on its chosen ids -- only where scipy and the reference sources are present, skipped elsewhere;
  * star_dist2d_np / star_dist3d_np == the compiled reference (oracle/_ref) on every SD case;
  * targets_ref == the generators' lines (model2d.py:63-104, model3d.py:66-104) restated here on the oracle pieces, on every batch;
  * the regimes the cases are named for are reached (asserted on the data, in the reference's terms).

Half steps in 2D: lrint's round-half-even decides the pixel only where a direction component is exactly 0.5, i.e. sinf(k * (float)(2 pi / R))
== 0.5f (or the cosine).  With glibc's sinf / cosf that holds for R = 12 (sinf of k = 1) and for no k of R = 6;
test_half_steps_are_taken prints both and asserts that the R = 12 case really visits .5 coordinates and depends on the rounding mode.  The 3D lattice rays take half
steps by construction."""
import ast
import os
import warnings

import numpy as np
import pytest

import _target_cases as T

REF = "/root/reference/stardist"


def _small(c):
    return T.labels(c["id"]).size <= 2600 and "ids" not in c


@pytest.mark.parametrize("id", [c["id"] for c in T.EDT2D + T.EDT3D if _small(c)])
def test_edt_box_equals_exhaustive_oracle(id):
    from oracle import port
    c = T.BY_ID[id]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = port.edt_prob(T.labels(id), anisotropy=c["aniso"])
        full = T.edt_prob_box(T.labels(id), c["aniso"], exhaustive=True)
    assert np.array_equal(T.edt_want(id), want), T.describe(T.edt_want(id), want, T.labels(id))
    assert np.array_equal(T.edt_want(id), full), T.describe(T.edt_want(id), full, T.labels(id))


def test_face_neighbour_search_equals_full_box_search():
    """the shortcut of edt_prob_box on mid-sized cases of every generator, every anisotropy kind"""
    for id in ("edt2-ellipses-a2", "edt2-annulus-a2", "edt2-voronoi-a2", "edt2-borders-a0", "edt3-ellipses-a3", "edt3-cshape-a2",
               "edt3-voronoi-a1", "edt3-band-zx-a2"):
        c = T.BY_ID[id]
        full = T.edt_prob_box(T.labels(id), c["aniso"], exhaustive=True)
        assert np.array_equal(T.edt_want(id), full), (id, T.describe(T.edt_want(id), full, T.labels(id)))


@pytest.fixture(scope="module")
def ref_edt():
    """the reference's _edt_prob_scipy, from its source file, on scipy"""
    try:
        from scipy.ndimage import distance_transform_edt, find_objects
    except ImportError:
        pytest.skip("needs scipy")
    path = os.path.join(REF, "utils.py")
    if not os.path.isfile(path):
        pytest.skip("needs the reference sources")
    ns = {"np": np, "warnings": warnings, "find_objects": find_objects, "distance_transform_edt": distance_transform_edt}
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name == "_edt_prob_scipy":
            exec(compile(ast.Module([node], []), path, "exec"), ns)
    return ns["_edt_prob_scipy"]


@pytest.mark.parametrize("id", T.ids(T.EDT2D + T.EDT3D))
def test_edt_box_equals_reference_function(ref_edt, id):
    c = T.BY_ID[id]
    lab = T.labels(id)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = ref_edt(lab, anisotropy=c["aniso"])
    if "ids" in c:
        want = np.where(np.isin(lab, c["ids"]), want, 0).astype(np.float32)
    got = T.edt_want(id)
    assert got.dtype == want.dtype == np.float32
    assert np.array_equal(got, want), T.describe(got, want, lab)


@pytest.mark.parametrize("id", T.ids(T.SD2D + T.SD3D))
def test_star_dist_np_equals_compiled_reference(refmods, id):
    c = T.BY_ID[id]
    refmods.set_threads(8)
    lab = T.labels(id)
    u16 = np.ascontiguousarray(T._as_u16(lab))
    if "n_rays" in c:
        want = refmods.stardist2d().c_star_dist(u16, np.int32(c["n_rays"]), np.int32(c["grid"][0]), np.int32(c["grid"][1]))
    else:
        dz, dy, dx = (np.ascontiguousarray(v, np.float32) for v in c["rays"]().vertices.T)
        want = refmods.stardist3d().c_star_dist3d(u16, dz, dy, dx, int(len(dz)), *c["grid"])
    got = T.sd_want(id)
    assert got.dtype == np.float32 and np.array_equal(got, want), T.describe(got, want)


def _generator_lines(Y, grid, edt, n_rays=None, rays=None, anisotropy=None):
    """model2d.py:64-103 / model3d.py:69-104, in the reference's order of statements, on the oracle pieces"""
    from oracle import port
    nd = Y[0].ndim
    ss = tuple(slice(0, None, g) for g in grid)
    mask_neg_labels = tuple(y[ss] < 0 for y in Y)                                                   # :64 / :69
    has_neg_labels = any(m.any() for m in mask_neg_labels)
    if has_neg_labels:
        mask_neg_labels = np.stack(mask_neg_labels)
        Y = tuple(np.maximum(y, 0) for y in Y)                                                      # :69 / :77
    if nd == 2:
        prob = np.stack([edt(lbl[ss], None) for lbl in Y])                                          # :71
        dist = np.stack([port.star_dist(lbl, n_rays, grid=grid) for lbl in Y])                      # :82
    else:
        prob = np.stack([edt(lbl, anisotropy)[ss] for lbl in Y])                                    # :86
        dist = np.stack([port.star_dist3D(lbl, rays.vertices, grid=grid) for lbl in Y])             # :92
    prob = np.expand_dims(prob, -1)
    R = dist.shape[-1]
    dist_and_mask = np.empty(dist.shape[:-1] + (R + 1,), np.float32)                                # :98-100 / :101
    dist_and_mask[..., :-1] = dist
    dist_and_mask[..., -1:] = prob
    if has_neg_labels:
        prob[mask_neg_labels] = -1                                                                  # :103 / :104
    return prob[..., 0], dist_and_mask


@pytest.mark.parametrize("id", T.ids(T.BATCH2D + T.BATCH3D))
def test_batch_reference_equals_generator_lines(refmods, id):
    from oracle import port
    c = T.BY_ID[id]
    Y = T.labels(id)
    small = Y[0].size <= 10000

    def edt(a, an):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return port.edt_prob(a, anisotropy=an) if small else T.edt_prob_box(a, an)
    prob, dtm = _generator_lines(Y, c["grid"], edt, n_rays=c.get("n_rays"), rays=c["rays"]() if "rays" in c else None, anisotropy=c.get("aniso"))
    wp, wd = T.batch_want(id)
    assert np.array_equal(wp, prob), T.describe(wp, prob)
    assert np.array_equal(wd, dtm), T.describe(wd, dtm)
    # every item takes the branch it is meant to take, in the reference's terms
    nd = Y[0].ndim
    ss = tuple(slice(0, None, g) for g in c["grid"])
    clips = any((np.asarray(y)[ss] < 0).any() for y in Y)
    seen = tuple(T.batch_branch(np.maximum(y, 0) if clips else y, c["grid"], nd) for y in Y)
    assert seen == c["want"], (id, seen)
    assert ("negon" in id or "clips" in id) == clips
    if "negoff" in id and not clips:
        assert any((np.asarray(y) < 0).any() for y in Y)                       # negative ids that only lie off the grid reach the kernels ...
        assert (T._as_u16(Y[0]) == 65535).any()                                 # ... as 65535 in star_dist
        assert (wp >= 0).all()


def test_batches_cover_every_branch_dtype_and_grid():
    for L, grids in ((T.BATCH2D, {(1, 1), (2, 2), (2, 4)}), (T.BATCH3D, {(1, 1, 1), (1, 2, 2), (2, 2, 2)})):
        assert {b for c in L for b in c["want"]} == {"plain", "empty", "constant", "sparse"}
        assert grids <= {tuple(c["grid"]) for c in L}
        assert {np.dtype(np.uint16), np.dtype(np.int32), np.dtype(np.int64)} <= {np.asarray(y).dtype for c in L for y in T.labels(c["id"])}
        assert all(3 <= len(T.labels(c["id"])) <= 4 for c in L)
    assert {c["aniso"] is None for c in T.BATCH3D} == {True, False}


def _spans(lab, axis):
    """some object covers a whole line along `axis` (it reaches both borders there)"""
    return lab.shape[axis] > 1 and any((lab == l).all(axis=axis).any() for l in np.unique(lab) if l > 0)


def test_edt_regimes_are_reached():
    L2, L3 = {c["id"]: T.labels(c["id"]) for c in T.EDT2D}, {c["id"]: T.labels(c["id"]) for c in T.EDT3D}
    for a in range(2):
        assert any(_spans(l, a) for l in L2.values()), a
    for a in range(3):
        assert any(_spans(l, a) for l in L3.values()), a
    assert _spans(L3["edt3-band-zx-a2"], 0) and _spans(L3["edt3-band-zx-a2"], 2)            # one object that spans two axes
    assert _spans(L2["edt2-256-band"], 1) and _spans(L3["edt3-train-a3"], 0) and _spans(L3["edt3-train-a3"], 2)
    big = L2["edt2-2048"]
    assert big.shape == (2048, 2048) and (big[940:1061, 1040:1161] == 1).all()             # the centre of object 1 is > 60 px from any other pixel
    assert 1 in T.BY_ID["edt2-2048"]["ids"] and len(T.BY_ID["edt2-2048"]["ids"]) > 30
    assert L2["edt2-256-a0"].shape == (256, 256) and L3["edt3-train-a0"].shape == (48, 96, 96)
    assert max(int((L2["edt2-256-a0"] == l).any(0).sum()) for l in range(1, 11)) > 64          # wider than the early stop's first steps
    assert {l.shape[-1] for l in L2.values()} >= {1} and {l.shape[0] for l in L2.values()} >= {1}
    for a in range(3):
        assert any(l.shape[a] == 1 for l in L3.values()), a
    for id in ("edt2-one-bg-a0", "edt3-one-bg-a0"):
        lab = {**L2, **L3}[id]
        assert (lab == 0).sum() == 1 and (lab == 1).sum() == lab.size - 1
    for id in ("edt2-one-obj2-a0", "edt3-one-obj2-a0"):
        lab = {**L2, **L3}[id]
        assert (lab == 2).sum() == 1 and (lab == 1).sum() == lab.size - 1
    for id in ("edt2-voronoi-a0", "edt3-voronoi-a0", "edt2-256-voronoi"):
        assert ({**L2, **L3}[id] > 0).all()
    ring = L2["edt2-annulus-a0"]
    cy, cx = ring.shape[0] // 2, ring.shape[1] // 2
    assert ring[cy, cx] == 2 and (ring[cy, :cx] == 1).any() and (ring[cy, cx:] == 1).any() and (ring[:cy, cx] == 1).any()     # a hole, filled by another object
    cs = L2["edt2-cshape-a0"]
    assert (cs == 1).sum() < (ring == 1).sum() and not (cs[cy, cx + 3:] == 1).any() and (cs[cy, :cx] == 1).any()           # the ring with a gap
    two = L2["edt2-twocomp-a0"]
    row = two[-1]
    assert row[0] == 1 and row[-1] == 1 and (row == 2).any() and (row == 0).any()                # 1 | 0 | 2 | 0 | 1 along the last row
    ch = L2["edt2-checker-a0"]
    assert len(np.unique(ch)) == (ch > 0).sum() + 1 and (ch[::2, 1::2] == 0).all()
    bd = L2["edt2-borders-a0"]
    assert all(bd[p] > 0 for p in ((0, 0), (0, -1), (-1, 0), (-1, -1), (0, bd.shape[1] // 2), (bd.shape[0] // 2, 0)))
    dy = lambda a: a is not None and all(float(v * 8).is_integer() for v in a)                   # noqa: E731
    for L in (T.EDT2D, T.EDT3D):
        kinds = {("none" if c["aniso"] is None else "dyadic" if dy(c["aniso"]) else "other") for c in L}
        assert kinds == {"none", "dyadic", "other"}
    assert any(c["aniso"] == (7.14, 1.0, 1.09) for c in T.EDT3D) and any(c["aniso"] == (1.9, 1.1, 0.7) for c in T.EDT3D)
    assert any("const" in c["id"] for c in T.EDT2D) and any("const" in c["id"] for c in T.EDT3D)


def test_star_dist_regimes_are_reached():
    c = T.BY_ID["sd2-2048"]
    assert 2048 * 2048 * c["n_rays"] > 2 * T.GRID_CAP_THREADS * 8                                # > 16 trips of the stride loop
    assert 256 * 256 * 32 == T.GRID_CAP_THREADS                                                  # the training patch sits exactly at the cap
    assert {c["n_rays"] for c in T.SD2D} >= {1, 3, 4, 6, 12, 17, 32, 64, 300}
    assert {tuple(c["grid"]) for c in T.SD2D} >= {(1, 1), (2, 2), (1, 4), (3, 1), (4, 4)}
    for c in T.SD2D:
        if c["id"].startswith("sd2-g"):
            assert all(s % g for s, g in zip(T.labels(c["id"]).shape, c["grid"]) if g > 1)    # extents the grid does not divide
    assert T.labels("sd2-h1").shape[0] == 1 and T.labels("sd2-w1").shape[1] == 1
    wide = T.labels("sd2-wide-ids")
    assert {65535, 65536, 65537, 131073} <= set(np.unique(wide).tolist())
    assert set(np.unique(T._as_u16(wide)).tolist()) == {0, 1, 65535}                             # 65536 is background, 65537 and 131073 are 1
    relabelled = np.unique(wide, return_inverse=True)[1].reshape(wide.shape)
    assert not np.array_equal(T.sd_want("sd2-wide-ids"), T.star_dist2d_np(relabelled, 16))       # the wrapped ids really collide
    assert (T.sd_want("sd2-wide-ids")[wide == 65536] == 0).all()
    bd = T.labels("sd2-borders")
    assert all(bd[p] > 0 for p in ((0, 0), (0, -1), (-1, 0), (-1, -1)))
    c3 = T.BY_ID["sd3-train"]
    assert T.labels("sd3-train").shape == (48, 96, 96) and len(c3["rays"]()) == 96 and c3["grid"] == (1, 2, 2)
    f = T.labels("sd3-faces")
    for a in range(3):
        assert (np.take(f, 0, axis=a) > 0).any() and (np.take(f, -1, axis=a) > 0).any()
    V = T.lattice_rays().vertices
    assert len(V) == 124 and set(np.unique(V).tolist()) == {-1.0, -0.5, 0.0, 0.5, 1.0}


def test_half_steps_are_taken():
    """see the module docstring: which n_rays give a component of exactly 0.5 with this C library, and that the case visits .5 coordinates"""
    exact = {R: bool((np.abs(np.concatenate(T.dirs2d(R))) == np.float32(0.5)).any()) for R in (6, 12)}
    print("components of exactly 0.5:", exact)
    assert exact[12], exact
    cos, sin = T.dirs2d(12)
    k = int(np.flatnonzero(np.abs(sin) == np.float32(0.5))[0])
    x = np.cumsum(np.full(9, sin[k], np.float32), dtype=np.float32)
    assert (x[::2] % 1 == 0.5).all()                                                             # .5, 1.5, ...: ties for lrint at every other step
    assert T.BY_ID["sd2-r12"]["n_rays"] == 12 and (T.labels("sd2-r12") > 0).sum() > 200
    # the rounding mode matters on the case itself: round-half-away gives another result
    lab = T.labels("sd2-r12")
    rint = np.rint
    try:
        np.rint = lambda a: np.where(a >= 0, np.floor(a + np.float32(0.5)), np.ceil(a - np.float32(0.5)))
        other = T.star_dist2d_np(lab, 12)
    finally:
        np.rint = rint
    assert not np.array_equal(other, T.sd_want("sd2-r12"))
