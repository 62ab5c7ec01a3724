"""CPU: the case lists of test_gpu_unet_ops_exact.py (_unet_ops_cases.py) reach the regimes their names claim -- from the launch
arithmetic of stardist_amd/csrc/unet_ops.hip restated there and checked here against the source text -- and its references are right:
the pooling reference against torch's CPU max-pool, the up-sampling + concatenation against torch.nn.Upsample + torch.cat, the integer
head references against float64, with the exactness preconditions of the integer family."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_cases as CC
import _unet_ops_cases as K


def test_restated_constants_match_the_source():
    caps, per_block, dot_threads, lds = K.source_constants()
    assert caps == K.CAP
    assert per_block == K.PER_BLOCK
    assert dot_threads == 256 and lds == K.HEAD_LDS
    assert K.per_pass("maxpool") == K.per_pass("maxpool_split16") == K.per_pass("pack") == K.per_pass("unpack") == 4194304
    assert K.per_pass("upcat") == 262144 * 256 and K.per_pass("bias_act_cl4") == 65536 * 256
    assert [K.per_pass("bias_act_dot", C) for C in (32, 64, 128, 256)] == [8192 * 32, 8192 * 16, 8192 * 8, 8192 * 4]
    assert K.per_pass("dot_combine") == 262144 and K.per_pass("head_rows") == 98304


def test_a_changed_cap_is_noticed(tmp_path):
    src = open(K.SOURCE).read()
    changed = src.replace("if (blocks > 262144) blocks = 262144;", "if (blocks > 131072) blocks = 131072;")
    assert changed != src
    p = tmp_path / "unet_ops.hip"
    p.write_text(changed)
    assert K.source_constants(str(p))[0] != K.CAP


def test_pool_cases_reach_their_regimes():
    small = K.POOL_SMALL
    assert {c.pool for c in small} == {(1, 2, 2), (2, 2, 2), (1, 4, 2)} and any(c.shape[0] > 1 and c.pool[0] == 1 for c in small)
    assert {c.C for c in small} == {4, 32, 48, 96, 128}
    for c in small:                                                        # a remainder on every pooled axis
        assert all(s % p for s, p in zip(c.shape, c.pool) if p > 1), c
        assert K.loops("maxpool", K.pool_items(c, False)) == c.loops == 1
    for cases, split, kernel in ((K.POOL_LOOP_F32, False, "maxpool"), (K.POOL_LOOP_SPLIT, True, "maxpool_split16")):
        assert [c.loops for c in cases] == [1, 2, 3]
        for c in cases:
            assert all(s % p for s, p in zip(c.shape, c.pool) if p > 1)
            assert K.loops(kernel, K.pool_items(c, split)) == c.loops, (c, K.passes(kernel, K.pool_items(c, split)))
        assert K.passes(kernel, K.pool_items(cases[0], split)) == 1.0     # exactly one pass: the last thread of the last block has work
        assert 1 < K.passes(kernel, K.pool_items(cases[1], split)) < 2 and K.passes(kernel, K.pool_items(cases[2], split)) > 2
    b = K.POOL_BIG
    assert int(np.prod(b.shape)) * b.C > 1 << 31 and b.pool == (2, 2, 2)


def test_upcat_pack_and_bias_act_cases_reach_their_regimes():
    assert {c.up for c in K.UPCAT if c.shape[0] > 1} == set(range(1, 8)) and {c.up for c in K.UPCAT if c.shape[0] == 1} >= {1, 2, 3}
    assert {(c.ca, c.cb) for c in K.UPCAT} == {(96, 48), (48, 96), (4, 4), (128, 64)}
    for c in K.UPCAT:
        assert K.loops("upcat", K.upcat_items(c)) == c.loops, c
        assert not any((c.up >> k) & 1 and c.shape[2 - k] % 2 for k in range(3))
    assert any(c.loops == 2 for c in K.UPCAT)
    assert any(c.shape[1] == c.shape[2] and c.up in (1, 2) for c in K.UPCAT) and any(c.shape[1] != c.shape[2] and c.up in (1, 2) for c in K.UPCAT)
    u = K.UPCAT_BIG
    assert int(np.prod(u.shape)) * (u.ca + u.cb) * 4 > 1 << 32
    packs = K.pack_cases()
    assert {C for _, C in packs} == {32, 96, 256}
    for C in (32, 96, 256):
        got = sorted(K.passes("pack", n * (C // 8)) for n, c in packs if c == C)
        assert got[0] < 1 and got[-1] > 1 and (C == 96 or 1.0 in got), (C, got)
    for c in K.BIAS_ACT:
        assert K.loops(c.path, K.bias_act_items(c)) == c.loops, c
        cl4 = c.inner == 1 and c.C % 4 == 0 and not any(c.offset)
        assert (c.path == "bias_act_cl4") == cl4
    assert {c.path for c in K.BIAS_ACT if c.loops == 2} == {"bias_act_cl4", "bias_act"}
    assert any(c.C % 2 for c in K.BIAS_ACT) and any(c.inner > 1 for c in K.BIAS_ACT)
    assert {c.offset for c in K.BIAS_ACT} >= {(1, 0, 0), (0, 1, 0), (0, 0, 1)}                       # each pointer misaligned on its own
    assert K.BIAS_ACT_BIG.n_outer * K.BIAS_ACT_BIG.C > 1 << 31


def test_head_cases_reach_their_regimes():
    assert {C for C, _ in K.DOT} == {32, 64, 128, 256}
    for C in (32, 64, 128, 256):
        p = sorted(K.passes("bias_act_dot", n, C) for c, n in K.DOT if c == C)
        assert p[0] == 1.0 and p[1] == 2.0 and 2 < p[2] < 3
    assert {n % 32 for n in K.COMBINE_N} == set(range(32))
    assert min(K.COMBINE_N) < K.per_pass("dot_combine") < max(K.COMBINE_N) and K.per_pass("dot_combine") in K.COMBINE_N
    assert {K.head_ct(R) for _, R in K.HEAD} == {1, 2, 3, 4} and {R for _, R in K.HEAD} == {7, 32, 33, 64, 96, 100}
    assert {C for C, _ in K.HEAD} == {32, 64, 128, 256} and (64, 100) in K.HEAD
    assert all(K.head_lds(C, R) <= K.HEAD_LDS and C % 8 == 0 for C, R in K.HEAD)
    assert {n % 32 for n in K.HEAD_RESIDUES} == set(range(32)) and {1, 31, 32, 33} <= set(K.HEAD_RESIDUES)
    assert 2 < K.passes("head_rows", K.HEAD_LOOP_ROWS) < 3
    sets = K.head_row_sets(K.HEAD_N_PIX, 1)
    assert sorted(sets["permutation"]) == list(range(K.HEAD_N_PIX)) and bool((np.diff(sets["descending"]) == -1).all())
    assert len(set(sets["all equal"])) == 1 and len(set(sets["duplicates"])) < len(sets["duplicates"])


def test_special_data_holds_what_it_claims():
    pool = (2, 2, 2)
    x = K.special_values((8, 10, 12, 32), 3, pool)
    assert not np.isnan(x).any()
    v = x.reshape(4, 2, 5, 2, 6, 2, 32).transpose(0, 2, 4, 6, 1, 3, 5).reshape(-1, 8)
    bits = v.view(np.uint32)
    neg0, pos0 = bits == 0x80000000, bits == 0
    assert (neg0.any(1) & pos0.any(1)).any()                                               # -0.0 and +0.0 in one window
    assert ((neg0 | pos0).all(1) & neg0.any(1) & pos0.any(1)).any()                        # ... and nothing else
    assert (v < 0).all(1).any() and np.isneginf(v).all(1).any() and np.isposinf(v).any()   # all-negative windows, one of -inf only
    assert ((v[:, :1] == v).all(1) & (v[:, 0] != 0)).any()                                 # ties
    tiny = (np.abs(v) < np.finfo(np.float32).tiny) & (v != 0)
    assert tiny.all(1).any()                                                               # denormals only
    assert (x == K.F16_MAX).any() and (x == K.ABOVE_F16_MAX).any() and float(K.ABOVE_F16_MAX) > 65504.0
    assert np.float16(K.F16_MAX) == np.float16(65504) and np.isinf(K.np_split16(np.full((1, 32), 65520.0, np.float32)).view(np.float16)[0, 0])
    y = K.with_nans(x, 4, pool)
    w = y.reshape(4, 2, 5, 2, 6, 2, 32).transpose(0, 2, 4, 6, 1, 3, 5).reshape(-1, 8)
    n = np.isnan(w)
    sign = w.view(np.uint32) >> 31
    assert n.all(1).any() and (n.sum(1) == 1).any() and (n & (sign == 1)).any() and (n & (sign == 0)).any()
    rng = np.random.RandomState(5)
    a, b = rng.randint(-1, 2, (50, 64)).astype(np.float32), rng.randint(-1, 2, (50, 64)).astype(np.float32)
    want = CC.two_scale(torch.from_numpy(a), torch.from_numpy(b)).numpy()
    assert np.array_equal(K.two_scale_values((50, 64), 5).view(np.uint32), want.view(np.uint32))    # the family of _conv_cases.two_scale


@pytest.mark.parametrize("c", K.POOL_SMALL, ids=lambda c: c.name)
def test_pool_reference_equals_torch(c):
    """data without NaN and without zeros of both signs in one window (where torch's order is open)"""
    x = K.special_values(c.shape + (c.C,), 7, c.pool)
    x[x == 0] = 0.0
    x = K.fill_remainder(x, c.pool, np.float32(np.inf))
    got = K.pool_ref(x, c.pool)
    t = torch.from_numpy(x).permute(3, 0, 1, 2)[None]
    want = F.max_pool3d(t, c.pool)[0].permute(1, 2, 3, 0).numpy()
    assert got.shape == K.pool_out_shape(c) + (c.C,)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    other = K.fill_remainder(x.copy(), c.pool, np.float32(-3.0e38))                         # the remainder is not read: any sentinel, the same result
    assert np.array_equal(K.pool_ref(other, c.pool).view(np.uint32), got.view(np.uint32))


def test_pool_reference_orders_zeros_and_propagates_nan():
    z = np.array([-0.0, 0.0, -0.0, -1.0], np.float32)
    for perm in ([0, 1, 2, 3], [1, 0, 3, 2], [3, 2, 1, 0]):
        x = z[perm].reshape(1, 2, 2, 1)
        assert K.pool_ref(x, (1, 2, 2)).view(np.uint32).item() == 0                        # +0 beats -0 wherever it stands
    assert K.pool_ref(np.array([-0.0, -1.0, -0.0, -np.inf], np.float32).reshape(1, 2, 2, 1), (1, 2, 2)).view(np.uint32).item() == 0x80000000
    for nan in np.array([0x7FC00000, 0xFFC00000], np.uint32).view(np.float32):
        x = np.array([np.inf, nan, -1.0, 2.0], np.float32).reshape(1, 2, 2, 1)
        assert np.isnan(K.pool_ref(x, (1, 2, 2))).all()
    assert np.isnan(K.pool_ref(np.full((1, 2, 2, 1), np.nan, np.float32), (1, 2, 2))).all()
    k = K.order_key(np.array([-np.inf, -1.0, -1e-40, -0.0, 0.0, 1e-40, 1.0, np.inf], np.float32))
    assert bool((np.diff(k.astype(np.int64)) > 0).all())
    assert K.same_bits(np.array([np.nan, 1.0, -0.0], np.float32), np.array([-np.nan, 1.0, 0.0], np.float32)).tolist() == [True, True, False]


@pytest.mark.parametrize("c", [c for c in K.UPCAT if c.loops == 1], ids=lambda c: "%s %d+%d" % (c.name, c.ca, c.cb))
def test_upcat_reference_equals_torch(c):
    D, H, W = c.shape
    sa = (D >> ((c.up >> 2) & 1), H >> ((c.up >> 1) & 1), W >> (c.up & 1))
    a, b = K.special_values(sa + (c.ca,), 1), K.special_values(c.shape + (c.cb,), 2)
    got = K.upcat_ref(a, b, c.up)
    ta, tb = torch.from_numpy(a).permute(3, 0, 1, 2)[None], torch.from_numpy(b).permute(3, 0, 1, 2)[None]
    scale = tuple(float(s // q) for s, q in zip(c.shape, sa))
    want = torch.cat([torch.nn.Upsample(scale_factor=scale, mode="nearest")(ta), tb], 1)[0].permute(1, 2, 3, 0).numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_split16_of_special_values():
    x = K.special_values((40, 64), 9)
    x = np.where(np.abs(x) <= K.F16_MAX, x, np.float32(1.0))
    back = K.np_unsplit16(K.np_split16(x))
    assert bool((np.abs(back.astype(np.float64) - x) <= 2.0 ** -22 * np.abs(x) + 2.0 ** -36).all())     # the 22 bits, and the floor of subnormal terms
    big = np.abs(x) >= 2.0 ** -24
    assert np.array_equal(np.signbit(back[big]), np.signbit(x[big]))
    t = K.two_scale_values((50, 64), 5)
    assert np.array_equal(K.np_unsplit16(K.np_split16(t)).view(np.uint32), t.view(np.uint32))
    inf = K.np_split16(np.full((1, 32), np.inf, np.float32)).view(np.float16)
    assert np.isposinf(inf[0, :32]).all() and np.isnan(inf[0, 32:]).all()                # the pair of an infinity: (inf, NaN)


def test_bias_act_reference():
    x, y, b = K.special_values((50, 8, 1), 1), K.special_values((50, 8, 1), 2), K.special_values((8,), 3)
    with np.errstate(invalid="ignore", over="ignore"):
        want = torch.relu(torch.from_numpy((x + y) + b.reshape(1, 8, 1))).numpy()
    got = K.bias_act_ref(x, y, b, 1)
    ok = ~np.isnan(want)                                                                 # torch's ReLU keeps a NaN; the kernels' gives +0
    assert np.array_equal(got[ok], want[ok]) and bool((got[~ok].view(np.uint32) == 0).all()) and (~ok).any()
    assert bool((K.relu_ref(np.array([-0.0, np.nan, -1.0], np.float32)).view(np.uint32) == 0).all())


def test_integer_head_references_are_exact():
    for C in (32, 256):
        x, b, w, wb = K.dot_data(C, 1000, C)
        for act in (0, 1):
            f, d = K.dot_ref(x, b, act, w, wb)
            f64 = x.astype(np.float64) + b
            f64 = np.maximum(f64, 0) if act else f64
            assert np.array_equal(f, f64) and np.array_equal(d, f64 @ w.astype(np.float64) + float(wb))
            terms = K.lane_terms(f, w)
            assert np.array_equal(K.butterfly_ref(terms, wb), d.astype(np.float32))       # any order: the same float32
            assert np.array_equal(terms.astype(np.float64).sum(1) + float(wb), d)
    with pytest.raises(AssertionError):
        K.dot_ref(np.full((2, 32), 2.0 ** 20, np.float32), None, 0, np.ones(32, np.float32), 0)
    for C, R in K.HEAD:
        feat, W, b = K.head_data(C, R, 300, C + R)
        rows = K.head_row_sets(300, 2)["permutation"][:100]
        want = np.maximum(feat[rows].astype(np.float64) @ W.astype(np.float64).T + b, 1.0)
        assert np.array_equal(K.head_ref(feat, rows, W, b, 1.0), want.astype(np.float32)) and float(want.min()) == 1.0 < float(want.max())
        assert float(K.head_ref(feat, None, W, None, -np.inf).min()) < 0
    # float data: the butterfly order is one definite float32 sum, and it is not the sequential one
    rng = np.random.RandomState(1)
    t = rng.standard_normal((2000, 32)).astype(np.float32)
    seq = t[:, 0].copy()
    for k in range(1, 32):
        seq = seq + t[:, k]
    bf = K.butterfly_ref(t, 0.0)
    assert float(np.abs(bf.astype(np.float64) - t.astype(np.float64).sum(1)).max()) < 1e-5 and not np.array_equal(bf, seq)


def test_marks():
    per_plane = 416 * 416 * 32
    m = K.marks(416, per_plane, 1)
    assert 0 in m and 415 in m and (1 << 31) // per_plane in m and all(0 <= p < 416 for p in m)
