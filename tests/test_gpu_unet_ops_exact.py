"""GPU: the kernels between the convolutions (stardist_amd/csrc/unet_ops.hip), through the C ABI, compared EXACTLY -- bit patterns, no
tolerance except the logistic function's -- with plain numpy references on the CPU (_unet_ops_cases.py; test_cpu_unet_ops_cases.py
proves the references and the regimes of the case lists without a GPU).

  * every kernel is a grid-stride loop under a block cap: each has a case inside one pass, at its boundary and over it
  * data: special values (ties, zeros of both signs, infinities, all-negative windows, denormals, the fp16 range edge), NaNs of both
    signs, the two-scale family, and for the heads integers whose sums are exact in any order (reference: an int64 matmul)
  * every output starts as a NaN bit pattern that no kernel produces; one guard element behind it, inside the same allocation, must
    still hold that pattern afterwards
  * offsets past 2^31 and 2^32 elements, compared on planes at the ends and around the marks (skipped when the device is too small)
  * the special-value rule of include/stardist_hip.h: max-pooling propagates a NaN of either sign in both forms, the range flags of
    sd_split16_pack_device and of the convolution's split16 output treat a NaN alike."""
import ctypes

import numpy as np
import pytest
import torch

import _unet_ops_cases as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 0x7FC5A5A5                                  # a NaN (two fp16 halves: a NaN and an ordinary number) no kernel writes
NEG_INF = float("-inf")


def _call(name, *args):
    from stardist_amd.lib import _native as N
    N.dcall(torch.empty(0, device=DEV), name, *args)


def _vp(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Out:
    """n float32 outputs pre-filled with SENTINEL, and four guard words behind them inside the same allocation"""

    def __init__(self, n):
        self.buf = torch.empty(n + 4, dtype=torch.int32, device=DEV).fill_(SENTINEL)
        self.t = self.buf[:n].view(torch.float32)

    def check(self, what):
        assert bool((self.buf[-4:] == SENTINEL).all()), "%s: written past the end" % what
        left = int((self.buf[:-4] == SENTINEL).sum())
        assert left == 0, "%s: %d of %d elements were not written" % (what, left, self.buf.numel() - 4)

    def numpy(self, shape):
        return self.t.cpu().numpy().reshape(shape)


def _same(got, want, what, half=False, origin=None):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = K.same_bits(got, want, half)
    if ok.all():
        return
    if half:
        got, want = got.view(np.float16), want.view(np.float16)
    bad = np.argwhere(~ok)
    u = np.uint16 if half else np.uint32
    first = [(tuple(int(v) for v in ix), "%x" % got.view(u)[tuple(ix)], "%x" % want.view(u)[tuple(ix)], float(got[tuple(ix)]), float(want[tuple(ix)]))
             for ix in bad[:6]]
    pytest.fail("%s: %d of %d elements differ%s; (index, got bits, want bits, got, want): %r" % (
        what, len(bad), ok.size, "" if origin is None else " (rows / planes %s)" % (origin,), first))


def _need(gb):
    free = torch.cuda.mem_get_info()[0]
    if free < gb * 1e9:
        pytest.skip("needs %d GB of free device memory, the device reports %.1f GB" % (gb, free / 1e9))


# ---- max pooling -----------------------------------------------------------------------------------------------------------------
def _pool(xd, shape, C, pool, split):
    """xd: device tensor (D, H, W, C) (split16 words when split) -> Out of the pooled tensor"""
    O = tuple(s // p for s, p in zip(shape, pool))
    out = Out(int(np.prod(O)) * C)
    _call("sd_maxpool_split16_ndhwc_device" if split else "sd_maxpool_ndhwc_device", _vp(xd), C, *shape, *pool, _vp(out.t))
    return out, O + (C,)


def _pack(xd, C, flag=None):
    out = Out(xd.numel())
    _call("sd_split16_pack_device", _vp(xd), xd.numel() // C, C, _vp(out.t), _vp(flag))
    return out


def _unpack(sd, C):
    out = Out(sd.numel())
    _call("sd_split16_unpack_device", _vp(sd), sd.numel() // C, C, _vp(out.t))
    return out


def _pool_families(c):
    shape = c.shape + (c.C,)
    yield "special", K.fill_remainder(K.special_values(shape, 11, c.pool), c.pool, np.float32(np.nan))
    yield "nan", K.fill_remainder(K.with_nans(K.special_values(shape, 12, c.pool), 13, c.pool), c.pool, np.float32(3.0e38))
    yield "two-scale", K.fill_remainder(K.two_scale_values(shape, 14), c.pool, np.float32(np.inf))


@pytest.mark.parametrize("c", K.POOL_SMALL, ids=lambda c: c.name)
def test_max_pool_special_values(c):
    """f32, and for channel counts in 32-channel chunks split16 (== the split of the f32 reference), with the remainder behind the last
    whole window holding what must not be read: a NaN, or a value above everything else"""
    for family, x in _pool_families(c):
        want = K.pool_ref(x, c.pool)
        assert np.isnan(want).any() == (family == "nan")
        xd = _dev(x)
        out, oshape = _pool(xd, c.shape, c.C, c.pool, False)
        out.check("f32 %s %s" % (family, c.name))
        _same(out.numpy(oshape), want, "f32 %s %s" % (family, c.name))
        if c.C % 32 == 0:
            packed = _pack(xd, c.C)
            packed.check("pack %s %s" % (family, c.name))
            _same(packed.numpy(x.shape), K.np_split16(x), "pack %s %s" % (family, c.name), half=True)
            out, oshape = _pool(packed.t, c.shape, c.C, c.pool, True)
            out.check("split16 %s %s" % (family, c.name))
            _same(out.numpy(oshape), K.np_split16(want), "split16 %s %s" % (family, c.name), half=True)


def test_max_pool_nan_rule_small_windows():
    """the rule itself on three windows per form: nothing but NaN, one positive NaN, one negative NaN (beside +inf and -inf)"""
    nan_p, nan_n = np.array([0x7FC00000, 0xFFC00000], np.uint32).view(np.float32)
    x = np.zeros((1, 2, 6, 32), np.float32)
    x[0, :, 0:2] = nan_p
    x[0, :, 2:4] = np.array([[np.inf, nan_p], [1.0, -np.inf]], np.float32)[:, :, None]
    x[0, :, 4:6] = np.array([[-np.inf, -np.inf], [nan_n, -np.inf]], np.float32)[:, :, None]
    xd = _dev(x)
    out, oshape = _pool(xd, (1, 2, 6), 32, (1, 2, 2), False)
    got = out.numpy(oshape)
    print("f32 pool: all-NaN window, one +NaN, one -NaN ->", got[0, 0, :, 0])
    sp, _ = _pool(_pack(xd, 32).t, (1, 2, 6), 32, (1, 2, 2), True)
    gs = sp.numpy(oshape).view(np.float16).reshape(3, 64)
    print("split16 pool (hi, lo') ->", gs[:, 0], gs[:, 32])
    assert np.isnan(got).all() and np.isnan(gs).all()


def _int_tensor(shape, seed, lo=-3, hi=4):
    """device float32 tensor of small integers (ties everywhere), generated on the device in slabs along the first axis"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.empty(shape, dtype=torch.float32, device=DEV)
    flat = x.view(shape[0], -1)
    step = max(1, (1 << 28) // flat.shape[1])
    for z in range(0, shape[0], step):
        n = min(step, shape[0] - z)
        flat[z:z + n] = torch.randint(lo, hi, (n, flat.shape[1]), generator=g, device=DEV, dtype=torch.int16).float()
    return x


@pytest.mark.parametrize("split", [False, True], ids=["f32", "split16"])
@pytest.mark.parametrize("k", range(3), ids=["one pass exactly", "two passes, ragged", "three passes"])
def test_max_pool_grid_stride_loop(k, split):
    """integer data made on the device; every element must be written (no sentinel left), and every output row is compared, in slabs of
    rows, with the reference of the input rows copied back"""
    c = (K.POOL_LOOP_SPLIT if split else K.POOL_LOOP_F32)[k]
    kernel = "maxpool_split16" if split else "maxpool"
    assert K.loops(kernel, K.pool_items(c, split)) == c.loops
    _, H, W = c.shape
    xd = _int_tensor((1, H, W, c.C), 20 + k)
    xd[0, (H // 2) * 2:] = 100.0                                                # the remainder: above everything else
    xd[0, :, (W // 2) * 2:] = 100.0
    src = _pack(xd, c.C).t if split else xd
    out, oshape = _pool(src, c.shape, c.C, c.pool, split)
    out.check("%s %s" % (kernel, c.name))
    o = out.t.view(oshape)[0]
    for r0 in range(0, oshape[1], 128):
        r1 = min(r0 + 128, oshape[1])
        want = K.pool_ref(xd[:, 2 * r0:2 * r1].cpu().numpy(), c.pool)[0]
        assert float(want.max()) <= 3.0
        _same(o[r0:r1].cpu().numpy(), K.np_split16(want) if split else want, "%s %s" % (kernel, c.name), half=split, origin=(r0, r1))


# ---- split16 pack / unpack -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pix,C", K.pack_cases(), ids=str)
def test_pack_unpack_around_a_pass_boundary(n_pix, C):
    """two-scale values (both terms carry weight) with the special values in the first and last pixels and around the boundary"""
    x = K.two_scale_values((n_pix, C), n_pix % 1000 + C)
    edge = K.per_pass("pack") // (C // 8)
    for p0 in (0, edge - 3, n_pix - 6):
        m = min(6, n_pix - p0)
        x[p0:p0 + m] = K.with_nans(K.special_values((m, C), p0 % 97), 5)
    x[1, 0] = np.inf
    xd = _dev(x)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    packed = _pack(xd, C, flag)
    packed.check("pack")
    s = packed.numpy(x.shape)
    want = K.np_split16(x)
    _same(s, want, "pack", half=True)
    assert int(flag.item()) == 2                                               # the infinities and the value above 65504
    back = _unpack(packed.t, C)
    back.check("unpack")
    _same(back.numpy(x.shape), K.np_unsplit16(want), "unpack")


def test_range_flags_treat_nan_alike():
    """a NaN is not a range error: neither sd_split16_pack_device nor the split16 output of a convolution raises the flag for it (it
    stays a NaN in the tensor); an infinity and a value above 65504 raise both"""
    from stardist_amd.models import unet as U
    x = K.two_scale_values((500, 32), 1)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    for value, want in ((np.nan, 0), (-np.nan, 0), (np.inf, 2), (K.ABOVE_F16_MAX, 2), (K.F16_MAX, 0)):
        y = x.copy()
        y[250, 7] = value
        flag.zero_()
        s = _pack(_dev(y), 32, flag).numpy(y.shape).view(np.float16).reshape(500, 64)
        assert int(flag.item()) == want, (value, int(flag.item()))
        assert np.isnan(s[250, 7]) == np.isnan(value)
    xt = _dev(K.two_scale_values((1, 40, 64, 32), 2)).permute(0, 3, 1, 2)
    for value, want in ((float("nan"), 0), (float("inf"), 2), (7.0e4, 2)):
        conv = torch.nn.Conv2d(32, 32, 3, padding=1).to(DEV)
        with torch.no_grad(), U.force_conv_mode("f16x3"):
            conv.weight.zero_(); conv.bias.zero_(); conv.bias[5] = value
            conv.__dict__["_sd_split_out"] = True
            U.range_flag(DEV).zero_()
            y = U._hand_conv(conv, [(xt, 0)], 0)                              # linear: the bias reaches the output as it is
            got = int(U.range_flag(DEV).item())
            U.range_flag(DEV).zero_()
        assert U.is_split16(y) and (got & 2) == want, (value, got)
        h = y.permute(0, 2, 3, 1).contiguous().cpu().numpy().view(np.float16).reshape(-1, 64)
        assert np.isnan(h[:, 5]).all() == (value != value)


def test_split16_pool_keeps_the_first_of_two_pairs_with_one_key():
    """two pairs with the same value and the same hi differ only in the sign of a zero lo' (the producers never write -0 there): the
    first in scan order (dy, dx) is copied"""
    words = np.zeros((2, 2, 64), np.float16)
    words[..., :32] = 1.0
    words[0, 0, 32:] = -0.0
    for flip in (False, True):
        w = words[::-1, ::-1] if flip else words
        out, _ = _pool(_dev(np.ascontiguousarray(w).view(np.float32).reshape(1, 2, 2, 32)), (1, 2, 2), 32, (1, 2, 2), True)
        got = out.numpy((64 // 2,)).view(np.float16)
        assert bool((got[:32] == 1.0).all()) and bool((np.signbit(got[32:]) == (not flip)).all()), (flip, got)


# ---- up-sampling + concatenation ------------------------------------------------------------------------------------------------
def _upcat(ad, bd, c):
    out = Out(int(np.prod(c.shape)) * (c.ca + c.cb))
    _call("sd_upcat_ndhwc_device", _vp(ad), c.ca, c.up, _vp(bd), c.cb, *c.shape, _vp(out.t))
    return out


@pytest.mark.parametrize("c", [c for c in K.UPCAT if c.loops == 1], ids=lambda c: "%s %d+%d %s" % (c.name, c.ca, c.cb, c.shape))
def test_upcat_special_values(c):
    D, H, W = c.shape
    sa = (D >> ((c.up >> 2) & 1), H >> ((c.up >> 1) & 1), W >> (c.up & 1))
    for family, (a, b) in (("special", (K.with_nans(K.special_values(sa + (c.ca,), 41), 42), K.with_nans(K.special_values(c.shape + (c.cb,), 43), 44))),
                           ("two-scale", (K.two_scale_values(sa + (c.ca,), 45), K.two_scale_values(c.shape + (c.cb,), 46)))):
        out = _upcat(_dev(a), _dev(b), c)
        out.check(c.name)
        _same(out.numpy(c.shape + (c.ca + c.cb,)), K.upcat_ref(a, b, c.up), "upcat %s %s" % (family, c))


def _upcat_rows(c, ad, bd, out, ranges, what):
    """compare the output rows [r0, r1) (r0, r1 even) of a 2D case with the reference of the source rows copied back"""
    D, H, W = c.shape
    assert D == 1
    shy = (c.up >> 1) & 1
    o = out.t.view(H, W, c.ca + c.cb)
    a2, b2 = ad.view(H >> shy, -1, c.ca), bd.view(H, W, c.cb)
    for r0, r1 in ranges:
        want = K.upcat_ref(a2[r0 >> shy:((r1 - 1) >> shy) + 1][None].cpu().numpy(), b2[r0:r1][None].cpu().numpy(), c.up & 3)[0]
        _same(o[r0:r1].cpu().numpy(), want, what, origin=(r0, r1))


def test_upcat_grid_stride_loop():
    """over one pass: no element unwritten, every row compared (in slabs)"""
    c = [c for c in K.UPCAT if c.loops == 2][0]
    D, H, W = c.shape
    ad, bd = _int_tensor((1, H // 2, W // 2, c.ca), 45), _int_tensor((1, H, W, c.cb), 46)
    out = _upcat(ad, bd, c)
    out.check(c.name)
    _upcat_rows(c, ad, bd, out, [(r, min(r + 100, H)) for r in range(0, H, 100)], "upcat over one pass")


# ---- bias + activation -----------------------------------------------------------------------------------------------------------
def _bias_act(x, add, bias, c, act):
    args = (_vp(x),) + ((_vp(add),) if add is not None else ()) + (_vp(bias), c.n_outer, c.C, c.inner, act)
    _call("sd_add_bias_act_device" if add is not None else "sd_bias_act_device", *args)


def _off(a, off):
    """device copy of the flat float32 array a, `off` floats behind a 16-byte boundary"""
    return torch.empty(a.size + 4, device=DEV)[off:off + a.size].copy_(_dev(a.reshape(-1)))


@pytest.mark.parametrize("c", K.BIAS_ACT, ids=lambda c: c.name)
def test_bias_act_special_values_and_loop(c):
    """in place, so the guard words stand before and behind the tensor itself; x, the addend or the bias one float off 16-byte alignment
    -- each on its own -- takes the generic kernel"""
    n = c.n_outer * c.C * c.inner
    shape = (c.n_outer, c.C, c.inner)
    ox, oa, ob = c.offset
    if c.loops == 1:
        families = [(K.with_nans(K.special_values(shape, 51), 52), K.special_values(shape, 53), K.special_values((c.C,), 57)),
                    (K.two_scale_values(shape, 58), K.two_scale_values(shape, 59), K.two_scale_values((c.C,), 60))]
    else:
        rng = np.random.RandomState(54)
        x, y = rng.randint(-3, 4, shape).astype(np.float32), rng.randint(-3, 4, shape).astype(np.float32)
        x[:2], x[-2:] = K.special_values((2,) + shape[1:], 55), K.special_values((2,) + shape[1:], 56)
        families = [(x, y, K.special_values((c.C,), 57))]
    for x, y, bias in families:
        bias[np.abs(bias) > 100] = 0.5
        xd0, yd, bd = _dev(x.reshape(-1)), _off(y, oa), _off(bias, ob)
        assert (yd.data_ptr() % 16 != 0) == bool(oa) and (bd.data_ptr() % 16 != 0) == bool(ob)
        for add in (None, yd):
            for act in (0, 1):
                if c.loops > 1 and (add is None) == bool(act):                 # (the large cases: two of the four combinations)
                    continue
                buf = torch.empty(n + 8, dtype=torch.int32, device=DEV).fill_(SENTINEL)
                t = buf[4 + ox:4 + ox + n].view(torch.float32)
                assert (t.data_ptr() % 16 != 0) == bool(ox)
                t.copy_(xd0)
                _bias_act(t, add, bd, c, act)
                assert bool((buf[4 + ox + n:] == SENTINEL).all()) and bool((buf[:4 + ox] == SENTINEL).all()), "written outside the tensor"
                want = K.bias_act_ref(x, None if add is None else y, bias, act)
                _same(t.cpu().numpy().reshape(shape), want, "%s add %s act %d" % (c.name, add is not None, act))


# ---- the one-channel head ----------------------------------------------------------------------------------------------------------
def _dot(xd, out, bias, n, C, act, w, wb, sigm, dot):
    _call("sd_bias_act_dot_device", _vp(xd), _vp(out), _vp(bias), n, C, act, _vp(w), _vp(wb), sigm, _vp(dot))


def _combine(part, G, n, wb, sigm, out):
    _call("sd_dot_combine_device", _vp(part), G, n, _vp(wb), sigm, _vp(out))


@pytest.mark.parametrize("C,n", K.DOT, ids=str)
def test_bias_act_dot_integer_data(C, n):
    """every LPP at one pass, two and two with a ragged tail: features and dot product exact; out of place, in place, without the feature
    store, without a bias; the logistic output within 2e-6 of float64 and bit-identical to sd_dot_combine_device on the same terms"""
    x, b, w, wb = K.dot_data(C, n, C + n % 100)
    xd, bd, wd, wbd = _dev(x), _dev(b), _dev(w), _dev(np.array([wb], np.float32))
    for act in (0, 1):
        f, d = K.dot_ref(x, b, act, w, wb)
        feat, dot = Out(n * C), Out(n)
        _dot(xd, feat.t, bd, n, C, act, wd, wbd, 0, dot.t)
        feat.check("features"); dot.check("dot")
        _same(feat.numpy((n, C)), f.astype(np.float32), "features C %d act %d" % (C, act))
        _same(dot.numpy((n,)), d.astype(np.float32), "dot C %d act %d" % (C, act))
    # in place, then (the features now hold bias + activation) only read: out == nullptr, bias == nullptr
    buf = Out(n * C)
    buf.t.copy_(xd.view(-1))
    dot = Out(n)
    _dot(buf.t, buf.t, bd, n, C, 1, wd, wbd, 0, dot.t)
    buf.check("in place"); dot.check("dot in place")
    _same(buf.numpy((n, C)), f.astype(np.float32), "features in place")
    _same(dot.numpy((n,)), d.astype(np.float32), "dot in place")
    dot, prob = Out(n), Out(n)
    _dot(buf.t, None, None, n, C, 0, wd, wbd, 0, dot.t)
    _dot(buf.t, None, None, n, C, 0, wd, wbd, 1, prob.t)
    dot.check("dot only"); prob.check("prob")
    _same(dot.numpy((n,)), d.astype(np.float32), "dot of stored features")
    _same(buf.numpy((n, C)), f.astype(np.float32), "features after a read-only pass")
    p = prob.numpy((n,))
    err = float(np.abs(p.astype(np.float64) - K.logistic64(d)).max())
    print("C %d n %d: logistic |error| %.3g" % (C, n, err))
    assert err <= 2e-6, err
    terms = _dev(K.lane_terms(f, w))
    both = Out(n)
    _combine(terms, C // 32, n, wbd, 1, both.t)
    both.check("combine")
    _same(both.numpy((n,)), p, "sd_dot_combine_device against sd_bias_act_dot_device, logistic")
    # no feature store and no dot product asked for is an error; a plain epilogue (w == nullptr) writes only the features
    feat = Out(n * C)
    _dot(xd, feat.t, bd, n, C, 1, None, None, 0, None)
    feat.check("plain epilogue")
    _same(feat.numpy((n, C)), f.astype(np.float32), "plain epilogue")


@pytest.mark.parametrize("G", K.COMBINE_G)
def test_dot_combine_every_residue_around_a_pass_boundary(G):
    rng = np.random.RandomState(G)
    n_max = max(K.COMBINE_N)
    part = rng.randint(-5, 6, (n_max, G * 8)).astype(np.float32)
    K.assert_exact(part)
    want = part.astype(np.int64).sum(1) + 3
    pd, wbd = _dev(part), _dev(np.array([3.0], np.float32))
    for n in K.COMBINE_N:
        out = Out(n)
        _combine(pd, G, n, wbd, 0, out.t)
        out.check("combine G %d n %d" % (G, n))
        got = out.numpy((n,))
        _same(got, want[:n].astype(np.float32), "combine G %d n %d" % (G, n))
    prob = Out(n_max)
    _combine(pd, G, n_max, None, 1, prob.t)
    prob.check("combine, logistic")
    assert float(np.abs(prob.numpy((n_max,)).astype(np.float64) - K.logistic64(want - 3)).max()) <= 2e-6


@pytest.mark.parametrize("C", [32, 64, 128, 256])
def test_both_forms_of_the_head_keep_the_butterfly_order_on_float_data(C):
    """real-valued features: the order of the sum shows in the low bits.  Both forms must give the float32 sum in the order of the xor
    butterfly over the per-lane terms (reference: the same sum in numpy) -- and hence each other's bits"""
    n = 20011
    rng = np.random.RandomState(C)
    f = np.maximum(rng.standard_normal((n, C)), 0).astype(np.float32)
    w = (rng.standard_normal(C) * 0.2).astype(np.float32)
    wb = np.float32(0.37)
    terms = K.lane_terms(f, w)
    want = K.butterfly_ref(terms, wb)
    seq = terms[:, 0].copy()
    for k in range(1, terms.shape[1]):
        seq = seq + terms[:, k]
    assert not np.array_equal(seq + wb, want)                                  # the order matters on this data
    fd, wd, wbd, td = _dev(f), _dev(w), _dev(np.array([wb], np.float32)), _dev(terms)
    for sigm in (0, 1):
        a, b = Out(n), Out(n)
        _dot(fd, None, None, n, C, 0, wd, wbd, sigm, a.t)
        _combine(td, C // 32, n, wbd, sigm, b.t)
        a.check("bias_act_dot"); b.check("dot_combine")
        if sigm == 0:
            _same(a.numpy((n,)), want, "sd_bias_act_dot_device, butterfly order")
            _same(b.numpy((n,)), want, "sd_dot_combine_device, butterfly order")
        else:
            assert float(np.abs(a.numpy((n,)).astype(np.float64) - K.logistic64(want)).max()) <= 2e-6
        _same(b.numpy((n,)), a.numpy((n,)), "the two forms of the head, sigm %d" % sigm)


# ---- the distance head -------------------------------------------------------------------------------------------------------------
def _head(fd, C, rows, n, Wd, bd, R, clamp):
    out = Out(n * R)
    _call("sd_head_rows_device", _vp(fd), C, _vp(rows), n, _vp(Wd), _vp(bd), R, ctypes.c_float(clamp), _vp(out.t))
    out.check("head rows C %d R %d n %d" % (C, R, n))
    return out.numpy((n, R))


@pytest.mark.parametrize("C,R", K.HEAD, ids=str)
def test_head_rows_integer_data(C, R):
    """every CT and C: dense rows, a permutation, descending, all-equal and duplicate rows, n_rows with every residue modulo 32, a clamp
    that bites and none, with and without bias"""
    n_pix = K.HEAD_N_PIX
    feat, W, b = K.head_data(C, R, n_pix, C * 1000 + R)
    fd, Wd, bd = _dev(feat), _dev(W), _dev(b)
    dense = K.head_ref(feat, None, W, b, -np.inf)
    assert float(dense.min()) < 1.0 < float(dense.max())
    _same(_head(fd, C, None, n_pix, Wd, bd, R, NEG_INF), dense, "dense")
    _same(_head(fd, C, None, n_pix, Wd, bd, R, 1.0), np.maximum(dense, np.float32(1.0)), "dense, clamped")
    _same(_head(fd, C, None, n_pix, Wd, None, R, NEG_INF), K.head_ref(feat, None, W, None, -np.inf), "dense, no bias")
    sets = K.head_row_sets(n_pix, C + R)
    for name, rows in sets.items():
        rd = _dev(rows)
        _same(_head(fd, C, rd, len(rows), Wd, bd, R, NEG_INF), dense[rows], name)
        _same(_head(fd, C, rd, len(rows), Wd, bd, R, 1.0), np.maximum(dense[rows], np.float32(1.0)), name + ", clamped")
    perm = sets["permutation"]
    pd = _dev(perm)
    for n in K.HEAD_RESIDUES:
        _same(_head(fd, C, pd, n, Wd, bd, R, NEG_INF), dense[perm[:n]], "permutation, %d rows" % n)
        _same(_head(fd, C, None, n, Wd, bd, R, NEG_INF), dense[:n], "dense, %d rows" % n)


@pytest.mark.parametrize("C,R", [(32, 32), (64, 100)], ids=str)
def test_head_rows_grid_stride_loop(C, R):
    """two passes of the persistent tiles and a ragged third: selected rows (with repeats) and dense"""
    n = K.HEAD_LOOP_ROWS
    feat, W, b = K.head_data(C, R, n, 7)
    fd, Wd, bd = _dev(feat), _dev(W), _dev(b)
    dense = K.head_ref(feat, None, W, b, -np.inf)
    _same(_head(fd, C, None, n, Wd, bd, R, NEG_INF), dense, "dense over two passes")
    rows = np.random.RandomState(8).randint(0, 5000, n).astype(np.int64)
    _same(_head(fd, C, _dev(rows), n, Wd, bd, R, 0.0), np.maximum(dense[rows], 0), "rows over two passes")


# ---- whole path: pack -> split16 pool -> unpack against the f32 pool ---------------------------------------------------------------
@pytest.mark.parametrize("shape,pool", [((1, 70, 90), (1, 2, 2)), ((10, 22, 26), (2, 2, 2))], ids=["2D", "3D"])
@pytest.mark.parametrize("family", ["integer", "special", "nan"])
def test_level_chain_is_the_same_in_both_forms(shape, pool, family):
    """one U-Net level: the pooled f32 tensor, and pack -> pool -> unpack.  Equal bit for bit on integers; on special values equal to the
    22-bit value of the reference (unsplit(split(.))), a NaN staying a NaN in both"""
    C = 64
    if family == "integer":
        x = np.random.RandomState(3).randint(0, 2049, shape + (C,)).astype(np.float32)
    else:
        x = K.special_values(shape + (C,), 61, pool)
        x = np.where(np.abs(x) > K.F16_MAX, np.float32(0.75), x)                # (inside the range: infinities have no 22-bit value)
        if family == "nan":
            x = K.with_nans(x, 62, pool)
    want = K.pool_ref(x, pool)
    xd = _dev(x)
    f32, oshape = _pool(xd, shape, C, pool, False)
    sp, _ = _pool(_pack(xd, C).t, shape, C, pool, True)
    back = _unpack(sp.t, C)
    for o in (f32, sp, back):
        o.check(family)
    _same(f32.numpy(oshape), want, "f32 pool")
    w22 = K.np_unsplit16(K.np_split16(want))
    if family == "integer":
        assert np.array_equal(w22, want)
    _same(back.numpy(oshape), w22, "pack -> pool -> unpack")
    assert np.array_equal(np.isnan(back.numpy(oshape)), np.isnan(f32.numpy(oshape)))


# ---- offsets past 2^31 and 2^32 elements -------------------------------------------------------------------------------------------
def test_max_pool_past_2_31_elements():
    """a (416, 416, 416, 32) level, f32 and split16: 2.3 x 10^9 input elements; output planes whose windows lie at the ends and around
    the 2^31-element mark of the input"""
    c = K.POOL_BIG
    D, H, W = c.shape
    _need(24)
    xd = _int_tensor((D, H, W, c.C), 71)
    planes = sorted({p // 2 for p in K.marks(D, H * W * c.C, 72)})
    assert any((2 * p + 1) * H * W * c.C > 1 << 31 for p in planes)
    wants = {p: K.pool_ref(xd[2 * p:2 * p + 2].cpu().numpy(), c.pool)[0] for p in planes}
    out, oshape = _pool(xd, c.shape, c.C, c.pool, False)
    out.check("f32 pool")
    o = out.t.view(oshape)
    for p in planes:
        _same(o[p].cpu().numpy(), wants[p], "f32 pool of %s" % c.name, origin=p)
    del out, o
    packed = _pack(xd, c.C)
    del xd
    out, _ = _pool(packed.t, c.shape, c.C, c.pool, True)
    out.check("split16 pool")
    o = out.t.view(oshape)
    for p in planes:
        _same(o[p].cpu().numpy(), K.np_split16(wants[p]), "split16 pool of %s" % c.name, half=True, origin=p)


def test_pack_unpack_past_2_31_elements():
    C, n_pix = 32, (1 << 31) // 32 + 4099
    _need(40)
    rows = 8192
    assert n_pix % rows                                                        # a ragged tail
    xd = _int_tensor((n_pix, C), 73, -2048, 2049)
    xd *= 1.0 + 2.0 ** -13                                                     # both terms carry weight
    packed = _pack(xd, C)
    packed.check("pack")
    back = _unpack(packed.t, C)
    back.check("unpack")
    s, b = packed.t.view(n_pix, C), back.t.view(n_pix, C)
    for p in K.marks(-(-n_pix // rows), rows * C, 74):
        sl = slice(p * rows, min((p + 1) * rows, n_pix))
        x = xd[sl].cpu().numpy()
        _same(s[sl].cpu().numpy(), K.np_split16(x), "pack", half=True, origin=p)
        _same(b[sl].cpu().numpy(), K.np_unsplit16(K.np_split16(x)), "unpack", origin=p)
    assert n_pix * C > 1 << 31


def test_upcat_output_past_2_32_bytes():
    c = K.UPCAT_BIG
    D, H, W = c.shape
    _need(8)
    ad, bd = _int_tensor((1, H // 2, W // 2, c.ca), 75), _int_tensor((1, H, W, c.cb), 76)
    out = _upcat(ad, bd, c)
    out.check(c.name)
    per_row = W * (c.ca + c.cb)
    rows = sorted({0, 1, H - 2, H - 1} | {r + d for m in (1 << 29, 1 << 30) for r in [m // per_row] for d in (-1, 0, 1)} |
                  set(int(v) for v in np.random.RandomState(77).choice(H, 4, replace=False)))
    assert H * per_row * 4 > 1 << 32 and any(r * per_row * 4 > 1 << 32 for r in rows)
    _upcat_rows(c, ad, bd, out, [(r & ~1, (r & ~1) + 2) for r in rows], "upcat past 2^32 bytes")


def test_bias_act_past_2_31_elements():
    c = K.BIAS_ACT_BIG
    _need(12)
    n = c.n_outer * c.C
    buf = torch.empty(n + 4, dtype=torch.int32, device=DEV)
    buf[n:] = SENTINEL
    x = buf[:n].view(torch.float32).view(c.n_outer, c.C)
    rows = 8192
    g = torch.Generator(device=DEV).manual_seed(78)
    for z in range(0, c.n_outer, 1 << 22):
        m = min(1 << 22, c.n_outer - z)
        x[z:z + m] = torch.randint(-3, 4, (m, c.C), generator=g, device=DEV, dtype=torch.int8).float()
    marks = K.marks(-(-c.n_outer // rows), rows * c.C, 79)
    before = {p: x[p * rows:(p + 1) * rows].cpu().numpy() for p in marks}
    bias = np.random.RandomState(80).randint(-2, 3, c.C).astype(np.float32)
    _call("sd_bias_act_device", _vp(x), _vp(_dev(bias)), c.n_outer, c.C, 1, 1)
    assert bool((buf[n:] == SENTINEL).all())
    for p in marks:
        want = K.bias_act_ref(before[p][:, :, None], None, bias, 1)[:, :, 0]
        _same(x[p * rows:(p + 1) * rows].cpu().numpy(), want, "bias_act past 2^31 elements", origin=p)
    assert n > 1 << 31 and any((p + 1) * rows * c.C > 1 << 31 for p in marks)


def test_head_rows_past_2_32_elements():
    """rows[i] * C past 2^31 and 2^32 elements of the feature tensor: rows at the marks and at the ends"""
    C, R = 32, 32
    n_pix = (1 << 32) // C + 5003
    _need(24)
    fd = _int_tensor((n_pix, C), 81, 0, 4)
    rng = np.random.RandomState(82)
    rows = np.concatenate([[0, 1, n_pix - 1, n_pix - 2], [m // C + d for m in (1 << 31, 1 << 32) for d in range(-40, 41)],
                           rng.randint(0, n_pix, 200)]).astype(np.int64)
    rows = rows[rng.permutation(len(rows))]
    assert int(rows.max()) * C > 1 << 32
    _, W, b = K.head_data(C, R, 1, 83)
    feat = fd[_dev(rows)].cpu().numpy()
    want = K.head_ref(feat, None, W, b, -np.inf)
    _same(_head(fd, C, _dev(rows), len(rows), _dev(W), _dev(b), R, NEG_INF), want, "rows past 2^32 elements")
