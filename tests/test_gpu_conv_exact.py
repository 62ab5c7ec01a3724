"""GPU: the inference convolutions (csrc/conv3x3.hip, conv3x3_bf16.hip, conv3x3_f16.hip, conv_general.hip) compared EXACTLY -- outputs
with ==, no tolerance anywhere -- with a plain reference on the CPU, at the kernels' edges and at the sizes the README's numbers are quoted
on.  The cases, the data and the references live in _conv_cases.py; test_cpu_conv_cases.py checks without a GPU that the case lists
reach the regimes named below and that the exactness preconditions hold on the references alone.

  * ternary family (all kernel families: 'hand' f32 MFMA, 'bf16x6', 'f16x3' and its one-workgroup-per-CU instance, the general kernel):
    inputs, weights, biases and residuals in {-1, 0, 1}.  Every product is exact in f32 and in every operand split, every partial sum an
    integer far below 2^24, so any summation order gives the same f32: the result must EQUAL float32 conv2d / conv3d on the CPU (exact
    for the same reason) + bias (+ residual), ReLU.
  * two-scale family (f16x3): x = a (1 + b 2^-13), w = c (1 + d 2^-13) with ternary a, b, c, d, so that hi = a, lo' = a b / 4 and the
    cross-term accumulator (added as acc0 + acc1 2^-11) carries weight; expected: the kernel's own statement evaluated on the CPU from the
    split terms, which is a float32 for every element (asserted on the reference).
  * every output buffer starts as NaN (torch.empty is patched while the package allocates): an element no lane writes fails.
  * forms: f32 / split16 in, out, both; two sources with nearest up-sampling (anisotropic pool included); residual epilogue; fused
    probability head with and without the feature store; the layer on selected rows; the one-channel first layer (f32 and split16);
    the general kernel's layers (7^3 stem, strided with TensorFlow 'same' padding on odd extents, 1x1x1 projection, 3-channel first layer,
    5x5, 48-channel layers with sd_upcat_ndhwc_device).
  * shapes: ragged tiles over every residue, W < TW, H < TH, H = 1, D = 1, 2; the persistent loop with fewer / exactly as many / more
    tiles than workgroups; every distinct layer of StarDist2D(Config2D(n_rays=32)) at 2048^2, of StarDist3D(Config3D(rays=96)) at 256^3
    and of the 3D_demo ResNet on a 32-plane slab of 256^3 (taken from the models' own modules); activations past 2^31 bytes, 2^32 bytes /
    2^31 elements and 2^32 elements (the last compared on slabs; needs ~50 GB of device memory, skips only if the device reports less).
  * whole networks: the default 2D and 3D models with integer weights (activations grow by at most 1 per layer, asserted on the CPU
    evaluation): the GPU features equal the CPU's in every conv mode, split16 activations on and off."""
import contextlib

import numpy as np
import pytest
import torch

import _conv_cases as C
from _exact import nan_empty
from test_gpu_split16 import np_split16

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ["hand", "bf16x6", "f16x3", "f16x3-1wg"]


@contextlib.contextmanager
def _mode(mode):
    """the conv mode `mode` for the 3x3 layers over 32-channel chunks; '-1wg': the split-fp16 kernel's one-workgroup-per-CU instance"""
    from stardist_amd.lib import _native as N
    from stardist_amd.models import unet as U
    one = mode.endswith("-1wg")
    if one:
        N.check(N.lib().sd_set_option(b"conv_f16_workgroups_per_cu", 1))
    try:
        with U.force_conv_mode(mode.split("-")[0]), U.force_split16(True):
            yield
    finally:
        if one:
            N.check(N.lib().sd_set_option(b"conv_f16_workgroups_per_cu", 2))


def _conv_module(l, w, b):
    nd = len(l.shape)
    Conv = torch.nn.Conv2d if nd == 2 else torch.nn.Conv3d
    conv = Conv(w.shape[1], l.co, l.k, stride=l.stride, padding=0 if l.tf_same else l.k // 2)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    return conv.to(DEV)


def _run(l, conv, srcs, res, mode, form="f32", dot=None, no_store=False):
    """the layer through models/unet._hand_conv; form: 'f32', 'in' (split16 sources), 'out' (split16 output), 'both'"""
    from stardist_amd.models import unet as U
    with torch.no_grad(), _mode(mode), nan_empty():
        U.range_flag(DEV).zero_()
        ts = [(U.split16_pack(t) if form in ("in", "both") else t, up) for t, (_, up) in zip(srcs, l.srcs)]
        conv.__dict__["_sd_split_out"] = form in ("out", "both")
        try:
            y = U._hand_conv(conv, ts, l.act, res=res, tf_same=l.tf_same, dot=dot, no_store=no_store)
        finally:
            conv.__dict__["_sd_split_out"] = False
    assert y is not None, "layer not taken by a hand-written kernel"
    assert int(U.range_flag(DEV).item()) == 0
    if y is not U.NO_STORE:
        assert U.is_split16(y) == (form in ("out", "both"))
    return y


def _coords(flat, shape):
    return tuple(int(v) for v in np.unravel_index(int(flat), shape))


def _same(got, want, what, origin=0):
    """got, want: CPU tensors of one shape (channels-last storage order irrelevant: compared by index)"""
    if torch.equal(got, want):
        return
    bad = ~(got == want)
    idx = bad.flatten().nonzero().flatten()
    first = [(_coords(i, got.shape), float(got.flatten()[i]), float(want.flatten()[i])) for i in idx[:6]]
    pytest.fail("%s: %d of %d elements differ (%d NaN); index (1, c, *spatial)%s, got, want: %r" % (
        what, int(bad.sum()), bad.numel(), int(torch.isnan(got).sum()), " with plane origin %d" % origin if origin else "", first))


def _same_split16(got, want_f32, what):
    """a split16 tensor == numpy's split of the exact f32 result, bit for bit"""
    g = C.np_cl(got).view(np.uint32)
    w = np_split16(C.np_cl(want_f32)).view(np.uint32)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        pytest.fail("%s: %d of %d words differ, first at (*spatial, word) %s: %08x want %08x" % (
            what, len(bad), g.size, tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])]))


def _check_ternary(l, modes, forms=("f32",), slab=None, density=None):
    """the ternary layer `l` in every mode and form against the CPU; slab: compare (and evaluate the reference) in z slabs of that many planes"""
    srcs, w, b, res = C.layer_data(l, density)
    conv = _conv_module(l, w, b)
    dsrcs = [t.to(DEV) for t in srcs]
    dres = res.to(DEV) if res is not None else None
    x = C.cat_input(l, srcs)
    outs = {}
    for mode in modes:
        for form in forms:
            if form != "f32" and not mode.startswith("f16x3"):
                continue
            outs[(mode, form)] = _run(l, conv, dsrcs, dres, mode, form)
    O = C.out_shape(l)
    for key, y in outs.items():
        assert tuple(y.shape) == (1, l.co) + O, (key, tuple(y.shape))
    ranges = [(None, None)] if slab is None else [(z, min(z + slab, O[0])) for z in range(0, O[0], slab)]
    for z0, z1 in ranges:
        want = C.ternary_reference(l, x, w, b, res, z0, z1)
        for (mode, form), y in outs.items():
            part = y if z0 is None else y[:, :, z0:z1]
            what = "%s %s %s" % (mode, form, l)
            if form in ("out", "both"):
                _same_split16(part, want, what)
            else:
                _same(part.cpu(), want, what, z0 or 0)


# ---- ragged tiles and the persistent loop --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_ragged_tiles_every_residue(mode):
    for l in C.SWEEP2D + C.SWEEP3D:
        _check_ternary(l, [mode])


@pytest.mark.parametrize("l", C.LOOP, ids=str)
def test_persistent_loop_regimes(l):
    _check_ternary(l, MODES)


# ---- the forms -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", [C.FORM2D, C.FORM3D] + C.TWO_SRC, ids=str)
def test_forms_f32_split16_and_two_sources(l):
    _check_ternary(l, MODES, forms=("f32", "in", "out", "both"))


@pytest.mark.parametrize("l", C.RESIDUAL, ids=str)
def test_residual_epilogue(l):
    _check_ternary(l, MODES)


@pytest.mark.parametrize("l", C.FUSED_HEAD, ids=str)
@pytest.mark.parametrize("split", [False, True])
def test_fused_probability_head(l, split):
    """sd_conv3_f16x3_dot_ndhwc_device / the fmt entry with a head: the stored features are exact; the per-lane terms are the dot products
    of 4 consecutive channels of the features with the head weights (test_gpu_heads.py), integers with ternary weights: compared exactly.
    The no-store variant gives the same terms and writes no features"""
    from stardist_amd.models import unet as U
    srcs, w, b, _ = C.layer_data(l)
    conv = _conv_module(l, w, b)
    dsrcs = [t.to(DEV) for t in srcs]
    hw = C.tern((l.co,), C.seed_of(l, 6))
    dhw = hw.to(DEV)
    want = C.ternary_reference(l, C.cat_input(l, srcs), w, b, None)
    n_pix = int(np.prod(l.shape))
    f = torch.from_numpy(C.np_cl(want)).reshape(n_pix, l.co)
    want_terms = (f * hw).reshape(n_pix, l.co // 4, 4).sum(-1)
    for mode in ("f16x3", "f16x3-1wg"):
        holder, h2 = [], []
        y = _run(l, conv, dsrcs, None, mode, "in" if split else "f32", dot=(dhw, holder))
        _same(y.cpu(), want, "features %s %s" % (mode, l))
        assert len(holder) == 1
        _same(holder[0].cpu(), want_terms, "head terms %s %s" % (mode, l))
        r = _run(l, conv, dsrcs, None, mode, "in" if split else "f32", dot=(dhw, h2), no_store=True)
        assert r is U.NO_STORE and len(h2) == 1
        _same(h2[0].cpu(), want_terms, "head terms without the store %s %s" % (mode, l))


def _border_rows(shape, seed, n_random=500):
    """linear pixel indices: first and last pixel, every corner, pixels on every face, random ones, a duplicate"""
    n_pix = int(np.prod(shape))
    rng = np.random.RandomState(seed)
    corners = [np.ravel_multi_index(c, shape) for c in np.ndindex(*(2,) * len(shape)) for c in [tuple(i * (s - 1) for i, s in zip(c, shape))]]
    faces = []
    for d in range(len(shape)):
        for side in (0, shape[d] - 1):
            for _ in range(8):
                p = [rng.randint(0, s) for s in shape]
                p[d] = side
                faces.append(np.ravel_multi_index(tuple(p), shape))
    rows = np.concatenate([[0, n_pix - 1, 0], corners, faces, rng.randint(0, n_pix, n_random)]).astype(np.int64)
    return rows


@pytest.mark.parametrize("l", C.ROWS, ids=str)
@pytest.mark.parametrize("split", [False, True])
def test_layer_on_selected_rows(l, split):
    from stardist_amd.models import unet as U
    srcs, w, b, _ = C.layer_data(l)
    conv = _conv_module(l, w, b)
    want = torch.from_numpy(C.np_cl(C.ternary_reference(l, srcs[0], w, b, None))).reshape(-1, l.co)
    rows = _border_rows(l.shape, 3)
    x = srcs[0].to(DEV)
    for n in (len(rows), 1, 31, 33):                                   # a partial last wave
        r = torch.from_numpy(rows[:n]).to(DEV)
        with torch.no_grad(), _mode("f16x3"), nan_empty():
            got = U.conv_rows(conv, U.split16_pack(x) if split else x, l.act, r)
        _same(got.cpu(), want[rows[:n]], "rows %s" % (l,))


@pytest.mark.parametrize("l", C.FIRST_LAYER, ids=str)
def test_one_channel_first_layer(l):
    """sd_conv3 with one input channel (exact f32 in every mode) and sd_conv3_c1x32_split16_device"""
    _check_ternary(l, ["hand", "f16x3"], forms=("f32", "out"))


@pytest.mark.parametrize("l", C.GENERAL, ids=str)
def test_general_kernel(l):
    assert not C.is_conv3(l)
    _check_ternary(l, ["f16x3"])


@pytest.mark.parametrize("shape,c_up,c_skip,pool,co", C.UPCAT48, ids=str)
def test_up_level_of_48_channel_network(shape, c_up, c_skip, pool, co):
    """unet_n_filter_base = 48: UpSampling + Concatenate by sd_upcat_ndhwc_device, then the general kernel"""
    from stardist_amd.models import unet as U
    l = C.L(shape, [(c_up, tuple(int(p == 2) for p in pool)), (c_skip, 0)], co)
    srcs, w, b, _ = C.layer_data(l)
    conv = _conv_module(l, w, b)
    with torch.no_grad(), nan_empty():
        assert U._hand_conv(conv, [(srcs[0].to(DEV), l.srcs[0][1]), (srcs[1].to(DEV), 0)], 1) is None      # not in 32-channel chunks
        y = U._upcat_general(conv, srcs[0].to(DEV), srcs[1].to(DEV), pool, 1)
    assert y is not None
    _same(y.cpu(), C.ternary_reference(l, C.cat_input(l, srcs), w, b, None), str(l))


# ---- the two-scale family ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", C.TWO_SCALE, ids=str)
def test_two_scale_cross_terms(l):
    dens = C.two_scale_density(l)
    parts, wparts, bias = C.two_scale_data(l, dens)
    want = C.two_scale_reference(l, parts, wparts, bias)
    assert float((want != want.round()).float().mean()) > 0.2                 # the cross terms show in the expected values
    conv = _conv_module(l, C.two_scale(*wparts), bias)
    dsrcs = [C.two_scale(a, b).to(DEV) for a, b in parts]
    for mode in ("f16x3", "f16x3-1wg"):
        for form in ("f32", "in", "out", "both"):
            y = _run(l, conv, dsrcs, None, mode, form)
            if form in ("out", "both"):
                _same_split16(y, want, "%s %s %s" % (mode, form, l))
            else:
                _same(y.cpu(), want, "%s %s %s" % (mode, form, l))


# ---- the networks' own layers at the headline sizes ----------------------------------------------------------------------------
def _need(gb):
    free = torch.cuda.mem_get_info()[0]
    if free < gb * 1e9:
        pytest.skip("needs %d GB of free device memory, the device reports %.1f GB" % (gb, free / 1e9))


@pytest.mark.parametrize("i", range(14))
def test_layers_of_the_2d_model_at_2048(i):
    layers = C.headline_layers("2d")
    assert len(layers) == 14
    _check_ternary(layers[i], MODES if C.is_conv3(layers[i]) and layers[i].srcs[0][0] != 1 else ["f16x3"])


@pytest.mark.parametrize("i", range(10))
def test_layers_of_the_3d_model_at_256(i):
    layers = C.headline_layers("3d")
    assert len(layers) == 10
    l = layers[i]
    _need(45)
    _check_ternary(l, MODES if l.srcs[0][0] != 1 else ["f16x3"], slab=32 if l.shape[0] > 64 else None)


@pytest.mark.parametrize("i", range(8))
def test_layers_of_the_3d_demo_resnet_on_a_slab_of_256(i):
    layers = C.headline_layers("resnet")
    assert len(layers) == 8
    l = layers[i]
    _check_ternary(l, MODES if C.is_conv3(l) else ["f16x3"])


# ---- offsets past 2^31 and 2^32 ------------------------------------------------------------------------------------------------
def test_output_past_2_32_bytes_and_2_31_elements():
    l = C.BIG_OUT
    assert int(np.prod(l.shape)) * l.co > 1 << 31
    _need(45)
    _check_ternary(l, MODES, slab=24)


def _marks(l, c):
    """planes that hold the element offsets 2^31 and 2^32 of a (D, H, W, c) tensor, with their neighbours"""
    per_plane = l.shape[1] * l.shape[2] * c
    out = set()
    for m in (1 << 31, 1 << 32):
        z = m // per_plane
        out.update(p for p in (z - 1, z, z + 1) if 0 <= p < l.shape[0])
    return out


def test_input_and_output_past_2_32_elements():
    """a 560^3 block as the sharded 1024^3 leg cuts it, 32 -> 32: 5.6 x 10^9 elements per activation.  Compared on slabs: the first and
    last 4 planes, the planes around the 2^31- and 2^32-element marks of input and output, and 8 planes chosen by a fixed seed; the CPU
    reference is evaluated per plane from the device input copied back.  sd_conv3_f16x3_rows_device on pixels of those planes as well
    (element offsets past 2^31 and 2^32)."""
    from stardist_amd.models import unet as U
    l = C.BIG_BOTH
    D, H, W = l.shape
    ci = l.srcs[0][0]
    assert D * H * W * ci > 1 << 32 and D * H * W * l.co > 1 << 32
    _need(50)
    g = torch.Generator(device=DEV).manual_seed(11)
    xd = torch.empty((1, D, H, W, ci), dtype=torch.float32, device=DEV)
    for z in range(0, D, 16):
        n = min(16, D - z)
        xd[0, z:z + n] = torch.randint(-1, 2, (n, H, W, ci), generator=g, device=DEV, dtype=torch.int8).float()
    x = xd.permute(0, 4, 1, 2, 3)                                            # (1, C, D, H, W), channels-last storage
    w, b = C.tern((l.co, ci, 3, 3, 3), 12), C.tern((l.co,), 13)
    conv = _conv_module(l, w, b)
    rng = np.random.RandomState(14)
    planes = sorted(set(range(4)) | set(range(D - 4, D)) | _marks(l, ci) | _marks(l, l.co) | set(int(v) for v in rng.choice(D, 8, replace=False)))
    assert any(p * H * W * ci > 1 << 32 for p in planes)
    refs = {}
    for p in planes:
        lo, hi = max(p - 1, 0), min(p + 2, D)
        xs = torch.nn.functional.pad(x[:, :, lo:hi].cpu(), (0, 0, 0, 0, lo - (p - 1), (p + 2) - hi))
        refs[p] = C.epilogue(l, torch.nn.functional.conv3d(xs, w, padding=(0, 1, 1)), b, None)
    for mode in MODES:
        y = _run(l, conv, [x], None, mode)
        for p in planes:
            _same(y[:, :, p:p + 1].cpu(), refs[p], "%s plane %d of %s" % (mode, p, l), p)
        del y
    rows, want = [], []
    for p in planes:
        pix = np.concatenate([[0, W - 1, H * W - W, H * W - 1], rng.randint(0, H * W, 60)])
        rows.append(p * H * W + pix)
        want.append(torch.from_numpy(C.np_cl(refs[p])).reshape(H * W, l.co)[pix])
    rows = np.concatenate(rows).astype(np.int64)
    assert int(rows.max()) * ci > 1 << 32
    with torch.no_grad(), _mode("f16x3"), nan_empty():
        got = U.conv_rows(conv, x, l.act, torch.from_numpy(rows).to(DEV))
    _same(got.cpu(), torch.cat(want), "rows of %s" % (l,))


# ---- whole networks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [2, 3])
def test_whole_network_features_exact(nd):
    """the default models with integer weights (C.set_integer_weights): all activations up to the features layer are non-negative integers
    that fp16 holds exactly (asserted on the CPU evaluation, which is then exact); the GPU forward pass -- max-pooling, up-sampling,
    concatenation, split16 activations included -- must give the same features in every conv mode, split16 on and off"""
    from stardist_amd.models import Config2D, Config3D, StarDist2D, StarDist3D
    from stardist_amd.models import unet as U
    Model, cfg, S = (StarDist2D, Config2D(n_rays=32), C.NET2D) if nd == 2 else (StarDist3D, Config3D(rays=96), C.NET3D)
    cpu = Model(cfg, basedir=None, device="cpu", seed=0)
    C.set_integer_weights(cpu.net, 21).eval()
    g = torch.Generator().manual_seed(22)
    x = torch.randint(0, 3, (1, 1) + S, generator=g).float()
    want, peak = C.features_cpu(cpu.net, x)
    assert peak <= 2048 and bool((want == want.round()).all()) and float(want.max()) >= 2
    gpu = Model(cfg, basedir=None, device=DEV, seed=0)
    gpu.net.load_state_dict(cpu.net.state_dict())
    gpu.net.eval()
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last if nd == 2 else torch.channels_last_3d)
    for mode in MODES:
        for split in (True, False):
            with torch.no_grad(), _mode(mode), U.force_split16(split), nan_empty():
                feat = gpu.net(xd, sparse_head=True)[1]
            assert gpu.net.head_mode == "sparse" and tuple(feat.shape) == tuple(want.shape)
            _same(feat.cpu(), want, "features of the %dD network, %s, split16 %s" % (nd, mode, split))
