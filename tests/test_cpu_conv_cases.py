"""CPU: the case lists of test_gpu_conv_exact.py (_conv_cases.py) reach the regimes they were chosen for -- from the partition of the
3x3 kernels restated there (conv3x3_layout.h constants, the launch code of conv3x3_host.h) -- and the exactness
preconditions of its two data families hold on the CPU references alone."""
import os
import re

import numpy as np
import torch

import _conv_cases as C
from test_gpu_split16 import np_split16, np_unsplit16

CSRC = os.path.join(C.ROOT, "stardist_amd", "csrc")


def test_restated_constants_match_the_layout_header():
    src = open(os.path.join(CSRC, "conv3x3_layout.h")).read()
    m = re.search(r"constexpr int TH = (\d+), TW = (\d+);", src)
    assert (int(m.group(1)), int(m.group(2))) == (C.TH, C.TW)
    assert int(re.search(r"constexpr int CHUNK = (\d+);", src).group(1)) == C.CHUNK
    assert int(re.search(r"constexpr int MAX_CHUNKS = (\d+);", src).group(1)) == C.MAX_CHUNKS
    # the grid of the persistent launches: one formula (conv3x3_host.h), two workgroups per CU for the f16 form (or one, by option), one for the others
    host = open(os.path.join(CSRC, "conv3x3_host.h")).read()
    assert "(long long)(per_cu * cus / P.groups) * P.groups" in host and "const long long want = (long long)P.n_tiles * P.groups;" in host
    f16 = open(os.path.join(CSRC, "conv3x3_f16.hip")).read()
    assert "const int per_cu = sd::option(sd::OPT_CONV_F16_WGS) == 1 ? 1 : 2;" in f16 and "persistent_grid(all, attr_done, lds, P, per_cu, blocks)" in f16
    for other in ("conv3x3_bf16.hip", "conv3x3.hip"):
        assert "persistent_grid(kern, attr_done, lds, P, 1, blocks)" in open(os.path.join(CSRC, other)).read()


def test_ragged_tile_regimes_are_reached():
    sweep = C.SWEEP2D + C.SWEEP3D
    assert all(C.is_conv3(l) for l in sweep)
    assert {l.shape[-1] % C.TW for l in sweep} == set(range(C.TW))
    assert {l.shape[-2] % C.TH for l in sweep} == set(range(C.TH))
    assert any(l.shape[-1] < C.TW for l in sweep) and any(l.shape[-2] < C.TH for l in sweep)
    assert any(len(l.shape) == 2 and l.shape[0] == 1 for l in sweep)                           # H = 1
    assert any(l.shape[-1] == 1 for l in sweep)
    assert {1, 2, 3} <= {l.shape[0] for l in C.SWEEP3D}                                       # D = 1, D = 2, an inner plane
    forms = [C.FORM2D, C.FORM3D] + C.TWO_SRC + C.RESIDUAL + C.FUSED_HEAD + C.ROWS + C.TWO_SCALE
    assert all(C.is_conv3(l) for l in forms + C.FIRST_LAYER + C.LOOP)
    assert all(l.shape[-1] % C.TW and l.shape[-2] % C.TH for l in (C.FORM2D, C.FORM3D))      # ragged on both axes
    ups = {l.srcs[0][1] for l in C.TWO_SRC}
    assert {(1, 1), (1, 1, 1), (0, 1, 1)} <= ups
    assert not any(C.is_conv3(l) for l in C.GENERAL)
    ks = {(l.k, l.stride, l.srcs[0][0]) for l in C.GENERAL}
    assert (7, (1, 1, 1), 1) in ks and (3, (1, 2, 2), 32) in ks and (3, (2, 2, 2), 64) in ks and (1, (1, 2, 2), 32) in ks
    assert any(l.k == 5 for l in C.GENERAL) and any(l.srcs[0][0] == 3 for l in C.GENERAL) and any(l.srcs[0][0] == 48 for l in C.GENERAL)
    assert all(any(s % 2 for s in l.shape) for l in C.GENERAL if l.tf_same)                    # TensorFlow 'same' on odd extents


def test_persistent_loop_regimes_are_reached():
    h2, h3 = C.headline_layers("2d"), C.headline_layers("3d")
    for per_cu in (2, 1):
        got = {C.loop_regime(l.shape, l.co, per_cu) for l in C.LOOP + C.SWEEP2D}
        assert "fewer" in got and "exact" in got and any(isinstance(r, float) for r in got), (per_cu, got)
    assert any(len(l.shape) == 3 and C.loop_regime(l.shape, l.co, 2) == "exact" for l in C.LOOP)
    # the benchmark's ratios: 2048^2, 32 -> 32 and 32 -> 128 (32 and 128 iterations of 512 workgroups)
    by = {(l.srcs, l.co): C.loop_regime(l.shape, l.co, 2) for l in h2 if l.shape == C.HEADLINE2D}
    assert by[(((32, (0, 0)),), 32)] == 32.0 and by[(((32, (0, 0)),), 128)] == 128.0
    assert C.workgroups(C.HEADLINE2D, 128, 2) == (512, 16384 * 4)
    by3 = {(l.srcs, l.co): C.loop_regime(l.shape, l.co, 2) for l in h3 if l.shape == C.HEADLINE3D}
    assert by3[(((32, (0, 0, 0)),), 128)] == 256 * 32 * 8 * 4 / 512.0


def test_headline_layers_come_from_the_models():
    h2, h3, hr = C.headline_layers("2d"), C.headline_layers("3d"), C.headline_layers("resnet")
    assert (len(h2), len(h3), len(hr)) == (14, 10, 8)                  # (the GPU tests parametrise over these counts)
    assert all(C.is_conv3(l) for l in h2 + h3)
    assert h2[0].srcs == ((1, (0, 0)),) and h2[-1].co == 128 and h2[-1].shape == C.HEADLINE2D
    assert sum(len(l.srcs) == 2 for l in h2) == 3 and sum(len(l.srcs) == 2 for l in h3) == 2
    assert h3[-1].co == 128 and h3[-1].shape == C.HEADLINE3D
    assert hr[0].k == 7 and any(l.res for l in hr) and any(l.tf_same and l.stride == (1, 2, 2) for l in hr) and any(l.k == 1 for l in hr)
    assert all(l.shape[0] == 32 for l in hr)


def test_offset_cases_pass_the_marks():
    act = [l for l in C.headline_layers("3d") if l.shape == C.HEADLINE3D and l.srcs == ((32, (0, 0, 0)),) and l.co == 32]
    assert act and int(np.prod(C.HEADLINE3D)) * 32 * 4 == 1 << 31                             # 256^3 x 32: exactly 2^31 bytes ...
    assert int(np.prod(C.BIG_OUT.shape)) * C.BIG_OUT.srcs[0][0] * 4 > 1 << 31                 # ... and an input whose byte offsets pass it
    n_out = int(np.prod(C.BIG_OUT.shape)) * C.BIG_OUT.co
    assert n_out > 1 << 31 and n_out * 4 > 1 << 32                                            # 2^31 elements, 2^32 bytes
    n = int(np.prod(C.BIG_BOTH.shape))
    assert n * C.BIG_BOTH.srcs[0][0] > 1 << 32 and n * C.BIG_BOTH.co > 1 << 32                # 2^32 elements in and out
    assert C.is_conv3(C.BIG_OUT) and C.is_conv3(C.BIG_BOTH)


def test_ternary_reference_is_exact():
    """float32 convolution of ternary data == float64 convolution (small cases of every kind of layer)"""
    for l in [C.FORM2D, C.TWO_SRC[3], C.RESIDUAL[1], C.GENERAL[1], C.GENERAL[3], C.GENERAL[6]]:
        srcs, w, b, res = C.layer_data(l)
        x = C.cat_input(l, srcs)
        want = C.ternary_reference(l, x.double(), w.double(), b.double(), None if res is None else res.double())
        got = C.ternary_reference(l, x, w, b, res)
        assert tuple(got.shape) == (1, l.co) + C.out_shape(l)
        assert torch.equal(got.double(), want) and float(want.abs().max()) < 1 << 24
    l = C.FORM3D                                                                               # the slab evaluation == the whole
    srcs, w, b, res = C.layer_data(l)
    whole = C.ternary_reference(l, srcs[0], w, b, None)
    for z0, z1 in ((0, 2), (2, 5), (4, 6), (0, 6)):
        assert torch.equal(C.ternary_reference(l, srcs[0], w, b, None, z0, z1), whole[:, :, z0:z1])


def test_two_scale_split_is_what_the_family_states():
    """x = a (1 + b 2^-13): numpy's split16 (the activations' rule) gives hi = a, lo' = a b / 4 with hi + lo' 2^-11 == x bit for bit, and
    the weight packer of the C ABI (sd_conv3_f16x3_pack_weights_host) splits w = c (1 + d 2^-13) the same way"""
    a, b = C.tern((50, 64), 1).numpy(), C.tern((50, 64), 2).numpy()
    x = C.two_scale(torch.from_numpy(a), torch.from_numpy(b)).numpy()
    s = np_split16(x)
    assert np.array_equal(np_unsplit16(s).view(np.uint32), x.view(np.uint32))
    h = s.reshape(-1, 2, 32).view(np.float16).reshape(-1, 2, 64)
    assert np.array_equal(h[..., :32].astype(np.float32).reshape(x.shape), a)
    assert np.array_equal(h[..., 32:].astype(np.float32).reshape(x.shape), a * b * 0.25)
    assert 0.4 < float((a * b != 0).mean()) < 0.5                                              # lo' != 0 for 44 % of the elements
    from stardist_amd.lib import _native as N
    lib = N.lib()
    for ci, co, kz in ((32, 32, 1), (64, 32, 3)):
        shape = (co, ci) + ((3, 3, 3) if kz == 3 else (3, 3))
        c, d = C.tern(shape, 3).numpy(), C.tern(shape, 4).numpy()
        w = np.ascontiguousarray(C.two_scale(torch.from_numpy(c), torch.from_numpy(d)).numpy())
        out = np.empty(lib.sd_conv3_f16x3_packed_floats(ci, co, kz), np.float32)
        N.check(lib.sd_conv3_f16x3_pack_weights_host(N.ptr(w), ci, co, kz, N.ptr(out)))
        f16 = out[:-4].view(np.float16).reshape(co // 32, (ci // 32) * kz, 3, 3, 2, 2, 2, 32, 8)    # g, unit, dy, dx, block, plane, h, cout, j
        order = lambda v: np.transpose(v.reshape(co // 32, 32, ci // 32, 2, 2, 8, kz, 3, 3), (0, 2, 6, 7, 8, 3, 4, 1, 5)).reshape(f16[:, :, :, :, :, 0].shape)
        assert np.array_equal(f16[:, :, :, :, :, 0].astype(np.float32), order(c))
        assert np.array_equal(f16[:, :, :, :, :, 1].astype(np.float32), order(c * d * 0.25))


def test_two_scale_expected_values_are_float32():
    """the precondition of the two-scale family (asserted inside two_scale_reference) for every case: real channel and tap counts -- the
    length of the sums is what decides it -- at a reduced spatial extent (at most 24 per axis), which only changes how many outputs are
    looked at; the GPU test evaluates the same assertion at the full extents"""
    for l in C.TWO_SCALE:
        small = l._replace(shape=tuple(min(s, 24) for s in l.shape))
        dens = C.two_scale_density(l)
        assert dens == C.two_scale_density(small)
        parts, wparts, bias = C.two_scale_data(small, dens)
        want = C.two_scale_reference(small, parts, wparts, bias)
        assert tuple(want.shape) == (1, l.co) + small.shape
        assert float((want != want.round()).float().mean()) > 0.2                              # the cross terms show
    assert C.two_scale_density(C.TWO_SCALE[-1]) is not None and sum(c for c, _ in C.TWO_SCALE[-1].srcs) == 512


def test_integer_network_weights_keep_activations_small():
    """set_integer_weights: the CPU evaluation of the default 2D model stays integral and grows by at most 1 per layer (small extent here;
    the GPU test asserts the bound at its own extent)"""
    from stardist_amd.models import Config2D, StarDist2D
    m = StarDist2D(Config2D(n_rays=32), basedir=None, device="cpu", seed=0)
    C.set_integer_weights(m.net, 21).eval()
    x = torch.randint(0, 3, (1, 1, 64, 96), generator=torch.Generator().manual_seed(22)).float()
    f, peak = C.features_cpu(m.net, x)
    n_layers = sum(isinstance(mod, torch.nn.Conv2d) for mod in m.net.modules())
    assert bool((f == f.round()).all()) and 2 <= float(f.max()) and peak <= 2 + n_layers
