"""Cases, data and CPU references of the exact inference-convolution tests (test_gpu_conv_exact.py); test_cpu_conv_cases.py checks on the
CPU that the case lists reach the kernels' regimes and that the exactness preconditions hold on the references alone.  Importable
without a GPU.

The work partition of the 3x3 / 3x3x3 kernels is restated from stardist_amd/csrc/conv3x3_layout.h (TH, TW, CHUNK, MAX_CHUNKS) and the
launch code of conv3x3_f16.hip (conv3_f16x3_launch: tiles = D * ceil(H / TH) * ceil(W / TW), c_out / 32 groups of output channels,
floor(workgroups per CU * CUs / groups) * groups persistent workgroups, at most tiles * groups) and conv3x3_bf16.hip (one per CU).

Data families (see test_gpu_conv_exact.py):
  ternary    inputs, weights, biases, residuals in {-1, 0, 1}: every product and partial sum is a small integer, exact in f32 in any
             order and in every operand split (fp16 hi = x, lo' = 0; bf16 hi = x)
  two-scale  x = a (1 + b 2^-13), w = c (1 + d 2^-13), a, b, c, d ternary: sdconv::split2_f16 (the rule of both the activations and
             sd_conv3_f16x3_pack_weights_host) gives hi = a, lo' = a b / 4, so the cross-term accumulator of the split-fp16 kernel
             carries weight; the expected value is the kernel's statement hi.hi + 2^-11 (hi.lo' + lo'.hi) + bias, which must be
             representable in float32 (two_scale_reference asserts it: a precondition on the input, not a tolerance)."""
import json
import os
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the partition, restated ---------------------------------------------------------------------------------------------------
TH, TW = 8, 32                   # conv3x3_layout.h: output tile (rows, columns)
CHUNK, MAX_CHUNKS = 32, 16
CUS = 256                        # compute units of an MI355X (hipDeviceAttributeMultiprocessorCount)

# shape: output extent (H, W) or (D, H, W); srcs: ((channels, up per axis), ...) -- up 1: the source has half the resolution on that axis;
# k / stride: kernel size and strides; tf_same: TensorFlow 'same' padding; act: 0 linear, 1 ReLU; res: residual added before the activation
Layer = namedtuple("Layer", "shape srcs co k stride tf_same act res")


def L(shape, srcs, co, k=3, stride=None, tf_same=False, act=1, res=False):
    nd = len(shape)
    srcs = tuple((int(c), (int(up),) * nd if isinstance(up, int) else tuple(int(u) for u in up)) for c, up in srcs)
    return Layer(tuple(int(s) for s in shape), srcs, int(co), int(k), tuple(stride) if stride else (1,) * nd, bool(tf_same), int(act), bool(res))


def is_conv3(l):
    """the layer goes to csrc/conv3x3*.hip (models/unet._hand_conv); otherwise to conv_general.hip"""
    cs = [c for c, _ in l.srcs]
    if not (l.k == 3 and all(s == 1 for s in l.stride) and not l.tf_same):
        return False
    if cs == [1]:
        return l.co % 4 == 0 and not l.res
    return all(c % CHUNK == 0 for c in cs) and sum(cs) <= CHUNK * MAX_CHUNKS and l.co % 32 == 0


def n_tiles(shape):
    D = 1 if len(shape) == 2 else shape[0]
    H, W = shape[-2:]
    return D * (-(-H // TH)) * (-(-W // TW))


def workgroups(shape, co, per_cu):
    """(launched, wanted) workgroups of a 3x3 layer over 32-channel chunks"""
    groups = co // 32
    blocks = max((per_cu * CUS // groups) * groups, groups)
    want = n_tiles(shape) * groups
    return min(blocks, want), want


def loop_regime(shape, co, per_cu):
    """'fewer': less work than the persistent launch holds; 'exact': one tile per workgroup; 'more': the loop runs (a float: iterations)"""
    groups = co // 32
    blocks = max((per_cu * CUS // groups) * groups, groups)
    want = n_tiles(shape) * groups
    return "fewer" if want < blocks else ("exact" if want == blocks else want / blocks)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
# ragged tiles: every residue of W mod TW and of H mod TH, W < TW, H < TH, H = 1 (2D); D = 1, 2, 3 (3D)
SWEEP2D = [L((9 + (w % 8), w), [(32, 0)], 32) for w in range(33, 65)] + \
          [L((1, 40), [(32, 0)], 32), L((5, 7), [(32, 0)], 64), L((3, 1), [(32, 0)], 32), L((20, 31), [(64, 0)], 32), L((7, 100), [(32, 0)], 32, act=0)]
SWEEP3D = [L((1, 9, 33), [(32, 0)], 32), L((2, 8, 40), [(32, 0)], 32), L((3, 17, 31), [(32, 0)], 64), L((5, 7, 70), [(64, 0)], 32, act=0),
           L((2, 1, 5), [(32, 0)], 32)]
# the persistent loop at f16x3's two workgroups per CU (512) and one (256, also bf16x6): fewer / exactly as many / more tiles x groups
LOOP = [L((64, 1024), [(32, 0)], 32),        # 256 tiles: fewer (2 per CU), exact (1 per CU)
        L((128, 1024), [(32, 0)], 32),       # 512 tiles: exact (2 per CU), 2 iterations (1 per CU)
        L((64, 512), [(32, 0)], 128),        # 128 tiles x 4 groups = 512
        L((4, 32, 512), [(32, 0)], 64),      # 3D: 256 tiles x 2 groups = 512
        L((136, 2048), [(32, 0)], 32)]       # 1088 tiles: 2 full iterations and a ragged third (2 per CU)
# every form of the ternary family, at extents with ragged tiles on both axes
FORM2D = L((43, 75), [(32, 0)], 64)
FORM3D = L((6, 19, 41), [(32, 0)], 64)
TWO_SRC = [L((48, 80), [(64, 1), (32, 0)], 32), L((42, 66), [(128, 1), (128, 0)], 128), L((6, 18, 44), [(64, 1), (32, 0)], 32),
           L((5, 18, 44), [(32, (0, 1, 1)), (32, 0)], 32), L((4, 10, 36), [(256, 1), (256, 0)], 256)]
RESIDUAL = [L((41, 70), [(64, 0)], 64, res=True), L((6, 18, 40), [(64, 0)], 64, res=True), L((5, 17, 33), [(32, 0)], 32, res=True, act=0)]
FUSED_HEAD = [L((37, 70), [(32, 0)], 128), L((5, 19, 33), [(32, 0)], 128), L((40, 33), [(64, 0)], 256, act=0)]
ROWS = [L((70, 90), [(32, 0)], 128), L((9, 20, 37), [(32, 0)], 128), L((33, 40), [(64, 0)], 64), L((6, 10, 12), [(64, 0)], 32)]
FIRST_LAYER = [L((61, 83), [(1, 0)], 32), L((7, 21, 34), [(1, 0)], 32), L((1, 9, 5), [(1, 0)], 32), L((264, 300), [(1, 0)], 32)]
GENERAL = [L((20, 40, 70), [(1, 0)], 32, k=7, act=0),                                    # the ResNet stem
           L((13, 33, 71), [(32, 0)], 64, stride=(1, 2, 2), tf_same=True),              # strided, TensorFlow 'same' on odd extents
           L((9, 21, 35), [(64, 0)], 64, stride=(2, 2, 2), tf_same=True),
           L((9, 21, 35), [(64, 0)], 64, stride=(2, 2, 2), tf_same=True, res=True),
           L((13, 33, 71), [(32, 0)], 64, k=1, stride=(1, 2, 2), tf_same=True, act=0),   # the shortcut projection
           L((90, 130), [(3, 0)], 32),                                                   # the 3-channel first layer
           L((48, 81), [(32, 0)], 32, k=5),
           L((50, 70), [(48, 0)], 48), L((6, 20, 30), [(48, 0)], 96)]                    # unet_n_filter_base = 48
UPCAT48 = [((44, 60), 96, 48, (2, 2), 48), ((4, 20, 28), 96, 48, (1, 2, 2), 48)]        # (shape, c up, c skip, pool, c_out)
# two-scale family (f16x3): f32, split16 in + out, two sources; the last: 512 channels x 27 taps, the longest sums a layer can have
TWO_SCALE = [L((43, 75), [(32, 0)], 64), L((6, 19, 41), [(32, 0)], 64, act=0), L((48, 80), [(64, 1), (32, 0)], 32),
             L((6, 18, 44), [(64, 1), (32, 0)], 32), L((128, 1024), [(32, 0)], 32), L((4, 10, 36), [(256, 1), (256, 0)], 256)]
# offsets: the activation passes 2^31 bytes (HEADLINE3D holds 256^3 x 32); 2^32 bytes and 2^31 elements; 2^32 elements in and out
BIG_OUT = L((264, 256, 256), [(32, 0)], 128)
BIG_BOTH = L((560, 560, 560), [(32, 0)], 32)
HEADLINE2D, HEADLINE3D, RESNET_SLAB = (2048, 2048), (256, 256, 256), (32, 256, 256)
NET2D, NET3D = (1024, 1024), (128, 128, 128)           # the whole-network tests


def demo3d_config():
    from stardist_amd.models import Config3D
    with open(os.path.join(ROOT, "tests", "golden", "pretrained", "StarDist3D", "3D_demo", "config.json")) as fh:
        conf = json.load(fh)
    keys = ("n_rays", "grid", "anisotropy", "backbone", "resnet_n_blocks", "resnet_kernel_size", "resnet_n_filter_base",
            "resnet_n_conv_per_block", "resnet_activation", "resnet_batch_norm", "net_conv_after_resnet")
    return Config3D(**{k: (tuple(conf[k]) if isinstance(conf[k], list) else conf[k]) for k in keys})


def planned_layers(net, extent):
    """the distinct convolution layers (as Layer tuples, heads excluded) a forward pass of the StarDistNet `net` runs on an input of
    `extent`, read from the model's own modules in graph order"""
    from stardist_amd.models import unet as U
    nd = net.nd
    out = []

    def add(conv, shape, srcs, act, stride=None, tf_same=False, res=False):
        k = set(int(v) for v in conv.kernel_size)
        assert len(k) == 1 and sum(c for c, _ in srcs) == conv.in_channels
        l = L(shape, srcs, conv.out_channels, k=k.pop(), stride=stride, tf_same=tf_same, act=act, res=res)
        if l not in out:
            out.append(l)

    def seq(mods, shape, c):
        for m in mods:
            conv, _, kind = m.parts()
            add(conv, shape, [(c, 0)], kind)
            c = conv.out_channels
        return c
    shape, c = tuple(extent), None
    for st in net.pre:
        c = seq(st["convs"], shape, st["convs"][0][0].in_channels)
        shape = tuple(s // p for s, p in zip(shape, st.pool))
    bb = net.backbone
    if isinstance(bb, U.UNetBlock):
        skips = []
        c = bb.down[0][0][0].in_channels
        for blk in bb.down:
            c = seq(blk, shape, c)
            skips.append((c, shape))
            shape = tuple(s // p for s, p in zip(shape, bb.pool))
        c = seq(bb.middle, shape, c)
        for blk, (cs, sshape) in zip(bb.up, reversed(skips)):
            conv, _, kind = blk[0].parts()
            add(conv, sshape, [(c, tuple(int(p == 2) for p in bb.pool)), (cs, 0)], kind)
            shape = sshape
            c = seq(blk[1:], shape, conv.out_channels)
    else:
        for m in bb:
            if isinstance(m, U.ConvAct):
                c = seq([m], shape, m[0].in_channels)
                continue
            kind = lambda a: 0 if isinstance(a, torch.nn.Identity) else 1
            stages = m._stages()
            oshape = tuple(-(-s // p) for s, p in zip(shape, m.pool))
            add(stages[0][0], shape, [(c, 0)], kind(stages[0][2]), stride=m.pool, tf_same=True)     # (strided: `shape` is the input extent)
            if m.proj is not None:
                add(m.proj, shape, [(c, 0)], 0, stride=m.pool, tf_same=True)
            c = stages[0][0].out_channels
            for conv, _, act in stages[1:]:
                add(conv, oshape, [(c, 0)], kind(m.act) if act is None else kind(act), res=act is None)
            shape = oshape
    if isinstance(net.features, U.ConvAct):
        conv, _, kind = net.features.parts()
        add(conv, shape, [(c, 0)], kind)
    return out


def headline_layers(which):
    """'2d': StarDist2D(Config2D(n_rays=32)) at 2048^2; '3d': StarDist3D(Config3D(rays=96)) at 256^3; 'resnet': the 3D_demo ResNet on a
    32-plane slab of 256^3 -- from the planned layers of the model itself"""
    from stardist_amd.models import Config2D, Config3D, StarDist2D, StarDist3D
    if which == "2d":
        return planned_layers(StarDist2D(Config2D(n_rays=32), basedir=None, device="cpu", seed=0).net, HEADLINE2D)
    if which == "3d":
        return planned_layers(StarDist3D(Config3D(rays=96), basedir=None, device="cpu", seed=0).net, HEADLINE3D)
    return planned_layers(StarDist3D(demo3d_config(), basedir=None, device="cpu", seed=0).net, RESNET_SLAB)


# ---- data ----------------------------------------------------------------------------------------------------------------------
def seed_of(l, salt=0):
    return (hash((l.shape, l.srcs, l.co, l.k, l.stride, l.tf_same, l.act, l.res)) & 0x7FFFFFF) * 8 + salt


def tern(shape, seed, density=None):
    """ternary float32 CPU tensor: values in {-1, 0, 1}; density: fraction of non-zeros (default 2/3)"""
    g = torch.Generator().manual_seed(int(seed))
    t = torch.randint(-1, 2, shape, generator=g, dtype=torch.int8).float()
    if density is not None:
        t *= (torch.rand(shape, generator=g) < density * 1.5).float()
    return t


def cl_tensor(shape_cl, seed, density=None):
    """(1, C, *S) channels-last view of a ternary tensor generated as (1, *S, C)"""
    t = tern((1,) + tuple(shape_cl), seed, density)
    nd = len(shape_cl) - 1
    return t.permute(0, nd + 1, *range(1, nd + 1))


def src_shape(l, k):
    c, up = l.srcs[k]
    return tuple(s >> u for s, u in zip(in_shape(l), up)) + (c,)


def in_shape(l):
    """input extent: the output extent unless the layer is strided (the cases then state the INPUT extent in `shape`)"""
    return l.shape


def out_shape(l):
    return tuple(-(-s // st) for s, st in zip(l.shape, l.stride))


def layer_data(l, density=None):
    """ternary (sources [(1, c, *S) channels-last], weight (co, ci, *k), bias (co,), residual or None) of a layer"""
    nd = len(l.shape)
    srcs = [cl_tensor(src_shape(l, k), seed_of(l, k), density) for k in range(len(l.srcs))]
    ci = sum(c for c, _ in l.srcs)
    w = tern((l.co, ci) + (l.k,) * nd, seed_of(l, 3), density)
    b = tern((l.co,), seed_of(l, 4))
    res = cl_tensor(out_shape(l) + (l.co,), seed_of(l, 5)) if l.res else None
    return srcs, w, b, res


def cat_input(l, srcs):
    """Concatenate([UpSampling(src0), src1]) as the reference's graph has it: (1, ci, *S)"""
    xs = []
    for t, (_, up) in zip(srcs, l.srcs):
        for d, u in enumerate(up):
            if u:
                t = t.repeat_interleave(2, dim=2 + d)
        xs.append(t)
    return xs[0] if len(xs) == 1 else torch.cat(xs, 1)


def tf_pads(n, k, s):
    total = max(k - s, 0) if n % s == 0 else max(k - n % s, 0)
    return total // 2, total - total // 2


def conv_ref(l, x, w, z0=None, z1=None):
    """float32 conv of the concatenated input x (1, ci, *S) on the CPU, no bias; z0, z1: the output planes [z0, z1) only (3x3x3, stride 1)"""
    nd = len(l.shape)
    f = F.conv2d if nd == 2 else F.conv3d
    if z0 is not None:
        assert nd == 3 and l.k == 3 and not l.tf_same and all(s == 1 for s in l.stride)
        D = l.shape[0]
        lo, hi = max(z0 - 1, 0), min(z1 + 1, D)
        xs = F.pad(x[:, :, lo:hi], (0, 0, 0, 0, lo - (z0 - 1), (z1 + 1) - hi))
        return f(xs, w, padding=(0, 1, 1))
    if l.tf_same:
        pads = []
        for d in reversed(range(nd)):
            pads += list(tf_pads(x.shape[2 + d], l.k, l.stride[d]))
        return f(F.pad(x, pads), w, stride=l.stride)
    return f(x, w, stride=l.stride, padding=l.k // 2)


def epilogue(l, y, b, res):
    y = y + b.view((1, -1) + (1,) * len(l.shape))
    if res is not None:
        y = y + res
    return torch.relu(y) if l.act else y


def ternary_reference(l, x, w, b, res, z0=None, z1=None):
    """act(conv(x) + b (+ res)) in float32 on the CPU: exact for ternary data (integers below 2^24 in any order)"""
    r = res if (res is None or z0 is None) else res[:, :, z0:z1]
    return epilogue(l, conv_ref(l, x, w, z0, z1), b, r)


def two_scale(base, fine):
    """base (1 + fine 2^-13) in float32: exact"""
    return base * (1.0 + fine * 2.0 ** -13)


def two_scale_data(l, density=None):
    """((a, b) per source, (c, d), bias) ternary parts of the two-scale family"""
    nd = len(l.shape)
    parts = [(cl_tensor(src_shape(l, k), seed_of(l, 10 + k), density), cl_tensor(src_shape(l, k), seed_of(l, 20 + k))) for k in range(len(l.srcs))]
    ci = sum(c for c, _ in l.srcs)
    wshape = (l.co, ci) + (l.k,) * nd
    return parts, (tern(wshape, seed_of(l, 30), density), tern(wshape, seed_of(l, 31))), tern((l.co,), seed_of(l, 32))


def two_scale_reference(l, parts, wparts, bias):
    """the split-fp16 kernel's statement on the two-scale data: conv(x_hi, w_hi) + 2^-11 (conv(x_hi, w_lo') + conv(x_lo', w_hi)) + bias with
    hi = a, lo' = a b / 4 (no lo.lo term), then the activation -- each convolution in float32 (integers and multiples of 1/4: exact), combined
    in float64.  Asserts the precondition: every expected value survives a round trip through float32.  -> float32"""
    hi = cat_input(l, [a for a, _ in parts])
    lo = cat_input(l, [a * b * 0.25 for a, b in parts])
    c, d = wparts
    acc0 = conv_ref(l, hi, c).double() + bias.double().view((1, -1) + (1,) * len(l.shape))
    acc1 = conv_ref(l, hi, c * d * 0.25).double() + conv_ref(l, lo, c).double()
    want = acc0 + acc1 * 2.0 ** -11
    assert bool((want.float().double() == want).all()), "the expected value is not a float32: reduce the density of this case"
    assert float(acc0.abs().max()) < 2 ** 24 and float(acc1.abs().max()) < 2 ** 22
    want = want.float()
    return torch.relu(want) if l.act else want


# density of non-zeros of the two-scale cases: sums of 512 x 27 terms stay representable with fewer of them
def two_scale_density(l):
    return 0.25 if sum(c for c, _ in l.srcs) * l.k ** len(l.shape) > 4096 else None


def np_cl(t):
    """(1, C, *S) tensor -> numpy (*S, C)"""
    nd = t.dim() - 2
    return t[0].permute(*(list(range(1, nd + 1)) + [0])).contiguous().cpu().numpy()


# ---- whole networks with integer weights -----------------------------------------------------------------------------------------
def set_integer_weights(net, seed):
    """every convolution of `net`: per output channel one tap of weight +1 and one of -1 (distinct (input channel, tap) positions, drawn from
    the seed), bias in {0, 1}.  With non-negative integer inputs every activation behind a ReLU is a non-negative integer that grows by at
    most 1 per layer (relu(x_p - x_q + bias) <= max x + 1): the features stay far inside the range where fp16 holds integers exactly."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.Conv3d)):
                co = m.out_channels
                per = m.weight[0].numel()
                w = torch.zeros((co, per))
                pos = torch.randint(0, per, (co,), generator=g)
                neg = (pos + 1 + torch.randint(0, max(per - 1, 1), (co,), generator=g)) % per
                w[torch.arange(co), pos] = 1.0
                if per > 1:
                    w[torch.arange(co), neg] = -1.0
                m.weight.copy_(w.view_as(m.weight))
                if m.bias is not None:
                    m.bias.copy_(torch.randint(0, 2, (co,), generator=g).float())
    return net


def features_cpu(net, x):
    """(features (1, C, *S) float32, largest activation) of the CPU evaluation of net's modules on x (1, c, *S)"""
    from stardist_amd.models import unet as U
    peak = [0.0]

    def hook(m, inp, out):
        peak[0] = max(peak[0], float(out.abs().max()))
    hs = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.Conv3d))]
    try:
        with torch.no_grad():
            for st in net.pre:
                x = U.max_pool(st["convs"](x), st.pool)
            f = net.features(net.backbone(x))
    finally:
        for h in hs:
            h.remove()
    return f, peak[0]
