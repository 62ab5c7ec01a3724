"""Cases, data and CPU references of the exact tests of the kernels between the convolutions (stardist_amd/csrc/unet_ops.hip;
test_gpu_unet_ops_exact.py); test_cpu_unet_ops_cases.py checks on the CPU that the case lists reach the regimes their names claim, that
the constants restated here are the ones in the source, and that the references are right.  Importable without a GPU; numpy only.

Every kernel of unet_ops.hip is a grid-stride loop under a block cap: a launch holds `cap * items per block` items per pass, a larger
problem takes the loop again.  PER_BLOCK / CAP restate the launch code; passes(kernel, n_items) is the number of passes.

Data families:
  special    float32 with ties inside a window, -0.0 and +0.0 in one window, +-inf, all-negative windows, denormals, the fp16 range edge
             (65504 and the next float above it); with_nans() adds NaNs of both signs (a window with one, a window of nothing else)
  two-scale  the values a (1 + b 2^-13) of _conv_cases.two_scale (both split16 terms carry weight)
  integer    small integers: features >= 0 behind the ReLU, ternary weights, small integer biases -- every partial sum of a head stays
             below 2^24 (asserted by the references), so every summation order gives the same float32 and an int64 matmul is the reference

The special-value rule (include/stardist_hip.h): max-pooling PROPAGATES a NaN -- a window that holds one gives NaN,
whatever its sign -- in the f32 and in the split16 form alike; otherwise the maximum in the total order -inf < ... < -0 < +0 < ... < +inf.
The ReLU of the epilogues is v > 0 ? v : +0 (a NaN and -0 give +0).  Where a result is NaN only its class is compared (same_bits)."""
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "stardist_amd", "csrc", "unet_ops.hip")

# ---- the launch arithmetic, restated -------------------------------------------------------------------------------------------
# kernel -> block cap; items per block (bias_act_dot: pixels per block = 256 / LPP, LPP = C / 4; head_rows: 4 waves x 32 rows)
CAP = dict(maxpool=256 * 64, maxpool_split16=256 * 64, pack=256 * 64, unpack=256 * 64, upcat=262144, bias_act_cl4=65536, bias_act=65536,
           bias_act_dot=256 * 32, dot_combine=256 * 32, head_rows=256 * 3)
PER_BLOCK = dict(maxpool=256, maxpool_split16=256, pack=256, unpack=256, upcat=256, bias_act_cl4=256, bias_act=256, dot_combine=32,
                 head_rows=128)
HEAD_LDS = 64 * 1024


def per_pass(kernel, C=None):
    """items one pass of the grid-stride loop holds (maxpool / upcat / bias_act_cl4: channel quads; maxpool_split16 / pack / unpack:
    (pixel, 8-channel octet); bias_act: values; bias_act_dot / dot_combine: pixels; head_rows: rows)"""
    if kernel == "bias_act_dot":
        return CAP[kernel] * (256 // (C // 4))
    return CAP[kernel] * PER_BLOCK[kernel]


def passes(kernel, n_items, C=None):
    return n_items / per_pass(kernel, C)


def loops(kernel, n_items, C=None):
    """iterations of the loop in the busiest thread"""
    return -(-int(n_items) // per_pass(kernel, C))


def source_constants(path=SOURCE):
    """(CAP, PER_BLOCK, bias_act_dot's threads per block, head_rows' LDS limit) read from the launch code of unet_ops.hip"""
    src = open(path).read()
    parts = re.split(r'\n(?:extern "C" |static )int (\w+)\(', src)
    body = dict(zip(parts[1::2], parts[2::2]))

    def prod(s):
        return int(np.prod([int(v) for v in s.split("*")]))

    def cap(fn):
        caps = {prod(m) for m in re.findall(r"blocks > ([\d *]+)\) blocks = ", body[fn])} | \
               {prod(m) for m in re.findall(r"blocks < (\d+) \? blocks : ", body[fn])}
        assert len(caps) == 1, (fn, caps)
        return caps.pop()

    def per(fn, var):
        m = re.search(r"\(%s \+ (\d+)\) / (\d+)" % var, body[fn])
        assert int(m.group(1)) + 1 == int(m.group(2))
        return int(m.group(2))
    fns = dict(maxpool="sd_maxpool_ndhwc_device", maxpool_split16="sd_maxpool_split16_ndhwc_device", pack="sd_split16_pack_device",
               unpack="sd_split16_unpack_device", upcat="sd_upcat_ndhwc_device", bias_act_cl4="bias_act_impl", bias_act="bias_act_impl",
               bias_act_dot="sd_bias_act_dot_device", dot_combine="sd_dot_combine_device", head_rows="sd_head_rows_device")
    caps = {k: cap(f) for k, f in fns.items()}
    pb = dict(maxpool=per(fns["maxpool"], "n4"), maxpool_split16=per(fns["maxpool_split16"], "n"), pack=per(fns["pack"], "n"),
              unpack=per(fns["unpack"], "n"), upcat=per(fns["upcat"], "n4"), bias_act_cl4=per("bias_act_impl", "n4"),
              bias_act=per("bias_act_impl", "n"), dot_combine=per(fns["dot_combine"], "n_pix"),
              head_rows=per(fns["head_rows"], "n_rows") * per(fns["head_rows"], "tiles"))
    dot_threads = int(re.search(r"const long long per_block = (\d+) / lpp;", body[fns["bias_act_dot"]]).group(1))
    assert "blocks = (n_pix + per_block - 1) / per_block" in body[fns["bias_act_dot"]]
    lds = prod(re.search(r"lds > ([\d *]+) \|\|", body[fns["head_rows"]]).group(1))
    # the loops really are grid-stride loops over these items
    for text in ("const long long stride = (long long)gridDim.x * blockDim.x;", "const long long groups = (long long)gridDim.x * (256 / LPP);",
                 "const long long per = (long long)gridDim.x * 32;", "tile += (long long)gridDim.x * 4"):
        assert text in src, text
    return caps, pb, dot_threads, lds


# ---- the cases -----------------------------------------------------------------------------------------------------------------
# max-pool: input extent (D, H, W) (2D: D = 1), channels, pool (pz, py, px); loops: iterations of the grid-stride loop the name claims
Pool = namedtuple("Pool", "name shape C pool loops")
# whole tensors, special values: every pool, every channel count, a remainder on every pooled axis
POOL_SMALL = [Pool("2x2 c4", (1, 37, 51), 4, (1, 2, 2), 1), Pool("2x2 c32", (1, 39, 53), 32, (1, 2, 2), 1),
              Pool("2x2 c48", (1, 33, 47), 48, (1, 2, 2), 1), Pool("2x2x2 c96", (9, 19, 23), 96, (2, 2, 2), 1),
              Pool("1x2x2 c128", (5, 19, 23), 128, (1, 2, 2), 1), Pool("4x2 c32", (1, 38, 51), 32, (1, 4, 2), 1),
              Pool("2x2x2 c32", (7, 21, 19), 32, (2, 2, 2), 1), Pool("4x2 c96", (1, 23, 13), 96, (1, 4, 2), 1)]
# the loop (2D, integer data with ties, compared on bands of output rows): exactly one pass, two with a ragged second, three
POOL_LOOP_F32 = [Pool("one pass exactly", (1, 513, 1025), 128, (1, 2, 2), 1), Pool("two passes, ragged", (1, 731, 735), 128, (1, 2, 2), 2),
                 Pool("three passes", (1, 1031, 1027), 128, (1, 2, 2), 3)]
POOL_LOOP_SPLIT = [Pool("one pass exactly", (1, 1025, 1025), 128, (1, 2, 2), 1), Pool("two passes, ragged", (1, 1041, 1021), 128, (1, 2, 2), 2),
                   Pool("three passes", (1, 1461, 1469), 128, (1, 2, 2), 3)]
POOL_BIG = Pool("416^3 x 32", (416, 416, 416), 32, (2, 2, 2), None)


def pool_out_shape(c):
    return tuple(s // p for s, p in zip(c.shape, c.pool))


def pool_items(c, split):
    return int(np.prod(pool_out_shape(c))) * (c.C // 8 if split else c.C // 4)


# upcat: output extent (D, H, W), channels of the up-sampled and of the skip tensor, up mask (1: x, 2: y, 4: z)
Upcat = namedtuple("Upcat", "name shape ca cb up loops")
UPCAT = [Upcat("2D up %d" % up, (1, 18, 26), ca, cb, up, 1) for up, (ca, cb) in zip((1, 2, 3), ((96, 48), (48, 96), (4, 4)))] + \
        [Upcat("3D up %d" % up, (6, 10, 14), ca, cb, up, 1) for up, (ca, cb) in
         zip(range(1, 8), ((96, 48), (48, 96), (4, 4), (128, 64), (96, 48), (48, 96), (128, 64)))] + \
        [Upcat("square", (1, 24, 24), 4, 4, 1, 1), Upcat("square", (1, 24, 24), 4, 4, 2, 1),
         Upcat("over one pass", (1, 1200, 1180), 128, 64, 3, 2)]
UPCAT_BIG = Upcat("output past 2^32 bytes", (1, 2400, 2400), 128, 64, 3, None)


def upcat_items(c):
    return int(np.prod(c.shape)) * ((c.ca + c.cb) // 4)


# pack / unpack: (pixels, channels) one below, at and one above the boundary of a pass
def pack_cases():
    out = []
    for C in (32, 96, 256):
        edge = per_pass("pack") // (C // 8)                # (96 channels: 12 octets per pixel do not divide a pass; edge is then just below it)
        out += [(edge - 1, C), (edge, C), (edge + 1, C)]
    return out


# bias_act: the cl4 path, and the generic one: odd C, inner > 1, and x / the addend / the bias one float off 16-byte alignment, each alone
# (offset: floats off for (x, addend, bias); a misaligned addend only counts where there is one: sd_bias_act_device then takes cl4)
BiasAct = namedtuple("BiasAct", "name n_outer C inner offset path loops")
BIAS_ACT = [BiasAct("cl4", 4099, 32, 1, (0, 0, 0), "bias_act_cl4", 1), BiasAct("cl4 c48", 1001, 48, 1, (0, 0, 0), "bias_act_cl4", 1),
            BiasAct("odd channels", 3001, 7, 1, (0, 0, 0), "bias_act", 1), BiasAct("inner", 3, 6, 1001, (0, 0, 0), "bias_act", 1),
            BiasAct("x misaligned", 2000, 32, 1, (1, 0, 0), "bias_act", 1), BiasAct("addend misaligned", 2000, 32, 1, (0, 1, 0), "bias_act", 1),
            BiasAct("bias misaligned", 2000, 32, 1, (0, 0, 1), "bias_act", 1), BiasAct("all misaligned", 2000, 32, 1, (1, 1, 1), "bias_act", 1),
            BiasAct("cl4 over one pass", 65536 * 256 * 4 // 128 + 77, 128, 1, (0, 0, 0), "bias_act_cl4", 2),
            BiasAct("generic over one pass", 65536 * 256 // 7 + 5000, 7, 1, (0, 0, 0), "bias_act", 2)]
BIAS_ACT_BIG = BiasAct("cl4 past 2^31 elements", (1 << 31) // 32 + 4099, 32, 1, (0, 0, 0), "bias_act_cl4", None)


def bias_act_items(c):
    n = c.n_outer * c.C * c.inner
    return n // 4 if c.path == "bias_act_cl4" else n


# bias_act_dot: (C, pixels): one pass, exactly two, two and a ragged tail
DOT = [(C, n) for C in (32, 64, 128, 256) for n in (per_pass("bias_act_dot", C), 2 * per_pass("bias_act_dot", C), 2 * per_pass("bias_act_dot", C) + 77)]
# dot_combine: every residue of n_pix mod 32 around the boundary of a pass, per G
COMBINE_G = (1, 2, 4, 8)
COMBINE_N = [per_pass("dot_combine") - 16 + r for r in range(32)]
# head_rows: (C, R) -- every CT = ceil(R / 32), every C, inside the LDS limit
HEAD = [(32, 7), (64, 32), (128, 33), (64, 64), (128, 96), (64, 100), (256, 32)]
HEAD_N_PIX = 3001
HEAD_RESIDUES = list(range(1, 34)) + [64 + r for r in range(0, 32, 5)] + [1000 + r for r in range(32)]
HEAD_LOOP_ROWS = 2 * per_pass("head_rows") + 1000                       # two passes and a ragged third


def head_ct(R):
    return -(-R // 32)


def head_lds(C, R):
    return C * (head_ct(R) * 32 + 1) * 4


# ---- split16 (the statement of the form in numpy) ------------------------------------------------------------------------------
def np_split16(x_cl):
    """numpy statement of the form for a channels-last array (..., C), C % 32 == 0: float32 array of the same shape holding, per pixel
    and 32-channel chunk, 32 float16 hi terms then 32 float16 lo' terms (hi = fp16(x), lo' = fp16((x - hi) * 2^11), round to nearest even)"""
    x = np.ascontiguousarray(x_cl, np.float32)
    C = x.shape[-1]
    assert C % 32 == 0
    v = x.reshape(-1, C // 32, 32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = ((v - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    both = np.concatenate([hi, lo], axis=-1)                     # (n, chunks, 64) float16
    return np.ascontiguousarray(both).view(np.float32).reshape(x.shape)


def np_unsplit16(s_cl):
    s = np.ascontiguousarray(s_cl, np.float32)
    C = s.shape[-1]
    h = s.reshape(-1, C // 32, 32).view(np.float16).reshape(-1, C // 32, 64)
    with np.errstate(invalid="ignore"):
        return (h[..., :32].astype(np.float32) + h[..., 32:].astype(np.float32) * np.float32(2.0 ** -11)).reshape(s.shape)


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def same_bits(got, want, half=False):
    """boolean array: the elements agree bit for bit, or are both NaN.  half: float32 arrays that hold split16 words, compared per fp16 term"""
    f, u = (np.float16, np.uint16) if half else (np.float32, np.uint32)
    g, w = np.ascontiguousarray(got).view(f), np.ascontiguousarray(want).view(f)
    return (g.view(u) == w.view(u)) | (np.isnan(g) & np.isnan(w))


# ---- data --------------------------------------------------------------------------------------------------------------------------
F16_MAX = np.float32(65504.0)
ABOVE_F16_MAX = np.nextafter(F16_MAX, np.float32(np.inf), dtype=np.float32)
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 6e-8, -6e-8, 2.0 ** -14, F16_MAX, -F16_MAX, ABOVE_F16_MAX,
                     -ABOVE_F16_MAX, 1.0, -1.0, 1.0 + 2.0 ** -13, 1.0 - 2.0 ** -13, 0.5, -0.5, 2.0, -2.0], np.float32)
# (no finite value whose hi overflows: beside an infinity in one window its pair (inf, -inf) ties with the infinity's (inf, NaN), and
#  a tensor that holds either is flagged as outside the range anyway)


def special_values(shape, seed, window=None):
    """float32 (*shape) of the `special` family (no NaN).  window: (D, H, W) pool of a (D, H, W, C) tensor -- whole windows are then given
    a class: all negative, only zeros of both signs, all equal, all -inf, only denormals, only -0.0"""
    rng = np.random.RandomState(seed)
    x = np.round(rng.standard_normal(shape) * 4).astype(np.float32) / np.float32(4)                  # quarter steps: ties are common
    pick = rng.randint(0, 3, shape) == 0
    x[pick] = SPECIALS[rng.randint(0, len(SPECIALS), int(pick.sum()))]
    if window is not None:
        O = tuple(s // p for s, p in zip(shape[:3], window))
        C = shape[3]
        v = x[:O[0] * window[0], :O[1] * window[1], :O[2] * window[2]].reshape(O[0], window[0], O[1], window[1], O[2], window[2], C)
        cls = rng.randint(0, 16, (O[0], 1, O[1], 1, O[2], 1, C))
        neg = -np.abs(v) - np.float32(0.25)
        zeros = np.where(rng.randint(0, 2, v.shape) == 0, np.float32(0.0), np.float32(-0.0))
        den = np.where(rng.randint(0, 2, v.shape) == 0, np.float32(1e-40), np.float32(-3e-41)) * rng.randint(1, 4, v.shape).astype(np.float32)
        for k, rep in ((8, neg), (9, zeros), (10, v[:, :1, :, :1, :, :1]), (11, np.float32(-np.inf)), (12, den), (13, np.float32(-0.0))):
            v[...] = np.where(cls == k, rep, v)                                                        # (v is a view of x)
    return x


def with_nans(x, seed, window=None):
    """a copy of x with NaNs of both signs (quiet, with and without payload) on about 2 % of the elements; window: also whole windows of NaN"""
    rng = np.random.RandomState(seed)
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFFFFFFF, 0x7F800001], np.uint32).view(np.float32)
    y = x.copy()
    pick = rng.randint(0, 50, x.shape) == 0
    y[pick] = nans[rng.randint(0, len(nans), int(pick.sum()))]
    if window is not None:
        O = tuple(s // p for s, p in zip(x.shape[:3], window))
        v = y[:O[0] * window[0], :O[1] * window[1], :O[2] * window[2]].reshape(O[0], window[0], O[1], window[1], O[2], window[2], x.shape[3])
        cls = rng.randint(0, 24, (O[0], 1, O[1], 1, O[2], 1, x.shape[3]))
        v[...] = np.where(cls == 0, nans[0], np.where(cls == 1, nans[1], v))
    return y


def two_scale_values(shape, seed):
    """a (1 + b 2^-13), a and b ternary: _conv_cases.two_scale as numpy (exact in float32)"""
    rng = np.random.RandomState(seed)
    a, b = rng.randint(-1, 2, shape).astype(np.float32), rng.randint(-1, 2, shape).astype(np.float32)
    return a * (np.float32(1) + b * np.float32(2.0 ** -13))


def fill_remainder(x, pool, value):
    """the planes / rows / columns of x (D, H, W, C) behind the last whole window <- value (Keras 'valid' never reads them)"""
    for ax, p in enumerate(pool):
        n = (x.shape[ax] // p) * p
        x[(slice(None),) * ax + (slice(n, None),)] = value
    return x


# ---- references ------------------------------------------------------------------------------------------------------------------
def order_key(x):
    """int32 keys in the total order of float32 (-inf < ... < -0 < +0 < ... < +inf; NaNs at the ends by sign); its own inverse"""
    b = np.ascontiguousarray(x, np.float32).view(np.int32)
    return np.where(b < 0, b ^ np.int32(0x7FFFFFFF), b)


def pool_ref(x, pool):
    """Keras MaxPooling 'valid', stride = pool, of x (D, H, W, C) float32: the maximum of each window in the total order, NaN where the
    window holds a NaN (the special-value rule)"""
    O = tuple(s // p for s, p in zip(x.shape[:3], pool))
    v = x[:O[0] * pool[0], :O[1] * pool[1], :O[2] * pool[2]].reshape(O[0], pool[0], O[1], pool[1], O[2], pool[2], x.shape[3])
    key = order_key(v).max(axis=(1, 3, 5))
    out = np.where(key < 0, key ^ np.int32(0x7FFFFFFF), key).view(np.float32).copy()
    out[np.isnan(v).any(axis=(1, 3, 5))] = np.nan
    return out


def upcat_ref(a, b, up):
    """Concatenate([UpSampling(a), b]) of channels-last (D, H, W, C) arrays; up: bit 0 x, 1 y, 2 z"""
    for ax, bit in ((0, 4), (1, 2), (2, 1)):
        if up & bit:
            a = np.repeat(a, 2, axis=ax)
    return np.concatenate([a, b], axis=-1)


def relu_ref(v):
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, v, np.float32(0.0)).astype(np.float32)


def bias_act_ref(x, addend, bias, act):
    """act((x + addend) + bias) in float32, in the kernel's order; x (n_outer, C, inner), bias (C,)"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = x if addend is None else x + addend
        v = v + bias.reshape(1, -1, 1)
    return relu_ref(v) if act else v.astype(np.float32)


def assert_exact(*arrays):
    """the precondition of the integer family: integers whose absolute sum stays below 2^24 (so does every partial sum in any order)"""
    for a in arrays:
        a = np.asarray(a)
        assert np.array_equal(a, np.round(a)) and float(np.abs(a).max(initial=0)) < 1 << 24


def dot_data(C, n, seed):
    """integer family of the one-channel head: x (n, C) in [-3, 3], bias (C,) in [-2, 2], w (C,) ternary, wb"""
    rng = np.random.RandomState(seed)
    return (rng.randint(-3, 4, (n, C)).astype(np.float32), rng.randint(-2, 3, C).astype(np.float32), rng.randint(-1, 2, C).astype(np.float32),
            np.float32(rng.randint(-3, 4)))


def dot_ref(x, bias, act, w, wb):
    """(features int64 (n, C), d int64 (n,)) of sd_bias_act_dot_device; asserts that the absolute sum of every dot product is < 2^24"""
    f = x.astype(np.int64) + (0 if bias is None else bias.astype(np.int64))
    if act:
        f = np.maximum(f, 0)
    assert_exact(x, w)
    assert int((np.abs(f) @ np.abs(w.astype(np.int64))).max()) + abs(int(wb)) < 1 << 24
    return f, f @ w.astype(np.int64) + int(wb)


def logistic64(d):
    return 1.0 / (1.0 + np.exp(-np.asarray(d, np.float64)))


def lane_terms(f, w):
    """the per-lane terms of k_bias_act_dot in float32, in its order: ((f0 w0 + f1 w1) + f2 w2) + f3 w3 of four consecutive channels"""
    t = (f.astype(np.float32) * w.astype(np.float32)).reshape(f.shape[0], -1, 4)
    return ((t[..., 0] + t[..., 1]) + t[..., 2]) + t[..., 3]


def butterfly_ref(terms, wb):
    """float32 sum of a pixel's L terms in the order of the xor butterfly (d[s] += d[s ^ o], o = L / 2 .. 1), then + wb: what both forms
    of the head state, for data on which the order matters"""
    d = terms.astype(np.float32).copy()
    idx = np.arange(d.shape[1])
    o = d.shape[1] // 2
    while o:
        d = d + d[:, idx ^ o]
        o //= 2
    return d[:, 0] + np.float32(wb)


def head_data(C, R, n_pix, seed):
    """integer family of the distance head: features (n_pix, C) in [0, 3], W (R, C) ternary, bias (R,) in [-4, 4]"""
    rng = np.random.RandomState(seed)
    return rng.randint(0, 4, (n_pix, C)).astype(np.float32), rng.randint(-1, 2, (R, C)).astype(np.float32), rng.randint(-4, 5, R).astype(np.float32)


def head_ref(feat, rows, W, bias, clamp):
    """max(clamp, bias + feat[rows] . W^T) by an int64 matmul -> float32; asserts the exactness precondition"""
    f = feat.astype(np.int64) if rows is None else feat.astype(np.int64)[rows]
    assert_exact(feat, W)
    b = np.zeros(W.shape[0], np.int64) if bias is None else bias.astype(np.int64)
    assert int((np.abs(f) @ np.abs(W.astype(np.int64)).T).max()) + int(np.abs(b).max()) < 1 << 24
    d = (f @ W.astype(np.int64).T + b).astype(np.float32)
    return np.maximum(d, np.float32(clamp))


def head_row_sets(n_pix, seed):
    """name -> int64 row indices: a permutation, descending, all equal, duplicates"""
    rng = np.random.RandomState(seed)
    perm = rng.permutation(n_pix).astype(np.int64)
    return {"permutation": perm, "descending": np.arange(n_pix - 1, -1, -1, dtype=np.int64), "all equal": np.full(777, n_pix - 1, np.int64),
            "duplicates": rng.permutation(np.repeat(perm[:500], 3))}


# ---- large offsets -------------------------------------------------------------------------------------------------------------
def marks(n_planes, per_plane, seed, n_random=3):
    """planes of a tensor of n_planes x per_plane elements to compare: the first and the last, those around the 2^31- and 2^32-element
    marks, and a seeded handful"""
    out = {0, n_planes - 1}
    for m in (1 << 31, 1 << 32):
        z = m // per_plane
        out.update(p for p in (z - 1, z, z + 1) if 0 <= p < n_planes)
    out.update(int(v) for v in np.random.RandomState(seed).choice(n_planes, n_random, replace=False))
    return sorted(out)
