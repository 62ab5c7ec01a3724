"""Cases, data and references of the exact prediction tests (test_gpu_predict_exact.py): the driver around the network -- _predict_setup and
the pad-and-crop resizer, _tile_slices, the HIP-graph cache, _select_rows with a tile origin, the per-tile border rule, the grid scaling
of the points and filter_points.  test_cpu_predict_cases.py checks on the CPU that the exactness preconditions hold, that the cases
reach what they are meant to reach, and that the exact comparison CAN fail (a shortened tile overlap).  Importable without a GPU.

Data families:
  integer  C.set_integer_weights on every convolution, the heads included, and inputs in {0, 1, 2}: every activation, the distances and
           the probability logit are small integers, the same float32 in any summation order, kernel form and tile position
  shift    set_shift_weights(net, axis, sign): every convolution has one +1 tap per output channel, at the extreme tap of `axis` on the
           side `sign` (centred on the other axes), bias 0 -- the network moves information along one axis in one direction as far as its
           receptive field goes.  The image (shift_image) is built from the tile plan: isolated impulses just beyond the read region of
           every cut tile, on the side the network looks towards, at every distance 1 .. reach + 2.  All weights and inputs are
           non-negative, so the network is monotone: an impulse a tile does not see can only lower its result, never cancel.

Tile plans (the default 2D U-Net: blocks of 8, overlap 52 -> 56 = 7 blocks): an axis of n tiles has at most ceil(n / 2) distinct tile extents
unless a block edge falls on a rounding tie, and an axis with n_tiles > blocks has one block per tile.  A search over all plans of the
default model finds at most 9 distinct tile shapes within 16 tiles when one axis is clamped (10 without a clamped axis), and 24 tiles as
the fewest that give 10 with one: MANY below is that plan (96 x 120, n_tiles (13, 2): 12 x 2 tiles of at most 96 x 120 pixels)."""
import contextlib
import copy
from collections import namedtuple

import numpy as np
import torch

import _conv_cases as C
from _exact import select_numpy

# shape: the image as given to predict (laid out as `axes`); n_tiles per IMAGE axis; seed: of the integer weights -- the first from 31 on with
# which at least a tenth of the probability logits lies on either side of 0 (a property of the data: evaluated on the CPU reference)
Case = namedtuple("Case", "name nd cfg shape axes n_tiles seed")

CASES = [
    Case("plain2d", 2, dict(n_rays=32), (200, 232), "YX", (3, 3), 40),
    Case("padded2d", 2, dict(n_rays=32), (197, 230), "YX", (3, 2), 40),                       # -> 200 x 232: both axes padded
    # grids: the smallest extents at which the middle of three tiles is cut on both sides and each of two tiles on one
    Case("grid22", 2, dict(n_rays=32, grid=(2, 2)), (368, 256), "YX", (3, 2), 31),            # blocks of 16, overlap 106 -> 112
    Case("grid42", 2, dict(n_rays=32, grid=(4, 2)), (736, 256), "YX", (3, 2), 35),            # blocks of (32, 16), overlap (214, 110) -> (224, 112)
    Case("class2d", 2, dict(n_rays=32, n_classes=2, n_channel_in=3), (3, 152, 232), "CYX", (1, 2, 3), 40),
    Case("unet3d", 3, dict(rays=16, grid=(1, 2, 2)), (64, 128, 184), "ZYX", (2, 2, 3), 31),   # blocks of (4, 8, 8), overlap (26, 50, 50) -> (28, 56, 56)
    Case("resnet3d", 3, dict(rays=16, backbone="resnet", grid=(1, 2, 2)), (40, 96, 112), "ZYX", (2, 2, 3), 32),   # blocks of (1, 2, 2), overlap (17, 30, 30)
    Case("many2d", 2, dict(n_rays=32), (96, 120), "YX", (13, 2), 40),                         # 12 blocks on Y: n_tiles is clamped
]
BY_NAME = {c.name: c for c in CASES}
MANY = BY_NAME["many2d"]


def make_model(case, device="cpu"):
    from stardist_amd.models import Config2D, Config3D, StarDist2D, StarDist3D
    Model, Config = (StarDist2D, Config2D) if case.nd == 2 else (StarDist3D, Config3D)
    m = Model(Config(**case.cfg), basedir=None, device=device, seed=0)
    m.net.eval()
    return m


def integer_model(case, device="cpu"):
    m = make_model(case, "cpu")
    C.set_integer_weights(m.net, case.seed)
    return m if str(device) == "cpu" else like(m, device)


def like(cpu_model, device):
    """a fresh model of the same config on `device` with the weights of cpu_model"""
    case_cfg = cpu_model.config
    m = type(cpu_model)(case_cfg, basedir=None, device=device, seed=0)
    m.net.load_state_dict(cpu_model.net.state_dict())
    m.net.eval()
    return m


def spatial_axes(case):
    return [i for i, a in enumerate(case.axes) if a != "C"]


def spatial_shape(case):
    return tuple(case.shape[i] for i in spatial_axes(case))


def tiles_spatial(case):
    return tuple(case.n_tiles[i] for i in spatial_axes(case))


# ---- weights ---------------------------------------------------------------------------------------------------------------------
def set_shift_weights(net, axis, sign):
    """every convolution of `net`: output channel co reads input channel co % ci through ONE tap of weight +1, the first (sign < 0) or
    the last (sign > 0) tap along the spatial axis `axis`, the centre tap on the other axes; bias 0.  sign > 0: an output pixel reads the
    input at a HIGHER index -- the network looks towards the end of the axis.  1x1 convolutions (heads, shortcuts) copy."""
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.Conv3d)):
                k = tuple(m.kernel_size)
                tap = [kk // 2 for kk in k]
                tap[axis] = k[axis] - 1 if sign > 0 else 0
                w = torch.zeros_like(m.weight)
                co = torch.arange(m.out_channels)
                w[(co, co % m.in_channels) + tuple(tap)] = 1.0
                m.weight.copy_(w)
                if m.bias is not None:
                    m.bias.zero_()
    return net


def shift_model(case, axis, sign):
    m = make_model(case, "cpu")
    set_shift_weights(m.net, axis, sign)
    return m


# ---- the tile plan ---------------------------------------------------------------------------------------------------------------
def plan(model, case):
    """(padded spatial shape, blocks per spatial axis, [(tile, src, dst)] as tuples of slices over the spatial axes) of model's own
    _tile_slices for the case -- with whatever overlap the model answers at the time of the call"""
    axes_net = model.config.axes
    div_by = model._axes_div_by(axes_net)
    sp = [i for i, a in enumerate(axes_net) if a != "C"]
    padded = tuple(-(-s // div_by[i]) * div_by[i] for s, i in zip(spatial_shape(case), sp))
    x = torch.empty(padded + (model.config.n_channel_in,), device="meta")
    n_tiles = tiles_spatial(case) + (1,)
    out = [tuple(tuple(part[i] for i in sp) for part in t) for t in model._tile_slices(x, n_tiles, axes_net, div_by)]
    return padded, tuple(div_by[i] for i in sp), out


def tile_shapes(tiles):
    return [tuple(s.stop - s.start for s in t[0]) for t in tiles]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def integer_image(case, salt=1):
    g = torch.Generator().manual_seed(case.seed * 16 + salt)
    return torch.randint(0, 3, case.shape, generator=g).float().numpy()


def shift_image(model, case, axis, sign, reach):
    """the image of a shift network, from the tile plan of `model` (see the module docstring): for every tile whose read region is cut on
    the side the network looks towards, impulses of value 1 .. 3 at the distances 1 .. reach + 2 beyond the read region along `axis`, each
    at its own position on the other axes (a lattice of pitch `block + 1` inside the tile's destination region, so that neighbouring
    distances land in different pooling blocks).  Impulses beyond the (unpadded) image are left out; every channel carries the image."""
    padded, blocks, tiles = plan(model, case)
    shape = spatial_shape(case)
    nd = len(shape)
    img = np.zeros(shape, np.float32)
    others = [d for d in range(nd) if d != axis]
    for tile, _, dst in tiles:
        t = tile[axis]
        if (sign > 0 and t.stop >= padded[axis]) or (sign < 0 and t.start <= 0):
            continue
        # the lattice of positions on the other axes, inside this tile's destination region (where the seam error would show)
        lat = [list(range(dst[d].start, min(dst[d].stop, shape[d]), blocks[d] + 1)) for d in others]
        n_lat = int(np.prod([len(v) for v in lat]))
        if n_lat == 0:
            continue
        for j, dist in enumerate(range(1, reach + 3)):
            q = t.stop - 1 + dist if sign > 0 else t.start - dist
            if not 0 <= q < shape[axis]:
                continue
            pos = [0] * nd
            pos[axis] = q
            r = j % n_lat
            for d, v in zip(reversed(others), reversed(lat)):
                pos[d] = v[r % len(v)]
                r //= len(v)
            img[tuple(pos)] = max(img[tuple(pos)], 1 + j % 3)
    if "C" in case.axes:
        ci = case.axes.index("C")
        img = np.repeat(np.expand_dims(img, ci), case.shape[ci], axis=ci)
    return img


# ---- references ------------------------------------------------------------------------------------------------------------------
def evaluate(net, x):
    """the module graph of the StarDistNet `net` on x (1, c, *S) on the CPU, in the dtype of x (net.double() for the float64 reference):
    dict(features, logit (1, 1, *S'), dist (1, R, *S') unclamped, class_logit or None, peak: the largest activation behind a convolution)"""
    from stardist_amd.models import unet as U
    peak = [0.0]

    def hook(m, inp, out):
        peak[0] = max(peak[0], float(out.abs().max()))
    hs = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.Conv3d))]
    try:
        with torch.no_grad():
            for st in net.pre:
                x = U.max_pool(st["convs"](x), st.pool)
            base = net.backbone(x)
            f = net.features(base)
            out = dict(features=f, logit=net.prob(f), dist=net.dist(f), class_logit=None)
            if net.n_classes is not None:
                out["class_logit"] = net.prob_class(net.features_class(base))
    finally:
        for h in hs:
            h.remove()
    out["peak"] = peak[0]
    return out


def _cl(t):
    """(1, C, *S) -> numpy (*S, C)"""
    nd = t.dim() - 2
    return t[0].permute(*(list(range(1, nd + 1)) + [0])).contiguous().numpy()


def reference(model, img, axes, double=True):
    """what predict(img) must return, from the evaluation of the CPU model's module graph on the padded image (the model's own
    _predict_setup pads it), cropped by its resizer: dict(logit, prob = sigmoid(logit) in float64, dist (clamped at the float32 1e-3),
    prob_class (float64 softmax) or None: float64 arrays; f32: the evaluation in float32 before the crop; f64: in float64 (double=False:
    None, and the float32 evaluation stands in -- test_cpu_predict_cases.py asserts for every case that the two are equal); padded: the
    padded spatial shape)"""
    x, axes, axes_net, div_by, resizer, _, grid, _, channel = model._predict_setup(img, axes, None, None)
    nd = model.config.n_dim
    xc = x.permute(*([nd] + list(range(nd)))).unsqueeze(0).contiguous()
    f32 = evaluate(model.net, xc.float())
    f64 = evaluate(copy.deepcopy(model.net).double(), xc.double()) if double else None
    ev = f64 if double else f32
    sp = axes_net.replace("C", "")
    logit = resizer.after(torch.from_numpy(_cl(ev["logit"].double())[..., 0]), sp).numpy()
    dist = resizer.after(torch.from_numpy(_cl(ev["dist"].double())), axes_net).numpy()
    out = dict(logit=logit, prob=1.0 / (1.0 + np.exp(-logit)), dist=np.maximum(dist, np.float64(np.float32(1e-3))), prob_class=None,
               f32=f32, f64=f64, padded=tuple(x.shape[:channel]))
    if ev["class_logit"] is not None:
        cl = resizer.after(torch.from_numpy(_cl(ev["class_logit"].double())), axes_net)
        out["prob_class"] = torch.softmax(cl, dim=-1).numpy()
    return out


@contextlib.contextmanager
def scalar_heads():
    """torch.sigmoid / torch.softmax as functions of the VALUE alone, for the CPU model (whose heads are torch's): torch's vectorised CPU
    sigmoid gives a pixel in the remainder of a vector another last bit than the same logit in its body, so a tile and the whole image
    differ by one ulp at a few pixels with no error anywhere.  Here every distinct value goes through math.exp once (float64, rounded
    to float32 at the end).  The GPU tests need none of this: there the package's own head kernels run, and their bits are the subject."""
    import math
    sigmoid, softmax = torch.sigmoid, torch.softmax

    def lookup(x, f):
        u, inv = torch.unique(x, return_inverse=True)
        return torch.tensor([f(v) for v in u.tolist()], dtype=torch.float64)[inv]

    def sig(x):
        return lookup(x, lambda v: 1.0 / (1.0 + math.exp(-v)) if v >= 0 else math.exp(v) / (1.0 + math.exp(v))).to(x.dtype)

    def soft(x, dim):
        e = lookup(x - x.max(dim, keepdim=True).values, math.exp)
        total = 0
        for part in e.unbind(dim):
            total = total + part
        return (e / total.unsqueeze(dim)).to(x.dtype)
    torch.sigmoid, torch.softmax = sig, soft
    try:
        yield
    finally:
        torch.sigmoid, torch.softmax = sigmoid, softmax


@contextlib.contextmanager
def cpu_threads(n=8):
    """at most n (and no more than there are) torch CPU threads inside, the previous number after it: tests that run the compiled reference
    leave the OpenMP runtime they share with torch at ONE thread (oracle.ref.set_threads), which the 3D cases here would feel.  The
    integer data give the same bits with any number of threads."""
    import os
    before = torch.get_num_threads()
    torch.set_num_threads(max(1, min(n, os.cpu_count() or 1)))
    try:
        yield
    finally:
        torch.set_num_threads(before)


def slab(case, axis):
    """the case reduced to two blocks on every spatial axis but `axis` and tiled along `axis` alone: what a shift network along `axis`
    needs on the CPU (it moves nothing across the other axes); the GPU tests run the shift networks on the whole case"""
    model = make_model(case)
    div_by = model._axes_div_by(model.config.axes.replace("C", ""))
    sp = spatial_axes(case)
    shape, n_tiles = list(case.shape), list(case.n_tiles)
    for d, i in enumerate(sp):
        if d != axis:
            shape[i], n_tiles[i] = 2 * div_by[d], 1
    return case._replace(name="%s-slab%d" % (case.name, axis), shape=tuple(shape), n_tiles=tuple(n_tiles))


def measure_reach(model, axis, sign):
    """how far the shift network of `model` (set_shift_weights(net, axis, sign)) carries an impulse along `axis`, in input pixels, as the
    reference project measures its receptive field: an impulse in the middle of a zero image, the outermost output pixel (times the grid)
    that differs from the zero image's.  Pooling makes the reach depend on where in a block of div_by the impulse sits: -> one reach per
    position in the block.  max() of it is the receptive field; boundary_reach() picks the one that matters at a tile edge."""
    cfg = model.config
    nd = cfg.n_dim
    div_by = model._axes_div_by(cfg.axes.replace("C", ""))
    rf = model._receptive_field_radius()
    shape = [div_by[d] * 2 for d in range(nd)]
    half = -(-(rf[axis] + 2 * div_by[axis]) // div_by[axis]) * div_by[axis]
    shape[axis] = 2 * half
    g = cfg.grid[axis]
    zero = evaluate(model.net, torch.zeros([1, cfg.n_channel_in] + shape))
    out = []
    for a in range(div_by[axis]):
        x = torch.zeros([1, cfg.n_channel_in] + shape)
        pos = [0] * nd
        pos[axis] = half + a
        x[(0, slice(None)) + tuple(pos)] = 1.0
        one = evaluate(model.net, x)
        diff = torch.zeros(zero["logit"].shape[2:], dtype=torch.bool)
        for k in ("logit", "dist", "class_logit"):
            if one[k] is not None:
                diff |= (one[k] != zero[k]).any(1)[0]
        idx = diff.nonzero()[:, axis]
        if idx.numel() == 0:                 # (a strided convolution's extreme tap never reads this position)
            out.append(0)
        else:
            out.append(int(half + a - int(idx.min()) * g) if sign > 0 else int(int(idx.max()) * g - half - a))
    assert max(out) > 0
    return out


def boundary_reach(reaches, sign):
    """the reach of the first pixel beyond a tile's read region: read regions end on block edges, so beyond the high end (sign > 0: the side
    the network looks towards) that pixel starts a block, beyond the low end it ends one.  Pixels further out sit later in the block but are
    further away by as much or more, so this is the overlap a block-aligned tile plan needs."""
    return reaches[0] if sign > 0 else reaches[-1]


def shortened_overlap(model, axis, overlap):
    """patch _axes_tile_overlap on the instance: `overlap` on the spatial axis `axis`, the model's own answer on the others"""
    own = type(model)._axes_tile_overlap
    name = model.config.axes.replace("C", "")[axis]

    def patched(query_axes):
        return tuple(overlap if a == name else v for a, v in zip(query_axes, own(model, query_axes)))
    model._axes_tile_overlap = patched
    return model


def sparse_numpy(prob, dist, prob_class, grid, padded, shape, prob_thresh, b):
    """what predict_sparse must return, from the dense prediction (prob, dist[, prob_class]) of the same image (as predict returns it: the
    pad already cropped): the pixels with prob > prob_thresh (strictly) that lie at least b grid steps inside the PADDED grid (`padded`:
    the padded image's spatial shape), in C order; points = grid index x grid, and only points inside the image (`shape`, unpadded) stay.
    -> (prob (n,), dist (n, R) clamped at 1e-3, prob_class (n, K) or None, points (n, nd) int64)"""
    grid = np.asarray(grid, np.int64)
    full = [p // g for p, g in zip(padded, grid)]
    bs = [(b, max(0, b - (f - s))) for f, s in zip(full, prob.shape)]
    p, d, idx = select_numpy(prob, dist, prob_thresh, bs)
    pc = None if prob_class is None else np.asarray(prob_class)[tuple(idx.T)]
    pts = idx * grid
    keep = np.all(pts < np.asarray(shape, np.int64), axis=1)
    return p[keep], d[keep], (None if pc is None else pc[keep]), pts[keep]


def c_order(res):
    """a predict_sparse result (prob, dist[, prob_class], points) with its rows sorted by point, first axis slowest"""
    order = np.lexsort(res[-1].T[::-1])
    return tuple(r[order] for r in res)
