"""Augmentation of training patches, on the host and -- the same bits -- on the device.

    aug = Compose([FlipRot90(), Warp(elastic_grid=5, elastic_amount=3.0), IntensityScaleShift(), AdditiveNoise()])
    model.train(X, Y, validation_data=..., augmenter=aug)

Every object here is a plain `augmenter(x, y) -> (x, y)` callable (numpy / scipy only, so it also serves the reference package), split
into its random part and its arithmetic:

    draw(shape) -> params       every random draw of one sample, small host data
    apply_host(x, y, params)    the definition: numpy and scipy.ndimage.map_coordinates
    __call__(x, y)              apply_host(x, y, draw(x.shape))

and Compose adds apply_device(xb, yb, params_list): the chain of a whole batch in one kernel launch (csrc/augment.hip; two with an
elastic Warp, whose displacement field is one utils.zoom_linear launch), equal to apply_host per sample bit for bit, NaN for NaN.
TrainData2D / TrainData3D take that route when the batch goes to a HIP device: the host then draws, the device computes, and a
training run has the history of the host route.

The order inside a Compose is fixed, whatever order the list has: FlipRot90, Warp, IntensityScaleShift, AdditiveNoise; at most one of
each.  Labels take the two spatial steps only.

DRAWS.  All of them are np.random.uniform calls, in this order, and their number depends on the constructor arguments and len(shape)
alone -- never on the extents or on a value drawn -- so the np.random stream after a sample is the same on every route:
    FlipRot90            k = len(axes) uniforms whose ranks are the permutation of the axes (made even where the extents differ and the
                         permutation is dropped), then k uniforms, one per axis: flip where < 0.5
    Warp                 the angle, the scale, then with elastic_grid the control grid, len(axes) * elastic_grid ** len(axes) uniforms
                         in (-1, 1), component by component in C order
    IntensityScaleShift  the scale, the shift
    AdditiveNoise        sigma, then the two 32-bit key words (floor(u * 2**32))

The arithmetic (csrc/augment.h states it once more, per pixel, for the kernel and the tests' host harness):
    FlipRot90   np.transpose by the drawn permutation of `axes` (only when they have one extent), then np.flip of the drawn axes.
    Warp        one resampling.  Coordinate of output pixel i along axis d in float64, every operation rounding on its own:
                c[d] = ((o[d] + M[d][0] i[0]) + M[d][1] i[1] (+ M[d][2] i[2])) + float64(disp[d][i]);  M rotates by the angle and scales
                by 1 / scale in the plane of `axes`, o = centre - M centre with centre = (n - 1) / 2; disp is the control grid
                (elastic_amount * U(-1, 1), float32, elastic_grid points along each axis of `axes`) brought to the patch size by
                utils.zoom_linear.  Image: scipy.ndimage.map_coordinates(order=1, mode=mode, cval=0, output=float32); labels: order=0,
                output=int32.  mode is 'reflect' or 'constant'.
    IntensityScaleShift   x * float32(scale) + float32(shift) in float32: two roundings.
    AdditiveNoise         x + float32(sigma) * n in float32: two roundings.  n is NOT np.random.normal: it is an Irwin-Hall variate, n =
                float32(g), g = (S - (6 * 2**32 - 6)) * 2**-32 in float64 (exact), S the integer sum of the twelve 32-bit words of three
                Philox4x32-10 blocks with counter (pixel index low word, high word, params['sample'], block 0 / 1 / 2) and the drawn
                key.  Mean 0, variance 1, |g| < 6, excess kurtosis -0.1; no transcendental function, so host and device agree bit for
                bit.  params['sample'] is 0 from draw() (every sample has its own key); set it to give samples that share a key
                different noise.
"""
import math

import numpy as np

__all__ = ["FlipRot90", "Warp", "IntensityScaleShift", "AdditiveNoise", "Compose", "philox4x32_10", "irwin_hall_noise"]

# a row of the parameter table of sd_augment_batch_device: struct augment::Sample of csrc/augment.h
_SAMPLE_DTYPE = np.dtype([("M", "<f8", (3, 3)), ("o", "<f8", (3,)), ("base", "<i8"), ("step", "<i8", (3,)), ("scale", "<f4"), ("shift", "<f4"),
                          ("sigma", "<f4"), ("key", "<u4", (2,)), ("sample", "<u4"), ("comp", "<i4", (3,)), ("pad", "<i4")])
assert _SAMPLE_DTYPE.itemsize == 168
_F_WARP, _F_REFLECT, _F_INTENSITY, _F_NOISE = 1, 2, 4, 8


def _default_axes(axes, nd):
    """the plane of FlipRot90 and Warp: both axes of an image, the yx plane (1, 2) of a volume"""
    if nd not in (2, 3):
        raise ValueError("patches of 2 or 3 dimensions expected")
    axes = tuple(range(nd - 2, nd)) if axes is None else tuple(int(a) % nd for a in axes)
    if len(set(axes)) != len(axes) or not axes:
        raise ValueError("axes must name different axes")
    return axes


def _pair(v, name):
    lo, hi = (float(v), float(v)) if np.isscalar(v) else (float(v[0]), float(v[1]))
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError("%s must be finite" % name)
    return lo, hi


# ---- Philox4x32-10 and the noise ---------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., Random123) on arrays: counter = four arrays (or scalars) of 32-bit words, key = two 32-bit words;
    returns the four output words as uint32 arrays of the common shape"""
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.asarray(w, np.uint64) & m32 for w in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [w.astype(np.uint32) for w in c]


def irwin_hall_noise(n_pixels, key, sample=0, first=0):
    """g of the module docstring for pixels first ... first + n_pixels - 1 of one sample, float64 (every value a multiple of 2**-32)"""
    pix = np.arange(first, first + n_pixels, dtype=np.uint64)
    lo, hi = pix & np.uint64(0xFFFFFFFF), pix >> np.uint64(32)
    S = np.zeros(n_pixels, np.int64)
    for blk in range(3):
        for w in philox4x32_10((lo, hi, np.uint64(int(sample) & 0xFFFFFFFF), np.uint64(blk)), key):
            S += w.astype(np.int64)
    return (S - np.int64(6 * 2 ** 32 - 6)).astype(np.float64) * 2.0 ** -32


# ---- the four operations -----------------------------------------------------------------------------------------------------------
class _Op(object):
    def __call__(self, x, y):
        return self.apply_host(x, y, self.draw(np.shape(x)))


class FlipRot90(_Op):
    """A random permutation of `axes` (applied when they have one extent) and random flips along them: every flip and 90 degree
    rotation of the plane.  axes=None: both axes of an image, (1, 2) of a volume.  params: {'perm': nd axes, 'flip': nd bools}"""
    name = "flip"

    def __init__(self, axes=None):
        self.axes = axes

    def draw(self, shape):
        nd = len(shape)
        axes = _default_axes(self.axes, nd)
        order = np.argsort(np.random.uniform(size=len(axes)), kind="stable")
        flips = np.random.uniform(size=len(axes)) < 0.5
        perm, flip = list(range(nd)), [False] * nd
        if len(set(int(shape[a]) for a in axes)) == 1:
            for a, j in zip(axes, order):
                perm[a] = axes[int(j)]
        for a, f in zip(axes, flips):
            flip[a] = bool(f)
        return {"perm": tuple(perm), "flip": tuple(flip)}

    @staticmethod
    def apply_host(x, y, params):
        flipped = tuple(d for d, f in enumerate(params["flip"]) if f)
        return tuple(np.flip(np.transpose(np.asarray(a), params["perm"]), flipped) for a in (x, y))


class Warp(_Op):
    """One resampling by a rotation (angle drawn from `rotate`, radians) and an isotropic zoom (factor drawn from `scale`) about the
    patch centre in the plane of two `axes`, plus, with elastic_grid, a smooth random displacement of up to elastic_amount pixels along
    each of them.  params: {'M': (nd, nd) float64, 'o': (nd,) float64, 'grid': float32 (2, *control grid) or None, 'axes', 'mode'}"""
    name = "warp"

    def __init__(self, rotate=(-math.pi, math.pi), scale=(0.8, 1.25), elastic_grid=None, elastic_amount=0.0, axes=None, mode="reflect"):
        self.rotate, self.scale = _pair(rotate, "rotate"), _pair(scale, "scale")
        if min(self.scale) <= 0:
            raise ValueError("scale must be positive")
        if elastic_grid is not None and (int(elastic_grid) != elastic_grid or elastic_grid < 1):
            raise ValueError("elastic_grid must be None or a positive integer")
        if mode not in ("reflect", "constant"):
            raise ValueError("mode must be 'reflect' or 'constant'")
        if axes is not None and len(tuple(axes)) != 2:
            raise ValueError("Warp works in the plane of two axes")
        self.elastic_grid = None if elastic_grid is None else int(elastic_grid)
        self.elastic_amount, self.axes, self.mode = float(elastic_amount), axes, mode

    def draw(self, shape):
        nd = len(shape)
        a0, a1 = axes = _default_axes(self.axes, nd)
        angle = np.random.uniform(*self.rotate)
        zoom = np.random.uniform(*self.scale)
        grid = None
        if self.elastic_grid is not None:
            gshape = tuple(self.elastic_grid if d in axes else 1 for d in range(nd))
            grid = (self.elastic_amount * np.random.uniform(-1, 1, size=(2,) + gshape)).astype(np.float32)
        M = np.eye(nd, dtype=np.float64)
        cs, sn = math.cos(angle) / zoom, math.sin(angle) / zoom
        M[a0, a0], M[a0, a1], M[a1, a0], M[a1, a1] = cs, -sn, sn, cs
        return {"M": M, "o": self.offset(M, shape), "grid": grid, "axes": axes, "mode": self.mode}

    @staticmethod
    def offset(M, shape):
        """o = centre - M centre, the sum from axis 0 on: the one place it is computed, for both routes"""
        nd = len(shape)
        o = np.zeros(nd, np.float64)
        for d in range(nd):
            acc = 0.0
            for e in range(nd):
                acc = acc + float(M[d][e]) * ((int(shape[e]) - 1) / 2)
            o[d] = (int(shape[d]) - 1) / 2 - acc
        return o

    @staticmethod
    def zoom_factors(grid_shape, shape):
        """the zoom that brings a control grid (2, *grid_shape) to (2, *shape); raises where scipy's rounding would give another shape"""
        from .utils import _zoom_out_shape
        zoom = (1.0,) + tuple(int(n) / int(g) for n, g in zip(shape, grid_shape))
        if _zoom_out_shape((2,) + tuple(grid_shape), zoom) != (2,) + tuple(int(n) for n in shape):
            raise ValueError("a control grid %s does not zoom to the patch shape %s exactly" % (tuple(grid_shape), tuple(shape)))
        return zoom

    @staticmethod
    def coordinates(params, shape):
        """the (nd, *shape) float64 sampling coordinates of the docstring's formula"""
        from .utils import zoom_linear
        nd = len(shape)
        M, o = params["M"], params["o"]
        idx = np.indices(shape, dtype=np.float64)
        disp = None
        if params.get("grid") is not None:
            grid = np.ascontiguousarray(params["grid"], np.float32)
            disp = zoom_linear(grid, Warp.zoom_factors(grid.shape[1:], shape))
        out = np.empty((nd,) + tuple(shape), np.float64)
        for d in range(nd):
            c = float(o[d]) + float(M[d][0]) * idx[0]
            for e in range(1, nd):
                c = c + float(M[d][e]) * idx[e]
            if disp is not None and d in params["axes"]:
                c = c + disp[params["axes"].index(d)].astype(np.float64)
            out[d] = c
        return out

    @staticmethod
    def apply_host(x, y, params):
        from scipy.ndimage import map_coordinates
        x, y = np.asarray(x, np.float32), np.asarray(y)
        c = Warp.coordinates(params, x.shape)
        return (map_coordinates(x, c, output=np.float32, order=1, mode=params["mode"], cval=0),
                map_coordinates(y, c, output=np.int32, order=0, mode=params["mode"], cval=0))


class IntensityScaleShift(_Op):
    """x * s + o with s drawn from `scale` and o from `shift`, in float32.  params: {'scale': float32, 'shift': float32}"""
    name = "intensity"

    def __init__(self, scale=(0.6, 2.0), shift=(-0.2, 0.2)):
        self.scale, self.shift = _pair(scale, "scale"), _pair(shift, "shift")

    def draw(self, shape):
        return {"scale": np.float32(np.random.uniform(*self.scale)), "shift": np.float32(np.random.uniform(*self.shift))}

    @staticmethod
    def apply_host(x, y, params):
        x = np.asarray(x, np.float32) * np.float32(params["scale"])
        return x + np.float32(params["shift"]), y


class AdditiveNoise(_Op):
    """x + sigma * n with sigma drawn from `sigma` and n the counter-based Irwin-Hall Gaussian of the module docstring (variance 1,
    support +-6; not np.random.normal), in float32.  params: {'sigma': float32, 'key': two 32-bit words, 'sample': 0}"""
    name = "noise"

    def __init__(self, sigma=(0.0, 0.02)):
        self.sigma = _pair(sigma, "sigma")

    def draw(self, shape):
        sigma = np.float32(np.random.uniform(*self.sigma))
        key = tuple(min(int(u * 2.0 ** 32), 2 ** 32 - 1) for u in np.random.uniform(size=2))
        return {"sigma": sigma, "key": key, "sample": 0}

    @staticmethod
    def apply_host(x, y, params):
        x = np.asarray(x, np.float32)
        n = irwin_hall_noise(x.size, params["key"], params.get("sample", 0)).astype(np.float32).reshape(x.shape)
        n = np.float32(params["sigma"]) * n
        return x + n, y


_ORDER = (FlipRot90, Warp, IntensityScaleShift, AdditiveNoise)


class Compose(_Op):
    """At most one of each operation, applied in the fixed order FlipRot90, Warp, IntensityScaleShift, AdditiveNoise.  params: a dict
    {'flip' / 'warp' / 'intensity' / 'noise': the operation's params}"""

    def __init__(self, ops):
        ops = list(ops)
        self.ops = []
        for cls in _ORDER:
            mine = [op for op in ops if isinstance(op, cls)]
            if len(mine) > 1:
                raise ValueError("a Compose takes at most one %s" % cls.__name__)
            self.ops += mine
        if len(self.ops) != len(ops):
            raise ValueError("a Compose takes FlipRot90, Warp, IntensityScaleShift and AdditiveNoise objects only")

    def draw(self, shape):
        return {op.name: op.draw(shape) for op in self.ops}

    @staticmethod
    def apply_host(x, y, params):
        for cls in _ORDER:
            if cls.name in params:
                x, y = cls.apply_host(x, y, params[cls.name])
        return x, y

    @staticmethod
    def table(params_list, shape):
        """(flags, the packed table as a _SAMPLE_DTYPE array, the stacked control grids (B, 2, *grid) or None) of a batch"""
        nd, B = len(shape), len(params_list)
        names = set(params_list[0]) if B else set()
        if any(set(p) != names for p in params_list) or not names <= set(cls.name for cls in _ORDER):
            raise ValueError("the params of one batch must come from one Compose")
        tab = np.zeros(B, _SAMPLE_DTYPE)
        stride = [int(np.prod(shape[d + 1:], dtype=np.int64)) for d in range(nd)]
        tab["comp"] = -1
        tab["M"][:] = np.eye(3)
        tab["scale"] = 1
        flags, grids = 0, None
        for b, p in enumerate(params_list):
            perm, flip = (p["flip"]["perm"], p["flip"]["flip"]) if "flip" in p else (tuple(range(nd)), (False,) * nd)
            if sorted(perm) != list(range(nd)) or len(flip) != nd or any(shape[perm[d]] != shape[d] for d in range(nd)):
                raise ValueError("FlipRot90 params do not fit the patch shape %s" % (tuple(shape),))
            for d in range(nd):
                tab["step"][b, d] = -stride[perm[d]] if flip[d] else stride[perm[d]]
                tab["base"][b] += (shape[d] - 1) * stride[perm[d]] if flip[d] else 0
            if "intensity" in p:
                tab["scale"][b], tab["shift"][b] = p["intensity"]["scale"], p["intensity"]["shift"]
            if "noise" in p:
                tab["sigma"][b], tab["key"][b], tab["sample"][b] = p["noise"]["sigma"], p["noise"]["key"], p["noise"].get("sample", 0)
            if "warp" in p:
                w = p["warp"]
                if np.shape(w["M"]) != (nd, nd) or np.shape(w["o"]) != (nd,):
                    raise ValueError("Warp params do not fit the patch shape %s" % (tuple(shape),))
                tab["M"][b, :nd, :nd], tab["o"][b, :nd] = w["M"], w["o"]
                if w.get("grid") is not None:
                    for j, a in enumerate(w["axes"]):
                        tab["comp"][b, a] = j
        if "warp" in names:
            modes = set(p["warp"]["mode"] for p in params_list)
            has_grid = set(p["warp"].get("grid") is not None for p in params_list)
            if len(modes) != 1 or len(has_grid) != 1 or not modes <= {"reflect", "constant"}:
                raise ValueError("the Warp params of one batch must share the mode and the control grid's shape")
            flags |= _F_WARP | (_F_REFLECT if modes == {"reflect"} else 0)
            if has_grid == {True}:
                grids = np.stack([np.ascontiguousarray(p["warp"]["grid"], np.float32) for p in params_list])
        flags |= (_F_INTENSITY if "intensity" in names else 0) | (_F_NOISE if "noise" in names else 0)
        return flags, tab, grids

    @staticmethod
    def apply_device(xb, yb, params_list):
        """the chain on a batch: xb float32 (B, *patch) and yb int32 (B, *patch) on a HIP device, one params per sample; returns new
        tensors (xb', yb') with xb'[b], yb'[b] == apply_host(xb[b], yb[b], params_list[b]).  One upload of the packed table (and one of
        the control grids), one kernel launch (and one zoom_linear launch), no host synchronisation"""
        import ctypes
        import torch
        from .lib import _native as N
        from .utils import zoom_linear
        if not (torch.is_tensor(xb) and torch.is_tensor(yb) and xb.is_cuda and yb.device == xb.device):
            raise ValueError("apply_device takes two tensors on one HIP device")
        if xb.dtype != torch.float32 or yb.dtype != torch.int32 or xb.shape != yb.shape or xb.dim() not in (3, 4):
            raise ValueError("apply_device takes a float32 and an int32 tensor of one shape (B, *patch), patches of 2 or 3 dimensions")
        B, shape = int(xb.shape[0]), tuple(int(n) for n in xb.shape[1:])
        if B != len(params_list) or B < 1:
            raise ValueError("one params object per sample expected")
        xb, yb = xb.contiguous(), yb.contiguous()
        flags, tab, grids = Compose.table(params_list, shape)
        d_tab = torch.from_numpy(tab.view(np.uint8).reshape(-1)).to(xb.device)
        d_disp, n_disp = None, 0
        if grids is not None:
            n_disp = int(grids.shape[1])
            zoom = Warp.zoom_factors(grids.shape[2:], shape)
            d_disp = zoom_linear(torch.from_numpy(grids.reshape((B * n_disp,) + grids.shape[2:])).to(xb.device), zoom)
            if tuple(d_disp.shape) != (B * n_disp,) + shape or d_disp.dtype != torch.float32:
                raise ValueError("the displacement field does not have the patch shape")
        ox, oy = torch.empty_like(xb), torch.empty_like(yb)
        h_shape = (ctypes.c_int * len(shape))(*shape)
        N.dcall(xb, "sd_augment_batch_device", N.tptr(xb), N.tptr(yb), B, len(shape), ctypes.cast(h_shape, ctypes.c_void_p), flags,
                ctypes.c_void_p(tab.ctypes.data), N.tptr(d_tab), None if d_disp is None else N.tptr(d_disp), n_disp, N.tptr(ox), N.tptr(oy))
        return ox, oy
