"""The Python side of the hand-written inference layers (csrc/conv3x3*.hip, conv_general.hip, the pooling, up-sampling and head kernels):
kernel-form selection (conv_mode), the fp16 range flags, the split16 activation protocol, weight packing with batch-norm folding, and
every call into the library that a network pass makes.  models/unet.py holds the topology and calls in here.

GPU inference runs EVERY convolution, pooling and head of the network on the library's own kernels; a layer none of them covers
raises UnsupportedLayer with the layer's shape (there is no library / framework fallback on the device).  The plain torch modules
of models/unet.py remain what they are everywhere else: on the CPU (float64 references of the tests, the flagged CPU baseline of
bench.py) and under autograd.

Conv2D(3x3) / Conv3D(3x3x3) 'same' layers with 1 or a multiple of 32 (<= 512) input channels and a multiple of 32 output channels
-- including Concatenate([UpSampling(x), skip]) in front of them -- run as implicit GEMMs on the matrix cores with up-sampling,
concatenation, bias, batch-norm and activation folded in (_hand_conv: _classify, then _plan, then _launch).

The library is called as N.dcall(...) through the module attribute and every "is this tensor on the device" decision goes through
_on_device: a test replaces those two (and _flag_ptr) to run the dispatcher on CPU tensors."""
import collections
import ctypes
import os
import threading

import numpy as np
import torch
import torch.nn as nn

from ..lib import _native as N


class UnsupportedLayer(NotImplementedError):
    """a network layer that no hand-written kernel covers (GPU inference has no library fallback)"""


_CONV_MODES = ("f16x3", "bf16x6", "hand")
_mode_override = []


def conv_mode():
    """Which kernel the 3x3 / 3x3x3 layers over 32-channel chunks run on (STARDIST_AMD_CONV, read per call; force_conv_mode overrides):
      'f16x3' (default)   csrc/conv3x3_f16.hip: every f32 product as three fp16 x fp16 MFMA products (two fp16 terms per operand, the
                          cross terms in their own f32 accumulator) -- f32-accurate: layers and networks within 3e-6 of a float64
                          evaluation, the same 1e-5 tests as the exact kernel.  An activation outside the fp16 range raises a device
                          flag; the model then re-evaluates with 'bf16x6' (StarDistBase._net_forward).
      'bf16x6'            csrc/conv3x3_bf16.hip: six bf16 x bf16 products per f32 product (three bf16 terms per operand); no range limit
      'hand' / 'f32'      csrc/conv3x3.hip: exact f32 MFMA kernel (one fma chain per output)
    The one-channel first layer and the general kernel (csrc/conv_general.hip) are exact f32 in every mode."""
    if _mode_override:
        return _mode_override[-1]
    m = os.environ.get("STARDIST_AMD_CONV", "f16x3")
    return "hand" if m in ("hand", "f32") else (m if m in _CONV_MODES else "f16x3")


class force_conv_mode(object):
    """context manager: `with force_conv_mode("bf16x6"): ...` (takes precedence over the environment variable)"""

    def __init__(self, mode):
        assert mode in _CONV_MODES, mode
        self.mode = mode

    def __enter__(self):
        _mode_override.append(self.mode)
        return self

    def __exit__(self, *exc):
        _mode_override.pop()
        return False


_range_flags = {}
N_FLAG_SLOTS = 256
_slot_counter = [0]


class _PerThread(threading.local):
    """state of the forward pass a thread is running: the flag tensor of ITS model (two threads predicting with two models on one
    device each report into their own words), and whether a layer asked for the pass to be repeated (split16_replan)"""

    def __init__(self):
        self.flag_stack = []
        self.replan = False


_tls = _PerThread()


def range_flag(device):
    """the device word the split-fp16 convolutions OR with 1 when an activation they READ lies outside the fp16 range (|x| > 65504 or
    infinite; a NaN simply propagates into the result as it does in any float32 evaluation) -- the default word, used by layers
    evaluated outside a model's forward pass (one per device)"""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _range_flags:
        _range_flags[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _range_flags[key]


class use_range_flags(object):
    """context manager: inside it every split-fp16 layer reports into ITS OWN word of `flags` (int32 tensor of N_FLAG_SLOTS words owned by
    the calling model -- two models on one device do not share state, and the captured HIP graphs keep pointing at their model's words):
    StarDistBase._net_forward reads the words after a pass and moves exactly the offending layers to the bf16x6 form"""

    def __init__(self, flags):
        assert flags.dtype == torch.int32 and flags.numel() == N_FLAG_SLOTS
        self.flags = flags

    def __enter__(self):
        _tls.flag_stack.append(self.flags)
        return self

    def __exit__(self, *exc):
        _tls.flag_stack.pop()
        return False


def flag_slot(conv):
    """the word (1 .. N_FLAG_SLOTS - 1) a convolution module reports its range flag into; assigned on first use.  A model is not
    re-entrant: one thread at a time per model (its flag words and captured graphs are per model, the stack of active flag tensors per thread)"""
    s = conv.__dict__.get("_sd_flag_slot")
    if s is None:
        _slot_counter[0] = _slot_counter[0] % (N_FLAG_SLOTS - 1) + 1
        s = conv.__dict__["_sd_flag_slot"] = _slot_counter[0]
    return s


def _flag_ptr(conv, device):
    st = _tls.flag_stack
    if st and st[-1].device == torch.device(device):
        return st[-1].data_ptr() + 4 * flag_slot(conv)
    return range_flag(device).data_ptr()


# ---- split16 activations (include/stardist_hip.h "split16"; csrc/conv3x3_layout.h) -------------------------------------------------
# Between two split-fp16 layers an activation tensor travels as the two fp16 terms (hi, lo') the consuming kernel multiplies with --
# made once in the producer's epilogue instead of once per consumer workgroup and unit.  Same shape, strides and bytes per value as
# the f32 tensor it stands for (torch dtype float32, tagged with `_sd_split16`); results are bit-identical to the f32 form.
# Which layers write it is planned from the topology (StarDistNet._plan_split16: a layer whose every consumer is a 3x3 layer over
# 32-channel chunks, directly or through a max-pooling); a consumer that cannot read the form after all (pinned to bf16x6) unpacks it,
# clears the producer's mark and asks for the pass to be repeated (`split16_replan`), so a result never depends on the form.
_split16_override = []


def split16_replan(value=None):
    """the calling thread's "repeat the pass" request (set by _unpack_for, read and cleared by StarDistBase._net_forward)"""
    if value is not None:
        _tls.replan = bool(value)
    return _tls.replan


def split16_enabled():
    """split16 activations between split-fp16 layers (STARDIST_AMD_SPLIT16=0 or force_split16(False): f32 tensors everywhere)"""
    if _split16_override:
        return _split16_override[-1]
    return os.environ.get("STARDIST_AMD_SPLIT16", "1") != "0"


class force_split16(object):
    """context manager: `with force_split16(False): ...` (takes precedence over the environment variable)"""

    def __init__(self, on):
        self.on = bool(on)

    def __enter__(self):
        _split16_override.append(self.on)
        return self

    def __exit__(self, *exc):
        _split16_override.pop()
        return False


def is_split16(t):
    return bool(getattr(t, "_sd_split16", False))


def _tag_split16(t, producer):
    t._sd_split16 = True
    t._sd_producer = producer
    return t


_vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())                      # void* of a tensor's data, NULL for None
_cl = lambda nd: torch.channels_last if nd == 2 else torch.channels_last_3d


def split16_unpack(t):
    """the f32 tensor hi + lo' * 2^-11 of a split16 tensor (a consumer that only reads f32); a plain tensor is returned as it is"""
    if not is_split16(t):
        return t
    out = torch.empty_like(t)
    C = int(t.shape[1])
    N.dcall(t, "sd_split16_unpack_device", _vp(t), int(t.numel() // C), C, _vp(out))
    return out


def split16_pack(t, flag_ptr=None):
    """split16 form of a channels-last f32 tensor (1, C, *spatial), C a multiple of 32 (tests; sd_split16_pack_device)"""
    assert t.dtype == torch.float32 and t.shape[0] == 1 and t.shape[1] % 32 == 0 and t.is_contiguous(memory_format=_cl(t.dim() - 2))
    out = torch.empty_like(t)
    C = int(t.shape[1])
    N.dcall(t, "sd_split16_pack_device", _vp(t), int(t.numel() // C), C, _vp(out), ctypes.c_void_p(flag_ptr) if flag_ptr else None)
    return _tag_split16(out, None)


def _unpack_for(conv, t):
    """`conv` cannot read the split16 tensor t: f32 copy for this pass; its producer writes f32 from now on and the pass is repeated"""
    prod = getattr(t, "_sd_producer", None)
    if prod is not None and prod.__dict__.get("_sd_split_out"):
        prod.__dict__["_sd_split_out"] = False
        split16_replan(True)
    return split16_unpack(t)


def _on_device(t):
    """the tensor lives on a HIP device (the one place that asks: the seam of the CPU dispatch tests)"""
    return t.is_cuda


def _native_inference(x):
    """the hand-written path applies: tensor on a HIP device, no autograd, no autocast"""
    return _on_device(x) and not torch.is_grad_enabled() and not torch.is_autocast_enabled()


def _as_cl(t, cl):
    """t as a 16-byte aligned channels-last operand (a pooling layer may hand over a tensor in the default layout: one copy at its resolution)"""
    return t if t.is_contiguous(memory_format=cl) and t.data_ptr() % 16 == 0 else t.clone(memory_format=cl)


def _layer_desc(conv, srcs=None):
    return "%s %s -> %d, kernel %s, stride %s%s" % (
        type(conv).__name__, conv.in_channels if srcs is None else " + ".join(str(int(t.shape[1])) + ("(up)" if any(np.atleast_1d(u)) else "") for t, u in srcs),
        conv.out_channels, tuple(conv.kernel_size), tuple(conv.stride),
        "" if srcs is None else ", input %s" % (tuple(srcs[0][0].shape[2:]),))


def _bn_fold(conv, bn):
    """(kernel, bias) float32 numpy of conv followed by an inference BatchNormalization (csbdeep conv_block: Conv -> BN -> Activation,
    Keras moving statistics): w' = w * s, b' = (b - mean) * s + beta with s = gamma / sqrt(var + eps), folded in float64"""
    w = conv.weight.detach().double().cpu().numpy()
    b = conv.bias.detach().double().cpu().numpy() if conv.bias is not None else np.zeros(w.shape[0])
    if bn is not None:
        g = bn.weight.detach().double().cpu().numpy() if bn.weight is not None else np.ones(w.shape[0])
        beta = bn.bias.detach().double().cpu().numpy() if bn.bias is not None else np.zeros(w.shape[0])
        sc = g / np.sqrt(bn.running_var.detach().double().cpu().numpy() + bn.eps)
        w = w * sc.reshape((-1,) + (1,) * (w.ndim - 1))
        b = (b - bn.running_mean.detach().double().cpu().numpy()) * sc + beta
    return np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)


_FORM_PREFIX = {"conv3": "sd_conv3", "bf16x6": "sd_conv3_bf16x6", "f16x3": "sd_conv3_f16x3"}


class _WeightRange(ValueError):
    """a kernel with weights outside the fp16 range: the layer takes the bf16x6 form"""


def _packed_conv_weights(conv, form="conv3", bn=None):
    """(packed kernel, bias) on the device for the native layer `form`: 'conv3' (sd_conv3_ndhwc_device), 'bf16x6'
    (sd_conv3_bf16x6_ndhwc_device), 'f16x3' (sd_conv3_f16x3_ndhwc_device) or 'general' (sd_convg_ndhwc_device); an inference batch-norm
    layer behind the convolution is folded in.  Cached per module (inference: invalidated when a parameter changes)."""
    ver = lambda t: None if t is None else (t.data_ptr(), t._version)
    key = (ver(conv.weight), ver(conv.bias), str(conv.weight.device)) + \
        (() if bn is None else (ver(bn.weight), ver(bn.bias), ver(bn.running_mean), ver(bn.running_var), bn.eps))
    slot = "_sd_packed_" + form
    cache = conv.__dict__.get(slot)
    if cache is None or cache[0] != key:
        w, b = _bn_fold(conv, bn)
        co, ci = int(w.shape[0]), int(w.shape[1])
        k = tuple(int(v) for v in w.shape[2:])
        L = N.lib()
        if form == "general":
            kz, ky, kx = ((1,) + k) if len(k) == 2 else k
            n = int(L.sd_convg_packed_floats(ci, co, kz, ky, kx))
            if n < 0:
                raise ValueError("sd_convg: unsupported layer %d -> %d, kernel %s" % (ci, co, k))
            packed = np.zeros(n, np.float32)
            N.check(L.sd_convg_pack_weights_host(N.ptr(w), ci, co, kz, ky, kx, N.ptr(packed)))
        else:
            prefix = _FORM_PREFIX[form]
            kz = 3 if w.ndim == 5 else 1
            n = int(getattr(L, prefix + "_packed_floats")(ci, co, kz))
            if n < 0:
                raise ValueError("%s: unsupported channel counts %d -> %d" % (prefix, ci, co))
            packed = np.empty(n, np.float32)
            rc = getattr(L, prefix + "_pack_weights_host")(N.ptr(w), ci, co, kz, N.ptr(packed))
            if form == "f16x3" and rc == -2:
                conv.__dict__[slot] = (key, None, None)
                raise _WeightRange(L.sd_last_error().decode(errors="replace"))
            N.check(rc)
        has_bias = conv.bias is not None or bn is not None
        cache = (key, torch.from_numpy(packed).to(conv.weight.device), torch.from_numpy(b).to(conv.weight.device) if has_bias else None)
        conv.__dict__[slot] = cache
    if cache[1] is None:
        raise _WeightRange("weights outside the fp16 range")
    return cache[1], cache[2]


def tf_same_pad_before(n, k, s):
    """TensorFlow 'SAME': total = max(k - s, 0) if n % s == 0 else max(k - n % s, 0); the smaller half goes in front"""
    total = max(k - s, 0) if n % s == 0 else max(k - n % s, 0)
    return total // 2


def _general_conv(conv, x, kind, res=None, bn=None, tf_same=False):
    """act(conv(x) + bias (+ res)) by the general hand-written kernel (any kernel size / stride / channel counts; csrc/conv_general.hip).
    tf_same: Keras padding='same' semantics for a strided layer (asymmetric, computed from the input size) instead of conv.padding.
    None when the layer is not covered."""
    nd = x.dim() - 2
    if not (nd in (2, 3) and x.shape[0] == 1 and conv.groups == 1 and all(d == 1 for d in conv.dilation) and conv.weight.dtype == torch.float32
            and x.dtype == torch.float32 and _on_device(x) and x.device == conv.weight.device and x.shape[1] == conv.in_channels):
        return None
    k3 = (1,) * (3 - nd) + tuple(int(v) for v in conv.kernel_size)
    s3 = (1,) * (3 - nd) + tuple(int(v) for v in conv.stride)
    if int(N.lib().sd_convg_packed_floats(conv.in_channels, conv.out_channels, *k3)) < 0:
        return None
    S3 = (1,) * (3 - nd) + tuple(int(v) for v in x.shape[2:])
    if tf_same:
        p3 = tuple(tf_same_pad_before(n, k, st) for n, k, st in zip(S3, k3, s3))
        O3 = tuple(-(-n // st) for n, st in zip(S3, s3))
    else:
        if not all(isinstance(v, int) for v in conv.padding):
            return None
        p3 = (0,) * (3 - nd) + tuple(int(v) for v in conv.padding)
        O3 = tuple((n + 2 * p - k) // st + 1 for n, p, k, st in zip(S3, p3, k3, s3))
    if any(o <= 0 for o in O3):
        return None
    cl, co = _cl(nd), conv.out_channels
    x = _as_cl(x, cl)
    wp, bias = _packed_conv_weights(conv, "general", bn)
    out = torch.empty((1, co) + O3[3 - nd:], dtype=torch.float32, device=x.device, memory_format=cl)
    if res is not None and not (tuple(res.shape) == tuple(out.shape) and res.dtype == torch.float32 and res.is_contiguous(memory_format=cl)):
        return None
    N.dcall(x, "sd_convg_ndhwc_device", _vp(x), conv.in_channels, conv.in_channels, *S3, *k3, *s3, *p3, *O3, _vp(wp), _vp(bias), _vp(res),
            co, co, kind, _vp(out), co)
    return out


_MAX_CHUNK_CHANNELS = 512          # csrc/conv3x3_layout.h MAX_CHUNKS * 32


def is_chunked_3x3(conv, nd, cs=None, first=False):
    """`conv` is a layer of the matrix-core kernels (csrc/conv3x3*.hip): 3x3(x3), stride 1, 'same', no dilation, one group, a multiple of
    32 output channels, and sources of cs channels each (default: one source of conv.in_channels) in 32-channel chunks, at most
    _MAX_CHUNK_CHANNELS together.  first: the one-channel first layer (a multiple of 4 output channels) counts as well."""
    cs = [conv.in_channels] if cs is None else list(cs)
    if not (isinstance(conv, nn.Conv2d if nd == 2 else nn.Conv3d) and tuple(conv.kernel_size) == (3,) * nd and tuple(conv.stride) == (1,) * nd
            and tuple(conv.padding) == (1,) * nd and tuple(conv.dilation) == (1,) * nd and conv.groups == 1):
        return False
    if cs == [1]:
        return bool(first) and conv.out_channels % 4 == 0
    return all(c % 32 == 0 and c > 0 for c in cs) and sum(cs) <= _MAX_CHUNK_CHANNELS and conv.out_channels % 32 == 0


NO_STORE = object()          # _hand_conv(..., no_store=True): the layer ran without writing its output (fused head only)

_Layer = collections.namedtuple("_Layer", "nd cs ups shape")          # a 3x3 family layer: channels and up-sampling per source, output size
_Plan = collections.namedtuple("_Plan", "form in_split out_split dot skip_out")      # how it runs: kernel form, split16 sides, fused head, no store


def _classify(conv, srcs, kind, res, bn, tf_same):
    """None (not covered), "general" (one full-resolution source: the general kernel may take it) or the _Layer of a 3x3 family layer;
    registers `conv` as a reader with the producer of each source"""
    nd = 2 if isinstance(conv, nn.Conv2d) else (3 if isinstance(conv, nn.Conv3d) else 0)
    if not (nd and kind in (0, 1) and not torch.is_grad_enabled() and not torch.is_autocast_enabled()
            and conv.groups == 1 and conv.weight.dtype == torch.float32 and 1 <= len(srcs) <= 2) or (bn is not None and bn.training):
        return None
    cs, ups = [], []
    for t, up in srcs:
        if not (_on_device(t) and t.dtype == torch.float32 and t.dim() == nd + 2 and t.shape[0] == 1 and t.device == conv.weight.device):
            return None
        cs.append(int(t.shape[1]))
        ups.append(tuple(int(bool(v)) for v in up) if isinstance(up, (tuple, list)) else (int(bool(up)),) * nd)
    if sum(cs) != conv.in_channels:
        return None
    for t, _ in srcs:                                    # (who reads a layer's output: the range fallback pins the readers of a split16 tensor)
        prod = getattr(t, "_sd_producer", None)
        if prod is not None:
            prod.__dict__.setdefault("_sd_consumers", set()).add(conv)
    if tf_same or not is_chunked_3x3(conv, nd, cs, first=not any(ups[0]) and res is None):
        return "general" if len(srcs) == 1 and not any(ups[0]) else None
    shapes = {tuple(int(s) << u for s, u in zip(t.shape[2:], up)) for (t, _), up in zip(srcs, ups)}          # output = full resolution
    return _Layer(nd, cs, ups, shapes.pop()) if len(shapes) == 1 else None


def _plan(conv, layer, ts, res, bn, dot, no_store):
    """(_Plan, packed kernel, bias) of a 3x3 family layer reading the tensors ts: the form from the mode, the layer's pinned form and its
    weights' range; split16 sources all or none (a layer on another kernel form reads f32 only); split16 output as planned"""
    cs, co, mode = layer.cs, conv.out_channels, conv_mode()
    form = "conv3" if (cs == [1] or mode == "hand") else mode
    if form == "f16x3" and conv.__dict__.get("_sd_force_form") == "bf16x6":
        form = "bf16x6"                                  # this layer has seen an activation beyond the fp16 range (StarDistBase._net_forward)
    if form == "f16x3":
        try:
            wp, bias = _packed_conv_weights(conv, form, bn)
        except _WeightRange:
            form = "bf16x6"
    if form != "f16x3":
        wp, bias = _packed_conv_weights(conv, form, bn)
    in_split = form == "f16x3" and res is None and all(is_split16(t) for t in ts)
    out_split = bool(conv.__dict__.get("_sd_split_out")) and split16_enabled() and res is None and dot is None and mode == "f16x3" \
        and (form == "f16x3" or (cs == [1] and co == 32))
    fused = form == "f16x3" and dot is not None and res is None and dot[0].numel() == co and dot[0].data_ptr() % 16 == 0
    return _Plan(form, in_split, out_split, fused, bool(no_store) and fused and not out_split), wp, bias


def _launch(conv, layer, plan, wp, bias, ts, kind, res, dot):
    """run the planned layer: the layer output, NO_STORE, or None when the residual does not fit"""
    (nd, cs, ups, shape), co, cl = layer, conv.out_channels, _cl(layer.nd)
    if not plan.in_split:
        ts = [_unpack_for(conv, t) for t in ts]
    if res is not None and not (tuple(res.shape) == (1, co) + shape and res.dtype == torch.float32 and res.is_contiguous(memory_format=cl)):
        return None
    a, b = ts[0], (ts[1] if len(ts) == 2 else None)
    out = None if plan.skip_out else torch.empty((1, co) + shape, dtype=torch.float32, device=conv.weight.device, memory_format=cl)
    D, H, W = ((1,) + shape) if nd == 2 else shape
    part = torch.empty((D * H * W, co // 4), dtype=torch.float32, device=a.device) if plan.dot else None
    mask = lambda up: sum(v << k for k, v in enumerate(reversed(up)))                     # bit 0: x, 1: y, 2: z
    up0, (c1, up1) = mask(ups[0]), ((cs[1], mask(ups[1])) if b is not None else (0, 0))
    strided = [_vp(a), cs[0], cs[0], up0, _vp(b), c1, c1, up1]                            # the sources, with / without their channel strides
    packed = [_vp(a), cs[0], up0, _vp(b), c1, up1]
    geom = [D, H, W, 1 if nd == 2 else 3, _vp(wp), _vp(bias)]
    first_split = cs == [1] and plan.out_split                                            # the one-channel first layer writing split16
    flag = [ctypes.c_void_p(_flag_ptr(conv, a.device))] if plan.form == "f16x3" or first_split else []
    head = [_vp(dot[0]), _vp(part)] if plan.dot else [None, None]
    if first_split:
        N.dcall(a, "sd_conv3_c1x32_split16_device", _vp(a), *geom, kind, _vp(out), *flag)
    elif plan.form == "f16x3" and (plan.in_split or plan.out_split or plan.skip_out):
        N.dcall(a, "sd_conv3_f16x3_fmt_ndhwc_device", *packed, *geom, co, kind, _vp(out), int(plan.in_split), int(plan.out_split), *flag, *head)
    elif plan.dot:
        N.dcall(a, "sd_conv3_f16x3_dot_ndhwc_device", *strided, *geom, co, kind, _vp(out), *flag, *head)
    else:
        N.dcall(a, _FORM_PREFIX[plan.form] + "_res_ndhwc_device", *strided, *geom, _vp(res), co if res is not None else 0, co, kind, _vp(out), *flag)
    if plan.dot:
        dot[1].append(part)
    if plan.skip_out:
        return NO_STORE
    return _tag_split16(out, conv) if plan.out_split else out


def _hand_conv(conv, srcs, kind, res=None, bn=None, tf_same=False, dot=None, no_store=False):
    """act(conv(cat(srcs, 1)) + bias (+ res)) by a hand-written kernel; srcs = [(tensor (1, C, *spatial) channels-last float32, up)] with
    up = per-axis tuple of 0/1 (or one int for all axes): 1 where the source has half the output resolution and the reference
    up-samples it (nearest, x2) first.  res: residual added before the activation (resnet_block's Add); bn: inference batch-norm layer
    between convolution and activation (folded into kernel and bias).  3x3(x3) stride-1 'same' layers over 32-channel chunks (and the
    one-channel first layer) go to csrc/conv3x3*.hip, everything else with one full-resolution source to csrc/conv_general.hip.
    dot = (weights (c_out,), holder list): a one-channel head fused into the layer's epilogue when the split-fp16 kernel takes the layer
    (sd_conv3_f16x3_dot_ndhwc_device) -- holder[0] then receives the per-lane terms (n_pix, c_out / 4); left empty otherwise.
    no_store (with dot): when the fused head is taken the layer's own output is NOT written and NO_STORE is returned (the caller evaluates
    the layer on the pixels it needs with conv_rows); otherwise ignored.
    None when the layer is not covered (the callers raise UnsupportedLayer)."""
    layer = _classify(conv, srcs, kind, res, bn, tf_same)
    if layer is None:
        return None
    if layer == "general":
        return _general_conv(conv, _unpack_for(conv, srcs[0][0]), kind, res, bn, tf_same)
    ts = [t if is_split16(t) else _as_cl(t, _cl(layer.nd)) for t, _ in srcs]
    plan, wp, bias = _plan(conv, layer, ts, res, bn, dot, no_store)
    return _launch(conv, layer, plan, wp, bias, ts, kind, res, dot)


def conv_rows(conv, x, kind, rows, bn=None):
    """act(conv(x) + bias) on the pixels `rows` (int64 linear indices into x's spatial grid) of a 3x3(x3) layer the split-fp16 kernel takes:
    (len(rows), c_out) float32, bit-identical to the rows of the dense layer output (sd_conv3_f16x3_rows_device); x (1, C, *spatial)
    channels-last, f32 or split16"""
    nd = x.dim() - 2
    assert is_chunked_3x3(conv, nd), _layer_desc(conv)
    wp, bias = _packed_conv_weights(conv, "f16x3", bn)
    co = conv.out_channels
    out = torch.empty((int(rows.shape[0]), co), dtype=torch.float32, device=x.device)
    if rows.shape[0]:
        S = (1,) * (3 - nd) + tuple(int(v) for v in x.shape[2:])
        N.dcall(x, "sd_conv3_f16x3_rows_device", _vp(x), int(x.shape[1]), int(is_split16(x)), *S, 1 if nd == 2 else 3, _vp(wp), _vp(bias), co, kind,
                _vp(rows), int(rows.shape[0]), _vp(out))
    return out


def _upcat_general(conv, x, skip, pool, kind, bn=None):
    """coverage path of an up level the fused kernels do not take (e.g. n_filter_base = 48: 96 + 96 input channels): UpSampling +
    Concatenate materialised by the native one-pass kernel (sd_upcat_ndhwc_device), then the general convolution kernel.  None when
    not applicable."""
    nd = x.dim() - 2
    if not (nd in (2, 3) and all(p in (1, 2) for p in pool) and x.shape[0] == 1 and x.dtype == torch.float32 and skip.dtype == torch.float32
            and x.shape[1] % 4 == 0 and skip.shape[1] % 4 == 0 and x.shape[1] + skip.shape[1] == conv.in_channels
            and tuple(int(s) * int(p) for s, p in zip(x.shape[2:], pool)) == tuple(int(s) for s in skip.shape[2:])):
        return None
    cl = _cl(nd)
    a, b = _as_cl(_unpack_for(conv, x), cl), _as_cl(_unpack_for(conv, skip), cl)
    S = (1,) * (3 - nd) + tuple(int(v) for v in skip.shape[2:])
    up = sum((1 << k) for k, p in enumerate(reversed(pool)) if p == 2)                    # bit 0: x, 1: y, 2: z
    cat = torch.empty((1, a.shape[1] + b.shape[1]) + tuple(skip.shape[2:]), dtype=torch.float32, device=a.device, memory_format=cl)
    N.dcall(a, "sd_upcat_ndhwc_device", _vp(a), int(a.shape[1]), up, _vp(b), int(b.shape[1]), *S, _vp(cat))
    return _general_conv(conv, cat, kind, None, bn)


def _conv_bias_act(conv, x, kind, bn=None):
    """conv (+ folded batch-norm) + bias + (0 linear | 1 relu) of GPU inference by a hand-written kernel; None when the hand-written
    path does not apply (CPU, autograd, autocast: the caller runs the plain modules); raises UnsupportedLayer for a layer no kernel
    covers, or another activation (kind -1)"""
    if not (_native_inference(x) and x.dtype == torch.float32):
        return None
    y = _hand_conv(conv, [(x, 0)], kind, bn=bn)
    if y is None:
        raise UnsupportedLayer(_layer_desc(conv, [(x, 0)]) + ("" if kind >= 0 else ", activation other than linear / relu"))
    return y


def _native_max_pool(x, pool):
    """Keras MaxPooling ('valid', stride = pool) by the one-pass channels-last kernel (sd_maxpool_ndhwc_device, 64-bit indexing); the
    pooled split16 tensor == split16 of the pooled f32 tensor (x -> (hi, lo') is monotone): same readers, same bits"""
    nd = x.dim() - 2
    if not (nd in (2, 3) and x.shape[0] == 1 and x.dtype == torch.float32 and x.shape[1] % 4 == 0):
        raise UnsupportedLayer("MaxPooling %s on %s %s" % (pool, x.dtype, tuple(x.shape)))
    cl, split = _cl(nd), is_split16(x)
    if not split:
        x = _as_cl(x, cl)
    S = (1,) * (3 - nd) + tuple(int(v) for v in x.shape[2:])
    P = (1,) * (3 - nd) + pool
    out = torch.empty((1, x.shape[1]) + tuple(s // p for s, p in zip(x.shape[2:], pool)), dtype=torch.float32, device=x.device, memory_format=cl)
    if out.numel():
        N.dcall(x, "sd_maxpool_split16_ndhwc_device" if split else "sd_maxpool_ndhwc_device", _vp(x), int(x.shape[1]), *S, *P, _vp(out))
    return _tag_split16(out, getattr(x, "_sd_producer", None)) if split else out


def _head_rows(feat, rows, weight, bias, clamp_min):
    """the 1x1 head (weight (R, C, 1...), bias) on rows of the channels-last feature matrix feat (..., C): (len(rows), R), clamped from
    below; rows None = all (sd_head_rows_device: an fp32-MFMA GEMM with a fixed summation order per output)"""
    C, R = feat.shape[-1], weight.shape[0]
    feat = feat.reshape(-1, C)
    n = feat.shape[0] if rows is None else int(rows.shape[0])
    out = torch.empty((n, R), dtype=torch.float32, device=feat.device)
    if n:
        w = weight.detach().reshape(R, C).contiguous()
        N.dcall(feat, "sd_head_rows_device", _vp(feat), C, ctypes.c_void_p(rows.data_ptr() if rows is not None else None), n, _vp(w),
                ctypes.c_void_p(bias.data_ptr() if bias is not None else None), R, float(clamp_min), _vp(out))
    return out


def _prob_head(feat, part, C, n_pix, w, bias, prob):
    """the one-channel head over C feature channels into `prob`: from the per-lane terms `part` a fused layer left (sd_dot_combine_device:
    bit-identical to the other form on the same features, which are not re-read), or -- part None -- sd_bias_act_dot_device on the features"""
    b = ctypes.c_void_p(bias.data_ptr() if bias is not None else None)
    if part is not None:
        N.dcall(feat, "sd_dot_combine_device", _vp(part), C // 32, n_pix, b, 1, _vp(prob))
    else:
        N.dcall(feat, "sd_bias_act_dot_device", _vp(feat), None, None, n_pix, C, 0, _vp(w), b, 1, _vp(prob))
