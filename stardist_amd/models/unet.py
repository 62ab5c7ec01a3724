"""The StarDist network re-expressed in PyTorch-ROCm (channels_last, convolutions on MFMA).

Topology restated from the reference's Keras graph:
  StarDist2D._build          stardist/models/model2d.py:310-349
  StarDist3D._build_unet     stardist/models/model3d.py:360-399
  StarDist3D._build_resnet   stardist/models/model3d.py:402-447
  csbdeep.internals.blocks.unet_block / resnet_block (csbdeep>=0.8.0, not vendored; published
  semantics restated: 'same' zero padding, max-pool 'valid' stride=pool, nearest up-sampling,
  Concatenate([up, skip]) in that order).
Keras layer names are kept as module names so a Keras weight file maps 1:1 (kernel
(k..., cin, cout) -> torch (cout, cin, k...)).
U-Net parity against TensorFlow is unpinned in this environment (no TF, no weights).
"""
import functools
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

# the hand-written inference layers: everything that calls the library (re-exported: these ARE native_layers' objects)
from .native_layers import (  # noqa: F401
    N_FLAG_SLOTS, NO_STORE, UnsupportedLayer, _bn_fold, _conv_bias_act, _general_conv, _hand_conv, _head_rows, _layer_desc, _native_inference,
    _native_max_pool, _prob_head, _upcat_general, conv_mode, conv_rows, force_conv_mode, force_split16, is_chunked_3x3, is_split16, range_flag,
    split16_enabled, split16_pack, split16_replan, split16_unpack, tf_same_pad_before, use_range_flags)


def _act(name):
    if name in (None, "linear"):
        return nn.Identity()
    if name == "relu":
        return nn.ReLU(inplace=True)
    if name == "elu":
        return nn.ELU(inplace=True)
    if name == "sigmoid":
        return nn.Sigmoid()
    if name == "tanh":
        return nn.Tanh()
    raise ValueError("activation %s not supported" % name)


def act_kind(module):
    """the activation as the kernels' epilogues know it: 0 linear, 1 relu, -1 another one (not fused)"""
    return 0 if isinstance(module, nn.Identity) else (1 if isinstance(module, nn.ReLU) else -1)


class ConvAct(nn.Sequential):
    """[conv, activation] (or [conv, batch-norm, activation]) with the Keras layer's parameter names.  GPU inference: one launch of a
    hand-written kernel (bias, folded batch-norm and linear / relu activation in its epilogue); everywhere else the plain Sequential."""

    def parts(self):
        """(conv, batch-norm or None, kind) with kind 0 linear / 1 relu / -1 another activation"""
        conv, bn, act = (self[0], None, self[1]) if len(self) == 2 else (self[0], self[1], self[2])
        return conv, bn, act_kind(act)

    def forward(self, x):
        conv, bn, kind = self.parts()
        y = _conv_bias_act(conv, x, kind, bn)
        return super().forward(x) if y is None else y


def _conv(nd, cin, cout, k, act="relu", bias=True, batch_norm=False):
    k = tuple(k) if isinstance(k, (tuple, list)) else (k,) * nd
    Conv = nn.Conv2d if nd == 2 else nn.Conv3d
    assert all(kk % 2 == 1 for kk in k), "Keras 'same' padding restated for odd kernels only"
    conv = Conv(cin, cout, k, padding=tuple(kk // 2 for kk in k), bias=bias)
    if batch_norm:
        # csbdeep conv_block2/3 (csbdeep/internals/blocks.py): Conv -> BatchNormalization -> Activation; Keras defaults
        # epsilon = 1e-3, momentum 0.99 (inference uses the moving statistics)
        BN = nn.BatchNorm2d if nd == 2 else nn.BatchNorm3d
        return ConvAct(conv, BN(cout, eps=1e-3, momentum=0.01), _act(act))
    return ConvAct(conv, _act(act))


def max_pool(x, pool):
    """Keras MaxPooling ('valid', stride = pool).  GPU inference: the native one-pass channels-last kernel; everywhere else F.max_pool."""
    pool = tuple(int(p) for p in pool)
    if _native_inference(x):
        return _native_max_pool(x, pool)
    return (F.max_pool2d if x.dim() == 4 else F.max_pool3d)(x, pool)


class UNetBlock(nn.Module):
    """csbdeep unet_block(n_depth, n_filter_base, kernel_size, n_conv_per_depth, activation,
    last_activation, pool) without batch-norm/dropout (inference)."""

    def __init__(self, nd, cin, n_depth, n_filter_base, kernel_size, n_conv_per_depth, activation, last_activation, pool,
                 batch_norm=False):
        super().__init__()
        self.nd, self.n_depth, self.pool = nd, n_depth, tuple(pool)
        _conv = functools.partial(globals()["_conv"], batch_norm=batch_norm)
        self.down = nn.ModuleList()
        c = cin
        for n in range(n_depth):
            convs = []
            for i in range(n_conv_per_depth):
                convs.append(_conv(nd, c, n_filter_base * 2 ** n, kernel_size, activation)); c = n_filter_base * 2 ** n
            self.down.append(nn.Sequential(*convs))
        mid = []
        for i in range(n_conv_per_depth - 1):
            mid.append(_conv(nd, c, n_filter_base * 2 ** n_depth, kernel_size, activation)); c = n_filter_base * 2 ** n_depth
        mid.append(_conv(nd, c, n_filter_base * 2 ** max(0, n_depth - 1), kernel_size, activation)); c = n_filter_base * 2 ** max(0, n_depth - 1)
        self.middle = nn.Sequential(*mid)
        self.up = nn.ModuleList()
        for n in reversed(range(n_depth)):
            c = c + n_filter_base * 2 ** n          # concat [up, skip]
            convs = []
            for i in range(n_conv_per_depth - 1):
                convs.append(_conv(nd, c, n_filter_base * 2 ** n, kernel_size, activation)); c = n_filter_base * 2 ** n
            convs.append(_conv(nd, c, n_filter_base * 2 ** max(0, n - 1), kernel_size, activation if n > 0 else last_activation))
            c = n_filter_base * 2 ** max(0, n - 1)
            self.up.append(nn.Sequential(*convs))
        self.out_channels = c

    def forward(self, x):
        skips = []
        for blk in self.down:
            x = blk(x)
            skips.append(x)
            x = max_pool(x, self.pool)
        x = self.middle(x)
        for blk, skip in zip(self.up, reversed(skips)):
            if _native_inference(x):
                # UpSampling + Concatenate + Conv (+ BN) + bias + activation as ONE launch: the up-sampled and the concatenated tensors
                # of the reference's graph are never written
                first = blk[0]
                conv0, bn, kind = first.parts()
                srcs = [(x, tuple(p == 2 for p in self.pool)), (skip, 0)]
                y = _hand_conv(conv0, srcs, kind, bn=bn) if (all(p in (1, 2) for p in self.pool) and kind >= 0) else None
                if y is None and kind >= 0:
                    y = _upcat_general(conv0, x, skip, self.pool, kind, bn)      # coverage path (channel counts not in 32-chunks)
                if y is None:
                    raise UnsupportedLayer("up-level " + _layer_desc(conv0, srcs) + ", pool %s" % (self.pool,))
                x = blk[1:](y)
                continue
            x = F.interpolate(x, scale_factor=tuple(float(p) for p in self.pool), mode="nearest")
            x = blk(torch.cat([x, skip], dim=1))
        return x


class ResNetBlock(nn.Module):
    """csbdeep resnet_block(n_filter, kernel_size, pool, n_conv_per_block, batch_norm, activation): first conv strided by
    `pool`, last conv linear, 1x1 strided projection on the shortcut when shape changes, add, activation.
    batch_norm=True (model3d.py:402-412 hands resnet_batch_norm through): every convolution of the block is bias-free
    (use_bias = not batch_norm, the shortcut projection included) and each BODY convolution -- the last one too, i.e. before the
    Add -- is followed by a BatchNormalization; the projection has none."""

    def __init__(self, nd, cin, n_filter, kernel_size, pool, n_conv_per_block, activation, batch_norm=False):
        super().__init__()
        Conv = nn.Conv2d if nd == 2 else nn.Conv3d
        BN = nn.BatchNorm2d if nd == 2 else nn.BatchNorm3d
        k = tuple(kernel_size)
        pad = tuple(kk // 2 for kk in k)
        self.pool = tuple(pool)
        self.k = k
        bias = not batch_norm
        bn = (lambda: [BN(n_filter, eps=1e-3, momentum=0.01)]) if batch_norm else (lambda: [])       # Keras defaults (see _conv)
        self.first = Conv(cin, n_filter, k, stride=self.pool, padding=0, bias=bias)   # Keras 'same' + stride pads asymmetrically
        layers = bn() + [_act(activation)]
        for _ in range(n_conv_per_block - 2):
            layers += [Conv(n_filter, n_filter, k, padding=pad, bias=bias)] + bn() + [_act(activation)]
        layers += [Conv(n_filter, n_filter, k, padding=pad, bias=bias)] + bn()
        self.body = nn.Sequential(*layers)
        self.proj = None
        if any(p != 1 for p in self.pool) or cin != n_filter:
            self.proj = Conv(cin, n_filter, (1,) * nd, stride=self.pool, bias=bias)
        self.act = _act(activation)

    def _same_pad(self, x):
        """x zero-padded as TensorFlow 'SAME' pads it for the strided first convolution (F.pad order: last axis first)"""
        pads = []
        for n, k, s in reversed(list(zip(x.shape[2:], self.k, self.pool))):
            before = tf_same_pad_before(n, k, s)
            pads += [before, max((-(-n // s) - 1) * s + k - n, 0) - before]          # behind: the rest up to the output size ceil(n / s)
        return F.pad(x, pads)

    def _stages(self):
        """[(conv, batch-norm or None, activation module or None)] in graph order: the strided first convolution, then the body's"""
        BNs = (nn.BatchNorm2d, nn.BatchNorm3d)
        out, cur = [], [self.first, None, None]
        for m in self.body:
            if isinstance(m, (nn.Conv2d, nn.Conv3d)):
                out.append(tuple(cur))
                cur = [m, None, None]
            elif isinstance(m, BNs):
                cur[1] = m
            else:
                cur[2] = m
        out.append(tuple(cur))
        return out

    def _forward_hand(self, x):
        """the block on the hand-written kernels: strided first convolution (TensorFlow 'same' padding) with its activation, body
        convolutions, the strided 1x1 projection, and Add + Activation folded into the last convolution's epilogue; batch-norm layers
        folded into the (bias-free) kernels and a bias -- the last one before the Add, as the reference's graph has it"""
        kind, stages = act_kind, self._stages()
        if not (all(kind(a) >= 0 for _, _, a in stages[:-1]) and kind(self.act) >= 0):
            raise UnsupportedLayer("resnet_block activation %s" % type(self.act).__name__)
        if any(b is not None and b.training for _, b, _ in stages):
            raise UnsupportedLayer("resnet_block with batch-norm layers in training mode")

        def need(y, conv, src):
            if y is None:
                raise UnsupportedLayer("resnet_block " + _layer_desc(conv, [(src, 0)]))
            return y
        conv, bn, act = stages[0]
        y = need(_hand_conv(conv, [(x, 0)], kind(act), bn=bn, tf_same=True), conv, x)
        sc = x
        if self.proj is not None:
            sc = need(_hand_conv(self.proj, [(x, 0)], 0, tf_same=True), self.proj, x)
        for conv, bn, act in stages[1:]:
            last = act is None
            y = need(_hand_conv(conv, [(y, 0)], kind(self.act) if last else kind(act), res=sc if last else None, bn=bn), conv, y)
        return y

    def forward(self, x):
        if _native_inference(x):
            return self._forward_hand(x)
        y = self.body(self.first(self._same_pad(x)))
        if self.proj is not None:
            x = self.proj(x)
        return self.act(x + y)


class StarDistNet(nn.Module):
    """input (N,C,...) -> prob (N,1,...), dist (N,n_rays,...)[, prob_class (N,n_classes+1,...)]"""

    def __init__(self, config):
        super().__init__()
        cfg = config
        nd = cfg.n_dim
        self.nd = nd
        self.pre = nn.ModuleList()
        c = cfg.n_channel_in
        grid = np.asarray(cfg.grid)
        if cfg.backbone == "unet":
            pooled = np.ones(nd, int)
            while tuple(pooled) != tuple(grid):                       # model2d.py:317-325
                pool = 1 + (grid > pooled)
                pooled = pooled * pool
                convs = []
                for _ in range(cfg.unet_n_conv_per_depth):
                    convs.append(_conv(nd, c, cfg.unet_n_filter_base, cfg.unet_kernel_size, cfg.unet_activation)); c = cfg.unet_n_filter_base
                self.pre.append(nn.ModuleDict(dict(convs=nn.Sequential(*convs))))
                self.pre[-1].pool = tuple(int(p) for p in pool)
            self.backbone = UNetBlock(nd, c, cfg.unet_n_depth, cfg.unet_n_filter_base, cfg.unet_kernel_size,
                                      cfg.unet_n_conv_per_depth, cfg.unet_activation, cfg.unet_last_activation,
                                      cfg.unet_pool, cfg.unet_batch_norm)
            c = self.backbone.out_channels
            n_after, k_after, act_after = cfg.net_conv_after_unet, cfg.unet_kernel_size, cfg.unet_activation
        elif cfg.backbone == "resnet":                                 # model3d.py:402-447
            n_filter = cfg.resnet_n_filter_base
            blocks = [_conv(nd, c, n_filter, (7,) * nd, None),        # linear (no activation) model3d.py:416-417
                      _conv(nd, n_filter, n_filter, (3,) * nd, None)]
            c = n_filter
            pooled = np.ones(nd, int)
            for n in range(cfg.resnet_n_blocks):
                pool = 1 + (grid > pooled)
                pooled = pooled * pool
                if any(p > 1 for p in pool):
                    n_filter *= 2
                blocks.append(ResNetBlock(nd, c, n_filter, cfg.resnet_kernel_size, tuple(int(p) for p in pool),
                                          cfg.resnet_n_conv_per_block, cfg.resnet_activation, bool(getattr(cfg, "resnet_batch_norm", False))))
                c = n_filter
            self.backbone = nn.Sequential(*blocks)
            n_after, k_after, act_after = cfg.net_conv_after_resnet, cfg.resnet_kernel_size, cfg.resnet_activation
        else:
            raise ValueError(cfg.backbone)
        self.features = _conv(nd, c, n_after, k_after, act_after) if n_after > 0 else nn.Identity()
        cf = n_after if n_after > 0 else c
        Conv = nn.Conv2d if nd == 2 else nn.Conv3d
        self.prob = Conv(cf, 1, (1,) * nd)
        self.dist = Conv(cf, cfg.n_rays, (1,) * nd)
        self.n_classes = cfg.n_classes
        if cfg.n_classes is not None:
            self.features_class = _conv(nd, c, n_after, k_after, act_after) if n_after > 0 else nn.Identity()
            self.prob_class = Conv(cf, cfg.n_classes + 1, (1,) * nd)
        self._plan_split16()

    def _plan_split16(self):
        """mark (conv.__dict__["_sd_split_out"]) the layers whose output travels as a split16 tensor (see split16_enabled): 3x3(x3)
        stride-1 layers with relu / linear activation over 32-channel chunks (or the one-channel first layer with 32 outputs) whose EVERY
        reader is such a layer, directly or through a max-pooling.  U-Net backbones only (a ResNet block's shortcut and strided layers
        read f32)."""
        nd = self.nd

        def layer_ok(m, as_producer):
            if not isinstance(m, ConvAct):
                return False
            conv, _, kind = m.parts()          # (the one-channel first layer writes split16 with 32 outputs only)
            return kind >= 0 and is_chunked_3x3(conv, nd, first=as_producer) and (conv.in_channels != 1 or conv.out_channels == 32)

        readers = {}

        def feed(prods, reader):
            for p in prods:
                readers.setdefault(p, []).append(reader)

        def run(seq, cur):
            for m in seq:
                feed(cur, m)
                cur = [m]
            return cur
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv3d)):
                m.__dict__["_sd_split_out"] = False
        if not isinstance(self.backbone, UNetBlock):
            return
        cur = []
        for st in self.pre:
            cur = run(st["convs"], cur)
        bb = self.backbone
        if not all(p in (1, 2) for p in bb.pool):
            return
        skips = []
        for blk in bb.down:
            cur = run(blk, cur)
            skips.append(cur)
        cur = run(bb.middle, cur)
        for blk, skip in zip(bb.up, reversed(skips)):
            cur = run(blk, cur + skip)
        feed(cur, self.features)
        if self.n_classes is not None:
            feed(cur, self.features_class)
        for p, rs in readers.items():
            if layer_ok(p, True) and all(layer_ok(r, False) for r in rs):
                p.parts()[0].__dict__["_sd_split_out"] = True

    def _heads(self, base):
        """the plain graph: features conv, prob (Conv 1x1 + sigmoid), dist (Conv 1x1)[, class head] -- on the GPU every convolution is
        a hand-written kernel (64-bit indexing: no slabs whatever the volume), elsewhere the torch modules"""
        f = self.features(base)
        p = _conv_bias_act(self.prob, f, 0)
        prob = torch.sigmoid_(p) if p is not None else torch.sigmoid(self.prob(f))
        dist = _conv_bias_act(self.dist, f, 0)
        if dist is None:
            dist = self.dist(f)
        if self.n_classes is not None:
            return prob, dist, self._class_head(base)
        return prob, dist

    def _class_head(self, base):
        """softmax(prob_class(features_class(base))): the multi-class head (model2d.py:339-347, model3d.py:443-452)"""
        f = self.features_class(base)
        y = _conv_bias_act(self.prob_class, f, 0)
        return torch.softmax(y if y is not None else self.prob_class(f), dim=1)

    # ---- fused heads (GPU inference) ----------------------------------------------------------------------------------------
    # features conv -> ONE pass doing the probability head (sd_bias_act_dot_device) -> distance head as an fp32-MFMA
    # GEMM over the rows asked for (sd_head_rows_device): every pixel for the dense prediction, or -- sparse_head=True -- none here:
    # the caller selects the candidate pixels from the probabilities and evaluates the distance head on those rows only
    # (StarDistBase._predict_sparse_generator), so the dense n_rays-channel tensor of the reference's predict_sparse
    # (base.py:553-610: full prediction, then masking) is never written.  Both paths run the same kernels with a fixed summation
    # order per output, hence agree bit for bit.
    fused_heads = True                        # False: plain graph on the GPU as well (statistics hooks, A/B timing)

    def _fused_heads_ok(self, base):
        f = self.features
        if not (self.fused_heads and _native_inference(base) and base.shape[0] == 1 and base.dtype == torch.float32
                and isinstance(f, ConvAct) and len(f) == 2 and f[0].bias is not None):
            return False
        C, R = f[0].out_channels, self.dist.out_channels
        return act_kind(f[1]) >= 0 and C in (32, 64, 128, 256) and R <= 128 and C * (((R + 31) // 32) * 32 + 1) * 4 <= 64 * 1024

    # The sparse path without the dense feature tensor (round 6): the features layer runs with the probability head fused and WITHOUT its
    # store (head_mode "sparse_lazy": forward returns (prob, backbone output)); dist_rows then evaluates the layer on the candidate rows
    # (conv_rows, bit-identical to the dense layer) and the distance head on those.  2 GiB (2048^2) / 8.6 GB (256^3) are never written.
    # Measured (round 6): the row kernel costs 0.25 ms at 4e5 (2D) / 1.7e5 (3D) candidates (half of it the weight blocks every workgroup
    # stages, 0.1 ms the gathers), the dense store it replaces 0.15 ms at 2048^2 (2.1 GB) and 0.3 ms at 256^3 (8.6 GB): the dense tensor is
    # kept while it is small, from lazy_features_min_bytes on (and for the blocks of a sharded input: 10 GB / 90 GB each) it is not written.
    lazy_features = True                      # False (or STARDIST_AMD_LAZY_FEATURES=0): the dense feature tensor always
    lazy_features_min_bytes = 4 << 30

    def _lazy_ok(self, base):
        f = self.features
        if not (self.lazy_features and os.environ.get("STARDIST_AMD_LAZY_FEATURES", "1") != "0" and conv_mode() == "f16x3" and isinstance(f, ConvAct)):
            return False
        conv, bn, kind = f.parts()
        if int(np.prod(base.shape[2:])) * conv.out_channels * 4 < self.lazy_features_min_bytes:
            return False
        return (bn is None and kind >= 0 and is_chunked_3x3(conv, self.nd) and conv.__dict__.get("_sd_force_form") != "bf16x6"
                and base.shape[1] == conv.in_channels)

    def feature_rows(self, base_cl, rows):
        """features (after bias + activation) of the pixels `rows` from the backbone output given as its channels-last view (..., C_in)"""
        nd = base_cl.dim() - 1
        x = base_cl.permute(*([nd] + list(range(nd)))).unsqueeze(0)          # back to (1, C, *spatial): the channels-last tensor itself
        if getattr(self, "_lazy_split16", False):
            x._sd_split16 = True
        conv, _, kind = self.features.parts()
        return conv_rows(conv, x, kind, rows)

    def dist_rows(self, feat, rows, clamp_min, lazy=False, order=None):
        """distance head on rows of the channels-last feature matrix feat (n_pix, C): (len(rows), n_rays); rows None = all.
        lazy: `feat` is the BACKBONE output (head_mode "sparse_lazy") -- the features of the pixels `rows` are evaluated first (give the
        rows in SPATIAL order: the gathered 3x3 neighbourhoods then share cache lines) and the head runs on them, in the order `order`
        (indices into rows; None: as they are)"""
        if lazy:
            feat, rows = self.feature_rows(feat, rows), order
        return _head_rows(feat, rows, self.dist.weight, self.dist.bias, clamp_min)

    def _heads_fused(self, base, sparse_head):
        conv, kind = self.features[0], act_kind(self.features[1])
        nd, S, C = base.dim() - 2, tuple(base.shape[2:]), conv.out_channels
        wp = self.prob.weight.detach().reshape(-1).contiguous()
        prob = torch.empty((1, 1) + S, dtype=torch.float32, device=base.device)
        holder = []
        # features conv with bias + activation fused (64-bit indexing: no slabs); the split-fp16 kernel also takes the probability head's
        # dot product over each workgroup's 32 channels while the tile is in registers
        lazy = bool(sparse_head) and self._lazy_ok(base)
        feat = _hand_conv(conv, [(base, 0)], kind, dot=(wp, holder), no_store=lazy)
        if feat is None:
            raise UnsupportedLayer("features " + _layer_desc(conv, [(base, 0)]))
        self._lazy_now = feat is NO_STORE
        if feat is NO_STORE:
            self._lazy_split16 = is_split16(base)
            feat = base                       # what the caller gets in place of the features: dist_rows(..., lazy=True) works from it
        # ... the per-lane terms -> probabilities; without them the probability head alone: one read of the features
        _prob_head(feat, holder[0] if holder else None, C, int(np.prod(S)), wp, self.prob.bias, prob)
        if sparse_head:
            return prob, feat
        R = self.dist.out_channels
        dist = self.dist_rows(feat.permute(*([0] + list(range(2, nd + 2)) + [1])), None, float("-inf"))
        return prob, dist.view((1,) + S + (R,)).permute(*([0, nd + 1] + list(range(1, nd + 1))))

    def forward(self, x, sparse_head=False):
        """(prob, dist[, prob_class]); with sparse_head=True and the fused heads available: (prob, features[, prob_class]) and
        self.head_mode == "sparse" -- the distance head is then evaluated by the caller on the rows it selects (dist_rows)"""
        for st in self.pre:
            x = max_pool(st["convs"](x), st.pool)
        base = self.backbone(x)
        self.head_mode = "dense"
        if self._fused_heads_ok(base):
            out = self._heads_fused(base, sparse_head)
            if sparse_head:
                self.head_mode = "sparse_lazy" if getattr(self, "_lazy_now", False) else "sparse"
            if self.n_classes is not None:
                out = tuple(out) + (self._class_head(base),)
            return tuple(out)
        return self._heads(base)


def init_he_normal_(net, seed=0):
    """Seeded He-normal kernels / small biases: real weights are not available offline
    (.MISSING_LARGE_BLOBS); throughput is weight independent."""
    g = torch.Generator().manual_seed(seed)
    for m in net.modules():
        if isinstance(m, (nn.Conv2d, nn.Conv3d)):
            fan_in = m.in_channels * int(np.prod(m.kernel_size))
            with torch.no_grad():
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * float(np.sqrt(2.0 / fan_in)))
                if m.bias is not None:
                    m.bias.zero_()
    return net


def conv_macs_per_input_pixel(net, cfg):
    """analytic multiply-accumulates per INPUT pixel of the conv stack (for the MFMA roofline): counted by forward hooks on a CPU copy
    of the modules (the GPU inference path does not go through the modules' forward)."""
    import copy
    nd = cfg.n_dim
    size = 64 if nd == 2 else 32
    shape = tuple(size * g for g in cfg.grid)
    macs = [0.0]
    hooks = []
    net = copy.deepcopy(net).cpu()

    def hook(m, inp, out):
        k = float(np.prod(m.kernel_size))
        macs[0] += out.numel() / out.shape[0] * (m.in_channels * k)
    for m in net.modules():
        if isinstance(m, (nn.Conv2d, nn.Conv3d)):
            hooks.append(m.register_forward_hook(hook))
    with torch.no_grad():
        net(torch.zeros((1, cfg.n_channel_in) + shape))
    for h in hooks:
        h.remove()
    return macs[0] / float(np.prod(shape))
