"""StarDist3D training on the library's own kernels (the reference's StarDist3D.train, stardist/models/model3d.py:450-560, with the
losses of stardist/models/base.py:34-60, 315-325 and the data generator StarDistData3D, model3d.py:30-104, without classes).

  patches      TrainData3D: StarDistData3D's patch part on the 2D generator's restatement (training.TrainData2D: sample_patches,
               get_valid_inds, StarDistDataBase.get_valid_inds with foreground_prob, the max-filter and sample_ind_cache, csbdeep's
               RollingSequence.batch / choice): the same np.random draws in the same order, so np.random.seed(s) gives the reference's
               patches.  The augmenter runs on the host.
  targets      one upload of the batch's label patches; prob = edt_prob(lbl, anisotropy) of the FULL patch, sub-sampled by the grid
               afterwards (model3d.py:86-88, unlike 2D), by sd_edt_prob_device; dist = star_dist3D with the grid on the labels read as
               uint16 (sd_star_dist3d_device): equal to stardist_targets(..., rays=, grid=, anisotropy=) bit for bit.
  forward      the exact-f32 kernels of inference over the parameters of the model's StarDistNet, one sample at a time:
               sd_conv3_ndhwc_device (kz = 3, two sources, up bit 4 = z; with the residual epilogue sd_conv3_res_ndhwc_device for the
               last convolution of a ResNet block), sd_convg_ndhwc_device for the 7x7x7 stem, the strided first convolution of a block
               and its strided 1x1x1 projection (TensorFlow 'same' padding), sd_maxpool_ndhwc_device; the 1x1x1 heads and the losses
               are training.HeadsLoss with the batch and z folded into one axis.
  backward     csrc/train3d.hip: weight / bias gradients of 3x3x3 and of general (strided, 7x7x7, 1x1x1) convolutions, the data gradient
               of strided convolutions, the 3D max-pool and up-sampling adjoints; the data gradient of a stride-1 3x3x3 layer is the
               forward kernel on the flipped, transposed kernel; ReLU adjoints by sd_relu_mask_device (a ResNet block's Add + ReLU: one
               mask on the block output, the result feeds both branches).
  loss         sd_stardist_loss2d_device with n_pix = B * d * h * w (the 3D model uses the same losses and metrics; in train3d()
               sd_stardist_loss2d_metrics_device, the metrics per voxel).
  optimiser    training.Adam / ReduceLROnPlateau, the epoch loop and checkpoints of training.fit.
Scope: check_trainable3d() names the first setting outside it."""

import numpy as np
import torch

from .lib import _native as N
from .training import HeadsLoss, TrainData2D, _p, begin_training, fit


# ---- data ----------------------------------------------------------------------------------------------------------------------
class TrainData3D(TrainData2D):
    """StarDistData3D (no classes, one channel) on top of csbdeep's RollingSequence: sample(i) is what its __getitem__(i) draws (volume
    and label patches after the augmenter), batch_device(i) adds the targets, computed on the device"""
    _nd = 3

    def __init__(self, X, Y, batch_size, rays, length, patch_size=(128, 128, 128), grid=(1, 1, 1), anisotropy=None, augmenter=None,
                 foreground_prob=0, sample_ind_cache=True, maxfilter_patch_size=None):
        super().__init__(X, Y, batch_size, len(rays), length, patch_size=patch_size, grid=grid, augmenter=augmenter,
                         foreground_prob=foreground_prob, sample_ind_cache=sample_ind_cache, maxfilter_patch_size=maxfilter_patch_size)
        self.rays, self.anisotropy = rays, anisotropy

    def batch_device(self, i, device):
        """x (B, D, H, W, 1), prob_true (B, d, h, w), dist_true_mask (B, d, h, w, n_rays + 1): float32 device tensors"""
        X, Y = self.sample(i)
        x = torch.from_numpy(np.ascontiguousarray(np.stack(X)[..., None], np.float32)).to(device, non_blocking=False)
        prob, dtm = targets_device3d(Y, self.rays, self.grid, self.anisotropy, device)
        return x, prob, dtm


def targets_device3d(Y, rays, grid, anisotropy, device):
    """the targets of StarDistData3D.__getitem__ (model3d.py:66-104, no classes) for the label volumes Y (one shape) from ONE upload:
    prob_true (B, d, h, w) (-1 where the sub-sampled label is negative) and dist_true_mask (B, d, h, w, n_rays + 1) on `device`"""
    from .utils import edt_prob
    Y = [np.asarray(y) for y in Y]
    gz, gy, gx = (int(g) for g in grid)
    neg = [y[::gz, ::gy, ::gx] < 0 for y in Y]
    has_neg = any(m.any() for m in neg)
    if has_neg:
        Y = [np.maximum(y, 0) for y in Y]
    lab = np.stack(Y)
    if lab.size and int(lab.max()) >= 2 ** 31:
        raise ValueError("label ids must fit int32")
    B, Z, H, W = lab.shape
    R = len(rays)
    d_lab = torch.from_numpy(np.ascontiguousarray(lab, np.int32)).to(device)
    # star_dist3D reads the labels as unsigned short (the reference's geom3d casts with astype(np.uint16))
    d_u16 = d_lab.to(torch.uint16).contiguous()
    rz, ry, rx = (torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(device) for v in np.asarray(rays.vertices).T)
    samp = (1.0, 1.0, 1.0) if anisotropy is None else tuple(float(a) for a in anisotropy)
    d, h, w = (Z - 1) // gz + 1, (H - 1) // gy + 1, (W - 1) // gx + 1
    prob = torch.empty((B, d, h, w), dtype=torch.float32, device=device)
    dist = torch.empty((B, d, h, w, R), dtype=torch.float32, device=device)
    full = torch.empty((Z, H, W), dtype=torch.float32, device=device)
    for b in range(B):
        lo, hi = (int(lab[b].min()), int(lab[b].max())) if lab[b].size else (0, 0)
        if (lo == hi and lo > 0) or hi > 4 * lab[b].size + 1024:
            pf = edt_prob(d_lab[b], anisotropy=anisotropy)      # the special cases of edt_prob (constant volume, sparse huge ids)
        else:
            N.dcall(d_lab, "sd_edt_prob_device", _p(d_lab[b]), Z, H, W, samp[0], samp[1], samp[2], max(hi, 0), _p(full))
            pf = full
        prob[b] = pf[::gz, ::gy, ::gx]
        N.dcall(d_u16, "sd_star_dist3d_device", _p(d_u16[b]), Z, H, W, _p(rz), _p(ry), _p(rx), R, gz, gy, gx, _p(dist[b]))
    dtm = torch.cat([dist, prob[..., None]], dim=-1).contiguous()
    if has_neg:
        prob[torch.from_numpy(np.stack(neg)).to(device)] = -1
    return prob, dtm


# ---- scope ---------------------------------------------------------------------------------------------------------------------
def check_trainable3d(config):
    """raise NotImplementedError naming the first setting outside the scope of the native 3D training"""
    c = config

    def no(what):
        raise NotImplementedError("StarDist3D.train on the native kernels does not support %s" % what)

    def multiple_of_32(key):
        v = getattr(c, key)
        if v % 32 != 0 or v <= 0:
            no("%s = %d (a positive multiple of 32 only)" % (key, v))

    def act(key):
        if getattr(c, key) not in ("relu", "linear", None):
            no("%s = %r (relu or linear only)" % (key, getattr(c, key)))
    if getattr(c, "n_dim", 3) != 3:
        no("n_dim = %s (3D only)" % c.n_dim)
    if c.backbone not in ("unet", "resnet"):
        no("backbone = %r (unet or resnet only)" % c.backbone)
    if c.n_classes is not None:
        no("n_classes = %r (single class only)" % (c.n_classes,))
    if c.n_channel_in != 1:
        no("n_channel_in = %d (one input channel only)" % c.n_channel_in)
    if c.train_dist_loss not in ("mae", "mse"):
        no("train_dist_loss = %r ('mae' or 'mse' only)" % c.train_dist_loss)
    if getattr(c, "train_shape_completion", False):
        no("train_shape_completion = True")
    grid = tuple(int(g) for g in c.grid)
    if not all(g >= 1 and (g & (g - 1)) == 0 for g in grid):
        no("grid = %s (powers of two only)" % (grid,))
    if c.backbone == "unet":
        if c.unet_batch_norm:
            no("unet_batch_norm = True")
        if float(getattr(c, "unet_dropout", 0.0)) != 0.0:
            no("unet_dropout = %r" % c.unet_dropout)
        if tuple(c.unet_kernel_size) != (3, 3, 3):
            no("unet_kernel_size = %s (3x3x3 only)" % (tuple(c.unet_kernel_size),))
        multiple_of_32("unet_n_filter_base")
        if c.unet_n_filter_base * 2 ** c.unet_n_depth > 512:
            no("unet_n_filter_base * 2**unet_n_depth = %d (at most 512 channels per layer)" % (c.unet_n_filter_base * 2 ** c.unet_n_depth))
        if not all(p in (1, 2) for p in c.unet_pool):
            no("unet_pool = %s (1 or 2 per axis)" % (tuple(c.unet_pool),))
        multiple_of_32("net_conv_after_unet")
        act("unet_activation")
        act("unet_last_activation")
    else:
        if getattr(c, "resnet_batch_norm", False):
            no("resnet_batch_norm = True")
        if tuple(c.resnet_kernel_size) != (3, 3, 3):
            no("resnet_kernel_size = %s (3x3x3 only)" % (tuple(c.resnet_kernel_size),))
        multiple_of_32("resnet_n_filter_base")
        if c.resnet_n_conv_per_block < 2:
            no("resnet_n_conv_per_block = %d (at least 2)" % c.resnet_n_conv_per_block)
        # the blocks' strides as StarDistNet builds them (model3d.py:418-422): the filter count doubles with every strided block
        pooled, n_filter = np.ones(3, int), c.resnet_n_filter_base
        for _ in range(c.resnet_n_blocks):
            pool = 1 + (np.asarray(grid) > pooled)
            pooled = pooled * pool
            n_filter *= 2 if (pool > 1).any() else 1
        if n_filter > 512:
            no("resnet_n_filter_base with %d strided blocks = %d channels (at most 512 per layer)" % (int(np.log2(n_filter // c.resnet_n_filter_base)), n_filter))
        multiple_of_32("net_conv_after_resnet")
        act("resnet_activation")


# ---- layers --------------------------------------------------------------------------------------------------------------------
_perm_cache = {}


def _pack_perm(kind, ci, co, k3, device):
    """the packing of sd_conv3_pack_weights_host (kind 'conv3', kz = 3) / sd_convg_pack_weights_host ('convg', kernel k3) as a gather on
    the device: (index into [0, w.flatten()...], mask of the weight positions, the weight-independent rest of the packed array)"""
    key = (kind, ci, co, k3, str(device))
    p = _perm_cache.get(key)
    if p is None:
        L = N.lib()
        n_w = co * ci * int(np.prod(k3))
        if n_w >= 2 ** 24:
            raise ValueError("layer too large for the packing map (%d weights)" % n_w)
        outs = []
        for src in (np.arange(1, n_w + 1, dtype=np.float32), np.zeros(n_w, np.float32)):
            if kind == "conv3":
                n = int(L.sd_conv3_packed_floats(ci, co, 3))
                if n < 0:
                    raise ValueError("sd_conv3: unsupported layer %d -> %d" % (ci, co))
                out = np.zeros(n, np.float32)
                N.check(L.sd_conv3_pack_weights_host(N.ptr(src), ci, co, 3, N.ptr(out)))
            else:
                n = int(L.sd_convg_packed_floats(ci, co, *k3))
                if n < 0:
                    raise ValueError("sd_convg: unsupported layer %d -> %d, kernel %s" % (ci, co, k3))
                out = np.zeros(n, np.float32)
                N.check(L.sd_convg_pack_weights_host(N.ptr(src), ci, co, *k3, N.ptr(out)))
            outs.append(out)
        ones, zeros = outs
        is_w = ones.view(np.uint32) != zeros.view(np.uint32)
        idx = np.where(is_w, ones, 0).astype(np.int64)
        p = tuple(torch.from_numpy(a).to(device) for a in (idx, is_w, zeros))
        _perm_cache[key] = p
    return p


def _packed(w, kind):
    """packed device form of the kernel w (co, ci, kz, ky, kx)"""
    co, ci = int(w.shape[0]), int(w.shape[1])
    idx, is_w, rest = _pack_perm(kind, ci, co, tuple(int(k) for k in w.shape[2:]), w.device)
    flat = torch.cat([w.new_zeros(1), w.reshape(-1)])
    return torch.where(is_w, flat.index_select(0, idx), rest).contiguous()


def _full_shape(t, up):
    """(D, H, W) of the convolution whose source t (B, d, h, w, C) is read through the up-sampling bits `up` (1 x, 2 y, 4 z)"""
    return int(t.shape[1]) << ((up >> 2) & 1), int(t.shape[2]) << ((up >> 1) & 1), int(t.shape[3]) << (up & 1)


def _conv3_fwd(src0, src1, wp, bias, up0, co, relu, res=None):
    B = int(src0.shape[0])
    D, H, W = _full_shape(src0, up0)
    c0, c1 = int(src0.shape[4]), (int(src1.shape[4]) if src1 is not None else 0)
    out = torch.empty((B, D, H, W, co), dtype=torch.float32, device=src0.device)
    for b in range(B):
        args = [_p(src0[b]), c0, c0, up0, _p(src1[b]) if src1 is not None else None, c1, c1, 0, D, H, W, 3, _p(wp), _p(bias)]
        if res is None:
            N.dcall(src0, "sd_conv3_ndhwc_device", *args, co, int(relu), _p(out[b]))
        else:
            N.dcall(src0, "sd_conv3_res_ndhwc_device", *args, _p(res[b]), co, co, int(relu), _p(out[b]))
    return out


class Conv3x3x3(torch.autograd.Function):
    """act(conv3x3x3([UpSampling(src0) | src1]) + bias (+ res)): tensors (B, D, H, W, C) float32; up0: the forward kernels' bit mask
    for src0 (1 x, 2 y, 4 z); res: the residual of a ResNet block's Add, added before the activation (or None)"""

    @staticmethod
    def forward(ctx, src0, src1, weight, bias, res, up0, relu):
        co = int(weight.shape[0])
        y = _conv3_fwd(src0, src1, _packed(weight.detach(), "conv3"), bias.detach(), up0, co, relu, res)
        ctx.save_for_backward(src0, src1, weight, y)
        ctx.up0, ctx.relu, ctx.has_res = up0, relu, res is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        src0, src1, weight, y = ctx.saved_tensors
        gy = gy.contiguous()
        B, D, H, W, co = (int(v) for v in y.shape)
        c0, c1 = int(src0.shape[4]), (int(src1.shape[4]) if src1 is not None else 0)
        if ctx.relu:
            g = torch.empty_like(gy)
            N.dcall(gy, "sd_relu_mask_device", _p(gy), _p(y), gy.numel(), _p(g))
        else:
            g = gy
        dw = torch.empty(tuple(weight.shape), dtype=torch.float32, device=g.device)
        db = torch.empty((co,), dtype=torch.float32, device=g.device)
        N.dcall(g, "sd_conv3_wgrad_ndhwc_device", _p(g), co, _p(src0), c0, ctx.up0, _p(src1), c1, 0, B, D, H, W, _p(dw), _p(db))
        d0 = d1 = None
        if ctx.needs_input_grad[0] or (src1 is not None and ctx.needs_input_grad[1]):
            # 'same' convolution of g with the flipped, transposed kernel = d(concatenated input)
            wt = weight.detach().flip(2, 3, 4).transpose(0, 1).contiguous()
            dcat = _conv3_fwd(g, None, _packed(wt, "conv3"), None, 0, c0 + c1, False)
            if ctx.up0 or src1 is not None:
                d0 = torch.empty_like(src0)
                d1 = torch.empty_like(src1) if src1 is not None else None
                N.dcall(dcat, "sd_upcat3d_adjoint_ndhwc_device", _p(dcat), c0, ctx.up0, c1, B, D, H, W, _p(d0), _p(d1))
            else:
                d0 = dcat
        return d0, d1, dw, db, (g if ctx.has_res else None), None, None


class ConvG(torch.autograd.Function):
    """act(conv(x) + bias) of any kernel k3, stride s3 and padding p3 before the first element (output extent O3): the ResNet stem,
    the strided first convolution and the 1x1x1 projection of a block.  x (B, D, H, W, C) float32."""

    @staticmethod
    def forward(ctx, x, weight, bias, k3, s3, p3, O3, relu):
        B, D, H, W, ci = (int(v) for v in x.shape)
        co = int(weight.shape[0])
        wp = _packed(weight.detach(), "convg")
        out = torch.empty((B,) + tuple(O3) + (co,), dtype=torch.float32, device=x.device)
        for b in range(B):
            N.dcall(x, "sd_convg_ndhwc_device", _p(x[b]), ci, ci, D, H, W, *k3, *s3, *p3, *O3, _p(wp), _p(bias.detach()), None, 0, co,
                    int(relu), _p(out[b]), co)
        ctx.save_for_backward(x, weight, out)
        ctx.geo, ctx.relu = (k3, s3, p3, O3), relu
        return out

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        k3, s3, p3, O3 = ctx.geo
        gy = gy.contiguous()
        B, D, H, W, ci = (int(v) for v in x.shape)
        co = int(weight.shape[0])
        if ctx.relu:
            g = torch.empty_like(gy)
            N.dcall(gy, "sd_relu_mask_device", _p(gy), _p(y), gy.numel(), _p(g))
        else:
            g = gy
        dw = torch.empty(tuple(weight.shape), dtype=torch.float32, device=g.device)
        db = torch.empty((co,), dtype=torch.float32, device=g.device)
        N.dcall(g, "sd_convg_wgrad_ndhwc_device", _p(g), co, _p(x), ci, B, D, H, W, *k3, *s3, *p3, *O3, _p(dw), _p(db))
        dx = None
        if ctx.needs_input_grad[0]:
            wt = weight.detach().permute(2, 3, 4, 0, 1).contiguous()          # [kz][ky][kx][c_out][c_in]
            dx = torch.empty_like(x)
            N.dcall(g, "sd_convg_dgrad_ndhwc_device", _p(g), co, _p(wt), ci, B, D, H, W, *k3, *s3, *p3, *O3, _p(dx))
        return dx, dw, db, None, None, None, None, None


class MaxPool3(torch.autograd.Function):
    """Keras MaxPooling3D(pool) on (B, D, H, W, C); the adjoint routes to the first maximum of each window (scan order z, y, x)"""

    @staticmethod
    def forward(ctx, x, pz, py, px):
        B, D, H, W, C = (int(v) for v in x.shape)
        out = torch.empty((B, D // pz, H // py, W // px, C), dtype=torch.float32, device=x.device)
        if out.numel():
            for b in range(B):
                N.dcall(x, "sd_maxpool_ndhwc_device", _p(x[b]), C, D, H, W, pz, py, px, _p(out[b]))
        ctx.save_for_backward(x)
        ctx.pool = (pz, py, px)
        return out

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        g = g.contiguous()
        B, D, H, W, C = (int(v) for v in x.shape)
        gin = torch.empty_like(x)
        N.dcall(x, "sd_maxpool3d_adjoint_ndhwc_device", _p(x), _p(g), C, B, D, H, W, *ctx.pool, _p(gin))
        return gin, None, None, None


def _kind(act):
    return 0 if isinstance(act, torch.nn.Identity) else (1 if isinstance(act, torch.nn.ReLU) else -1)


def _conv_layer(conv, kind, src0, src1=None, up0=0, res=None):
    """one stride-1 convolution of the network with its activation: 3x3x3 on Conv3x3x3, any other ('same') kernel on ConvG"""
    if kind not in (0, 1):
        raise NotImplementedError("activation of layer %s" % (conv,))
    k3 = tuple(int(k) for k in conv.kernel_size)
    if k3 == (3, 3, 3) and tuple(conv.stride) == (1, 1, 1):
        return Conv3x3x3.apply(src0, src1, conv.weight, conv.bias, res, up0, kind == 1)
    if src1 is not None or up0 or res is not None or tuple(conv.stride) != (1, 1, 1):
        raise NotImplementedError("layer %s" % (conv,))
    p3 = tuple(int(p) for p in conv.padding)
    O3 = tuple(int(n) + 2 * p - k + 1 for n, p, k in zip(src0.shape[1:4], p3, k3))
    return ConvG.apply(src0, conv.weight, conv.bias, k3, (1, 1, 1), p3, O3, kind == 1)


def _convact(m, src0, src1=None, up0=0):
    conv, bn, kind = m.parts()
    if bn is not None:
        raise NotImplementedError("layer %s with batch norm" % (m,))
    return _conv_layer(conv, kind, src0, src1, up0)


def _resnet_block(blk, x):
    """csbdeep resnet_block (model3d.py:400-422): strided first convolution (TensorFlow 'same'), body, projection, Add + activation"""
    from .models.unet import tf_same_pad_before
    stages = blk._stages()
    if any(bn is not None for _, bn, _ in stages):
        raise NotImplementedError("resnet_block with batch norm")
    S3 = tuple(int(v) for v in x.shape[1:4])
    s3 = tuple(int(p) for p in blk.pool)
    O3 = tuple(-(-n // s) for n, s in zip(S3, s3))
    conv, _, act = stages[0]
    if s3 == (1, 1, 1):
        y = _conv_layer(conv, _kind(act), x)                            # stride 1: TF 'same' is the symmetric padding
    else:
        k3 = tuple(int(k) for k in conv.kernel_size)
        p3 = tuple(tf_same_pad_before(n, k, s) for n, k, s in zip(S3, k3, s3))
        if _kind(act) not in (0, 1):
            raise NotImplementedError("resnet_block activation %s" % type(act).__name__)
        y = ConvG.apply(x, conv.weight, conv.bias, k3, s3, p3, O3, _kind(act) == 1)
    sc = x
    if blk.proj is not None:
        sc = ConvG.apply(x, blk.proj.weight, blk.proj.bias, (1, 1, 1), s3, (0, 0, 0), O3, False)
    for conv, _, act in stages[1:]:
        if act is None:                                                   # the last convolution: + shortcut, then the block's activation
            y = _conv_layer(conv, _kind(blk.act), y, res=sc.contiguous())
        else:
            y = _conv_layer(conv, _kind(act), y)
    return y


def _up_mask(pool):
    return (1 if pool[2] == 2 else 0) | (2 if pool[1] == 2 else 0) | (4 if pool[0] == 2 else 0)


def train_loss3d(net, config, x, prob_true, dtm, metrics_out=None):
    """total loss (float64 device scalar, differentiable w.r.t. the net's parameters) of one batch and the losses (prob, dist, total) (a
    float64 device vector): the U-Net or ResNet of StarDistNet evaluated on the library's exact-f32 kernels.  x (B, D, H, W, 1),
    prob_true (B, d, h, w), dtm (B, d, h, w, n_rays + 1) float32 device tensors; metrics_out as in training.train_loss"""
    if config.backbone == "unet":
        for st in net.pre:
            for m in st["convs"]:
                x = _convact(m, x)
            x = MaxPool3.apply(x, *st.pool)
        bb = net.backbone
        skips = []
        for blk in bb.down:
            for m in blk:
                x = _convact(m, x)
            skips.append(x)
            x = MaxPool3.apply(x, *bb.pool)
        for m in bb.middle:
            x = _convact(m, x)
        for blk, skip in zip(bb.up, reversed(skips)):
            x = _convact(blk[0], x, skip, _up_mask(bb.pool))
            for m in blk[1:]:
                x = _convact(m, x)
    else:
        from .models.unet import ResNetBlock
        for m in net.backbone:
            x = _resnet_block(m, x) if isinstance(m, ResNetBlock) else _convact(m, x)
    feat = _convact(net.features, x)
    w = torch.cat([net.prob.weight, net.dist.weight], 0)
    b = torch.cat([net.prob.bias, net.dist.bias], 0)
    B, d, h, wd, C = (int(v) for v in feat.shape)
    c = config
    args = (c.train_dist_loss == "mse", c.train_loss_weights[0], c.train_loss_weights[1], c.train_background_reg, torch.is_grad_enabled(),
            metrics_out)
    # the 1x1x1 heads and the losses are per voxel: batch and z fold into one axis
    return HeadsLoss.apply(feat.reshape(B * d, h, wd, C), w, b, prob_true.reshape(B * d, h, wd).contiguous(),
                           dtm.reshape(B * d, h, wd, -1).contiguous(), args)


# ---- the loop ------------------------------------------------------------------------------------------------------------------
def train3d(model, X, Y, validation_data, augmenter=None, seed=None, epochs=None, steps_per_epoch=None):
    """StarDist3D.train (see the module docstring); returns the History (a dict) of training.HISTORY_KEYS with one entry per epoch"""
    from .rays3d import rays_from_json
    cfg = model.config
    check_trainable3d(cfg)
    epochs, steps_per_epoch = begin_training(model, validation_data, seed, epochs, steps_per_epoch)
    rays = rays_from_json(cfg.rays_json)
    data_kwargs = dict(rays=rays, patch_size=cfg.train_patch_size, grid=cfg.grid, anisotropy=cfg.anisotropy,
                       foreground_prob=cfg.train_foreground_only, sample_ind_cache=cfg.train_sample_cache)
    n_data_val = len(validation_data[0])
    n_take = cfg.train_n_val_patches if cfg.train_n_val_patches is not None else n_data_val
    dev = model.device
    data_val = TrainData3D(validation_data[0], validation_data[1], batch_size=n_take, length=1, **data_kwargs)
    Xv, Yv = data_val.sample(0)
    bs = int(cfg.train_batch_size)
    val_batches = []
    for i in range(0, len(Xv), bs):
        xv = torch.from_numpy(np.ascontiguousarray(np.stack(Xv[i:i + bs])[..., None], np.float32)).to(dev)
        val_batches.append((xv,) + targets_device3d(Yv[i:i + bs], rays, cfg.grid, cfg.anisotropy, dev) + (len(Xv[i:i + bs]),))
    model.data_train = data_train = TrainData3D(X, Y, batch_size=bs, augmenter=augmenter, length=epochs * steps_per_epoch, **data_kwargs)
    return fit(model, data_train, val_batches, train_loss3d, epochs, steps_per_epoch)
