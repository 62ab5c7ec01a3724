"""StarDist3D training on the library's own kernels (the reference's StarDist3D.train, stardist/models/model3d.py:450-560, with the
losses of stardist/models/base.py:34-60, 315-325 and the data generator StarDistData3D, model3d.py:30-127): what
has no 2D counterpart.  The 3x3x3 layer, the max-pool, the U-Net walk, the heads and losses, the loop and the common scope checks are
those of training.py on five-axis tensors.

  patches      TrainData3D: StarDistData3D's patch part on the 2D generator's restatement (training.TrainData2D: sample_patches,
               get_valid_inds, StarDistDataBase.get_valid_inds with foreground_prob, the max-filter and sample_ind_cache, csbdeep's
               RollingSequence.batch / choice): the same np.random draws in the same order, so np.random.seed(s) gives the reference's
               patches.  The augmenter runs on the host, or, a stardist_amd.augment.Compose, on the device (training.py).
  targets      one upload of the batch's label patches; prob = edt_prob(lbl, anisotropy) of the FULL patch, sub-sampled by the grid
               afterwards (model3d.py:86-88, unlike 2D), by sd_edt_prob_device; dist = star_dist3D with the grid on the labels read as
               uint16 (sd_star_dist3d_device): equal to stardist_targets(..., rays=, grid=, anisotropy=) bit for bit.
  forward      the exact-f32 kernels of inference over the parameters of the model's StarDistNet, one sample at a time:
               sd_conv3_ndhwc_device (kz = 3, two sources, up bit 4 = z; with the residual epilogue sd_conv3_res_ndhwc_device for the
               last convolution of a ResNet block), sd_convg_ndhwc_device for the 7x7x7 stem, the strided first convolution of a block
               and its strided 1x1x1 projection (TensorFlow 'same' padding), sd_maxpool_ndhwc_device; the 1x1x1 heads and the losses
               are training.HeadsLoss with the batch and z folded into one axis.
  backward     csrc/train3d.hip: weight / bias gradients of 3x3x3 and of general (strided, 7x7x7, 1x1x1) convolutions, the data gradient
               of strided convolutions, the max-pool and up-sampling adjoints; the data gradient of a stride-1 3x3x3 layer is the
               forward kernel on the flipped, transposed kernel; ReLU adjoints by sd_relu_mask_device (a ResNet block's Add + ReLU: one
               mask on the block output, the result feeds both branches).
  loss         sd_stardist_loss2d_device with n_pix = B * d * h * w (the 3D model uses the same losses and metrics; in train3d()
               sd_stardist_loss2d_metrics_device, the metrics per voxel).
  optimiser    training.Adam / ReduceLROnPlateau, the epoch loop and checkpoints of training.fit (training.run_training).
  classes      a model with n_classes: training.class_targets_device on the volume patches (d = the zoom along z as well) and the class
               head / class loss of training.heads_loss, with the batch and z folded; see training.py.
Scope: check_trainable3d() names the first setting outside it."""

import numpy as np
import torch

from .lib import _native as N
from .training import (TrainData2D, _conv_layer, _convact, _device_labels, _finish_targets, _multiple_of_32, _p, _packed, _relu_or_linear,
                       _upload_labels, check_scope, class_targets_device, heads_loss, run_training, unet_forward)


# ---- data ----------------------------------------------------------------------------------------------------------------------
class TrainData3D(TrainData2D):
    """StarDistData3D (one channel) on top of csbdeep's RollingSequence: sample(i) is what its __getitem__(i) draws (volume
    and label patches after the augmenter), batch_device(i) adds the targets, computed on the device"""
    _nd = 3

    def __init__(self, X, Y, batch_size, rays, length, patch_size=(128, 128, 128), grid=(1, 1, 1), anisotropy=None, augmenter=None,
                 foreground_prob=0, sample_ind_cache=True, maxfilter_patch_size=None, n_classes=None, classes=None):
        super().__init__(X, Y, batch_size, len(rays), length, patch_size=patch_size, grid=grid, augmenter=augmenter,
                         foreground_prob=foreground_prob, sample_ind_cache=sample_ind_cache, maxfilter_patch_size=maxfilter_patch_size,
                         n_classes=n_classes, classes=classes)
        self.rays, self.anisotropy = rays, anisotropy

    def batch_device(self, i, device):
        """x (B, D, H, W, 1), prob_true (B, d, h, w), dist_true_mask (B, d, h, w, n_rays + 1): float32 device tensors; with n_classes
        also prob_class_true (B, d, h, w, n_classes + 1)"""
        x, Y = self.patches(i, device)
        return (x[..., None],) + targets_device3d(Y, self.rays, self.grid, self.anisotropy, device, self.batch_classes(i))


def targets_device3d(Y, rays, grid, anisotropy, device, classes=None):
    """the targets of StarDistData3D.__getitem__ (model3d.py:66-127) for the label volumes Y (one shape; host arrays, or one int32 device
    tensor (B, Z, H, W) as in training.targets_device) from ONE upload: prob_true
    (B, d, h, w) (-1 where the sub-sampled label is negative) and dist_true_mask (B, d, h, w, n_rays + 1) on `device`; with classes =
    (training.ClassTables, the volumes' indices into them) also prob_class_true (B, d, h, w, n_classes + 1)"""
    from .utils import edt_prob
    gz, gy, gx = (int(g) for g in grid)
    if torch.is_tensor(Y):
        ranges, neg, d_lab, d_u16 = _device_labels(Y, grid, False)
    else:
        lab, neg, d_lab, d_u16 = _upload_labels(Y, grid, device)
        ranges = [(int(v.min()), int(v.max())) if v.size else (0, 0) for v in lab]
    B, Z, H, W = (int(n) for n in d_lab.shape)
    R = len(rays)
    rz, ry, rx = (torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(device) for v in np.asarray(rays.vertices).T)
    samp = (1.0, 1.0, 1.0) if anisotropy is None else tuple(float(a) for a in anisotropy)
    d, h, w = (Z - 1) // gz + 1, (H - 1) // gy + 1, (W - 1) // gx + 1
    prob = torch.empty((B, d, h, w), dtype=torch.float32, device=device)
    dist = torch.empty((B, d, h, w, R), dtype=torch.float32, device=device)
    full = torch.empty((Z, H, W), dtype=torch.float32, device=device)
    for b in range(B):
        lo, hi = ranges[b]
        if (lo == hi and lo > 0) or hi > 4 * Z * H * W + 1024:
            pf = edt_prob(d_lab[b], anisotropy=anisotropy)      # the special cases of edt_prob (constant volume, sparse huge ids)
        else:
            N.dcall(d_lab, "sd_edt_prob_device", _p(d_lab[b]), Z, H, W, samp[0], samp[1], samp[2], max(hi, 0), _p(full))
            pf = full
        prob[b] = pf[::gz, ::gy, ::gx]
        N.dcall(d_u16, "sd_star_dist3d_device", _p(d_u16[b]), Z, H, W, _p(rz), _p(ry), _p(rx), R, gz, gy, gx, _p(dist[b]))
    if classes is None:
        return _finish_targets(prob, dist, neg)
    return _finish_targets(prob, dist, neg) + (class_targets_device(d_lab, neg, grid, *classes),)


# ---- scope ---------------------------------------------------------------------------------------------------------------------
def check_trainable3d(config, classes="auto"):
    """raise NotImplementedError naming the first setting outside the scope of the native 3D training; classes: train()'s argument"""
    c = config
    no = check_scope(c, 3, ("unet", "resnet"), classes)
    if c.backbone == "resnet":
        if getattr(c, "resnet_batch_norm", False):
            no("resnet_batch_norm = True")
        if tuple(c.resnet_kernel_size) != (3, 3, 3):
            no("resnet_kernel_size = %s (3x3x3 only)" % (tuple(c.resnet_kernel_size),))
        _multiple_of_32(c, "resnet_n_filter_base", no)
        if c.resnet_n_conv_per_block < 2:
            no("resnet_n_conv_per_block = %d (at least 2)" % c.resnet_n_conv_per_block)
        # the blocks' strides as StarDistNet builds them (model3d.py:418-422): the filter count doubles with every strided block
        pooled, n_filter = np.ones(3, int), c.resnet_n_filter_base
        for _ in range(c.resnet_n_blocks):
            pool = 1 + (np.asarray([int(g) for g in c.grid]) > pooled)
            pooled = pooled * pool
            n_filter *= 2 if (pool > 1).any() else 1
        if n_filter > 512:
            no("resnet_n_filter_base with %d strided blocks = %d channels (at most 512 per layer)" % (int(np.log2(n_filter // c.resnet_n_filter_base)), n_filter))
        _multiple_of_32(c, "net_conv_after_resnet", no)
        _relu_or_linear(c, "resnet_activation", no)


# ---- layers --------------------------------------------------------------------------------------------------------------------
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


def _kind(act):
    return 0 if isinstance(act, torch.nn.Identity) else (1 if isinstance(act, torch.nn.ReLU) else -1)


def _same_conv(m, x):
    """a stride-1 'same' convolution of the ResNet outside its blocks: 3x3x3 on the common layer, any other kernel (the 7x7x7 stem) on
    ConvG"""
    conv, bn, kind = m.parts()
    k3 = tuple(int(k) for k in conv.kernel_size)
    if k3 == (3, 3, 3):
        return _convact(m, x)
    if bn is not None or kind not in (0, 1) or tuple(conv.stride) != (1, 1, 1):
        raise NotImplementedError("layer %s" % (m,))
    p3 = tuple(int(p) for p in conv.padding)
    O3 = tuple(int(n) + 2 * p - k + 1 for n, p, k in zip(x.shape[1:4], p3, k3))
    return ConvG.apply(x, conv.weight, conv.bias, k3, (1, 1, 1), p3, O3, kind == 1)


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


def train_loss3d(net, config, x, prob_true, dtm, metrics_out=None, prob_class_true=None):
    """total loss (float64 device scalar, differentiable w.r.t. the net's parameters) of one batch and the losses (prob, dist, total) (a
    float64 device vector): the U-Net or ResNet of StarDistNet evaluated on the library's exact-f32 kernels.  x (B, D, H, W, 1),
    prob_true (B, d, h, w), dtm (B, d, h, w, n_rays + 1) float32 device tensors; metrics_out and, for a multi-class model,
    prob_class_true (B, d, h, w, n_classes + 1) as in training.train_loss"""
    if config.backbone == "unet":
        x = unet_forward(net, x)
    else:
        from .models.unet import ResNetBlock
        for m in net.backbone:
            x = _resnet_block(m, x) if isinstance(m, ResNetBlock) else _same_conv(m, x)
    return heads_loss(net, config, x, prob_true, dtm, metrics_out, prob_class_true)


# ---- the loop ------------------------------------------------------------------------------------------------------------------
def train3d(model, X, Y, validation_data, classes="auto", augmenter=None, seed=None, epochs=None, steps_per_epoch=None):
    """StarDist3D.train (see the module docstring); returns the History (a dict) of training.HISTORY_KEYS (a multi-class model:
    HISTORY_KEYS_MULTICLASS) with one entry per epoch"""
    def data(cfg):
        from .rays3d import rays_from_json
        rays = rays_from_json(cfg.rays_json)
        return TrainData3D, dict(rays=rays, anisotropy=cfg.anisotropy), \
            lambda Y, dev, cls=None: targets_device3d(Y, rays, cfg.grid, cfg.anisotropy, dev, cls)
    return run_training(model, X, Y, validation_data, augmenter, seed, epochs, steps_per_epoch, check_trainable3d, data, train_loss3d, classes)
