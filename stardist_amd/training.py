"""Training on the library's own kernels: StarDist2D.train (the reference's stardist/models/model2d.py train, with the losses of
stardist/models/base.py:34-60, 315-325 and the data generator StarDistData2D without shape completion), and everything StarDist3D.train
(training3d.py) shares with it.  The layers, the U-Net walk, the loop and the scope checks are written once for images (B, H, W, C) and
volumes (B, D, H, W, C): an image is the D = 1, kz = 1 case of the same native calls.

  patches      sample_patches / get_valid_inds (stardist/sample_patches.py), StarDistDataBase.get_valid_inds (base.py:129-224) and
               csbdeep's RollingSequence.batch / utils.choice, restated with the same np.random draws in the same order: np.random.seed(s)
               gives the reference's patches.  A plain augmenter callable runs on the host, as there; a stardist_amd.augment.Compose
               runs on the device when the batch goes there: the host draws its parameters where it would have called it (the same
               np.random stream), the raw patches go up, one launch augments the batch and the targets start from the device labels.
  targets      one upload of the batch's label patches; prob (edt_prob of the grid-subsampled labels) and dist (star_dist with the grid) on
               the device by sd_edt_prob_device / sd_star_dist2d_device: equal to stardist_targets() bit for bit.
  forward      the exact-f32 kernels of inference (sd_conv3_ndhwc_device per sample; sd_maxpool_ndhwc_device, for images with the batch
               on the depth axis; the 1x1 heads on sd_convg_ndhwc_device with every axis before (h, w) on the depth axis) over the
               parameters of the model's StarDistNet; inference itself (StarDistBase._net_forward) is not involved.
  backward     weight / bias gradients by sd_conv_wgrad_ndhwc_device (3x3, and the heads) or sd_conv3_wgrad_ndhwc_device (3x3x3): two
               partitions of the same sum, each for its shapes; the ReLU adjoint (csrc/train2d.hip); the max-pool and up-sampling
               adjoints (sd_maxpool3d_adjoint_ndhwc_device, sd_upcat3d_adjoint_ndhwc_device of csrc/train3d.hip, D = 1 for images);
               the data gradient of a 3x3 / 3x3x3 layer is the forward kernel on the flipped, transposed kernel.
  loss         sd_stardist_loss2d_device: both losses and their gradients in one call; in train(), sd_stardist_loss2d_metrics_device,
               which adds the reference's Keras metrics (kld, relevant_mae, relevant_mse, dist_iou_metric) in the same passes.
  optimiser    Keras' Adam (epsilon 1e-7) and ReduceLROnPlateau on val_loss, as torch element-wise updates.
  classes      a model with n_classes (train(..., classes=...), the reference's _parse_classes_arg): ClassTables (per image the table
               label id -> class code) and sd_class_targets_device give prob_class on the device in one launch per batch, equal to the
               reference's mask_to_categorical + scipy.ndimage.zoom(..., 1 / grid, order=0) + negative-label mask; the class head
               (features_class on the common layer, the 1x1 prob_class in ClassHeadLoss) and sd_class_loss_device, the weighted
               categorical cross entropy and its gradient on the logits.  The total is w0 prob + w1 dist + w2 prob_class; the history
               gains prob_class_loss / val_prob_class_loss.  A single-class model runs what it ran before.
Scope (2D): U-Net backbone, one input channel, no batch norm / dropout, 'mae' / 'mse' distance loss, no shape completion, classes given
for a model of several classes; check_trainable() names the first setting outside it (the settings common to every backbone first, then
the U-Net's)."""
import ctypes
import math
import random
import threading
import warnings

import numpy as np
import torch

from .lib import _native as N


# ---- patch sampling ------------------------------------------------------------------------------------------------------------
def choice(population, k=1, replace=True):
    """csbdeep.utils.choice: python's `random`, seeded from np.random (one draw), its own state restored afterwards"""
    state = random.getstate()
    try:
        random.seed(np.random.randint(np.iinfo(int).min, np.iinfo(int).max))
        return random.choices(population, k=k) if replace else random.sample(population, k=k)
    finally:
        random.setstate(state)


def sample_patches(datas, patch_size, n_samples, valid_inds=None):
    """stardist/sample_patches.py sample_patches: n_samples patches of every array in `datas` at the same random centres"""
    if len(patch_size) != datas[0].ndim:
        raise ValueError()
    if not all(a.shape == datas[0].shape for a in datas):
        raise ValueError("all input shapes must be the same: %s" % (" / ".join(str(a.shape) for a in datas)))
    if not all(0 < s <= d for s, d in zip(patch_size, datas[0].shape)):
        raise ValueError("patch_size %s negative or larger than data shape %s along some dimensions" % (str(patch_size), str(datas[0].shape)))
    if valid_inds is None:
        valid_inds = tuple(_s.ravel() for _s in np.meshgrid(*tuple(np.arange(p // 2, s - p // 2 + 1) for s, p in zip(datas[0].shape, patch_size))))
    n_valid = len(valid_inds[0])
    if n_valid == 0:
        raise ValueError("no regions to sample from!")
    idx = choice(range(n_valid), n_samples, replace=(n_valid < n_samples))
    rand_inds = [v[idx] for v in valid_inds]
    return [np.stack([data[tuple(slice(_r - (_p // 2), _r + _p - (_p // 2)) for _r, _p in zip(r, patch_size))] for r in zip(*rand_inds)])
            for data in datas]


def get_valid_inds(img, patch_size, patch_filter=None):
    """stardist/sample_patches.py get_valid_inds: the centres of patches inside the image (and inside patch_filter's mask)"""
    if len(patch_size) != img.ndim:
        raise ValueError()
    if not all(0 < s <= d for s, d in zip(patch_size, img.shape)):
        raise ValueError("patch_size %s negative or larger than image shape %s along some dimensions" % (str(patch_size), str(img.shape)))
    if patch_filter is None:
        valid_inds = tuple(np.arange(p // 2, s - p + p // 2 + 1).astype(np.uint32) for p, s in zip(patch_size, img.shape))
        return tuple(s.ravel() for s in np.meshgrid(*valid_inds, indexing="ij"))
    patch_mask = patch_filter(img, patch_size)
    border_slices = tuple(slice(p // 2, s - p + p // 2 + 1) for p, s in zip(patch_size, img.shape))
    valid_inds = np.where(patch_mask[border_slices])
    return tuple((v + s.start).astype(np.uint32) for s, v in zip(border_slices, valid_inds))


def grid_divisible_patch_size(patch_size, grid):
    """stardist/utils.py grid_divisible_patch_size"""
    patch_size, grid = tuple(patch_size), tuple(grid)
    div = tuple(int(np.ceil(sh / g) * g) for sh, g in zip(patch_size, grid))
    if div != patch_size:
        warnings.warn("increasing patch_size from %s to %s, since it was not evenly divisible by grid %s" % (patch_size, div, grid))
    return div


class TrainData2D(object):
    """StarDistData2D (shape_completion=False) on top of csbdeep's RollingSequence: sample(i) is what its __getitem__(i) draws (image and
    label patches after the augmenter), batch_device(i) adds the targets, computed on the device"""
    _nd = 2

    def __init__(self, X, Y, batch_size, n_rays, length, patch_size=(256, 256), grid=(1, 1), augmenter=None, foreground_prob=0,
                 sample_ind_cache=True, maxfilter_patch_size=None, n_classes=None, classes=None):
        X = [np.asarray(x).astype(np.float32, copy=False) for x in X]
        if not (len(X) == len(Y) and len(X) > 0):
            raise ValueError("X and Y can't be empty and must have same length")
        if classes is None:
            classes = (None,) * len(X)          # every object ignored by the class loss
        elif n_classes is None:
            warnings.warn("Ignoring classes since n_classes is None")
        if len(classes) != len(X):
            raise ValueError("X and classes must have same length")
        self.n_classes, self.classes = n_classes, classes
        self.class_tables = ClassTables(classes, n_classes) if n_classes is not None else None
        self.data_size, self.batch_size = len(X), int(batch_size)
        self.length = 2 ** 63 - 1 if length is None else int(length)
        self.index_map = {}
        patch_size = grid_divisible_patch_size(patch_size, grid)
        nd = self._nd
        if len(patch_size) != nd or X[0].ndim != nd:
            raise ValueError("%dD images with one channel (no channel axis) expected" % nd)
        Y = [np.asarray(y) for y in Y]
        if not all(y.ndim == nd and x.ndim == nd and x.shape == y.shape for x, y in zip(X, Y)):
            raise ValueError("images and masks should have corresponding shapes/dimensions")
        if not all(x.shape >= tuple(patch_size) for x in X):
            raise ValueError("Some images are too small for given patch_size {patch_size}".format(patch_size=patch_size))
        if not 0 <= foreground_prob <= 1:
            raise ValueError("foreground_prob must lie in [0, 1]")
        if augmenter is None:
            augmenter = lambda *args: args
        if not callable(augmenter):
            raise ValueError("augmenter must be None or callable")
        self.X, self.Y, self.n_rays, self.grid = X, Y, int(n_rays), tuple(int(g) for g in grid)
        self.patch_size, self.augmenter, self.foreground_prob = patch_size, augmenter, foreground_prob
        self.maxfilter_patch_size = maxfilter_patch_size if maxfilter_patch_size is not None else self.patch_size
        self.sample_ind_cache = sample_ind_cache
        self._ind_cache_fg, self._ind_cache_all = {}, {}
        self.lock = threading.Lock()

    def __len__(self):
        return self.length

    # csbdeep RollingSequence
    def _index(self, loop):
        if loop not in self.index_map:
            self.index_map[loop] = np.random.permutation(self.data_size)
        return self.index_map[loop]

    def batch(self, i):
        pos = i * self.batch_size
        loop, pos_loop = pos // self.data_size, pos % self.data_size
        sl = slice(pos_loop, pos_loop + self.batch_size)
        index = self._index(loop)
        _loop = loop
        while sl.stop > len(index):
            _loop += 1
            index = np.concatenate((index, self._index(_loop)))
        return index[sl]

    def max_filter(self, y, patch_size):
        from scipy.ndimage import maximum_filter
        return maximum_filter(y, patch_size, mode="constant")

    # StarDistDataBase.get_valid_inds
    def get_valid_inds(self, k, foreground_prob=None):
        if foreground_prob is None:
            foreground_prob = self.foreground_prob
        foreground_only = np.random.uniform() < foreground_prob
        _ind_cache = self._ind_cache_fg if foreground_only else self._ind_cache_all
        if k in _ind_cache:
            inds = _ind_cache[k]
        else:
            patch_filter = (lambda y, p: self.max_filter(y, self.maxfilter_patch_size) > 0) if foreground_only else None
            inds = get_valid_inds(self.Y[k], self.patch_size, patch_filter=patch_filter)
            if self.sample_ind_cache:
                with self.lock:
                    _ind_cache[k] = inds
        if foreground_only and len(inds[0]) == 0:
            return self.get_valid_inds(k, foreground_prob=0)
        return inds

    def sample(self, i, draw_only=False):
        """(X, Y): the batch's image and label patches (tuples of 2D arrays) after the augmenter.  draw_only (an augmenter with draw()):
        (X, Y, params) with the raw patches and, drawn where the augmenter would have been called, each sample's parameters"""
        idx = self.batch(i)
        arrays = [sample_patches((self.Y[k], self.X[k]), patch_size=self.patch_size, n_samples=1, valid_inds=self.get_valid_inds(k)) for k in idx]
        X, Y = list(zip(*[(x[0], y[0]) for y, x in arrays]))
        if draw_only:
            return X, Y, [self.augmenter.draw(_x.shape) for _x in X]
        X, Y = tuple(zip(*tuple(self.augmenter(_x, _y) for _x, _y in zip(X, Y))))
        return X, Y

    def augments_on(self, device):
        """whether batches for `device` take the device route: an augmenter with draw() and apply_device(), and a HIP device"""
        return hasattr(self.augmenter, "draw") and hasattr(self.augmenter, "apply_device") and torch.device(device).type == "cuda"

    def patches(self, i, device):
        """(x, labels) of batch i: x float32 (B, *patch) on `device`; labels the augmented label patches, as a tuple of host arrays
        (the augmenter ran on the host) or, on the device route, as one int32 tensor (B, *patch) on the device"""
        if not self.augments_on(device):
            X, Y = self.sample(i)
            return torch.from_numpy(np.ascontiguousarray(np.stack(X), np.float32)).to(device, non_blocking=False), Y
        X, Y, params = self.sample(i, draw_only=True)
        lab = np.stack(Y)
        if lab.dtype.kind not in "iub" or lab.dtype.itemsize > 4 or lab.dtype == np.uint32:
            if lab.size and (int(lab.max()) >= 2 ** 31 or int(lab.min()) < -2 ** 31):
                raise ValueError("label ids must fit int32")
        x = torch.from_numpy(np.ascontiguousarray(np.stack(X), np.float32)).to(device, non_blocking=False)
        y = torch.from_numpy(np.ascontiguousarray(lab, np.int32)).to(device)
        return self.augmenter.apply_device(x, y, params)

    def batch_classes(self, i):
        """what the targets functions take as `classes` for batch i: (the class tables, the batch's image indices), or None for a
        single-class model.  Draws no random numbers: the permutation of batch(i) is the one sample(i) made."""
        return None if self.class_tables is None else (self.class_tables, self.batch(i))

    def batch_device(self, i, device):
        """x (B, H, W, 1), prob_true (B, h, w), dist_true_mask (B, h, w, n_rays + 1): float32 device tensors; with n_classes also
        prob_class_true (B, h, w, n_classes + 1)"""
        x, Y = self.patches(i, device)
        return (x[..., None],) + targets_device(Y, self.n_rays, self.grid, device, self.batch_classes(i))


def _upload_labels(Y, grid, device):
    """the start of both targets functions for the label arrays Y (one shape): (lab, neg, d_lab, d_u16) = the stacked labels on the
    host with negative ids clipped to 0, the masks of negative labels on the grid (None if there are none), ONE int32 upload of lab
    and its 2-byte copy (star_dist reads the labels as unsigned short: the reference's geom2d / geom3d cast with astype(np.uint16))"""
    Y = [np.asarray(y) for y in Y]
    on_grid = tuple(slice(None, None, int(g)) for g in grid)
    neg = [y[on_grid] < 0 for y in Y]
    if any(m.any() for m in neg):
        Y = [np.maximum(y, 0) for y in Y]
    else:
        neg = None
    lab = np.stack(Y)
    if lab.size and int(lab.max()) >= 2 ** 31:
        raise ValueError("label ids must fit int32")
    d_lab = torch.from_numpy(np.ascontiguousarray(lab, np.int32)).to(device)
    return lab, neg, d_lab, d_lab.to(torch.uint16).contiguous()


def _finish_targets(prob, dist, neg):
    """the end of both: (prob_true, dist_true_mask) from the device tensors prob and dist, prob_true = -1 where the label is negative"""
    dtm = torch.cat([dist, prob[..., None]], dim=-1).contiguous()
    if neg is not None:
        prob[neg if torch.is_tensor(neg) else torch.from_numpy(np.stack(neg)).to(prob.device)] = -1
    return prob, dtm


def _device_labels(d_raw, grid, on_grid):
    """_upload_labels for label patches that are on the device already (int32 (B, *patch), after a device augmenter): (ranges, neg,
    d_lab, d_u16) with the same clip (every sample, if any label ON THE GRID is negative), neg the mask of negative labels on the grid
    as a device tensor (None if there are none) and ranges the (min, max) per sample of what the host route looks at -- the clipped
    labels on the grid (on_grid, 2D) or of the whole patch (3D) -- from ONE read-back of 4 numbers per sample"""
    B = int(d_raw.shape[0])
    sub = d_raw[(slice(None),) + tuple(slice(None, None, int(g)) for g in grid)]
    lo_s, hi_s = torch.aminmax(sub.reshape(B, -1), dim=1)
    lo_f, hi_f = (lo_s, hi_s) if all(int(g) == 1 for g in grid) else torch.aminmax(d_raw.reshape(B, -1), dim=1)
    st = torch.stack([lo_s, hi_s, lo_f, hi_f], dim=1).cpu().numpy()
    lo, hi = (st[:, 0], st[:, 1]) if on_grid else (st[:, 2], st[:, 3])
    neg, d_lab = None, d_raw.contiguous()
    if (st[:, 0] < 0).any():
        neg, d_lab = sub < 0, d_lab.clamp_min(0)
        lo, hi = np.maximum(lo, 0), np.maximum(hi, 0)
    return [(int(a), int(b)) for a, b in zip(lo, hi)], neg, d_lab, d_lab.to(torch.uint16).contiguous()


def targets_device(Y, n_rays, grid, device, classes=None):
    """the targets of StarDistData2D.__getitem__ (model2d.py:63-119, shape_completion=False) for the label images Y (one shape; host
    arrays, or one int32 tensor (B, H, W) on the device, which is then not uploaded but asked for its ranges) from ONE
    upload: prob_true (B, h, w) (-1 where the label is negative) and dist_true_mask (B, h, w, n_rays + 1) on `device`; with classes =
    (ClassTables, the images' indices into them) also prob_class_true (B, h, w, n_classes + 1)"""
    from .utils import edt_prob
    gy, gx = int(grid[0]), int(grid[1])
    if torch.is_tensor(Y):
        ranges, neg, d_lab, d_u16 = _device_labels(Y, grid, True)
    else:
        lab, neg, d_lab, d_u16 = _upload_labels(Y, grid, device)
        ranges = [(int(sub.min()), int(sub.max())) if sub.size else (0, 0) for sub in (lab[b, ::gy, ::gx] for b in range(len(lab)))]
    B, H, W = (int(n) for n in d_lab.shape)
    d_sub = d_lab[:, ::gy, ::gx].contiguous()
    h, w = int(d_sub.shape[1]), int(d_sub.shape[2])
    prob = torch.empty((B, h, w), dtype=torch.float32, device=device)
    dist = torch.empty((B, h, w, n_rays), dtype=torch.float32, device=device)
    for b in range(B):
        lo, hi = ranges[b]
        if (lo == hi and lo > 0) or hi > 4 * h * w + 1024:
            prob[b] = edt_prob(d_sub[b])           # the special cases of edt_prob (constant image, sparse huge ids)
        else:
            N.dcall(d_sub, "sd_edt_prob_device", _p(d_sub[b]), 1, h, w, 1.0, 1.0, 1.0, max(hi, 0), _p(prob[b]))
        N.dcall(d_u16, "sd_star_dist2d_device", _p(d_u16[b]), H, W, int(n_rays), gy, gx, _p(dist[b]))
    if classes is None:
        return _finish_targets(prob, dist, neg)
    return _finish_targets(prob, dist, neg) + (class_targets_device(d_lab, neg, grid, *classes),)


# ---- class targets ---------------------------------------------------------------------------------------------------------------
CODE_IGNORE, CODE_MISSING = -1, -2            # the codes of sd_class_targets_device beside the class ids 0 ... n_classes
MISSING_LABEL_MESSAGE = "all gt labels should be present in class dict provided"


class ClassTables(object):
    """The `classes` of a data set (per image a dict label id -> class id, one integer, or None) as the tables sd_class_targets_device
    reads: per image (offset, entries, form, default code) and the codes (with the sorted label ids for form 1) of all images in one
    array, uploaded once per device.  A dict is a dense table over 0 ... max id where that is small, sorted ids otherwise (the split
    targets_device makes for edt_prob); an integer or None is the default code of a table that holds label 0 alone.  A class id outside
    0 ... n_classes raises here (mask_to_categorical's ValueError); a label that a dict does not hold is found on the device: the kernel
    raises the flag that check() reads."""

    def __init__(self, classes, n_classes):
        if not (np.issubdtype(type(n_classes), np.integer) and n_classes >= 1):
            raise ValueError("n_classes is '%s' but should be a positive integer" % (n_classes,))
        self.n_classes = int(n_classes)
        code = self._code
        meta, keys, codes, off = [], [], [], 0
        for cls in classes:
            if cls is None or np.issubdtype(type(cls), np.integer):
                k, c, form, dflt = np.zeros(1, np.int32), np.zeros(1, np.int32), 0, code(cls)
            elif isinstance(cls, dict):
                items = {int(k): code(v) for k, v in cls.items() if 0 <= k < 2 ** 31}
                items.setdefault(0, 0)            # background pixels are in no class unless the dict says so
                hi = max(items)
                if hi > 4 * len(items) + 1024:
                    k = np.array(sorted(items), np.int32)
                    c, form = np.array([items[i] for i in k.tolist()], np.int32), 1
                else:
                    k, c, form = np.zeros(hi + 1, np.int32), np.full(hi + 1, CODE_MISSING, np.int32), 0
                    c[list(items)] = list(items.values())
                dflt = CODE_MISSING
            else:
                raise ValueError("classes should be dict, single scalar, or None!")
            meta.append((off, len(c), form, dflt))
            keys.append(k)
            codes.append(c)
            off += len(c)
        if off >= 2 ** 31:
            raise ValueError("class tables too large")
        self.meta = np.array(meta, np.int32).reshape(-1, 4)
        self._host = (np.concatenate(keys), np.concatenate(codes))
        self._dev = {}

    def _code(self, cls):
        if cls is None:
            return CODE_IGNORE
        if np.issubdtype(type(cls), np.integer) and 0 <= cls <= self.n_classes:
            return int(cls)
        raise ValueError("Wrong class id '%s' (for n_classes=%s)" % (cls, self.n_classes))

    def device(self, device):
        """(keys, codes, flag) on `device`: the int32 tables and the int32 flag the kernel raises for a missing label"""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(a).to(device) for a in self._host) + (torch.zeros(1, dtype=torch.int32, device=device),)
        return self._dev[key]

    def check(self, flag_value=None):
        """raise the reference's ValueError if a batch since the last check held a label that its image's dict does not; flag_value:
        the flag as already read by the caller (one device only), None: read here (a host synchronisation)"""
        raised = bool(flag_value) if flag_value is not None else any(bool(int(d[2].item())) for d in self._dev.values())
        if raised:
            for d in self._dev.values():
                d[2].zero_()
            raise ValueError(MISSING_LABEL_MESSAGE)


_zoom_dev = {}


def _zoom_table_device(n, g, device):
    key = (int(n), int(g), str(device))
    if key not in _zoom_dev:
        from .utils import nearest_zoom_table
        _zoom_dev[key] = torch.from_numpy(np.array(nearest_zoom_table(n, g))).to(device)
    return _zoom_dev[key]


def class_targets_device(d_lab, neg, grid, tables, idx):
    """prob_class of StarDistData2D / StarDistData3D.__getitem__ (model2d.py:106-119, model3d.py:107-127) in one launch: d_lab the
    batch's int32 label patches on the device (B, [D,] H, W) and neg the negative-label masks on the grid (or None), both as
    _upload_labels returns them; tables the ClassTables of the data set, idx the batch's image indices.  mask_to_categorical per pixel,
    the reference's scipy.ndimage.zoom(..., 1 / grid, order=0) as one gather table per axis (utils.nearest_zoom_table: not [::g], and
    rows that scipy reads from outside the patch are 0 in every channel), then -1 at negative labels.  Returns float32
    (B, [d,] h, w, n_classes + 1).  A label missing from its dict raises the tables' flag (ClassTables.check), not an error here."""
    device = d_lab.device
    nd = d_lab.ndim - 1
    B, (D, H, W) = int(d_lab.shape[0]), _dhw(d_lab.shape[1:])
    tabs = [_zoom_table_device(n, g, device) for n, g in zip(_dhw(d_lab.shape[1:]), _dhw_grid(grid))]
    d, h, w = (int(t.numel()) for t in tabs)
    C = tables.n_classes + 1
    d_neg = None
    if neg is not None:
        d_neg = neg.contiguous() if torch.is_tensor(neg) else torch.from_numpy(np.ascontiguousarray(np.stack(neg))).to(device)
        if tuple(d_neg.shape) != (B,) + (d, h, w)[3 - nd:]:
            raise ValueError("the patch size must be divisible by the grid")
    meta = np.ascontiguousarray(tables.meta[np.asarray(idx, np.int64)])
    if len(meta) != B:
        raise ValueError("one image index per label patch expected")
    d_keys, d_codes, flag = tables.device(device)
    d_meta = torch.from_numpy(meta).to(device)
    out = torch.empty((B,) + (d, h, w)[3 - nd:] + (C,), dtype=torch.float32, device=device)
    N.dcall(d_lab, "sd_class_targets_device", _p(d_lab), B, D, H, W, _p(d_meta), _p(d_keys), _p(d_codes), *(_p(t) for t in tabs), d, h, w,
            _p(d_neg), C, _p(out), _p(flag))
    return out


# ---- scope ---------------------------------------------------------------------------------------------------------------------
def _multiple_of_32(c, key, no, wording="a positive multiple of 32 only"):
    v = getattr(c, key)
    if v % 32 != 0 or v <= 0:
        no("%s = %d (%s)" % (key, v, wording))


def _relu_or_linear(c, key, no):
    if getattr(c, key) not in ("relu", "linear", None):
        no("%s = %r (relu or linear only)" % (key, getattr(c, key)))


def check_scope(config, nd, backbones, classes="auto"):
    """the checks of check_trainable (nd = 2) and check_trainable3d (nd = 3): raise NotImplementedError naming the first setting outside
    the scope of the native training -- the settings common to every backbone, then those of the U-Net.  classes: the argument of
    train(); a model of several classes needs them given.  Returns the function that raises, for the checks of another backbone."""
    c = config

    def no(what):
        raise NotImplementedError("StarDist%dD.train on the native kernels does not support %s" % (nd, what))
    if getattr(c, "n_dim", nd) != nd:
        no("n_dim = %s (%dD only)" % (c.n_dim, nd))
    if c.backbone not in backbones:
        no("backbone = %r (%s only)" % (c.backbone, "U-Net" if backbones == ("unet",) else " or ".join(backbones)))
    if c.n_classes is not None and c.n_classes > 1 and isinstance(classes, str) and classes == "auto":
        no("n_classes = %r without classes (using classes = 'auto' for n_classes > 1 not supported)" % (c.n_classes,))
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
        if tuple(c.unet_kernel_size) != (3,) * nd:
            no("unet_kernel_size = %s (%s only)" % (tuple(c.unet_kernel_size), "x".join("3" * nd)))
        # (the wording of the 2D message is older than the 3D one's)
        _multiple_of_32(c, "unet_n_filter_base", no, *(("a multiple of 32 only",) if nd == 2 else ()))
        if c.unet_n_filter_base * 2 ** c.unet_n_depth > 512:
            no("unet_n_filter_base * 2**unet_n_depth = %d (at most 512 channels per layer)" % (c.unet_n_filter_base * 2 ** c.unet_n_depth))
        if not all(p in (1, 2) for p in c.unet_pool):
            no("unet_pool = %s (1 or 2 per axis)" % (tuple(c.unet_pool),))
        _multiple_of_32(c, "net_conv_after_unet", no)
        _relu_or_linear(c, "unet_activation", no)
        _relu_or_linear(c, "unet_last_activation", no)
    return no


def check_trainable(config, classes="auto"):
    """raise NotImplementedError naming the first setting outside the scope of the native training; classes: train()'s argument"""
    check_scope(config, 2, ("unet",), classes)


# ---- layers: tensors (B, H, W, C) or (B, D, H, W, C), float32; without a depth axis D = 1 and kz = 1 ----------------------------------
_perm_cache = {}


def _pack_perm(kind, ci, co, k3, device):
    """the packing of sd_conv3_pack_weights_host (kind 'conv3', kz = k3[0]) / sd_convg_pack_weights_host ('convg', kernel k3) as a gather
    on the device: (index into [0, w.flatten()...], mask of the weight positions, the weight-independent rest of the packed array --
    the small-channel form of the general kernel appends a tap table)"""
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
                n = int(L.sd_conv3_packed_floats(ci, co, k3[0]))
                if n < 0:
                    raise ValueError("sd_conv3: unsupported layer %d -> %d" % (ci, co))
                out = np.zeros(n, np.float32)
                N.check(L.sd_conv3_pack_weights_host(N.ptr(src), ci, co, k3[0], N.ptr(out)))
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
    """packed device form of the kernel w (co, ci, [kz,] ky, kx)"""
    co, ci = int(w.shape[0]), int(w.shape[1])
    idx, is_w, rest = _pack_perm(kind, ci, co, _dhw(w.shape[2:]), w.device)
    flat = torch.cat([w.new_zeros(1), w.reshape(-1)])
    return torch.where(is_w, flat.index_select(0, idx), rest).contiguous()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dhw_grid(grid):
    """the grid of two or three axes as (gz, gy, gx), gz = 1 when there is no depth axis"""
    return (1,) * (3 - len(grid)) + tuple(int(g) for g in grid)


def _dhw(extents):
    """the two or three extents as (D, H, W) integers, D = 1 when there is no depth axis"""
    return (1,) * (3 - len(extents)) + tuple(int(v) for v in extents)


def _conv3_fwd(src0, src1, wp, bias, up0, co, relu, res=None):
    """the convolution on the forward kernel, one call per sample; up0: src0 is read through the up-sampling bits (1 x, 2 y, 4 z)"""
    nd = src0.ndim - 2
    B, (D, H, W) = int(src0.shape[0]), (n << ((up0 >> i) & 1) for n, i in zip(_dhw(src0.shape[1:-1]), (2, 1, 0)))
    c0, c1 = int(src0.shape[-1]), (int(src1.shape[-1]) if src1 is not None else 0)
    out = torch.empty((B,) + (D, H, W)[3 - nd:] + (co,), dtype=torch.float32, device=src0.device)
    for b in range(B):
        args = [_p(src0[b]), c0, c0, up0, _p(src1[b]) if src1 is not None else None, c1, c1, 0, D, H, W, 3 if nd == 3 else 1, _p(wp), _p(bias)]
        if res is None:
            N.dcall(src0, "sd_conv3_ndhwc_device", *args, co, int(relu), _p(out[b]))
        else:
            N.dcall(src0, "sd_conv3_res_ndhwc_device", *args, _p(res[b]), co, co, int(relu), _p(out[b]))
    return out


class Conv3(torch.autograd.Function):
    """act(conv3([UpSampling(src0) | src1]) + bias (+ res)) for a 3x3 or 3x3x3 kernel (by the rank of the weight); up0: the forward
    kernels' bit mask for src0 (1 x, 2 y, 4 z); res: the residual of a ResNet block's Add, added before the activation (or None)"""

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
        B, co, (D, H, W) = int(y.shape[0]), int(y.shape[-1]), _dhw(y.shape[1:-1])
        c0, c1 = int(src0.shape[-1]), (int(src1.shape[-1]) if src1 is not None else 0)
        if ctx.relu:
            g = torch.empty_like(gy)
            N.dcall(gy, "sd_relu_mask_device", _p(gy), _p(y), gy.numel(), _p(g))
        else:
            g = gy
        dw = torch.empty(tuple(weight.shape), dtype=torch.float32, device=g.device)         # (the torch layout, dense)
        db = torch.empty((co,), dtype=torch.float32, device=g.device)
        # two partitions of the same sum, each for its shapes: the LDS-tiled kernel for images, taps spread over waves for volumes
        if weight.ndim == 4:
            N.dcall(g, "sd_conv_wgrad_ndhwc_device", _p(g), co, _p(src0), c0, ctx.up0, _p(src1), c1, 0, B, H, W, 3, _p(dw), _p(db))
        else:
            N.dcall(g, "sd_conv3_wgrad_ndhwc_device", _p(g), co, _p(src0), c0, ctx.up0, _p(src1), c1, 0, B, D, H, W, _p(dw), _p(db))
        d0 = d1 = None
        if ctx.needs_input_grad[0] or (src1 is not None and ctx.needs_input_grad[1]):
            # 'same' convolution of g with the flipped, transposed kernel = d(concatenated input)
            wt = weight.detach().flip(*range(2, weight.ndim)).transpose(0, 1).contiguous()
            dcat = _conv3_fwd(g, None, _packed(wt, "conv3"), None, 0, c0 + c1, False)
            if ctx.up0 or src1 is not None:
                d0 = torch.empty_like(src0)
                d1 = torch.empty_like(src1) if src1 is not None else None
                N.dcall(dcat, "sd_upcat3d_adjoint_ndhwc_device", _p(dcat), c0, ctx.up0, c1, B, D, H, W, _p(d0), _p(d1))
            else:
                d0 = dcat
        return d0, d1, dw, db, (g if ctx.has_res else None), None, None


class MaxPool(torch.autograd.Function):
    """Keras MaxPooling2D / MaxPooling3D(pool) on (B, H, W, C) / (B, D, H, W, C); the adjoint routes to the first maximum of each
    window (scan order z, y, x)"""

    @staticmethod
    def forward(ctx, x, *pool):
        C = int(x.shape[-1])
        pz, py, px = _dhw(pool)
        out = torch.empty((x.shape[0],) + tuple(int(n) // p for n, p in zip(x.shape[1:-1], pool)) + (C,), dtype=torch.float32, device=x.device)
        if out.numel():
            # images: the whole batch in one call, the batch on the depth axis (pz = 1); volumes: one call per sample
            for xb, ob in ([(x, out)] if x.ndim == 4 else zip(x, out)):
                N.dcall(x, "sd_maxpool_ndhwc_device", _p(xb), C, *(int(v) for v in xb.shape[:3]), pz, py, px, _p(ob))
        ctx.save_for_backward(x)
        ctx.pool = (pz, py, px)
        return out

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        g = g.contiguous()
        gin = torch.empty_like(x)
        N.dcall(x, "sd_maxpool3d_adjoint_ndhwc_device", _p(x), _p(g), int(x.shape[-1]), int(x.shape[0]), *_dhw(x.shape[1:-1]), *ctx.pool, _p(gin))
        return (gin,) + (None,) * (x.ndim - 2)


class HeadsLoss(torch.autograd.Function):
    """prob = sigmoid(Conv1x1(feat)), dist = Conv1x1(feat) (one 1 + n_rays channel convolution) and the loss of the batch against
    (prob_true, dist_true_mask): returns the total loss (float64 scalar) and, not differentiable, the losses (prob, dist, total).
    loss_args = (mse, w_prob, w_dist, reg, want_grad, metrics_out): a float64 device tensor of 4 as metrics_out receives the batch's
    metrics (kld, relevant_mae, relevant_mse, dist_iou_metric) from the same kernel passes; None: the losses alone"""

    @staticmethod
    def forward(ctx, feat, w_heads, b_heads, prob_true, dtm, loss_args):
        B, H, W, C = (int(v) for v in feat.shape)
        co = int(w_heads.shape[0])
        R = co - 1
        wp = _packed(w_heads.detach(), "convg")
        logits = torch.empty((B, H, W, co), dtype=torch.float32, device=feat.device)
        N.dcall(feat, "sd_convg_ndhwc_device", _p(feat), C, C, B, H, W, 1, 1, 1, 1, 1, 1, 0, 0, 0, B, H, W, _p(wp), _p(b_heads.detach()),
                None, 0, co, 0, _p(logits), co)
        prob = torch.sigmoid(logits[..., 0]).contiguous()
        dist = logits[..., 1:].contiguous()
        losses = torch.empty(3, dtype=torch.float64, device=feat.device)
        mse, w_prob, w_dist, reg, want_grad, metrics_out = loss_args
        # without autograd (validation) the kernel evaluates the losses only
        gz = torch.empty_like(prob) if want_grad else None
        gd = torch.empty_like(dist) if want_grad else None
        args = (_p(prob), _p(dist), _p(prob_true), _p(dtm), B * H * W, R, int(mse), float(w_prob), float(w_dist), float(reg), _p(losses), _p(gz),
                _p(gd))
        if metrics_out is None:
            N.dcall(prob, "sd_stardist_loss2d_device", *args)
        else:
            if not (metrics_out.dtype == torch.float64 and metrics_out.device == feat.device and metrics_out.numel() == 4
                    and metrics_out.is_contiguous()):
                raise ValueError("metrics_out: a contiguous float64 tensor of 4 on the device of the batch")
            N.dcall(prob, "sd_stardist_loss2d_metrics_device", *args, _p(metrics_out))
        ctx.save_for_backward(feat, w_heads, gz, gd)
        ctx.mark_non_differentiable(losses)
        return losses[2].clone(), losses

    @staticmethod
    def backward(ctx, gl, _):
        feat, w_heads, gz, gd = ctx.saved_tensors
        B, H, W, C = (int(v) for v in feat.shape)
        co = int(w_heads.shape[0])
        g = (torch.cat([gz[..., None], gd], dim=-1) * gl.to(torch.float32)).contiguous()
        dw = torch.empty(tuple(w_heads.shape), dtype=torch.float32, device=g.device)
        db = torch.empty((co,), dtype=torch.float32, device=g.device)
        N.dcall(g, "sd_conv_wgrad_ndhwc_device", _p(g), co, _p(feat), C, 0, None, 0, 0, B, H, W, 1, _p(dw), _p(db))
        wt = _packed(w_heads.detach().transpose(0, 1).contiguous(), "convg")
        dfeat = torch.empty_like(feat)
        N.dcall(g, "sd_convg_ndhwc_device", _p(g), co, co, B, H, W, 1, 1, 1, 1, 1, 1, 0, 0, 0, B, H, W, _p(wt), None, None, 0, C, 0, _p(dfeat), C)
        return dfeat, dw, db, None, None, None


class ClassHeadLoss(torch.autograd.Function):
    """logits = Conv1x1(feat) of the class head and the weighted categorical cross entropy of softmax(logits) against prob_class_true
    (sd_class_loss_device: the softmax is never written): returns w_class * loss (float64 scalar) and, not differentiable, (loss,
    w_class * loss).  class_weights: n_classes + 1 doubles on the device; want_grad False (validation): the loss only."""

    @staticmethod
    def forward(ctx, feat, weight, bias, target, class_weights, w_class, want_grad):
        B, H, W, C = (int(v) for v in feat.shape)
        co = int(weight.shape[0])
        if tuple(target.shape) != (B, H, W, co) or class_weights.numel() != co or class_weights.dtype != torch.float64:
            raise ValueError("prob_class_true %s for logits %s and %d float64 class weights expected"
                             % (tuple(target.shape), (B, H, W, co), co))
        wp = _packed(weight.detach(), "convg")
        logits = torch.empty((B, H, W, co), dtype=torch.float32, device=feat.device)
        N.dcall(feat, "sd_convg_ndhwc_device", _p(feat), C, C, B, H, W, 1, 1, 1, 1, 1, 1, 0, 0, 0, B, H, W, _p(wp), _p(bias.detach()),
                None, 0, co, 0, _p(logits), co)
        losses = torch.empty(2, dtype=torch.float64, device=feat.device)
        gz = torch.empty_like(logits) if want_grad else None
        N.dcall(feat, "sd_class_loss_device", _p(logits), _p(target), _p(class_weights), B * H * W, co, float(w_class), _p(losses), _p(gz))
        ctx.save_for_backward(feat, weight, gz)
        ctx.mark_non_differentiable(losses)
        return losses[1].clone(), losses

    @staticmethod
    def backward(ctx, gl, _):
        feat, weight, gz = ctx.saved_tensors
        B, H, W, C = (int(v) for v in feat.shape)
        co = int(weight.shape[0])
        g = (gz * gl.to(torch.float32)).contiguous()
        dw = torch.empty(tuple(weight.shape), dtype=torch.float32, device=g.device)
        db = torch.empty((co,), dtype=torch.float32, device=g.device)
        N.dcall(g, "sd_conv_wgrad_ndhwc_device", _p(g), co, _p(feat), C, 0, None, 0, 0, B, H, W, 1, _p(dw), _p(db))
        wt = _packed(weight.detach().transpose(0, 1).contiguous(), "convg")
        dfeat = torch.empty_like(feat)
        N.dcall(g, "sd_convg_ndhwc_device", _p(g), co, co, B, H, W, 1, 1, 1, 1, 1, 1, 0, 0, 0, B, H, W, _p(wt), None, None, 0, C, 0, _p(dfeat), C)
        return dfeat, dw, db, None, None, None, None


def _conv_layer(conv, kind, src0, src1=None, up0=0, res=None):
    """one stride-1 3x3 / 3x3x3 convolution of the network with its activation (kind 0 linear, 1 relu)"""
    if kind not in (0, 1):
        raise NotImplementedError("activation of layer %s" % (conv,))
    if any(int(k) != 3 for k in conv.kernel_size) or any(int(v) != 1 for v in conv.stride):
        raise NotImplementedError("layer %s" % (conv,))
    return Conv3.apply(src0, src1, conv.weight, conv.bias, res, up0, kind == 1)


def _convact(m, src0, src1=None, up0=0):
    conv, bn, kind = m.parts()
    if bn is not None:
        raise NotImplementedError("layer %s with batch norm" % (m,))
    return _conv_layer(conv, kind, src0, src1, up0)


def _up_mask(pool):
    """the forward kernels' up-sampling bits (1 x, 2 y, 4 z) of UpSampling(pool)"""
    return sum(bit for p, bit in zip(reversed(pool), (1, 2, 4)) if p == 2)


def unet_forward(net, x):
    """the U-Net of StarDistNet (the grid stem net.pre, the down levels, the middle, the up levels on their skips) on the layers above"""
    for st in net.pre:
        for m in st["convs"]:
            x = _convact(m, x)
        x = MaxPool.apply(x, *st.pool)
    bb = net.backbone
    skips = []
    for blk in bb.down:
        for m in blk:
            x = _convact(m, x)
        skips.append(x)
        x = MaxPool.apply(x, *bb.pool)
    for m in bb.middle:
        x = _convact(m, x)
    for blk, skip in zip(bb.up, reversed(skips)):
        x = _convact(blk[0], x, skip, _up_mask(bb.pool))
        for m in blk[1:]:
            x = _convact(m, x)
    return x


_class_weights = {}


def class_weights_device(config, device):
    """train_class_weights as float64 on the device (cached)"""
    key = (tuple(float(v) for v in config.train_class_weights), str(device))
    if key not in _class_weights:
        _class_weights[key] = torch.tensor(key[0], dtype=torch.float64, device=device)
    return _class_weights[key]


def heads_loss(net, config, x, prob_true, dtm, metrics_out, prob_class_true=None):
    """the feature convolution, the two heads as one 1x1 convolution and the losses on the backbone's output x: what train_loss
    returns.  The heads and the losses are per pixel: every axis before the last two spatial ones folds into one.  A multi-class net
    takes prob_class_true: its class head (features_class, a layer like features on x, and the 1x1 prob_class) and class loss follow,
    the total gains train_loss_weights[2] times the class loss and the losses become (prob, dist, total, prob_class)."""
    if (net.n_classes is None) != (prob_class_true is None):
        raise ValueError("prob_class_true is what a multi-class model takes, and only such a model")
    feat = _convact(net.features, x)
    w = torch.cat([net.prob.weight, net.dist.weight], 0)
    b = torch.cat([net.prob.bias, net.dist.bias], 0)
    h, wd, C = (int(v) for v in feat.shape[-3:])
    c = config
    args = (c.train_dist_loss == "mse", c.train_loss_weights[0], c.train_loss_weights[1], c.train_background_reg, torch.is_grad_enabled(),
            metrics_out)
    total, losses = HeadsLoss.apply(feat.reshape(-1, h, wd, C), w, b, prob_true.reshape(-1, h, wd).contiguous(),
                                    dtm.reshape(-1, h, wd, dtm.shape[-1]).contiguous(), args)
    if prob_class_true is None:
        return total, losses
    fc = _convact(net.features_class, x)
    K = int(prob_class_true.shape[-1])
    cls_total, cls = ClassHeadLoss.apply(fc.reshape(-1, h, wd, int(fc.shape[-1])), net.prob_class.weight, net.prob_class.bias,
                                         prob_class_true.reshape(-1, h, wd, K).contiguous(), class_weights_device(c, x.device),
                                         c.train_loss_weights[2], torch.is_grad_enabled())
    total = total + cls_total
    return total, torch.cat([losses[:2], total.detach()[None], cls[:1]])


def train_loss(net, config, x, prob_true, dtm, metrics_out=None, prob_class_true=None):
    """total loss (float64 device scalar, differentiable w.r.t. the net's parameters) of one batch and the losses (prob, dist, total) (a
    float64 device vector): the network of StarDistNet evaluated on the library's exact-f32 kernels.  x (B, H, W, 1), prob_true (B, h, w),
    dtm (B, h, w, n_rays + 1) float32 device tensors.  metrics_out (a float64 device tensor of 4, optional) receives the batch's
    metrics (kld, relevant_mae, relevant_mse, dist_iou_metric).  A multi-class model takes prob_class_true (B, h, w, n_classes + 1) as
    well: the total includes the class loss, which is appended to the losses: (prob, dist, total, prob_class)"""
    return heads_loss(net, config, unet_forward(net, x), prob_true, dtm, metrics_out, prob_class_true)


# ---- optimiser -----------------------------------------------------------------------------------------------------------------
class Adam(object):
    """Keras' Adam (beta_1 0.9, beta_2 0.999, epsilon 1e-7): lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), p -= lr_t m / (sqrt(v) + eps)"""

    def __init__(self, params, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
        self.params = list(params)
        self.lr, self.b1, self.b2, self.eps = float(lr), beta_1, beta_2, epsilon
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        self.t = 0

    @torch.no_grad()
    def step(self):
        self.t += 1
        lr_t = self.lr * math.sqrt(1 - self.b2 ** self.t) / (1 - self.b1 ** self.t)
        grads = [p.grad for p in self.params]
        torch._foreach_mul_(self.m, self.b1)
        torch._foreach_add_(self.m, grads, alpha=1 - self.b1)
        torch._foreach_mul_(self.v, self.b2)
        torch._foreach_addcmul_(self.v, grads, grads, value=1 - self.b2)
        denom = torch._foreach_sqrt(self.v)
        torch._foreach_add_(denom, self.eps)
        torch._foreach_addcdiv_(self.params, self.m, denom, value=-lr_t)


class ReduceLROnPlateau(object):
    """Keras' ReduceLROnPlateau on val_loss (mode min)"""

    def __init__(self, factor=0.1, patience=10, min_delta=1e-4, cooldown=0, min_lr=0, verbose=0, monitor="val_loss", mode="auto", **kw):
        if factor >= 1.0:
            raise ValueError("ReduceLROnPlateau does not support a factor >= 1.0.")
        if monitor != "val_loss" or mode not in ("auto", "min"):
            raise NotImplementedError("ReduceLROnPlateau: only monitor='val_loss', mode 'auto' / 'min'")
        self.factor, self.patience, self.min_delta, self.cooldown, self.min_lr, self.verbose = factor, patience, min_delta, cooldown, min_lr, verbose
        self.best, self.wait, self.cooldown_counter = np.inf, 0, 0

    def on_epoch_end(self, epoch, current, opt):
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.wait = 0
        if current < self.best - self.min_delta:
            self.best, self.wait = current, 0
        elif not self.cooldown_counter > 0:
            self.wait += 1
            if self.wait >= self.patience:
                old = float(np.float32(opt.lr))
                if old > np.float32(self.min_lr):
                    opt.lr = max(old * self.factor, self.min_lr)
                    if self.verbose:
                        print("\nEpoch %05d: ReduceLROnPlateau reducing learning rate to %s." % (epoch + 1, opt.lr))
                    self.cooldown_counter, self.wait = self.cooldown, 0


# ---- the loop ------------------------------------------------------------------------------------------------------------------
LOSS_NAMES = ("loss", "prob_loss", "dist_loss")
METRIC_NAMES = ("prob_kld", "dist_relevant_mae", "dist_relevant_mse", "dist_dist_iou_metric")
HISTORY_KEYS = LOSS_NAMES + METRIC_NAMES + tuple("val_" + k for k in LOSS_NAMES + METRIC_NAMES) + ("lr",)
# a multi-class model: Keras adds the third output's loss (the reference registers no metric for it)
_NAMES_MULTICLASS = LOSS_NAMES + ("prob_class_loss",) + METRIC_NAMES
HISTORY_KEYS_MULTICLASS = _NAMES_MULTICLASS + tuple("val_" + k for k in _NAMES_MULTICLASS) + ("lr",)


class History(dict):
    """what Keras' Model.fit returns, as the dict of its per-epoch values: hist["val_loss"] and hist.history["val_loss"] are the same
    list; .epoch the epoch indices, .params {verbose, epochs, steps}; multiclass: with prob_class_loss / val_prob_class_loss"""

    def __init__(self, epochs, steps, multiclass=False):
        super(History, self).__init__((k, []) for k in (HISTORY_KEYS_MULTICLASS if multiclass else HISTORY_KEYS))
        self.epoch = []
        self.params = {"verbose": 1, "epochs": int(epochs), "steps": int(steps)}

    @property
    def history(self):
        return self


def keras_epoch_metrics(values, n_pix):
    """the epoch values of the four metrics from their per-batch values (n_batches, 4) (kld, relevant_mae, relevant_mse,
    dist_iou_metric) and the batches' pixel counts, by Keras' Mean rules: kld is one scalar per batch, so every batch counts once; the
    three distance metrics are one value per pixel, so every batch counts with its pixels.  Returns a float64 tensor of 4 (on the
    device of `values`)."""
    values = torch.as_tensor(values, dtype=torch.float64)
    w = torch.as_tensor(n_pix, dtype=torch.float64).to(values.device)
    if values.ndim != 2 or values.shape[1] != 4 or w.shape != values.shape[:1]:
        raise ValueError("values (n_batches, 4) and one pixel count per batch expected")
    kld = values[:, 0].mean()
    dist = (values[:, 1:] * w[:, None]).sum(0) / w.sum()
    return torch.cat([kld[None], dist])


def train(model, X, Y, validation_data, classes="auto", augmenter=None, seed=None, epochs=None, steps_per_epoch=None):
    """StarDist2D.train (see the module docstring); returns the History (a dict) of HISTORY_KEYS (a multi-class model:
    HISTORY_KEYS_MULTICLASS) with one entry per epoch"""
    def data(cfg):
        return TrainData2D, dict(n_rays=cfg.n_rays), lambda Y, dev, cls=None: targets_device(Y, cfg.n_rays, cfg.grid, dev, cls)
    return run_training(model, X, Y, validation_data, augmenter, seed, epochs, steps_per_epoch, check_trainable, data, train_loss, classes)


def run_training(model, X, Y, validation_data, augmenter, seed, epochs, steps_per_epoch, check, data, loss_fn, classes="auto"):
    """the body of train and train3d: check(config, classes) for the scope, begin_training, the classes parsed as the reference does, the
    validation patches drawn once and cut into batches with their targets, the training generator, fit.  data(config) gives (the
    TrainData class, its keyword arguments beyond the patch settings, targets(Y, device, classes) -> (prob_true, dist_true_mask
    [, prob_class_true])); loss_fn is train_loss or train_loss3d."""
    cfg = model.config
    check(cfg, classes)
    epochs, steps_per_epoch, validation_data = begin_training(model, validation_data, seed, epochs, steps_per_epoch)
    multiclass = cfg.n_classes is not None
    classes = model._parse_classes_arg(classes, len(X)) if multiclass else None
    Data, data_kwargs, targets = data(cfg)
    data_kwargs = dict(data_kwargs, patch_size=cfg.train_patch_size, grid=cfg.grid, foreground_prob=cfg.train_foreground_only,
                       sample_ind_cache=cfg.train_sample_cache)
    if multiclass:
        data_kwargs["n_classes"] = cfg.n_classes
    n_data_val = len(validation_data[0])
    classes_val = model._parse_classes_arg(validation_data[2], n_data_val) if multiclass else None
    n_take = cfg.train_n_val_patches if cfg.train_n_val_patches is not None else n_data_val
    dev = model.device
    data_val = Data(validation_data[0], validation_data[1], batch_size=n_take, length=1, classes=classes_val, **data_kwargs)
    Xv, Yv = data_val.sample(0)
    cls_v = data_val.batch_classes(0)
    bs = int(cfg.train_batch_size)
    val_batches = []
    for i in range(0, len(Xv), bs):
        xv = torch.from_numpy(np.ascontiguousarray(np.stack(Xv[i:i + bs])[..., None], np.float32)).to(dev)
        tg = targets(Yv[i:i + bs], dev) if cls_v is None else targets(Yv[i:i + bs], dev, (cls_v[0], cls_v[1][i:i + bs]))
        val_batches.append((xv,) + tg + (len(Xv[i:i + bs]),))
    if cls_v is not None:
        cls_v[0].check()                            # a validation label that its dict does not hold: raised once, before training starts
    model.data_train = data_train = Data(X, Y, batch_size=bs, augmenter=augmenter, length=epochs * steps_per_epoch, classes=classes,
                                         **data_kwargs)
    return fit(model, data_train, val_batches, loss_fn, epochs, steps_per_epoch)


def begin_training(model, validation_data, seed, epochs, steps_per_epoch):
    """the checks and settings both train loops start with: a HIP device, np.random.seed(seed), epochs / steps_per_epoch from the config
    when not given, validation_data a pair (a multi-class model: a pair, which gets 'auto' as its classes, or a triple),
    train_patch_size divisible by what the network needs.  Returns (epochs, steps_per_epoch, validation_data)."""
    cfg = model.config
    if model.device.type != "cuda":
        raise RuntimeError("training runs on a HIP device (the model lives on %s)" % model.device)
    N.require_device()
    if seed is not None:
        np.random.seed(seed)
    if epochs is None:
        epochs = cfg.train_epochs
    if steps_per_epoch is None:
        steps_per_epoch = cfg.train_steps_per_epoch
    if cfg.n_classes is None:
        if not isinstance(validation_data, (list, tuple)) or len(validation_data) != 2:
            raise ValueError("validation_data must be a tuple (X_val, Y_val)")
    else:
        if not isinstance(validation_data, (list, tuple)):
            raise ValueError("validation_data must be a tuple (X_val, Y_val) or (X_val, Y_val, classes_val)")
        if len(validation_data) == 2:
            validation_data = tuple(validation_data) + ("auto",)
        if len(validation_data) != 3:
            raise ValueError("len(validation_data) = %d, but should be 3" % len(validation_data))
    div_by = model._axes_div_by(cfg.axes.replace("C", ""))
    for p, d, a in zip(cfg.train_patch_size, div_by, cfg.axes.replace("C", "")):
        if p % d != 0:
            raise ValueError("'train_patch_size' must be divisible by {d} along axis '{a}'".format(a=a, d=d))
    return epochs, steps_per_epoch, validation_data


def fit(model, data_train, val_batches, loss_fn, epochs, steps_per_epoch):
    """the epoch loop of both train functions: Adam steps on loss_fn(net, config, *data_train.batch_device(step, device), metrics_out=...),
    the validation losses and metrics of val_batches [(x, prob_true, dist_true_mask, n)] after each epoch, ReduceLROnPlateau, the
    checkpoints; returns the History.  The losses are averaged as before (training: over steps; validation: weighted by images), the
    metrics by Keras' rules (keras_epoch_metrics); one host synchronisation per epoch.  A multi-class model: the batches carry
    prob_class_true after dist_true_mask, the losses are four (the class loss last), and the flag of a label missing from its class
    dict comes to the host with the epoch's values."""
    import os
    cfg, dev = model.config, model.device
    net = model.net
    params = [p for p in net.parameters()]
    was = [p.requires_grad for p in params]
    for p in params:
        p.requires_grad_(True)
    opt = Adam(params, cfg.train_learning_rate)
    rlr = ReduceLROnPlateau(**dict(cfg.train_reduce_lr)) if cfg.train_reduce_lr is not None else None
    tables = getattr(data_train, "class_tables", None)
    n_loss = 3 if tables is None else 4
    names = LOSS_NAMES + METRIC_NAMES if tables is None else _NAMES_MULTICLASS
    history = History(epochs, steps_per_epoch, multiclass=tables is not None)
    ckpt = lambda name: os.path.join(model.logdir, os.path.splitext(name)[0] + ".npz")
    best = np.inf
    net.train()
    try:
        step = 0
        for epoch in range(epochs):
            acc = torch.zeros(n_loss, dtype=torch.float64, device=dev)
            met, met_pix = torch.empty((steps_per_epoch, 4), dtype=torch.float64, device=dev), []
            for i in range(steps_per_epoch):
                x, pt, dtm, *pc = data_train.batch_device(step, dev)
                step += 1
                for p in params:
                    p.grad = None
                loss, losses = loss_fn(net, cfg, x, pt, dtm, metrics_out=met[i], **(dict(prob_class_true=pc[0]) if pc else {}))
                loss.backward()
                acc += losses
                met_pix.append(pt.numel())
                opt.step()
            with torch.no_grad():
                vacc, nv = torch.zeros(n_loss, dtype=torch.float64, device=dev), 0
                vmet, vmet_pix = torch.empty((len(val_batches), 4), dtype=torch.float64, device=dev), []
                for j, (xv, ptv, dtmv, *pcv, n) in enumerate(val_batches):
                    vacc += loss_fn(net, cfg, xv, ptv, dtmv, metrics_out=vmet[j], **(dict(prob_class_true=pcv[0]) if pcv else {}))[1] * n
                    nv += n
                    vmet_pix.append(ptv.numel())
                ep = [acc / steps_per_epoch, keras_epoch_metrics(met, met_pix), vacc / nv, keras_epoch_metrics(vmet, vmet_pix)]
                if tables is not None:
                    ep.append(tables.device(dev)[2].to(torch.float64))
                ep = torch.cat(ep).tolist()
            if tables is not None:
                tables.check(ep.pop())
            tr, va = ep[:n_loss + 4], ep[n_loss + 4:]
            # Keras reports the total loss as the weighted sum of the outputs' losses
            for k, v in zip(names, [tr[2], tr[0], tr[1]] + tr[3:]):
                history[k].append(v)
            for k, v in zip(names, [va[2], va[0], va[1]] + va[3:]):
                history["val_" + k].append(v)
            history["lr"].append(opt.lr)
            history.epoch.append(epoch)
            if model.logdir is not None:
                if cfg.train_checkpoint is not None and va[2] < best:
                    best = va[2]
                    model.save_weights_npz(ckpt(cfg.train_checkpoint))
                if cfg.train_checkpoint_epoch is not None:
                    model.save_weights_npz(ckpt(cfg.train_checkpoint_epoch))
            if rlr is not None:
                rlr.on_epoch_end(epoch, va[2], opt)
    finally:
        for p, r in zip(params, was):
            p.grad = None
            p.requires_grad_(r)
        net.eval()
        # the captured inference graphs hold the packed form of the old kernels; the range fallbacks were decided on them as well
        model.__dict__.pop("_graphs", None)
        for mod in net.modules():
            mod.__dict__.pop("_sd_force_form", None)
    # csbdeep BaseModel._training_finished: last weights saved, the best ones loaded, the per-epoch file removed
    if model.logdir is not None:
        if cfg.train_checkpoint_last is not None:
            model.save_weights_npz(ckpt(cfg.train_checkpoint_last))
        if cfg.train_checkpoint is not None and os.path.exists(ckpt(cfg.train_checkpoint)):
            model.load_weights_npz(ckpt(cfg.train_checkpoint))
        if cfg.train_checkpoint_epoch is not None and os.path.exists(ckpt(cfg.train_checkpoint_epoch)):
            os.remove(ckpt(cfg.train_checkpoint_epoch))
    return history


def reference_losses(prob, dist, prob_true, dist_true_mask, dist_loss="mae", loss_weights=(1, 0.2), background_reg=1e-4):
    """the losses of sd_stardist_loss2d_device as differentiable torch expressions (any dtype; the tests evaluate them in float64):
    prob (B, h, w) after the sigmoid, dist (B, h, w, n_rays), prob_true (B, h, w), dist_true_mask (B, h, w, n_rays + 1).
    Returns (prob_loss, dist_loss, total)."""
    eps = 1e-7
    m = prob_true >= 0
    t, p = prob_true[m], prob[m].clamp(eps, 1 - eps)
    prob_loss = (-(t * torch.log(p + eps) + (1 - t) * torch.log(1 - p + eps))).mean()
    R = dist.shape[-1]
    dt, mask = dist_true_mask[..., :R], dist_true_mask[..., R:]
    e = dt - dist
    pen = e.abs() if dist_loss == "mae" else e * e
    per_pixel = (mask * pen).mean(-1) / (mask.mean() + eps)
    if background_reg > 0:
        per_pixel = per_pixel + background_reg * ((1 - mask) * dist.abs()).mean(-1)
    d_loss = per_pixel.mean()
    return prob_loss, d_loss, loss_weights[0] * prob_loss + loss_weights[1] * d_loss


def reference_class_loss(logits, prob_class_true, class_weights, from_logits=True):
    """the loss of sd_class_loss_device as a differentiable torch expression (any dtype; the tests evaluate it in float64): the
    reference's weighted_categorical_crossentropy (base.py:108-126) restated literally on the softmax of logits (..., n_classes + 1)
    (from_logits=False: on the probabilities given), prob_class_true of the same shape (negative: ignored), one weight per channel;
    Keras' mean over every pixel, the ignored ones included."""
    eps = 1e-7
    p = torch.softmax(logits, -1) if from_logits else logits
    w = torch.as_tensor(class_weights, dtype=p.dtype, device=p.device)
    t = prob_class_true.to(p.dtype)
    mask = (t >= 0).to(p.dtype)
    q = (p / (p + eps).sum(-1, keepdim=True)).clamp(eps, 1 - eps)
    return (-(w * mask * t * torch.log(q)).sum(-1)).mean()


def reference_metrics(prob, dist, prob_true, dist_true_mask):
    """the metrics of sd_stardist_loss2d_metrics_device as torch expressions (the tests evaluate them in float64; shapes as in
    reference_losses, any number of spatial axes): the values of one batch of the reference's kld, relevant_mae, relevant_mse and
    dist_iou_metric (base.py:68-104, 335-353), Keras' mean taken over each metric's values.  Returns (kld, mae, mse, iou)."""
    eps = 1e-7
    bce = lambda t, p: -(t * torch.log(p.clamp(eps, 1 - eps) + eps) + (1 - t) * torch.log(1 - p.clamp(eps, 1 - eps) + eps))
    m = prob_true >= 0
    tc, pc = prob_true[m].clamp(eps, 1), prob[m].clamp(eps, 1)
    kld = (bce(tc, pc) - bce(tc, tc)).mean()
    R = dist.shape[-1]
    dt, mask = dist_true_mask[..., :R], dist_true_mask[..., R:]
    norm = mask.mean() + eps
    e = dt - dist
    mae = ((mask * e.abs()).mean(-1) / norm).mean()
    mse = ((mask * e * e).mean(-1) / norm).mean()
    dp = dist.clamp_min(0)
    inter = torch.minimum(dt, dp).square().mean(-1)
    union = torch.maximum(dt, dp).square().mean(-1)
    iou = ((mask[..., 0] * (inter / (union + eps))) / norm).mean()
    return kld, mae, mse, iou
