"""What the GPU training tests (test_gpu_training.py, test_gpu_training3d.py, test_gpu_training_scale.py) share: the float64 restatement of
the layers' two-source input, the perturbation of a fresh network and the synthetic label images / volumes with their noisy images."""
import numpy as np
import torch

DEV = torch.device("cuda:0")


def f32(t):
    return None if t is None else t.float().to(DEV).contiguous()


def up_nearest(t, up):
    """channel-first (B, C, [d,] h, w) -> nearest up-sampling by 2 along the axes of the bit mask up (1 x, 2 y, 4 z)"""
    for axis, bit in ((-3, 4), (-2, 2), (-1, 1)):
        if up & bit:
            t = t.repeat_interleave(2, dim=axis)
    return t


def cat64(s0, s1, up):
    """[UpSampling(s0) | s1] of the channels-last s0, s1 (s1 may be None), channel-first; up: the bit mask of up_nearest"""
    first = (0, s0.ndim - 1) + tuple(range(1, s0.ndim - 1))
    x = up_nearest(s0.permute(*first), up)
    if s1 is not None:
        x = torch.cat([x, s1.permute(*first)], 1)
    return x


def randomise(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.randn(p.shape, generator=g).to(p.device) * 0.02)


def discs(shape, n, seed, rmin=4, rmax=11):
    """label image (or volume) of n discs (balls), later ones overwrite, and a noisy image of it"""
    rng = np.random.RandomState(seed)
    y = np.zeros(shape, np.int32)
    for i in range(1, n + 1):
        r = rng.randint(rmin, rmax)
        c = [rng.randint(0, s) for s in shape]
        sl = tuple(slice(max(0, ci - r), min(s, ci + r + 1)) for ci, s in zip(c, shape))
        g = np.ogrid[sl]
        m = sum((gi - ci) ** 2 for gi, ci in zip(g, c)) < r * r
        y[sl][m] = i
    x = (y > 0).astype(np.float32) + 0.1 * rng.randn(*shape).astype(np.float32)
    return x, y


def balls(shape, n, seed, rmin=3, rmax=7, aniso=(1, 1, 1)):
    """label volume of n balls (radius r / aniso per axis, later ones overwrite) and a noisy image of it"""
    rng = np.random.RandomState(seed)
    y = np.zeros(shape, np.int32)
    for i in range(1, n + 1):
        r = rng.randint(rmin, rmax)
        c = [rng.randint(0, s) for s in shape]
        rr = [max(1.0, r / a) for a in aniso]
        sl = tuple(slice(max(0, int(ci - ri)), min(s, int(ci + ri) + 1)) for ci, ri, s in zip(c, rr, shape))
        g = np.ogrid[sl]
        m = sum(((gi - ci) / ri) ** 2 for gi, ci, ri in zip(g, c, rr)) < 1
        y[sl][m] = i
    x = (y > 0).astype(np.float32) + 0.1 * rng.randn(*shape).astype(np.float32)
    return x, y
