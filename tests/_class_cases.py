"""What the tests of multi-class training (test_cpu_training_classes.py, test_gpu_training_classes.py) share: the shapes and grids of the
class targets, seeded label scenes with their class dicts, and the plain numpy composition of prob_class that the device kernel is held
to.  Nothing here needs a GPU.

  SHAPES2D, SHAPES3D   (patch shape, grid): the 48-, 32- and 56-long axes are ones where scipy's nearest zoom reads past the array
  scene                label patches of one shape for a batch, with the classes of each: several objects per class, an ignored object
                       (None), a class-0 object, a block of negative labels, and in one sample an object with an id above 2**30
  compose              mask_to_categorical per patch, the gather by utils.nearest_zoom_table per axis, then -1 at negative labels"""
import numpy as np

SHAPES2D = [((48, 40), (2, 2)), ((48, 40), (1, 4)), ((64, 64), (4, 4)), ((32, 56), (2, 2))]
SHAPES3D = [((8, 24, 20), (1, 2, 2)), ((8, 24, 20), (2, 1, 4)), ((16, 32, 32), (2, 4, 4))]
BIG_ID = 2 ** 30 + 12345


def scene(shape, n_classes, seed, B=2, n_obj=9):
    """(Y, classes): B int32 label patches of `shape` and per patch the dict label id -> class id.  Objects are boxes at seeded places
    (later ones paint over earlier ones); object k has class 1 + k % n_classes, except object 2 (None: ignored) and object 3 (class 0);
    patch 0 has a block of negative labels, the last patch one object with the id BIG_ID (a sparse table) reaching the far corner, so
    that the rows scipy's zoom drops or fills are not all background."""
    rng = np.random.RandomState(seed)
    Y, classes = [], []
    for b in range(B):
        y = np.zeros(shape, np.int32)
        cls = {}
        for k in range(1, n_obj + 1):
            lo = [rng.randint(0, max(1, s - 2)) for s in shape]
            sl = tuple(slice(l, l + rng.randint(2, max(3, s // 3))) for l, s in zip(lo, shape))
            y[sl] = k
            cls[k] = None if k == 2 else (0 if k == 3 else 1 + k % n_classes)
        if b == B - 1:
            y[tuple(slice(s - max(2, s // 4), s) for s in shape)] = BIG_ID
            cls[BIG_ID] = n_classes
        if b == 0:
            y[tuple(slice(0, max(2, s // 5)) for s in shape)] = -1
        for k in range(1, n_obj + 1):                     # every object is still there: each code is exercised
            if not (y == k).any():
                y[tuple(rng.randint(0, s) for s in shape)] = k
        Y.append(y)
        classes.append(cls)
    return Y, classes


def gather(a, grid):
    """scipy.ndimage.zoom(a, 1 / grid + (1,), order=0) of the channels-last array a through the per-axis tables: rows read from
    outside the array are 0"""
    from stardist_amd.utils import nearest_zoom_table
    for axis, g in enumerate(grid):
        t = nearest_zoom_table(a.shape[axis], g)
        a = np.where((t >= 0).reshape((-1,) + (1,) * (a.ndim - 1 - axis)), np.take(a, np.maximum(t, 0), axis=axis), 0)
    return a


def compose(Y, classes, n_classes, grid):
    """prob_class of StarDistData2D / 3D.__getitem__ for the label patches Y (one shape) with their classes, float32
    (B, [d,] h, w, n_classes + 1)"""
    from stardist_amd.utils import mask_to_categorical
    on_grid = tuple(slice(None, None, int(g)) for g in grid)
    neg = np.stack([y[on_grid] < 0 for y in Y])
    out = np.stack([gather(mask_to_categorical(np.maximum(y, 0), n_classes, c), grid) for y, c in zip(Y, classes)]).astype(np.float32)
    out[neg] = -1
    return out
