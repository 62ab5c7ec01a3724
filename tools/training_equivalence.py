"""Do two checkouts train to the same numbers?  Three seeded short trainings on synthetic discs / balls (2D U-Net, 3D U-Net, 3D ResNet):
  python tools/training_equivalence.py dump OUT.npz          every list of the returned History and every saved weight array
  python tools/training_equivalence.py compare A.npz B.npz   prints {item: identical} as JSON; exit status 1 if any item differs
The comparison is np.array_equal: the training kernels use no atomics, so one launch sequence gives one result."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "unet2d": dict(n_rays=32, grid=(2, 2), train_patch_size=(128, 128), train_batch_size=2),
    "unet3d": dict(backbone="unet", n_rays=16, grid=(1, 2, 2), anisotropy=(2, 1, 1), unet_n_depth=2, unet_n_filter_base=32,
                   net_conv_after_unet=32, train_patch_size=(16, 32, 32), train_batch_size=2),
    "resnet3d": dict(backbone="resnet", n_rays=16, grid=(1, 2, 2), anisotropy=(2, 1, 1), resnet_n_blocks=2, resnet_n_filter_base=32,
                     resnet_n_conv_per_block=3, net_conv_after_resnet=64, train_patch_size=(16, 32, 32), train_batch_size=2),
}
EPOCHS, STEPS = 3, 4


def dump(out):
    import tempfile
    import torch
    from stardist_amd.models import Config2D, Config3D, StarDist2D, StarDist3D
    from time_training import balls, discs
    res = {}
    for name, kw in CONFIGS.items():
        if name == "unet2d":
            model = StarDist2D(Config2D(**kw), basedir=None, device=torch.device("cuda:0"), seed=0)
            X, Y = zip(*[discs(160, 16, 100 + i) for i in range(6)])
        else:
            model = StarDist3D(Config3D(**kw), basedir=None, device=torch.device("cuda:0"), seed=0)
            X, Y = zip(*[balls((24, 40, 40), 12, 100 + i) for i in range(5)])
        hist = model.train(list(X[2:]), list(Y[2:]), validation_data=(list(X[:2]), list(Y[:2])), seed=0, epochs=EPOCHS, steps_per_epoch=STEPS)
        for k, v in hist.items():
            res["%s/history/%s" % (name, k)] = np.asarray(v, np.float64)
        with tempfile.TemporaryDirectory() as tmp:
            model.save_weights_npz(os.path.join(tmp, "w.npz"))
            with np.load(os.path.join(tmp, "w.npz")) as w:
                for k in w.files:
                    res["%s/weights/%s" % (name, k)] = w[k]
    np.savez(out, **res)
    print("wrote %d arrays to %s" % (len(res), out))


def compare(a, b):
    with np.load(a) as A, np.load(b) as B:
        same = {k: bool(k in B.files and np.array_equal(A[k], B[k])) for k in A.files}
        same.update({k: False for k in B.files if k not in A.files})
    print(json.dumps(same, indent=1))
    return all(same.values())


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
    else:
        sys.exit(__doc__)
