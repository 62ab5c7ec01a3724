"""Golden vectors for stardist_amd.spots.peak_local_max from scikit-image's skimage.feature.peak_local_max, on the inputs where
scikit-image is well defined: no two equal values anywhere (so no plateau, no unstable order), and for the label cases objects
with disjoint bounding boxes, a non-negative image and no border exclusion.

The default interpreter of the build image has no scikit-image; an Anaconda python that has it ships in the same image:

    /opt/conda/bin/python3.9 tests/golden/make_peaks_golden.py        # scikit-image 0.18.3

Only numpy inputs and outputs are stored, in tests/golden/peaks_reference.npz: the images, a JSON list of the cases (image, keywords,
how to compare) and scikit-image's coordinates per case."""
import json
import os

import numpy as np
import scipy.ndimage as ndi
import skimage
from skimage.feature import peak_local_max

HERE = os.path.dirname(os.path.abspath(__file__))
rng = np.random.RandomState(1)
out = {"skimage_version": np.array(skimage.__version__)}
cases = []


def tie_free(shape):
    a = ndi.gaussian_filter(rng.standard_normal(shape), 1.5)
    rank = np.argsort(np.argsort(a.ravel())).reshape(shape)
    img = (1 + rank * 0.001).astype(np.float32)
    assert len(np.unique(img)) == img.size
    return img


def add(image, compare, labels=None, **kw):
    more = dict(kw)
    if labels is not None:
        more["labels"] = out[labels]
    if more.get("num_peaks_per_label") is None:
        more.pop("num_peaks_per_label", None)
    want = peak_local_max(out[image].copy(), **more)
    out["coords_%d" % len(cases)] = np.asarray(want, np.int64).reshape(-1, out[image].ndim)
    cases.append({"image": image, "labels": labels, "compare": compare, "keywords": kw})


for k, shape in enumerate(((23, 31), (40, 17), (7, 9, 11))):
    out["image_%d" % k] = tie_free(shape)
    for d in (1, 2, 3):
        for kw in ({}, {"exclude_border": False}, {"threshold_rel": 0.6}, {"num_peaks": 5}, {"exclude_border": 2 if len(shape) == 2 else 1},
                   {"exclude_border": (2, 1) if len(shape) == 2 else (1, 0, 2)}):
            add("image_%d" % k, "order", min_distance=d, **kw)

# unsigned: scikit-image 0.18.3 sorts -intensities of the unsigned image, so its order is not by value; the set is
out["image_u16"] = (1 + rng.permutation(12 * 13)).astype(np.uint16).reshape(12, 13)
add("image_u16", "set", min_distance=1)
add("image_u16", "set", min_distance=2, exclude_border=False)

# labels: disjoint boxes, positive image, no border
out["image_l"] = tie_free((40, 50))
lab = np.zeros((40, 50), np.int64)
lab[2:12, 3:20], lab[15:30, 5:15], lab[14:38, 25:48], lab[20:25, 30:35] = 1, 2, 3, 0
out["labels_l"] = lab
for d in (1, 2):
    for k in (None, 2):
        add("image_l", "set", labels="labels_l", min_distance=d, exclude_border=False, num_peaks_per_label=k)

out["cases"] = np.array(json.dumps(cases))
np.savez_compressed(os.path.join(HERE, "peaks_reference.npz"), **out)
print(len(cases), "cases,", sum(len(out["coords_%d" % i]) for i in range(len(cases))), "peaks")
