"""Writes tests/golden/label_edit_reference.npz: scikit-image's skimage.segmentation.find_boundaries and clear_border and
skimage.morphology.remove_small_objects on the cases of tests/_label_edit_cases.py, with the inputs they were given, so that
tests/test_cpu_label_edit.py can tell a drifted case generator from a wrong result.  Needs scikit-image (0.18.3 wrote the committed
file):

    python tests/golden/make_label_edit_golden.py

Data only: keys "fb/<case>/img", "fb/<case>/c<connectivity>_<mode>_b<background>" (bool) and "fb/<case>/subpixel"; "cb/<case>/img",
"cb/<case>/mask" (where the case has one), "cb/<case>/out"; "rs/<case>/img", "rs/<case>/out"."""
import os
import sys
import warnings

import numpy as np
from skimage.morphology import remove_small_objects
from skimage.segmentation import clear_border, find_boundaries

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _label_edit_cases as C  # noqa: E402

RS_SKIPPED = ("blobs_huge_ids",)                    # scikit-image's np.bincount would need a table of 10^11 entries

out = {}
for name, img in C.FB.items():
    out["fb/%s/img" % name] = img
    for c, mode, background in C.fb_params(img):
        got = find_boundaries(img, connectivity=c, mode=mode, background=background)
        assert got.dtype == np.bool_ and got.shape == img.shape
        out["fb/%s/c%d_%s_b%d" % (name, c, mode, background)] = got
    out["fb/%s/subpixel" % name] = find_boundaries(img, mode="subpixel")
for name, (img, kw) in C.CB.items():
    out["cb/%s/img" % name] = img
    if "mask" in kw:
        out["cb/%s/mask" % name] = kw["mask"]
    got = clear_border(img, **kw)
    assert got.dtype == img.dtype and got.shape == img.shape
    out["cb/%s/out" % name] = got
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    for name, (img, kw) in C.RS.items():
        if name in RS_SKIPPED:
            continue
        out["rs/%s/img" % name] = img
        got = remove_small_objects(img, **kw)
        assert got.dtype == img.dtype and got.shape == img.shape
        out["rs/%s/out" % name] = got
np.savez_compressed(os.path.join(HERE, "label_edit_reference.npz"), **out)
print("wrote", len(out), "arrays")
