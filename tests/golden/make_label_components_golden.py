"""Writes tests/golden/label_components_reference.npz: scikit-image's skimage.measure.label (labels and count, every connectivity) on a
selection of the cases of tests/_label_cc_cases.py, with the inputs it was given, so that tests/test_cpu_label_components.py can tell a
drifted case generator from a wrong label image.  Needs scikit-image (0.18.3 wrote the committed file):

    python tests/golden/make_label_components_golden.py

Data only: keys "<case>/img", "<case>/background", "<case>/c<connectivity>/labels" (int32; scikit-image returns int64) and ".../n"."""
import os
import sys

import numpy as np
from skimage.measure import label

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _label_cc_cases as C  # noqa: E402

SELECTION = ("spiral", "comb", "diagonals", "rings", "helix", "comb3d", "random_small_0.59", "one_row",
             "blocks_u8", "blocks_u8_background_3", "blocks_u16_high", "blocks_i32_negative", "blocks_i32_background_-7", "blocks3d_u8")

out = {}
for name in SELECTION:
    img, background = C.case(name)
    out[name + "/img"] = img
    out[name + "/background"] = np.int64(background)
    for c in C.connectivities(name):
        lab, n = label(img, background=background, return_num=True, connectivity=c)
        assert lab.max() == n < 2 ** 31
        out["%s/c%d/labels" % (name, c)] = lab.astype(np.int32)
        out["%s/c%d/n" % (name, c)] = np.int64(n)
np.savez_compressed(os.path.join(HERE, "label_components_reference.npz"), **out)
print("wrote", len(out), "arrays")
