"""Writes tests/golden/expand_labels_reference.npz: scikit-image's skimage.segmentation.expand_labels at every distance of
tests/_expand_cases.py on a selection of its cases, with the inputs it was given, so that tests/test_cpu_expand_labels.py can tell a
drifted case generator from a wrong result.  Unit spacing only: scikit-image 0.18 has no `spacing`.  Needs scikit-image (0.18.3 wrote
the committed file):

    python tests/golden/make_expand_labels_golden.py

Data only: keys "<case>/lbl", "<case>/d<k>/distance" (float64) and "<case>/d<k>/out" (the case's dtype)."""
import os
import sys

import numpy as np
from skimage.segmentation import expand_labels

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _expand_cases as C  # noqa: E402

SELECTION = ("discs", "points", "lattice", "far_corner", "all_labelled", "one_column", "high_labels", "discs_u8", "discs_i64",
             "balls", "lattice3d", "corner3d", "plane_as_volume", "balls_u16", "discs_big")

out = {}
for name in SELECTION:
    lbl = C.case(name)
    out[name + "/lbl"] = lbl
    for k, distance in enumerate(C.distances(name)):
        grown = expand_labels(lbl, distance)
        assert grown.dtype == lbl.dtype and grown.shape == lbl.shape
        out["%s/d%d/distance" % (name, k)] = np.float64(distance)
        out["%s/d%d/out" % (name, k)] = grown
np.savez_compressed(os.path.join(HERE, "expand_labels_reference.npz"), **out)
print("wrote", len(out), "arrays")
