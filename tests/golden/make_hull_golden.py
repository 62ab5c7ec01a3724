"""Writes tests/golden/hull_reference.npz: scikit-image 0.18's regionprops_table columns label, area, convex_area, solidity and
feret_diameter_max on the cases GOLDEN of tests/_hull_cases.py, with the inputs it was given, so that tests/test_cpu_measure_hull.py
can tell a drifted case generator from a wrong table.  Needs scikit-image (0.18.3 wrote the committed file):

    python tests/golden/make_hull_golden.py
"""
import os
import sys

import numpy as np
import skimage
from skimage.measure import regionprops_table

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _hull_cases as H  # noqa: E402

PROPERTIES = ("label", "area", "convex_area", "solidity", "feret_diameter_max")

out = {"skimage_version": np.array(skimage.__version__)}
for name in H.GOLDEN:
    lbl = H.case(name)
    assert np.abs(lbl).max() < 2 ** 15
    out[name + "/lbl"] = lbl.astype(np.int16)
    table = regionprops_table(np.maximum(lbl, 0), properties=PROPERTIES)
    for key, col in table.items():
        out["%s/%s" % (name, key)] = np.asarray(col)
np.savez_compressed(os.path.join(HERE, "hull_reference.npz"), **out)
print("wrote", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "hull_reference.npz")), "bytes")
