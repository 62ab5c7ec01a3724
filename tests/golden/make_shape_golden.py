"""Writes tests/golden/shape_reference.npz: scikit-image 0.18's regionprops_table shape columns (equivalent_diameter, extent,
inertia_tensor, inertia_tensor_eigvals, major / minor_axis_length and, in 2D, eccentricity, orientation, perimeter, perimeter_crofton,
euler_number) on the cases GOLDEN of tests/_shape_cases.py, with the inputs it was given, so that tests/test_cpu_measure_shape.py can
tell a drifted case generator from a wrong table.  Needs scikit-image (0.18.3 wrote the committed file):

    python tests/golden/make_shape_golden.py
"""
import os
import sys

import numpy as np
from skimage.measure import regionprops_table

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _shape_cases as S  # noqa: E402

BOTH = ("label", "area", "equivalent_diameter", "extent", "inertia_tensor", "inertia_tensor_eigvals", "major_axis_length", "minor_axis_length")
FLAT = ("eccentricity", "orientation", "perimeter", "perimeter_crofton", "euler_number")

out = {}
for name in S.GOLDEN:
    lbl = S.case(name)
    assert np.abs(lbl).max() < 2 ** 15
    out[name + "/lbl"] = lbl.astype(np.int16)
    table = regionprops_table(np.maximum(lbl, 0), properties=BOTH + (FLAT if lbl.ndim == 2 else ()))
    for key, col in table.items():
        out["%s/%s" % (name, key)] = np.asarray(col)
np.savez_compressed(os.path.join(HERE, "shape_reference.npz"), **out)
print("wrote", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "shape_reference.npz")), "bytes")
