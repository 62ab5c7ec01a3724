"""Writes tests/golden/measure_reference.npz: scikit-image 0.18's regionprops_table (label, area, bbox-*, centroid-*, and mean_intensity
for the uint8 / uint16 images) on the small 2D and 3D cases of tests/_measure_cases.py, with the inputs it was given, so that
tests/test_cpu_measure.py can tell a drifted case generator from a wrong table.  Needs scikit-image (0.18.3 wrote the committed file):

    python tests/golden/make_measure_golden.py

The float32 images are left out on purpose: scikit-image's mean_intensity accumulates float32 in float32, and its table casts min and
max to int64."""
import os
import sys

import numpy as np
from skimage.measure import regionprops_table

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _measure_cases as C  # noqa: E402

out = {}
for nd, names in (("2d", ("2d_u16", "2d_u8_rgb")), ("3d", ("3d_u16", "3d_u8"))):
    lbl = C.case(names[0])[0]
    out[nd + "/lbl"] = lbl
    table = regionprops_table(np.maximum(lbl, 0), properties=("label", "area", "bbox", "centroid"))
    for key, col in table.items():
        out["%s/%s" % (nd, key)] = np.asarray(col)
    for name in names:
        img = C.case(name)[1]
        out[name + "/img"] = img
        planes = img.reshape(lbl.shape + (-1,))
        for c in range(planes.shape[-1]):
            t = regionprops_table(np.maximum(lbl, 0), intensity_image=np.ascontiguousarray(planes[..., c]), properties=("mean_intensity",))
            out["%s/mean_intensity-%d" % (name, c)] = np.asarray(t["mean_intensity"], np.float64)
np.savez_compressed(os.path.join(HERE, "measure_reference.npz"), **out)
print("wrote", len(out), "arrays")
