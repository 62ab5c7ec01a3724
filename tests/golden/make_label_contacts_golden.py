"""Writes tests/golden/label_contacts_reference.npz: the edge sets of scikit-image's skimage.future.graph.RAG(lbl, connectivity) on the
GOLDEN cases of tests/_label_contacts_cases.py, with the inputs they were given, so that tests/test_cpu_label_contacts.py can tell a
drifted case generator from a wrong result.  Needs scikit-image and networkx (scikit-image 0.18.3 wrote the committed file):

    python tests/golden/make_label_contacts_golden.py

RAG has a node for every value, 0 too, and unordered edges; they are stored as (min, max) rows, ascending -- what
label_contacts(background=True) lists as its pairs.  The contact counts have no counterpart in scikit-image.
Data only: keys "<case>/img" and "<case>/c<connectivity>" (int64, shape (edges, 2))."""
import os
import sys

import numpy as np
from skimage.future.graph import RAG

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _label_contacts_cases as C  # noqa: E402

out = {}
for name in C.GOLDEN:
    img = C.SMALL[name]
    out["%s/img" % name] = img
    for c in range(1, img.ndim + 1):
        edges = sorted((min(int(a), int(b)), max(int(a), int(b))) for a, b in RAG(np.array(img), connectivity=c).edges() if a != b)
        out["%s/c%d" % (name, c)] = np.array(edges, np.int64).reshape(len(edges), 2)
np.savez_compressed(os.path.join(HERE, "label_contacts_reference.npz"), **out)
print("wrote", len(out), "arrays")
