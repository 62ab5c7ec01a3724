"""Writes tests/golden/measure_table_parent.npz: the host route's numpy tables of measure_labels (every keyword at once), label_contacts
and point_neighbors on the cases GOLDEN_NAMES of tests/_table_exit_cases.py, as "<case>/<position>/<column>", and of the tables DERIVED
there a SHA-256 per column ("derived/<kind>/<case>", the two columns that go through the maths library in full beside it), so that
tests/test_cpu_table_exit.py holds the shared table exit (stardist_amd._route.table_exit) and the one array shim (_route.ops) to the
keys, order, dtypes and bytes of the code before them.

To be run on the PARENT of the commit that introduced table_exit (050a9bb wrote the committed file), with this script and
tests/_table_exit_cases.py copied into that checkout:

    python tests/golden/make_measure_table_golden.py

It is regenerated only by a change that means to alter a table."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import _table_exit_cases as T  # noqa: E402

out = {}
for name in T.GOLDEN_NAMES:
    for at, (key, col) in enumerate(T.run(name).items()):
        assert isinstance(col, np.ndarray)
        out["%s/%02d/%s" % (name, at, key)] = col
for kind, name in T.DERIVED:                                                # the derived columns: digests, and the libm columns in full
    table = T.derived(kind, name)
    out["derived/%s/%s" % (kind, name)] = T.digests(table)
    for key in T.LIBM:
        if key in table:
            out["derived/%s/%s/%s" % (kind, name, key)] = table[key]
np.savez_compressed(T.GOLDEN, **out)
print("wrote", len(out), "arrays,", os.path.getsize(T.GOLDEN), "bytes")
