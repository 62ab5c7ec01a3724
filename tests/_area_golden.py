"""The goldens of the 2D NMS's area enclosure (tests/golden/area_enclosure_small.npz, area_enclosure_golden.json) and the module that
recorded them and rebuilds their inputs from seeds (tests/golden/make_area_enclosure_golden.py)."""
import importlib.util
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def generator():
    spec = importlib.util.spec_from_file_location("make_area_enclosure_golden", os.path.join(GOLDEN, "make_area_enclosure_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def small():
    """{family: {array name: golden array}}"""
    z = np.load(os.path.join(GOLDEN, "area_enclosure_small.npz"))
    out = {}
    for key in z.files:
        fam, name = key.split("/")
        out.setdefault(fam, {})[name] = z[key]
    return out


def recorded():
    with open(os.path.join(GOLDEN, "area_enclosure_golden.json")) as fh:
        return json.load(fh)
