"""CPU: the preparation of the 2D NMS's per-polygon pass (FastPrep in stardist_amd/csrc/poly_pass.h: ring as 16-bit offsets, cleanup
list as a bit mask, edge codes as masks) compiled for the host writes, byte for byte, the PolyPrep<32> records of PrepWork::prepare
(clip_beam.h) -- the statement that tests/host/beam_check.cpp pins against the reference's Clipper."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _poly_families import families

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib(tmp_path_factory, src, name):
    so = str(tmp_path_factory.mktemp(name) / ("lib%s.so" % name))
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host", src), "-o", so], check=True)
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    ref = _lib(tmp_path_factory, "beam_prep_lib.cpp", "beamprep")
    ref.beam_prep_record_bytes.restype = ctypes.c_long
    new = _lib(tmp_path_factory, "poly_pass_lib.cpp", "polypass")
    return ref, new


def _records(fn, x, y, rec):
    n, R = x.shape
    out = np.full(n * rec, 0xAB, np.uint8)
    fn(x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), n, R, out.ctypes.data_as(ctypes.c_void_p))
    return out.reshape(n, rec)


@pytest.mark.parametrize("name", sorted(families(0)))
def test_fast_prepare_equals_prepwork(libs, name):
    ref, new = libs
    x, y = families(0)[name]
    rec = ref.beam_prep_record_bytes(x.shape[1])
    a = _records(ref.beam_prepare_host, x, y, rec)
    b = _records(new.poly_pass_prep_host, x, y, rec)
    bad = np.flatnonzero((a != b).any(1))
    assert len(bad) == 0, "%s: %d of %d records differ, first: polygon %d x=%s y=%s bytes %s" % (
        name, len(bad), len(a), bad[0], x[bad[0]].tolist(), y[bad[0]].tolist(), np.flatnonzero(a[bad[0]] != b[bad[0]])[:16].tolist())
