"""GPU: the 2D NMS's per-polygon pass (stardist_amd/csrc/poly_pass.h, launched as the NMS launches it through sd_poly_pass_device)
writes, byte for byte, (1) the polygon properties of the decision shortcut that the host statement in tests/host/poly_pass_lib.cpp
computes -- the arithmetic of the properties kernel the pass replaced, reductions in the device's butterfly order -- and (2) the
PolyPrep<32> records of PrepWork::prepare compiled for the host (tests/host/beam_prep_lib.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _poly_families import families

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROPS_BYTES = 32


def _lib(tmp_path_factory, src, name):
    so = str(tmp_path_factory.mktemp(name) / ("lib%s.so" % name))
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host", src), "-o", so], check=True)
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    prep = _lib(tmp_path_factory, "beam_prep_lib.cpp", "beamprep")
    prep.beam_prep_record_bytes.restype = ctypes.c_long
    props = _lib(tmp_path_factory, "poly_pass_lib.cpp", "polypass")
    props.poly_props_record_bytes.restype = ctypes.c_long
    assert props.poly_props_record_bytes() == PROPS_BYTES
    return prep, props


def _host(fn, x, y, rec, fill):
    n, R = x.shape
    out = np.full(n * rec, fill, np.uint8)
    fn(x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), n, R, out.ctypes.data_as(ctypes.c_void_p))
    return out.reshape(n, rec)


def _first_diff(name, x, y, a, b):
    bad = np.flatnonzero((a != b).any(1))
    return len(bad) == 0, "%s: %d of %d records differ, first: polygon %d x=%s y=%s bytes %s" % (
        name, len(bad), len(a), bad[0] if len(bad) else -1, x[bad[0]].tolist() if len(bad) else [], y[bad[0]].tolist() if len(bad) else [],
        np.flatnonzero(a[bad[0]] != b[bad[0]])[:16].tolist() if len(bad) else [])


@pytest.mark.parametrize("name", sorted(families(1)))
def test_pass_records_equal_host(libs, name):
    import torch
    from stardist_amd.lib import _native as N
    hprep, hprops = libs
    x, y = families(1)[name]
    n, R = x.shape
    rec = hprep.beam_prep_record_bytes(R)
    dev = torch.device("cuda")
    tx, ty = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    want_props = R >= 3
    dprops = torch.full((n * PROPS_BYTES,), 0xCD, dtype=torch.uint8, device=dev) if want_props else None
    dprep = torch.full((n * rec,), 0xAB, dtype=torch.uint8, device=dev)
    N.check(N.lib().sd_poly_pass_device(N.tptr(tx), N.tptr(ty), n, R, N.tptr(dprops) if want_props else None, N.tptr(dprep), N.current_stream()))
    torch.cuda.synchronize()
    ok, msg = _first_diff(name + " prep", x, y, dprep.cpu().numpy().reshape(n, rec), _host(hprep.beam_prepare_host, x, y, rec, 0xAB))
    assert ok, msg
    if want_props:
        ok, msg = _first_diff(name + " props", x, y, dprops.cpu().numpy().reshape(n, PROPS_BYTES), _host(hprops.poly_props_host, x, y, PROPS_BYTES, 0))
        assert ok, msg
        # the props-only form (the area-bound probe) writes the same records
        d2 = torch.full((n * PROPS_BYTES,), 0xCD, dtype=torch.uint8, device=dev)
        N.check(N.lib().sd_poly_pass_device(N.tptr(tx), N.tptr(ty), n, R, N.tptr(d2), None, N.current_stream()))
        torch.cuda.synchronize()
        assert torch.equal(d2, dprops)
