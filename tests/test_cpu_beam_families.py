"""CPU: the bound-slot sweep (stardist_amd/csrc/clip_beam.h, compiled for the host by tests/host/beam_families_check.cpp) on pair families
built to hit what its per-beam arithmetic depends on -- horizontals on a scan line, exact half-integer ties of TopX, vertices at the
edge of the 16-bit range, random 3- to 32-gons, identical and touching rings.  Pair by pair the tier-1 form (16-bit coordinates through
HostLds), the tier-2 form, clip_sweep.h's Sweep / SweepFull and the reference's compiled Clipper (oracle/_ref) must agree in twice-area,
join flag and failure status; a pair that a tier flags for capacity must be held by the next one."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "beam_families_check.cpp")


def _build(refmods, tmp_path_factory, name, defs):
    exe = str(tmp_path_factory.mktemp("beamfam") / name)
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.run(["g++", "-O2", "-std=c++17"] + defs + [SRC, "-o", exe, "-L" + ref_dir, "-lclipper_ref", "-Wl,-rpath," + ref_dir], check=True)
    return exe


@pytest.fixture(scope="module")
def harness(refmods, tmp_path_factory):
    return _build(refmods, tmp_path_factory, "beam_families_check", [])


@pytest.fixture(scope="module")
def counting_harness(refmods, tmp_path_factory):
    """the build that recomputes TopX at the top of every scan-beam and compares it with the stored Curr.X"""
    return _build(refmods, tmp_path_factory, "beam_families_check_curx", ["-DBEAM_VERIFY_CURX"])


def _run(exe, family, n, seed):
    r = subprocess.run([exe, "check", str(family), str(n), str(seed), "3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout)}, r.stdout


# family, pairs, seed: 1 horizontals, 2 ties, 3 offsets around +-32 767 / 32 768, 4 random (>= 200 000 pairs), 5 identical and touching
@pytest.mark.parametrize("family,n,seed", [(1, 40000, 1), (2, 40000, 2), (3, 40000, 3), (4, 200000, 4), (5, 40000, 5)])
def test_every_pair_equals_sweep_and_clipper(harness, family, n, seed):
    c, out = _run(harness, family, n, seed)
    assert c["pairs"] == n and c["mismatches"] == 0, out
    assert c["nonzero"] > n // 4, out                         # the pairs do overlap
    if family == 2:
        assert c["tie_edges"] > n, out                        # more than one edge per pair stands on an exact tie at some scan line
    if family == 3:
        assert 0 < c["tier1_flagged"] < n, out                # offsets beyond 16 bits are flagged, those within are held
    if family in (1, 5):
        assert c["with_joins"] > 0, out                       # coincident and horizontal edges do reach the join code


@pytest.mark.parametrize("family", [1, 2, 3, 4, 5])
def test_stored_curr_x_equals_recomputed_top_x(counting_harness, family):
    """the recomputation that the sweeps no longer do: zero differences over every edge and scan-beam of every sweep of the harness"""
    c, out = _run(counting_harness, family, 20000, 10 + family)
    assert c["mismatches"] == 0 and c["curx_differences"] == 0 and c["curx_checks"] > 100000, out
