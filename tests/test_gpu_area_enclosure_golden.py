"""GPU: every output of the area enclosure (stardist_amd/csrc/area_bounds.h pair_enclosure through sd_area_bounds_pairs_device) equals, bit for
bit, what the build of commit 2d2206f returned for the same seeded inputs (tests/golden/make_area_enclosure_golden.py): the small
families array by array, the large family by the crc32 of each array."""
import numpy as np
import pytest

import _area_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gen():
    return _area_golden.generator()


def test_small_families_equal_their_goldens(gen):
    from stardist_amd.lib import stardist2d as sd2
    gold = _area_golden.small()
    fams = gen.small_families()
    assert set(fams) == set(gold)
    for name, polys in fams.items():
        got = gen.encode(sd2.area_bounds_pairs(*polys))
        for arr in gen.ARRAYS:
            want = gold[name][arr]
            assert got[arr].dtype == want.dtype and got[arr].shape == want.shape, (name, arr)
            bad = np.flatnonzero(got[arr] != want)
            assert bad.size == 0, (name, arr, bad[:10], got[arr][bad[:10]], want[bad[:10]])


def test_large_family_equals_its_checksums(gen):
    """60 001 pairs: under the probe's grid (the blocks resident at once, eight pairs per block and trip) some wave takes at least three
    trips of the outer loop and the last trip is partial"""
    from stardist_amd.lib import _native as N, stardist2d as sd2
    rec = _area_golden.recorded()["large"]
    n = rec["n_pairs"]
    assert n == gen.N_LARGE
    grid = N.lib().sd_area_bounds_pairs_grid()
    assert grid > 0
    per_trip = 8 * grid
    assert n > 2 * per_trip and n % per_trip != 0, (n, grid)
    got = gen.encode(sd2.area_bounds_pairs(*gen.large_family()))
    assert {k: gen.crc(got[k]) for k in gen.ARRAYS} == rec["crc32"]
