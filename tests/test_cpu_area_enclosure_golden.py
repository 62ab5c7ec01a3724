"""CPU: the committed goldens of the area enclosure (tests/golden/area_enclosure_small.npz, recorded on the GPU) are the test they claim to
be: against the numpy statement of the enclosure (tests/_area_exact.py) their `usable`, K and T are right, and the set holds every kind
of pair the kernel treats differently."""
import numpy as np
import pytest

import _area_golden
from _area_exact import exact_area, near_pairs, plain


@pytest.fixture(scope="module")
def cases():
    """per small family: the inputs (int64), the goldens, and the statement's classification of every pair"""
    gen = _area_golden.generator()
    gold = _area_golden.small()
    out = {}
    for name, polys in gen.small_families().items():
        xa, ya, xb, yb = (v.astype(np.int64) for v in polys)
        _, K, same_orientation, _, _ = exact_area(xa, ya, xb, yb)
        simple = plain(xa, ya) & plain(xb, yb)
        ox, oy = (xa.min(1) + xa.max(1)) >> 1, (ya.min(1) + ya.max(1)) >> 1       # the centre of P's box; the window is 1023 about it
        ext = np.maximum.reduce([np.abs(xa - ox[:, None]).max(1), np.abs(ya - oy[:, None]).max(1), np.abs(xb - ox[:, None]).max(1), np.abs(yb - oy[:, None]).max(1)])
        zero_len = np.zeros(len(xa), bool)
        for x, y in ((xa, ya), (xb, yb)):
            zero_len |= ((np.roll(x, -1, 1) == x) & (np.roll(y, -1, 1) == y)).any(1)
        out[name] = dict(gold=gold[name], K=K, T=near_pairs(xa, ya, xb, yb), same_orientation=same_orientation, simple=simple, window=ext <= 1023,
                         zero_len=zero_len, n=len(xa))
    return out


def test_goldens_cover_the_families(cases):
    gen = _area_golden.generator()
    assert sum(g.nbytes for c in cases.values() for g in c["gold"].values()) < 100000
    for name, c in cases.items():
        assert set(c["gold"]) == set(gen.ARRAYS) and all(len(c["gold"][a]) == c["n"] for a in gen.ARRAYS), name
    big = [c["n"] for c in cases.values() if c["n"] > 500]
    assert len(big) >= 7 and all(n % 2 == 1 for n in big)                       # an odd count: the last wave's upper half idles
    assert cases["single_R32"]["n"] == 1
    rec = _area_golden.recorded()
    assert rec["large"]["n_pairs"] == gen.N_LARGE == 60001 and set(rec["large"]["crc32"]) == set(gen.ARRAYS)


def test_usable_K_and_T_are_the_statements(cases):
    """(the float-accumulation guard of the enclosure, the last reason a pair can be unusable, is far from these small polygons)"""
    for name, c in cases.items():
        want = c["same_orientation"] & c["simple"] & c["window"]
        usable = c["gold"]["usable"].astype(bool)
        assert np.array_equal(usable, want), (name, np.flatnonzero(usable != want)[:10])
        assert np.array_equal(c["gold"]["K"][usable], c["K"][usable]), name
        assert np.array_equal(c["gold"]["T"][usable], c["T"][usable]), name
        inside = ~c["window"]                                                    # beyond the window nothing is evaluated
        assert not c["gold"]["K"][inside].any() and not c["gold"]["T"][inside].any(), name


def test_every_kind_of_pair_is_present(cases):
    cat = lambda f: sum(int(f(c, c["gold"]["usable"].astype(bool)).sum()) for c in cases.values())
    counts = {
        "unusable by orientation": cat(lambda c, u: ~u & ~c["same_orientation"] & c["simple"] & c["window"]),
        "unusable by window": cat(lambda c, u: ~u & c["same_orientation"] & c["simple"] & ~c["window"]),
        "unusable by simplicity": cat(lambda c, u: ~u & c["same_orientation"] & ~c["simple"] & c["window"]),
        "usable, K = 0": cat(lambda c, u: u & (c["gold"]["K"] == 0)),
        "usable, K >= 8": cat(lambda c, u: u & (c["gold"]["K"] >= 8)),
        "usable, T >= 30": cat(lambda c, u: u & (c["gold"]["T"] >= 30)),
        "usable with a zero-length edge": cat(lambda c, u: u & c["zero_len"]),
        "with a zero-length edge": cat(lambda c, u: c["zero_len"]),
    }
    print(counts)
    assert all(v > 0 for v in counts.values()), counts
