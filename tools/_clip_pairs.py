"""The pairs of the sweep-latency probes (tools/time_clip_latency.py, tools/beam_phase_profile.py): bench-like star polygons, 32 rays,
radius ~ 14, centres offset by (9, 6) so that the overlap is near the NMS threshold.  One seeded stream: the first n pairs are the same
for every caller."""
import numpy as np

R = 32
NMAX = 1 << 17


def make_pairs():
    """-> xa, ya, xb, yb: int32 [NMAX, R]"""
    rng = np.random.default_rng(0)
    phi = 2 * np.pi * np.arange(R) / R

    def polys(n, shift):
        d = 14.0 * (1 + 0.15 * rng.standard_normal((n, R))).astype(np.float32)
        c = rng.uniform(200, 210, (n, 2)).astype(np.float32) + shift
        x = (c[:, 1:2] + d * np.cos(phi)).astype(np.int32); y = (c[:, 0:1] + d * np.sin(phi)).astype(np.int32)
        return x, y

    xa, ya = polys(NMAX, 0.0)
    xb, yb = polys(NMAX, np.float32([9.0, 6.0]))
    return xa, ya, xb, yb
