"""Integer polygon families (n_rays <= 32) for the tests of the 2D NMS's per-polygon pass (test_cpu_poly_pass.py, test_gpu_poly_pass.py):
star polygons as the NMS builds them, and the degenerate rings its properties and its preparation must treat exactly as before."""
import numpy as np


def star_polys(rng, n, R, radius, noise, spread):
    ang = np.float32(2 * np.pi / R)
    k = np.arange(R, dtype=np.int32)
    s = np.sin((ang * k).astype(np.float32)).astype(np.float32)
    c = np.cos((ang * k).astype(np.float32)).astype(np.float32)
    d = np.maximum((radius * (1 + noise * rng.uniform(-1, 1, (n, R)))).astype(np.float32), np.float32(1e-3))
    p = np.floor(rng.uniform(50, 50 + spread, (n, 2))).astype(np.float32)
    y = (p[:, :1] + d * s).astype(np.float32)
    x = (p[:, 1:] + d * c).astype(np.float32)
    return np.ascontiguousarray(x.astype(np.int64).astype(np.int32)), np.ascontiguousarray(y.astype(np.int64).astype(np.int32))


def _c(a):
    return np.ascontiguousarray(a.astype(np.int32))


def families(seed):
    rng = np.random.RandomState(seed)
    f = {}
    # the families of test_gpu_beam_prep.py with n_rays <= 32
    for R, radius, noise in [(32, 10, 0.1), (32, 3, 0.5), (32, 2, 0.9), (11, 10, 0.3), (5, 1, 0.5)]:
        f["star_R%d_r%d_n%g" % (R, radius, noise)] = star_polys(rng, 4000, R, radius, noise, 12)
    # radius 1-3: many duplicate vertices
    for radius in (1, 2, 3):
        f["tiny_r%d" % radius] = star_polys(rng, 4000, 32, radius, 0.6, 8)
    # R = 3 and R = 5
    f["star_R3"] = star_polys(rng, 4000, 3, 6, 0.5, 12)
    f["star_R5"] = star_polys(rng, 4000, 5, 4, 0.5, 12)
    # spikes (a vertex far out or at the centre) and fold-backs (a vertex repeats its predecessor's predecessor)
    x, y = star_polys(rng, 4000, 32, 10, 0.2, 12)
    x, y = x.copy(), y.copy()
    rows = np.arange(4000)
    i = rng.randint(0, 32, 4000)
    x[rows, i] += rng.randint(-30, 31, 4000)
    y[rows, i] += rng.randint(-30, 31, 4000)
    j = rng.randint(0, 32, 4000)
    x[rows, j] = x[rows, j - 2]
    y[rows, j] = y[rows, j - 2]
    f["spikes_foldbacks"] = (_c(x), _c(y))
    # all vertices equal; two distinct points
    p = rng.randint(-100, 100, (200, 2))
    f["all_equal"] = (_c(np.repeat(p[:, :1], 32, 1)), _c(np.repeat(p[:, 1:], 32, 1)))
    q = np.where(rng.rand(200, 32) < 0.5, 0, 1)
    f["two_points"] = (_c(p[:, :1] + 3 * q), _c(p[:, 1:] - 2 * q))
    # free lattice rings in a small box: self-intersections, collinear runs, vertices within half a step of an edge
    for R in (5, 12, 32):
        f["lattice_R%d" % R] = (_c(rng.randint(0, 7, (4000, R))), _c(rng.randint(0, 7, (4000, R))))
    # a vertex within half a step of a non-adjacent edge: the long edge of a thin wedge passes next to a lattice point
    x, y = star_polys(rng, 4000, 32, 12, 0.05, 12)
    x, y = x.copy(), y.copy()
    x[:, 8] = x[:, 0] + rng.randint(-1, 2, 4000)
    y[:, 8] = y[:, 24] + rng.randint(-1, 2, 4000)
    f["near_half_step"] = (_c(x), _c(y))
    # bounding boxes that just fit / just exceed the float window (2047), and rings beyond 16-bit offsets from vertex 0
    for ext in (2046, 2047, 2048, 32767, 32768, 70000):
        x, y = star_polys(rng, 500, 32, 10, 0.3, 12)
        x, y = x.copy(), y.copy()
        x[:, 5] = x[:, 0] + ext
        y[:, 20] = y[:, 0] - ext
        f["extent_%d" % ext] = (_c(x), _c(y))
    for radius in (1023.2, 1023.6, 1023.9, 1024.2):                            # convex rings whose box is about WINDOW wide
        f["big_star_r%g" % radius] = star_polys(rng, 500, 32, radius, 0.0, 12)
    x, y = f["big_star_r1023.6"]
    f["big_star_w2047"] = (_c(x + (np.arange(32) == 0)), y)                 # the rightmost vertex one step further out: box 2047 wide
    x, y = star_polys(rng, 500, 32, 10, 0.3, 12)
    f["far_origin"] = (_c(x.astype(np.int64) + 2 ** 30), _c(y.astype(np.int64) - 2 ** 30))
    return f
