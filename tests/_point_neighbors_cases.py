"""The cases of stardist_amd.utils.point_neighbors and the O(n m) numpy statement of its definition, shared by the CPU and the GPU tests.

The definition: a coordinate is scaled once, p[a] = fl(x[a] * spacing[a]); d2(q, p) = ((q0 - p0)^2 + (q1 - p1)^2) + (q2 - p2)^2 left to
right, every operation rounded in float64; candidates are ordered by (d2, index); within the radius means d2 <= fl(radius * radius); a
distance is sqrt(d2).  Without queries the points are their own queries and query i leaves out index i alone.

A case: points, queries (None: the points themselves), spacing, cell_sizes (the cell edges of the device grid to try besides the
automatic one, 0.0; they do not change any result) and calls, a list of (k, radius, count_only)."""
import functools

import numpy as np

KS = (1, 3, 8, 64)


def scaled(x, spacing):
    x = np.asarray(x)
    nd = x.shape[1]
    return x.astype(np.float64) * (np.full(nd, float(spacing)) if np.ndim(spacing) == 0 else np.asarray(spacing, np.float64))


def d2_matrix(points, queries=None, spacing=1):
    """(m, n) squared distances of the definition; the diagonal is inf without queries"""
    P = scaled(points, spacing)
    Q = P if queries is None else scaled(queries, spacing)
    d = Q[:, None, :] - P[None, :, :]
    s = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    if P.shape[1] == 3:
        s = s + d[..., 2] * d[..., 2]
    if queries is None:
        s = s.copy()
        np.fill_diagonal(s, np.inf)
    return s


def brute(s, k=None, radius=None, count_only=False):
    """the result dict of point_neighbors from the matrix of d2_matrix, with squared distances under "d2" besides "distances\""""
    m, n = s.shape
    r2 = None if radius is None else float(np.float64(radius) * np.float64(radius))
    if k is not None:
        idx = np.full((m, k), -1, np.int64)
        d2 = np.full((m, k), np.inf)
        w = min(k, n)
        if w and m:
            order = np.lexsort((np.broadcast_to(np.arange(n), s.shape), s), axis=1)[:, :w]
            d = np.take_along_axis(s, order, axis=1)
            keep = np.isfinite(d) if r2 is None else d <= r2
            idx[:, :w] = np.where(keep, order, -1)
            d2[:, :w] = np.where(keep, d, np.inf)
        return {"indices": idx, "distances": np.sqrt(d2), "d2": d2}
    inside = s <= r2
    counts = inside.sum(axis=1).astype(np.int64)
    if count_only:
        return {"counts": counts}
    rows, cols = np.nonzero(inside)                                         # row-major: ascending by index within a row
    d2 = s[rows, cols]
    return {"offsets": np.concatenate([np.zeros(1, np.int64), np.cumsum(counts, dtype=np.int64)]), "indices": cols.astype(np.int64),
            "distances": np.sqrt(d2), "d2": d2}


def lattice(*extents):
    return np.stack(np.meshgrid(*[np.arange(e) for e in extents], indexing="ij"), axis=-1).reshape(-1, len(extents)).astype(np.int64)


def _cases():
    rng = np.random.RandomState(20240611)
    every_k = [(k, None, False) for k in KS]
    c = {}

    def case(name, points, calls, queries=None, spacing=1, cell_sizes=()):
        c[name] = dict(points=points, queries=queries, spacing=spacing, cell_sizes=tuple(cell_sizes), calls=calls)

    # trivial sizes; k beyond n - 1 pads
    for nd in (2, 3):
        case("empty_%dd" % nd, np.zeros((0, nd)), every_k + [(None, 1.0, False), (None, 1.0, True), (2, 1.0, False)])
        case("one_%dd" % nd, np.full((1, nd), 3.5), every_k + [(None, 1.0, False), (None, 1.0, True)])
        case("two_%dd" % nd, np.array([[0.0] * nd, [1.0] + [2.0] * (nd - 1)]), every_k + [(None, 2.5, False), (None, 2.0, True)])
    case("five_points", rng.rand(5, 2), every_k + [(None, 0.5, False)])
    # uniform random points
    r2d, r3d = rng.rand(3000, 2) * 100, rng.rand(3000, 3) * 40
    case("random_2d", r2d, every_k + [(None, 4.6, False), (None, 4.6, True), (8, 4.6, False), (None, 1e-9, False), (None, 1e-9, True)])
    case("random_3d", r3d, every_k + [(None, 4.7, False), (None, 4.7, True), (8, 3.0, False)])
    case("random_3d_spacing", r3d, [(8, None, False), (None, 4.0, False), (None, 4.0, True)], spacing=(2.0, 0.7, 0.7))
    # integer lattices: every rank is a tie; radii that equal a distance exactly; points on cell faces
    lattice_calls = every_k + [(None, 1, False), (None, 5, False), (None, float(np.sqrt(np.float64(2))), False), (None, 5, True),
                               (8, float(np.sqrt(np.float64(2))), False)]
    case("lattice_2d", lattice(40, 40), lattice_calls, cell_sizes=(1.0, 0.5))
    case("lattice_3d", lattice(12, 12, 12), every_k + [(None, 1, False), (None, 2, True), (8, 1, False)], cell_sizes=(1.0, 0.5))
    case("lattice_2d_spacing", lattice(40, 40), [(3, None, False), (8, None, False), (None, 0.65, False), (None, 1.3, True)],
         spacing=0.65, cell_sizes=(0.65, 0.325))
    case("lattice_3d_spacing", lattice(12, 12, 12), [(8, None, False), (None, 0.65, False)], spacing=0.65, cell_sizes=(0.65, 0.325))
    # duplicates
    five = np.repeat(rng.rand(400, 2) * 30, 5, axis=0)[rng.permutation(2000)]
    case("five_fold", five, every_k + [(None, 0, False), (None, 0, True), (None, 1.5, False), (4, 0, False)])
    case("identical", np.full((500, 3), 7.25), [(1, None, False), (8, None, False), (64, None, False), (None, 0, True), (None, 0, False)])
    # degenerate boxes
    t = rng.rand(600) * 50
    case("collinear_2d", np.stack([t, 3 * t + 1], axis=1), [(1, None, False), (8, None, False), (None, 2.0, False)])
    case("axis_line_2d", np.stack([np.full(600, 2.0), t], axis=1), [(3, None, False), (None, 0.3, True)])
    case("coplanar_3d", np.concatenate([rng.rand(800, 2) * 20, np.full((800, 1), -4.0)], axis=1), [(8, None, False), (None, 1.5, False)])
    case("collinear_3d", np.stack([t, np.full(600, 1.0), np.full(600, 9.0)], axis=1), [(8, None, False), (None, 0.5, False)])
    # one far outlier: every other point in one cell, the outlier's walk crosses empty cells
    case("outlier", np.concatenate([rng.rand(2000, 2), [[1e6, 1e6]]]), [(1, None, False), (8, None, False), (None, 0.05, True)])
    # two clusters 10^4 cells apart
    clusters = np.concatenate([rng.rand(300, 2), rng.rand(300, 2) + [0.0, 1e4]])
    case("two_clusters", clusters, [(3, None, False), (64, None, False), (None, 0.1, False)], cell_sizes=(1.0,))
    case("two_clusters_query_between", clusters, [(3, None, False), (None, 6000.0, True)], queries=np.array([[0.5, 5000.0], [0.2, 4999.0]]),
         cell_sizes=(1.0,))
    # large coordinates; a near-tie of one ulp
    case("offset_2_40", rng.rand(1000, 2) * 64 + 2.0 ** 40, [(8, None, False), (None, 3.0, False)])
    x = 0.7
    case("one_ulp", np.array([[0.0, 0.0], [x, 0.0], [0.0, np.nextafter(x, 1.0)]]), [(1, None, False), (2, None, False), (None, x, False)])
    # a radius that covers everything
    case("all_within", rng.rand(700, 2), [(None, 2.0, False), (None, 2.0, True)])
    # a second point set
    case("queries_are_the_points", r2d[:1200], [(3, None, False), (None, 4.0, False), (None, 0, True)], queries=r2d[:1200].copy())
    far = np.array([[-1e5, 50.0], [50.0, 1e7], [1e3, 1e3], [50.0, 50.0], [-0.001, -0.001]])
    case("queries_outside", r2d[:1500], [(1, None, False), (8, None, False), (None, 2e5, True), (None, 30.0, False)], queries=far)
    case("queries_outside_3d", r3d[:1000], [(8, None, False), (None, 90.0, True)], queries=np.array([[-50.0, 20.0, 20.0], [20.0, 20.0, 300.0]]))
    case("no_queries", r2d[:50], [(3, None, False), (None, 5.0, False), (None, 5.0, True)], queries=np.zeros((0, 2)))
    case("spots_and_nuclei", r3d[:1500], [(1, None, False), (None, 5.0, False)], queries=rng.rand(900, 3) * 40, spacing=(2.0, 0.7, 0.7))
    return c


CASES = _cases()
# the cases without ties and near-ties: scipy's own order is the definition's there
TIE_FREE = ("random_2d", "random_3d", "random_3d_spacing", "outlier", "two_clusters", "spots_and_nuclei", "coplanar_3d")
LATTICES = ("lattice_2d", "lattice_3d", "lattice_2d_spacing", "lattice_3d_spacing")


@functools.lru_cache(maxsize=None)
def matrix(name):
    c = CASES[name]
    s = d2_matrix(c["points"], c["queries"], c["spacing"])
    s.setflags(write=False)
    return s


def expected(name, k, radius, count_only):
    return brute(matrix(name), k, radius, count_only)


def calls():
    """[(name, k, radius, count_only)] over all cases"""
    return [(name,) + call for name, c in CASES.items() for call in c["calls"]]


def call_id(v):
    return "%s-k%s-r%s%s" % (v[0], v[1], v[2], "-count" if v[3] else "")


# what raises ValueError before anything runs: (points, keywords)
ERRORS = [
    (np.zeros((4, 2)), dict(k=0)),
    (np.zeros((4, 2)), dict(k=65)),
    (np.zeros((4, 2)), dict(k=1.0)),
    (np.zeros((4, 2)), dict()),
    (np.array([[0.0, np.nan], [1.0, 2.0]]), dict(k=1)),
    (np.array([[0.0, np.inf], [1.0, 2.0]]), dict(radius=1.0)),
    (np.zeros((4, 4)), dict(k=1)),
    (np.zeros((4,)), dict(k=1)),
    (np.zeros((4, 2)), dict(count_only=True, k=2)),
    (np.zeros((4, 2)), dict(count_only=True)),
    (np.zeros((4, 2)), dict(count_only=True, k=2, radius=1.0)),
    (np.zeros((4, 2)), dict(radius=-1.0)),
    (np.zeros((4, 2)), dict(radius=np.inf)),
    (np.zeros((4, 2)), dict(k=1, queries=np.zeros((2, 3)))),
    (np.zeros((4, 2)), dict(k=1, queries=np.array([[np.nan, 0.0]]))),
    (np.zeros((4, 2)), dict(k=1, spacing=0)),
    (np.zeros((4, 2)), dict(k=1, spacing=(1, 2, 3))),
    (np.full((4, 2), 2.0 ** 499), dict(k=1, spacing=2.0)),
    (np.zeros((4, 2), np.complex128), dict(k=1)),
]
