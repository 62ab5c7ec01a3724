"""NMS scenes whose suppression graph is known by construction (tests/test_cpu_nms_graph_cases.py proves them against the compiled
reference, tests/test_gpu_nms_graph.py runs the HIP schedulers on them).

A scene is a set of discs (2D) or balls (3D) in NMS order -- best score first -- with a DESIGNED edge list: the pairs that overlap far above
the threshold; every other pair overlaps far below it.  The expected keep flags come from `greedy` below, a plain sequential loop over that
edge list, never from an NMS.  What the scenes load is the greedy scheduler: dependency chains as deep as the scene, one candidate with
thousands of neighbours, cliques, and many short chains at once.

Geometry.  Every ray length is radius * (1 + 0.02 u), u uniform in [-1, 1] from a fixed seed; every centre gets a non-integer offset
amp * ((0.37 k) mod 1, (0.61 k) mod 1, (0.83 k) mod 1) on top of a non-integer origin (k = index of construction), so no two candidates are
lattice translates of each other.  Margins (overlap / smaller area resp. volume of the discs / balls; the polygons and polyhedra inscribed
in them are checked pair by pair against the compiled reference in the CPU test):

  2D, threshold 0.3, radius 10:  designed neighbours 8 apart (0.50), others at least 16 apart (0.10) on straight parts.  The U-turns of the
      serpentine are arcs of 12 chords of length 8: second neighbours 16 cos(7.5 deg) = 15.86 apart there (0.11) -- a corner of two straight
      runs would put them 11.3 apart (0.32), so the fold has to be round.
  3D, threshold 0.25, radius 8:  designed neighbours 6 apart (0.46), others at least 12 apart (0.09); U-turns as in 2D (11.9 apart).
  ladder: a 4-cycle of equal discs with sides s has a diagonal of at most s sqrt(2), so "8 and at least 16" cannot be had.  The ladder takes
      the widest margins equal discs allow around the thresholds: 2D s = 10 (0.39) with diagonals 14.1 (0.18); 3D s = 7.5 (0.35) with
      diagonals 10.6 (0.15).
  hub: small discs (radius 3, pitch 7.3) / balls (radius 2, face-centred cubic, nearest neighbours 4.15 apart) are pairwise disjoint; the
      inner ones lie inside the hub polygon / polyhedron (overlap / smaller = 1), the outer ones outside its bounding box.

The hubs of SLOT_LIMIT_2D (hub radius 1000 and 1300, 49 061 to 72 601 candidates) are sized by the slot total of the neighbour lists, not by
the scheduler: tests/test_gpu_nms_slot_limits.py.
"""
import numpy as np

THR = {2: 0.3, 3: 0.25}
RADIUS = {2: 10.0, 3: 8.0}
STEP = {2: 8.0, 3: 6.0}
LADDER_STEP = {2: 10.0, 3: 7.5}
HUB_RADIUS = {2: 200.0, 3: 24.0}
SMALL_RADIUS = {2: 3.0, 3: 2.0}
RAY_NOISE = 0.02
TURN_CHORDS = 12


class Scene(object):
    """dist (n, R) f32, points (n, dim) f32 (y, x) / (z, y, x), scores (n,) f32 strictly falling, edges (E, 2) with i < j in NMS order, keep (n,)
    bool.  edge_dist = (lo, hi) bounds the centre distance of every designed edge among the ordinary candidates, non_edge_min every other
    pair of them (`big` = index of the hub, exempt from both).  labelings: int arrays; two candidates with different non-negative labels
    are claimed to have disjoint bounding boxes."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n(self):
        return len(self.dist)

    def rays(self):
        from stardist_amd.rays3d import Rays_GoldenSpiral
        r = Rays_GoldenSpiral(self.n_rays)
        return np.ascontiguousarray(r.vertices, np.float32), np.ascontiguousarray(r.faces, np.int32)


def greedy(n, edges):
    """the reference's sequential loop over a given edge list: a candidate still standing suppresses its lower-scored neighbours"""
    below = [[] for _ in range(n)]
    for i, j in edges:
        below[min(i, j)].append(max(i, j))
    keep = np.ones(n, bool)
    for i in range(n):
        if keep[i]:
            for j in below[i]:
                keep[j] = False
    return keep


def _frac(k, dim):
    k = np.asarray(k, np.float64)
    return np.stack([(0.37 * k) % 1, (0.61 * k) % 1, (0.83 * k) % 1][:dim], 1)


def _assemble(name, dim, pos, radius, rank, edges_c, n_rays, seed, amp=0.25, copies=(), **kw):
    """pos / radius / edges_c in construction order, rank[k] = place of candidate k in the NMS order; copies = (k_from, k_to) pairs whose
    rays and centre are duplicated exactly"""
    n = len(pos)
    rng = np.random.RandomState(seed)
    dist = np.asarray(radius, np.float64)[:, None] * (1 + RAY_NOISE * rng.uniform(-1, 1, (n, n_rays)))
    pts = np.asarray(pos, np.float64) + amp * _frac(np.arange(n), dim)
    for a, b in copies:
        dist[b] = dist[a]; pts[b] = pts[a]
    pts = pts - pts.min(0) + np.array([30.37, 31.61, 32.83][:dim]) + (np.asarray(radius).max() if n else 0)
    rank = np.asarray(rank, np.int64)
    order = np.argsort(rank)
    if edges_c is None:                                  # a clique too large to list: candidate 0 suppresses every other one
        edges, keep = None, np.arange(n) == 0
    else:
        edges = rank[np.asarray(edges_c, np.int64).reshape(-1, 2)]
        edges = np.sort(edges, 1)
        keep = greedy(n, edges)
    labelings = [np.asarray(l)[order] for l in kw.pop("labelings", [])]
    big = kw.pop("big", None)
    return Scene(name=name, dim=dim, n_rays=n_rays, thr=np.float32(THR[dim]),
                 dist=np.ascontiguousarray(dist[order], np.float32), points=np.ascontiguousarray(pts[order], np.float32),
                 scores=np.linspace(0.99, 0.5, n).astype(np.float32), edges=edges, keep=keep,
                 labelings=labelings, big=None if big is None else int(rank[big]), **kw)


def _path(n, step, layout):
    """n points `step` apart along a straight line, or along a serpentine of straight rows joined by half-circles of TURN_CHORDS chords"""
    if layout == "line":
        return np.stack([np.zeros(n), step * np.arange(n)], 1)
    assert layout == "serpentine"
    row = max(int(np.ceil(np.sqrt(n))), 2)
    p = np.zeros((n, 2)); heading, turn, run = 0.0, 1.0, 0
    for k in range(1, n):
        if run >= row:                                   # in a U-turn: TURN_CHORDS chords, each turned by pi / TURN_CHORDS
            heading += turn * np.pi / TURN_CHORDS
            if run == row + TURN_CHORDS - 1:
                run = -1; turn = -turn
        p[k] = p[k - 1] + step * np.array([np.sin(heading), np.cos(heading)])
        run += 1
    return p


def _embed(p2, dim):
    return p2 if dim == 2 else np.concatenate([np.zeros((len(p2), 1)), p2], 1)


def _ranks(n, order, seed):
    return np.arange(n) if order == "monotone" else np.random.RandomState(seed).permutation(n)


def chain(dim, n, order="monotone", layout="line", n_rays=None, seed=1):
    n_rays = n_rays or (32 if dim == 2 else 96)
    step = STEP[dim]
    two_apart = 2 * step * (np.cos(np.pi / (2 * TURN_CHORDS)) if layout == "serpentine" else 1.0)
    return _assemble("chain%dd-%d-%s-%s-r%d" % (dim, n, order, layout, n_rays), dim, _embed(_path(n, step, layout), dim), np.full(n, RADIUS[dim]),
                     _ranks(n, order, seed + n), [(k, k + 1) for k in range(n - 1)], n_rays, seed,
                     edge_dist=(step - 0.45, step + 0.45), non_edge_min=two_apart - 0.45, depth=n if order == "monotone" else None)


def ladder(dim, n, n_rays=None, seed=2):
    n_rays = n_rays or (32 if dim == 2 else 96)
    h, s = n // 2, LADDER_STEP[dim]
    pos = np.concatenate([np.stack([np.zeros(h), s * np.arange(h)], 1), np.stack([np.full(h, s), s * np.arange(h)], 1)])
    edges = [(k, k + 1) for k in range(h - 1)] + [(h + k, h + k + 1) for k in range(h - 1)] + [(k, h + k) for k in range(h)]
    return _assemble("ladder%dd-%d" % (dim, 2 * h), dim, _embed(pos, dim), np.full(2 * h, RADIUS[dim]), _ranks(2 * h, "random", seed), edges, n_rays, seed,
                     amp=0.1, edge_dist=(s - 0.2, s + 0.2), non_edge_min=s * np.sqrt(2) - 0.2)


def _inradius(dim, n_rays):
    """distance of the nearest face of the unit polygon / polyhedron from its centre"""
    if dim == 2:
        return float(np.cos(np.pi / n_rays))
    from stardist_amd.rays3d import Rays_GoldenSpiral
    r = Rays_GoldenSpiral(n_rays)
    V, F = np.asarray(r.vertices, np.float64), np.asarray(r.faces)
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    nrm = np.cross(b - a, c - a)
    return float(np.abs((nrm * a).sum(1) / np.linalg.norm(nrm, axis=1)).min())


def hub(dim, m, hub_first, n_rays=None, seed=3, hub_radius=None):
    """one large disc / ball (radius HUB_RADIUS unless given), m small ones inside it, m // 10 outside its bounding box; the small ones
    pairwise disjoint"""
    n_rays = n_rays or (32 if dim == 2 else 96)
    R, r = float(hub_radius or HUB_RADIUS[dim]), SMALL_RADIUS[dim]
    rs, amp = r * (1 + RAY_NOISE), 0.1 if dim == 2 else 0.015
    room = R * (1 - RAY_NOISE) * _inradius(dim, n_rays) - rs - (1.5 if dim == 2 else 0.1) - 2 * amp      # (2D: vertices are truncated to integers)
    if dim == 2:
        pitch = 7.3                                      # integer bounding boxes of neighbours stay apart: 7.3 - 0.1 > 2 * 3.06 + 1
        g = np.arange(-int(R / pitch) - 1, int(R / pitch) + 2) * pitch
        cand = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
        far = np.stack(np.meshgrid(g, R * (1 + RAY_NOISE) + rs + 4 + pitch * np.arange(int(np.ceil((m // 10) / float(len(g)))) + 1), indexing="ij"), -1).reshape(-1, 2)
        sep = pitch - amp
    else:
        a = 4.15 * np.sqrt(2)                            # face-centred cubic, nearest neighbours 4.15 apart: 4.15 - 0.052 > 2 * 2.04
        k = int(R / a) + 2
        g = np.stack(np.meshgrid(*[np.arange(-k, k + 1)] * 3, indexing="ij"), -1).reshape(-1, 3)
        cand = np.concatenate([(g + o) * a for o in ((0, 0, 0), (0, .5, .5), (.5, 0, .5), (.5, .5, 0))])
        far = cand[np.linalg.norm(cand, axis=1) < R] + np.array([0, 0, 2 * R * (1 + RAY_NOISE) + 2 * rs + 4])
        far = far[far[:, 2] - rs > R * (1 + RAY_NOISE) + 1]
        sep = 4.15 - 2 * amp * np.sqrt(3)
    nrm = np.linalg.norm(cand, axis=1)
    inner = cand[np.argsort(nrm, kind="stable")][:m]
    assert len(inner) == m and np.linalg.norm(inner, axis=1).max() <= room, (len(inner), np.linalg.norm(inner, axis=1).max(), room)
    outer = far[np.argsort(np.linalg.norm(far, axis=1), kind="stable")][:m // 10]
    assert len(outer) == m // 10
    pos = np.concatenate([np.zeros((1, dim)), inner, outer])
    n = len(pos)
    small_rank = np.random.RandomState(seed).permutation(n - 1)
    rank = np.concatenate([[0], 1 + small_rank]) if hub_first else np.concatenate([[n - 1], small_rank])
    lab_small = np.concatenate([[-1], np.arange(n - 1)])
    lab_hub = np.concatenate([[0], np.full(m, -1), 1 + np.arange(m // 10) * (dim == 2)])      # (3D: the hub against the outer ones only)
    return _assemble("hub%dd-%d-%s%s" % (dim, m, "first" if hub_first else "last", "-R%g" % R if hub_radius else ""), dim, pos, np.concatenate([[R], np.full(n - 1, r)]), rank,
                     [(0, 1 + k) for k in range(m)], n_rays, seed, amp=amp, edge_dist=None, non_edge_min=sep, big=0,
                     labelings=[lab_small, lab_hub] if dim == 2 else [lab_hub], m=m)


def clique(dim, k, duplicates=0, n_rays=None, seed=4, list_edges=True):
    """k near-coincident candidates (centres within one pixel); `duplicates` of them are exact copies of one candidate.  list_edges=False
    (the cliques of the capacity tests, whose k (k - 1) / 2 edges no list holds): edges is None, keep is the greedy result all the same --
    the best-scored candidate alone"""
    n_rays = n_rays or (32 if dim == 2 else 96)
    rng = np.random.RandomState(seed)
    pos = rng.uniform(0, 0.75, (k, dim))
    copies = []
    if duplicates:
        sel = rng.choice(np.arange(1, k), duplicates, replace=False)
        copies = [(int(sel[0]), int(b)) for b in sel[1:]]
    return _assemble("clique%dd-%d%s" % (dim, k, "-dup%d" % duplicates if duplicates else ""), dim, pos, np.full(k, RADIUS[dim]), _ranks(k, "random", seed),
                     [(a, b) for a in range(k) for b in range(a + 1, k)] if list_edges else None, n_rays, seed, copies=copies,
                     edge_dist=(0.0, 1.0 * np.sqrt(dim)), non_edge_min=None)


def forest(dim, n, n_rays=None, seed=5):
    """n // 3 chains of three candidates and n // 10 isolated ones, each in a cell of its own, the cells shuffled"""
    n_rays = n_rays or (32 if dim == 2 else 96)
    step, r = STEP[dim], RADIUS[dim] * (1 + RAY_NOISE)
    n_ch, n_iso = n // 3, n // 10
    cell = np.array(([2 * r + 3.6] * (dim - 1)) + [2 * step + 2 * r + 3.6])          # (.., y, x): a chain lies along x
    cells = n_ch + n_iso
    side = int(np.ceil((cells * cell[-1] / cell[0]) ** (1.0 / dim)))                 # cells per axis other than x
    nx = int(np.ceil(cells / float(side ** (dim - 1))))
    slots = np.stack(np.unravel_index(np.random.RandomState(seed).permutation(side ** (dim - 1) * nx)[:cells], (side,) * (dim - 1) + (nx,)), 1) * cell
    pos, edges, comp = [], [], []
    for c in range(cells):
        mid = slots[c] + 0.5 * cell - 0.125
        if c < n_ch:
            k0 = len(pos)
            for t in (-1, 0, 1):
                pos.append(mid + np.array([0] * (dim - 1) + [t * step])); comp.append(c)
            edges += [(k0, k0 + 1), (k0 + 1, k0 + 2)]
        else:
            pos.append(mid); comp.append(c)
    pos = np.array(pos)
    return _assemble("forest%dd-%d" % (dim, n), dim, pos, np.full(len(pos), RADIUS[dim]), _ranks(len(pos), "random", seed), edges, n_rays, seed,
                     edge_dist=(step - 0.45, step + 0.45), non_edge_min=2 * step - 0.45, labelings=[np.array(comp)])


# ---- the scenes of the tests: name -> factory (built on demand, cached per process)
_FACTORIES = {}


def _register(dim, f, *a, **kw):
    key = "%s%dd(%s)" % (f.__name__, dim, ",".join([str(v) for v in a] + ["%s=%s" % (k, kw[k]) for k in sorted(kw)]))
    _FACTORIES[key] = (f, (dim,) + a, kw)
    return key


# (1023..1025 in 2D, 255..257 in 3D: the round triage closes its lists per workgroup -- of 1024 resp. 256 candidates: a partial last wave,
# a full last wave, a second workgroup of one candidate)
CHAIN_N_2D = (1, 2, 5, 6, 7, 12, 13, 64, 600, 1023, 1024, 1025, 3000)
CHAIN_N_3D = (3, 40, 255, 256, 257, 400, 520, 3200)

CHAINS_2D = [_register(2, chain, n) for n in CHAIN_N_2D] + \
            [_register(2, chain, n, layout="serpentine") for n in (64, 600)] + \
            [_register(2, chain, 600, n_rays=R) for R in (8, 64)] + \
            [_register(2, chain, n, order="random") for n in (13, 600, 3000)] + \
            [_register(2, chain, 600, order="random", layout="serpentine")] + \
            [_register(2, chain, 600, order="random", n_rays=R) for R in (8, 64)]
HUBS_2D = [_register(2, hub, 2000, True), _register(2, hub, 2000, False)]
OTHERS_2D = [_register(2, ladder, 600), _register(2, clique, 300), _register(2, clique, 300, duplicates=20), _register(2, forest, 6000)]
SCENES_2D = CHAINS_2D + HUBS_2D + OTHERS_2D

CHAINS_3D = [_register(3, chain, n) for n in CHAIN_N_3D] + \
            [_register(3, chain, 400, layout="serpentine"), _register(3, chain, 400, n_rays=32)] + \
            [_register(3, chain, n, order="random") for n in (400, 3200)] + \
            [_register(3, chain, 400, order="random", n_rays=32)]
HUBS_3D = [_register(3, hub, 600, True), _register(3, hub, 600, False)]
OTHERS_3D = [_register(3, ladder, 400), _register(3, clique, 120), _register(3, clique, 120, duplicates=20), _register(3, forest, 1500)]
SCENES_3D = CHAINS_3D + HUBS_3D + OTHERS_3D

# ---- the slot-limit scenes of tests/test_gpu_nms_slot_limits.py: hubs so large that the slot total of the single-pass neighbour lists
# (tests/_nms2d_np.py: slot_capacities, the exact mirror; about n^2, every window covers nearly every cell) reaches the 32-bit limits of
# csrc/nms_rounds.h.  NOT in SCENES_2D: the option sweep over that list would allocate gigabytes per case.  SLOT_TOTALS: the mirrored
# totals, asserted by tests/test_cpu_nms_graph_cases.py.
#   below2d  hub radius 1000, the largest m in steps of 100 whose total stays 5 10^6 below 2^31 - 1: the slots, 8.6 GB of them
#   band2d   hub radius 1000, total in [2^31 + 5 10^6, 2^32 - 10^9]: the two-pass lists by size alone; hub first and hub last
#   wrap2d   hub radius 1300, total T with 10^8 <= T - 2^32 <= 2^31 - 10^8: a 32-bit sum would return T - 2^32, a plausible total
BELOW_2D = _register(2, hub, 44600, True, hub_radius=1000.0)
BAND_2D = [_register(2, hub, 52000, True, hub_radius=1000.0), _register(2, hub, 52000, False, hub_radius=1000.0)]
WRAP_2D = _register(2, hub, 66000, True, hub_radius=1300.0)
SLOT_LIMIT_2D = [BELOW_2D] + BAND_2D + [WRAP_2D]
SLOT_TOTALS = {BELOW_2D: 2138780136, BAND_2D[0]: 2744655308, BAND_2D[1]: 2744655308, WRAP_2D: 4796631484}
SLOT_LIMIT = 2 ** 31 - 1                                 # the slots are used below this total

# the compiled reference (one Qhull thread) takes the 3D scenes up to this many candidates in the CPU test; every 2D scene of SCENES_2D.
# REF_MAX_2D: the largest slot-limit scene it takes, the largest whose call stays within about 5 s on 8 threads; the larger ones are
# checked against the constructed flags only
REF_MAX_3D = 700
REF_MAX_2D = 35000

_BUILT = {}


def scene(key):
    if key not in _BUILT:
        f, a, kw = _FACTORIES[key]
        _BUILT[key] = f(*a, **kw)
    return _BUILT[key]


def is_monotone_chain(key):
    f, a, kw = _FACTORIES[key]
    return f is chain and kw.get("order", "monotone") == "monotone"


def rounds_2d_monotone(n, tail_div=6, tail_max=65536):
    """rounds sd_nms2d needs for a monotone chain, from its host loop: round r promotes the head of the chain and suppresses the next
    candidate, but the undecided count it reads back was taken before that suppression, so n - (2 r - 1) candidates go on to round r + 1;
    the tail batch starts -- never in round 1 -- once at most min(n // tail_div, tail_max) are undecided, and counts as a round"""
    t, nu, r = min(n // tail_div, tail_max), n, 0
    while nu > 0:
        r += 1
        if nu <= t and r > 1:
            break
        nu = max(n - (2 * r - 1), 0)
    return r
