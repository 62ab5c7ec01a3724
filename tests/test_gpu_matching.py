"""GPU: the device matching.  sd_label_overlap_device (csrc/overlap.hip) returns exactly the numpy overlap list (order included, bit-
identical from call to call); matching / matching_dataset on device tensors return the host path's namedtuples (integer fields equal,
float fields bit-identical for thresh > 0); a 16384^2 pair of ~8e5 objects completes with the analytic counts; optimize_thresholds
evaluates the same thresholds with the device matching as with the host's.  The host mirror is pinned to the reference by the CPU suite."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THRESHS = (0.1, 0.3, 0.5, 0.7, 0.9)


def _dev():
    import torch
    return torch.device("cuda:0")


def _up(y):
    import torch
    return torch.from_numpy(np.ascontiguousarray(y)).to(_dev())


def random_discs(shape, n, seed, rmin=3, rmax=10):
    """n discs (balls in 3D) at random centres, painted in id order (later ones cover earlier ones)"""
    rng = np.random.RandomState(seed)
    y = np.zeros(shape, np.int32)
    for i in range(1, n + 1):
        r = rng.randint(rmin, rmax)
        c = [rng.randint(0, s) for s in shape]
        sl = tuple(slice(max(0, ci - r), min(s, ci + r + 1)) for ci, s in zip(c, shape))
        g = np.ogrid[sl]
        m = sum((gi - ci) ** 2 for gi, ci in zip(g, c)) < r * r
        y[sl][m] = i
    return y


def lattice_discs(size, cell, seed):
    """one disc per cell of a size x size image (radius 3..6, centre jittered by 1 px, >= 4 px between discs): (labels, radius per id)"""
    rng = np.random.RandomState(seed)
    k = size // cell - 1
    n = k * k
    rad = rng.randint(3, 7, n)
    cy = (np.arange(n) // k + 1) * cell + rng.randint(-1, 2, n)
    cx = (np.arange(n) % k + 1) * cell + rng.randint(-1, 2, n)
    y = np.zeros((size, size), np.int32)
    for r in range(3, 7):
        dy, dx = np.nonzero(np.add.outer(np.arange(-r, r + 1) ** 2, np.arange(-r, r + 1) ** 2) < r * r)
        ids = np.flatnonzero(rad == r)
        y[(cy[ids, None] + dy - r), (cx[ids, None] + dx - r)] = ids[:, None].astype(np.int32) + 1
    return y, rad


def _same(h, d, exact=True):
    assert h._fields == d._fields
    for key in h._fields:
        u, v = getattr(h, key), getattr(d, key)
        if exact or key in ("tp", "fp", "fn", "n_true", "n_pred", "criterion"):
            assert type(u) == type(v) and u == v, (key, h.thresh, u, v)
        else:
            assert np.isclose(float(u), float(v), rtol=1e-6, atol=0), (key, h.thresh, u, v)


def _check_list(a, b):
    from stardist_amd import matching_sparse as S
    (t, p, c), mm_a, mm_b = S.label_overlap_device(_up(a), _up(b))
    rt, rp, rc = S.sparse_overlap(a, b)
    assert np.array_equal(t, rt) and np.array_equal(p, rp) and np.array_equal(c, rc)
    assert mm_a == (int(a.min()), int(a.max())) and mm_b == (int(b.min()), int(b.max()))
    return t, p, c


@pytest.mark.parametrize("case", ["2d_2048", "3d_128", "background", "identical", "huge_ids", "tiny"])
def test_overlap_list_equals_numpy(case):
    from stardist_amd import matching_sparse as S
    if case == "2d_2048":
        a = random_discs((2048, 2048), 12756, 1)
        b = np.roll(random_discs((2048, 2048), 12756, 1), (2, -3), axis=(0, 1))
        b[::7] = 0
    elif case == "3d_128":
        a = random_discs((128, 128, 128), 3000, 2, rmin=2, rmax=8)
        b = np.roll(a, 1, axis=0)
        b[random_discs((128, 128, 128), 300, 3) > 0] = 4000
    elif case == "background":
        a = b = np.zeros((333, 517), np.int32)
    elif case == "identical":
        a = b = random_discs((257, 1029), 400, 4)
    elif case == "huge_ids":
        a = random_discs((300, 301), 200, 5)
        b = np.roll(a, 3, axis=1)
        a = np.where(a > 0, 2 ** 31 - 1 - a, 0).astype(np.int32)
        b = np.where(b > 0, 2 ** 31 - 2 * b.astype(np.int64), 0).astype(np.int32)
    else:
        a = np.array([[0, 1, 1], [2, 0, 3]], np.int32)
        b = np.array([[1, 1, 0], [2, 2, 0]], np.int32)
    first = _check_list(a, b)
    second = S.label_overlap_device(_up(a), _up(b))[0]
    assert all(np.array_equal(x, y) for x, y in zip(first, second))


def test_overlap_unaligned_inputs_and_negative_labels():
    """views that start off the 16-byte grid take the scalar loads; a negative label leaves the list empty and reports the minimum"""
    from stardist_amd import matching_sparse as S
    a = random_discs((97, 211), 60, 6)
    b = np.roll(a, 2, axis=0)
    ta, tb = _up(a.ravel()), _up(b.ravel())
    (t, p, c), _, _ = S.label_overlap_device(ta[1:], tb[1:])
    rt, rp, rc = S.sparse_overlap(a.ravel()[1:], b.ravel()[1:])
    assert np.array_equal(t, rt) and np.array_equal(p, rp) and np.array_equal(c, rc)
    neg = a.copy()
    neg[5, 5] = -4
    (t, p, c), mm, _ = S.label_overlap_device(_up(neg), _up(b))
    assert len(t) == 0 and mm[0] == -4


def _device_equals_host(y_true, y_pred, threshs=THRESHS, criteria=("iou", "iot", "iop")):
    from stardist_amd import matching as M
    for crit in criteria:
        h = M.matching(y_true, y_pred, thresh=threshs, criterion=crit)
        d = M.matching(_up(y_true), _up(y_pred), thresh=threshs, criterion=crit)
        for a, b in zip(h, d):
            _same(a, b)
        _same(M.matching(y_true, y_pred, thresh=None, criterion=crit), M.matching(y_true, y_pred, thresh=None, criterion=crit, device=_dev()),
              exact=False)


def test_device_matching_shifted_discs():
    """the reference's test_matching.py scenes: a disc image against shifted copies of itself"""
    from stardist_amd import matching as M
    y = random_discs((256, 256), 60, 7, rmin=4, rmax=14)
    for shift in (0, 1, 3, 5, 10, 20):
        y2 = np.roll(y, shift, axis=1)
        _device_equals_host(y, y2, threshs=(0.1, 0.3, 0.5, 0.7, 0.9, 1.0), criteria=("iou",))
        h = M.matching(y, y2, thresh=0.5, report_matches=True)
        assert h == M.matching(_up(y), _up(y2), thresh=0.5, report_matches=True)


def test_device_matching_fixtures_and_model_predictions():
    """fixture masks (uint16 ground truth) against a seeded model's 2D prediction and against perturbed copies of themselves (3D)"""
    import os
    import sys
    import torch
    from stardist_amd.models import Config2D, StarDist2D
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    fx = np.load(os.path.join(root, "tests", "golden", "fixture_images.npz"))
    model = StarDist2D(Config2D(n_rays=32), basedir=None, device=_dev(), seed=0)
    img = torch.from_numpy(fx["img2d"].astype(np.float32) / 255).to(_dev())
    bench.calibrate_heads(model, img)
    labels, _ = model.predict_instances(img)
    assert labels.max() > 0
    _device_equals_host(fx["mask2d"], labels)
    m3 = fx["mask3d"]
    _device_equals_host(m3, np.roll(m3, 1, axis=2).astype(np.int32))
    _device_equals_host(m3, random_discs(m3.shape, 40, 8, rmin=2, rmax=6))


def test_device_matching_dataset_equals_host():
    from stardist_amd import matching as M
    Y = [random_discs((300, 280), 80, s) for s in range(4)]
    P = [np.roll(y, s + 1, axis=s % 2) for s, y in enumerate(Y)]
    for by_image in (False, True):
        h = M.matching_dataset(Y, P, thresh=THRESHS, by_image=by_image, show_progress=False)
        d = M.matching_dataset([_up(y) for y in Y], [_up(p) for p in P], thresh=THRESHS, by_image=by_image, show_progress=False)
        e = M.matching_dataset(Y, P, thresh=THRESHS, by_image=by_image, show_progress=False, parallel=True, device=_dev())
        for a, b, c in zip(h, d, e):
            _same(a, b)
            _same(a, c)


def test_device_matching_errors_and_dtypes():
    import torch
    from stardist_amd import matching as M
    y = random_discs((64, 70), 20, 9)
    p = np.roll(y, 2, axis=0)
    ref = M.matching(y, p, thresh=0.5)
    for dt in (np.uint8, np.uint16, np.int16, np.int64, np.uint32):
        _same(ref, M.matching(y.astype(dt), p, thresh=0.5, device=_dev()))
    _same(ref, M.matching(_up(y.astype(np.int64)), _up(p.astype(np.int16)), thresh=0.5))
    neg = y.copy()
    neg[0, 0] = -1
    for args, msg in [((neg, p), "y_true must be an array of non-negative integers."), ((y, -p), "y_pred must be an array of non-negative integers."),
                      ((y.astype(np.float32), p), "y_true must be an array of non-negative integers."),
                      ((y, p[:10]), "have different shapes")]:
        for conv in (lambda a: a, _up):
            with pytest.raises(ValueError, match=msg):
                M.matching(*map(conv, args), device=_dev())
    with pytest.raises(ValueError, match="not supported"):
        M.matching(_up(y), _up(p), criterion="dice")
    with pytest.raises(ValueError, match="2\\*\\*31"):
        M.matching(_up(y.astype(np.int64) + 2 ** 31), _up(p))
    assert isinstance(M.matching(_up(y), torch.from_numpy(p), thresh=(0.3, 0.5)), tuple)


def test_synthetic_2048_pair_equals_host():
    """the 2048^2 pair of 12 756 discs: device equals host for three thresholds (the host takes seconds, the device milliseconds)"""
    from stardist_amd import matching as M
    a = random_discs((2048, 2048), 12756, 11)
    b = random_discs((2048, 2048), 12756, 11)
    b = np.roll(b, (2, 1), axis=(0, 1))
    b[random_discs((2048, 2048), 2000, 12) > 0] = 0
    h = M.matching(a, b, thresh=[0.3, 0.5, 0.7])
    d = M.matching(_up(a), _up(b), thresh=[0.3, 0.5, 0.7])
    for x, y in zip(h, d):
        _same(x, y)


def test_scale_16384_shifted_copy_analytic():
    """16384^2, ~8e5 discs on a lattice, prediction = the same image shifted by (1, 2): every object matches its own copy, the IoU of a
    disc of radius r with its shifted self is known from the disc alone"""
    import torch
    from stardist_amd import matching as M
    y, rad = lattice_discs(16384, 18, 13)
    n = len(rad)
    assert n > 800000
    t = _up(y)
    p = torch.roll(t, shifts=(1, 2), dims=(0, 1))
    del y
    iou = {}
    for r in range(3, 7):
        d = np.add.outer(np.arange(-r - 3, r + 4) ** 2, np.arange(-r - 3, r + 4) ** 2) < r * r
        c = np.count_nonzero(d & np.roll(d, (1, 2), axis=(0, 1)))
        iou[r] = np.float32(np.float64(c) / np.float64(2 * np.count_nonzero(d) - c))
    res = M.matching(t, p, thresh=[0.3, 0.5, 0.7])
    for s in res:
        tp = int(sum(np.count_nonzero(rad == r) for r in iou if iou[r] >= s.thresh))
        assert (s.n_true, s.n_pred, s.tp, s.fp, s.fn) == (n, n, tp, n - tp, n - tp), (s, tp)
    assert abs(res[0].mean_matched_score - np.mean([iou[r] for r in rad])) < 1e-4


def test_optimize_thresholds_device_equals_host(tmp_path):
    """a seeded 2D model: the device evaluation visits the same thresholds and returns the same (prob, nms) as the host evaluation"""
    import os
    import sys
    import torch
    from stardist_amd.models import Config2D, StarDist2D
    from stardist_amd import utils
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    from oracle import synth
    X = [synth.s2d_nuclei_image(160, 160, seed=s) for s in (1, 2)]
    model = StarDist2D(Config2D(n_rays=32), basedir=None, device=_dev(), seed=0)
    bench.calibrate_heads(model, torch.from_numpy(X[0]).to(_dev()))
    Y = [model.predict_instances(x)[0] for x in X]
    Y = [np.roll(y, 2, axis=1).astype(np.uint16) for y in Y]
    seen = []
    orig = utils.optimize_threshold

    def spy(*args, **kw):
        kw["verbose"] = 2
        return orig(*args, **kw)
    import io
    import contextlib
    runs = []
    for device_eval in (True, False):
        if not device_eval:
            model._labels_device = None                                 # no hook: the host evaluation
        buf = io.StringIO()
        utils.optimize_threshold = spy
        try:
            with contextlib.redirect_stdout(buf):
                out = model.optimize_thresholds(X, Y, nms_threshs=[0.3, 0.5], save_to_json=False)
        finally:
            utils.optimize_threshold = orig
        evals = [line.split("thresh:")[1].split()[0] for line in buf.getvalue().splitlines() if "thresh:" in line and "accuracy" in line]
        runs.append((out, evals, [line.split("accuracy:")[1] for line in buf.getvalue().splitlines() if "accuracy:" in line]))
    del model._labels_device
    assert runs[0][1] == runs[1][1] and len(runs[0][1]) > 4
    assert runs[0][2] == runs[1][2]
    assert runs[0][0] == runs[1][0]
    seen.append(runs)
