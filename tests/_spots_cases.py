"""Cases of the spot tests (tests/test_cpu_spots.py, tests/test_gpu_spots.py): images for gaussian_filter, images and keywords for
peak_local_max, and the definition of peak_local_max as a loop over the pixels (brute_peaks)."""
import numpy as np

DTYPES = (np.uint8, np.uint16, np.float32)


def noise(shape, dtype, seed=0):
    rng = np.random.RandomState(seed)
    if dtype == np.float32:
        return (rng.standard_normal(shape) * 100).astype(np.float32)
    return rng.randint(0, np.iinfo(dtype).max + 1, shape).astype(dtype)


def tie_free(shape, seed=0, smooth=1.5):
    """float32, all values distinct: the rank transform 1 + rank * 0.001 of smoothed noise (smooth=0: of the noise itself)"""
    import scipy.ndimage as ndi
    a = ndi.gaussian_filter(np.random.RandomState(seed).standard_normal(shape), smooth)
    rank = np.argsort(np.argsort(a.ravel(), kind="stable"), kind="stable").reshape(shape)
    out = (1 + rank * 0.001).astype(np.float32)
    assert len(np.unique(out)) == out.size
    return out


# ----------------------------------------------------------------------------- gaussian_filter: (name, image, sigma, truncate)

def gauss_cases():
    cases = []
    for shape, sigma in (((3, 4), 5.0), ((1, 30), 2.0), ((2, 2, 2), 3.0), ((67, 131), (1.0, 2.5)), ((64, 65), (1.0, 2.5)),
                         ((5, 70, 33), (0.7, 1.0, 2.0)), ((9, 3, 129), (0.7, 1.0, 2.0)), ((17, 23), 1.3), ((12, 40), (0.0, 1.5)),
                         ((6, 9, 11), (2.0, 0.0, 0.5)), ((8, 8), 0.0), ((4, 5, 6), (0.0, 0.0, 0.0))):
        for k, dtype in enumerate(DTYPES):
            for truncate in (2.0, 4.0):
                name = "%s-%s-%s-t%g" % ("x".join(map(str, shape)), sigma, np.dtype(dtype).name, truncate)
                cases.append((name, noise(shape, dtype, len(cases)), sigma, truncate))
    return cases


def special_float_images():
    """float32 images with the values a filter can trip on: +-inf and NaN, denormals, the dtype's extremes"""
    a = noise((33, 70), np.float32, 5)
    a[3, 5], a[20, 60], a[10, 10], a[32, 69] = np.inf, -np.inf, np.nan, np.nan
    b = (np.random.RandomState(6).randint(0, 1 << 10, (20, 65)).astype(np.uint32)).view(np.float32)      # denormals, and zeros
    c = noise((9, 66), np.float32, 7) * np.float32(1e36)                                                   # sums that overflow float32
    return {"inf_nan": a, "denormals": b, "huge": c}


# ----------------------------------------------------------------------------- peak_local_max: the definition as a loop

def brute_peaks(img, min_distance=1, threshold_abs=None, threshold_rel=None, exclude_border=True, num_peaks=None, labels=None,
                num_peaks_per_label=None):
    """(coords, values, labels) by the definition of stardist_amd.spots.peak_local_max, one pixel at a time"""
    img = np.asarray(img)
    nd, shape = img.ndim, img.shape
    d = (min_distance,) * nd if np.isscalar(min_distance) else tuple(min_distance)
    if isinstance(exclude_border, bool):
        b = d if exclude_border else (0,) * nd
    else:
        b = (exclude_border,) * nd if np.isscalar(exclude_border) else tuple(exclude_border)
    empty = np.zeros((0, nd), np.int64), np.zeros(0, img.dtype), np.zeros(0, np.int32)
    vf = img.astype(np.float64)
    if not (~np.isnan(vf)).any():
        return empty
    thr = np.nanmin(vf) if threshold_abs is None else np.float64(threshold_abs)
    if threshold_rel is not None:
        thr = max(thr, np.float64(threshold_rel) * np.nanmax(vf))
    index = np.arange(img.size).reshape(shape)
    found = []
    for p in np.ndindex(shape):
        v = vf[p]
        if not v > thr:
            continue
        if any(not (w <= c < n - w) for c, n, w in zip(p, shape, b)):
            continue
        if labels is not None and labels[p] == 0:
            continue
        box = tuple(slice(max(c - k, 0), min(c + k + 1, n)) for c, k, n in zip(p, d, shape))
        rivals = np.ones(vf[box].shape, bool) if labels is None else labels[box] == labels[p]
        if (rivals & ((vf[box] > v) | ((vf[box] == v) & (index[box] < index[p])))).any():
            continue
        found.append((-v, int(index[p]), p))
    found.sort(key=lambda t: t[:2])
    if num_peaks_per_label is not None and labels is not None:
        seen, kept = {}, []
        for t in found:
            seen[int(labels[t[2]])] = seen.get(int(labels[t[2]]), 0) + 1
            if seen[int(labels[t[2]])] <= num_peaks_per_label:
                kept.append(t)
        found = kept
    if num_peaks is not None:
        found = found[:num_peaks]
    if not found:
        return empty
    coords = np.asarray([t[2] for t in found], np.int64).reshape(-1, nd)
    where = tuple(coords.T)
    return coords, img[where], (np.zeros(len(coords), np.int32) if labels is None else labels[where].astype(np.int32))


def _pair(shape, first, second, value=1.0, dtype=np.float32):
    a = np.zeros(shape, dtype)
    a[first] = a[second] = value
    return a


def peak_cases():
    """name -> (image, keywords): every mechanism of the definition and of the device pass (tiles are 16 x 64 pixels, 3D 4 x 4 x 64;
    the halo of a 2D window lives in LDS up to min_distance 36)"""
    C = {}
    const = np.full((20, 70), 3.0, np.float32)
    C["constant"] = (const, {})
    C["constant_low_threshold"] = (const, dict(threshold_abs=2.5, exclude_border=False))
    for d in (1, 2, 5):
        for gap in (d, d + 1):
            h = gap // 2
            kw = dict(min_distance=d, exclude_border=False)
            C["pair_d%d_gap%d_inside" % (d, gap)] = (_pair((40, 150), (5, 5), (5, 5 + gap)), kw)
            C["pair_d%d_gap%d_x_edge" % (d, gap)] = (_pair((40, 150), (5, 63 - h), (5, 63 - h + gap)), kw)
            C["pair_d%d_gap%d_y_edge" % (d, gap)] = (_pair((40, 150), (15 - h, 20), (15 - h + gap, 20)), kw)
            C["pair_d%d_gap%d_corner" % (d, gap)] = (_pair((40, 150), (15 - h, 63 - h), (15 - h + gap, 63 - h + gap)), kw)
            C["pair_d%d_gap%d_anti" % (d, gap)] = (_pair((40, 150), (15 - h, 63 - h + gap), (15 - h + gap, 63 - h)), kw)
            C["pair_d%d_gap%d_z_edge" % (d, gap)] = (_pair((12, 10, 70), (3 - h, 3, 63 - h), (3 - h + gap, 3, 63 - h + gap)), kw)
            C["pair_d%d_gap%d_zy" % (d, gap)] = (_pair((12, 10, 70), (5, 3 - h, 7), (5, 3 - h + gap, 7)), kw)
    ramp = np.arange(18 * 67, dtype=np.float32).reshape(18, 67)
    C["ramp_no_border"] = (ramp, dict(exclude_border=False))
    C["ramp"] = (ramp, {})
    C["ramp_3d"] = (np.arange(5 * 6 * 66, dtype=np.float32).reshape(5, 6, 66), dict(exclude_border=False, min_distance=2))
    bumps = np.zeros((30, 80), np.float32)
    bumps[5, 5], bumps[10, 70], bumps[20, 30], bumps[25, 66] = 4.0, 2.0, 1.0, 0.5
    C["value_equals_threshold"] = (bumps, dict(threshold_abs=2.0))
    C["abs_and_rel_abs_wins"] = (bumps, dict(threshold_abs=1.5, threshold_rel=0.2))
    C["abs_and_rel_rel_wins"] = (bumps, dict(threshold_abs=0.25, threshold_rel=0.25))
    C["rel_equals_value"] = (bumps, dict(threshold_rel=0.5))
    zeros = np.full((10, 70), -1.0, np.float32)
    zeros[4, 10], zeros[4, 11], zeros[7, 63], zeros[7, 64] = -0.0, 0.0, 0.0, -0.0
    C["signed_zeros"] = (zeros, dict(exclude_border=False))
    nans = noise((20, 70), np.float32, 11)
    nans[::3, ::2] = np.nan
    nans[10, 33] = 1e6
    nans[9:12, 32:35][np.arange(9).reshape(3, 3) != 4] = np.nan
    C["nan_neighbours"] = (nans, {})
    C["all_nan"] = (np.full((5, 9), np.nan, np.float32), dict(exclude_border=False))
    C["all_nan_threshold"] = (np.full((5, 9), np.nan, np.float32), dict(exclude_border=False, threshold_abs=-1.0))
    inf = noise((20, 70), np.float32, 12)
    inf[5, 5], inf[5, 6], inf[15, 64], inf[2, 2] = np.inf, np.inf, np.inf, -np.inf
    C["inf"] = (inf, {})
    C["inf_rel"] = (inf, dict(threshold_rel=0.5))
    u16 = noise((33, 70), np.uint16, 13)
    u16[7, 7], u16[7, 8], u16[20, 65] = 65535, 65535, 65535
    C["uint16_max"] = (u16, {})
    C["uint8_noise"] = (noise((40, 90), np.uint8, 14), dict(min_distance=2))
    C["uint8_noise_3d"] = (noise((9, 10, 70), np.uint8, 15), {})
    smooth = tie_free((34, 75), 16)
    for name, border in (("true", True), ("false", False), ("zero", 0), ("int", 3), ("tuple", (2, 7)), ("half", 17), ("beyond", (40, 0))):
        C["border_" + name] = (smooth, dict(min_distance=2, exclude_border=border))
    C["distance_1_3"] = (smooth, dict(min_distance=(1, 3)))
    C["distance_0"] = (smooth, dict(min_distance=0, threshold_rel=0.99))
    C["distance_0_uint8"] = (noise((20, 70), np.uint8, 17), dict(min_distance=0, threshold_abs=250))
    C["distance_0_2_1"] = (tie_free((7, 9, 70), 18), dict(min_distance=(0, 2, 1)))
    C["distance_3d"] = (tie_free((9, 11, 67), 19), dict(min_distance=2, num_peaks=7))
    C["distance_beyond_extent"] = (smooth, dict(min_distance=500, exclude_border=False))
    wide = tie_free((70, 140), 20)
    C["lds_tier_last"] = (wide, dict(min_distance=36, exclude_border=False))
    C["lds_tier_beyond"] = (wide, dict(min_distance=37, exclude_border=False))
    C["lds_tier_beyond_tied"] = (noise((70, 140), np.uint8, 21), dict(min_distance=37, exclude_border=3))
    C["num_peaks"] = (smooth, dict(num_peaks=4))
    C["num_peaks_0"] = (smooth, dict(num_peaks=0))
    # labels
    touch = np.zeros((20, 70), np.float32)
    touch[10, 30], touch[10, 31] = 5.0, 6.0
    lab = np.zeros((20, 70), np.int64)
    lab[5:15, 20:31], lab[5:15, 31:40] = 1, 2
    C["labels_touching"] = (touch, dict(labels=lab, exclude_border=False))
    img = tie_free((40, 90), 22)
    ids = np.zeros((40, 90), np.int64)
    ids[2:18, 3:40], ids[2:18, 40:88], ids[20:38, 5:50], ids[20:38, 60:85], ids[25:30, 65:70] = 1, 2 ** 31 - 1, 70000, 12, 5
    C["labels_sparse_ids"] = (img, dict(labels=ids, exclude_border=False))
    C["labels_int32"] = (img, dict(labels=np.minimum(ids, 9).astype(np.int32), min_distance=2))
    C["labels_per_label"] = (img, dict(labels=ids, exclude_border=False, num_peaks_per_label=2))
    C["labels_per_label_0"] = (img, dict(labels=ids, exclude_border=False, num_peaks_per_label=0))
    C["labels_num_peaks"] = (img, dict(labels=ids, exclude_border=False, num_peaks_per_label=3, num_peaks=7))
    C["labels_below_threshold"] = (img, dict(labels=ids, exclude_border=False, threshold_abs=float(img[25:30, 65:70].max())))
    C["labels_uint8_tied"] = (noise((40, 90), np.uint8, 23), dict(labels=ids, min_distance=2, num_peaks_per_label=5))
    ids3 = np.zeros((9, 11, 67), np.int32)
    ids3[1:8, 1:6, 2:40], ids3[1:8, 6:10, 2:66] = 4, 9
    C["labels_3d"] = (tie_free((9, 11, 67), 24), dict(labels=ids3, exclude_border=False, num_peaks_per_label=3))
    return C


# ----------------------------------------------------------------------------- scenes: nuclei as discs / balls, foci as planted blobs

def scene(shape, dtype=np.uint16, seed=0, spots=60):
    """(image, labels): discs (balls) of distinct ids on a jittered lattice, and an image of noise plus small Gaussian blobs at random
    places, some inside an object, some on the background"""
    rng = np.random.RandomState(seed)
    nd = len(shape)
    grid = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), axis=-1).astype(np.float64)
    labels = np.zeros(shape, np.int32)
    pitch = 28 if nd == 2 else 14
    centres = np.stack(np.meshgrid(*[np.arange(pitch // 2, n, pitch) for n in shape], indexing="ij"), axis=-1).reshape(-1, nd)
    for k, c in enumerate(centres + rng.randint(-3, 4, centres.shape)):
        labels[((grid - c) ** 2).sum(-1) <= (pitch * 0.36) ** 2] = k + 1
    img = rng.standard_normal(shape) * 4 + 100
    for c in rng.rand(spots, nd) * (np.asarray(shape) - 1):
        img += rng.uniform(60, 200) * np.exp(-((grid - c) ** 2).sum(-1) / (2 * 1.5 ** 2))
    return (img.astype(np.float32) if dtype == np.float32 else np.clip(np.rint(img), 0, np.iinfo(dtype).max).astype(dtype)), labels
