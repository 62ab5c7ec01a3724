"""GPU: the routing table of the label-image functions for real, on the rows tests/test_cpu_label_routes.py
cannot reach.  Every function is called with a device tensor, with a numpy array and device="cuda", with a host tensor and device="cuda"
and with a device tensor of a dtype its kernels do not take; on a 6 x 7 image and a 3 x 6 x 7 volume with two touching objects, one of
them with a one-pixel hole, and on copies of both whose ids are about 2^40 (the compaction of _route._device_labels); the relabel
functions, which refuse to compact and go through their host function instead, get ids of about 10^6, the most that host function
can take (scipy's find_objects keeps one slot per id).  Asserted, exactly: the result equals the host route's (the function on the numpy
array without device=), is of the kind and dtype the host route's result has for that input, and lives where PLACE, the table of section
3p written out, says.  These are the smallest shapes at which a wrong upload, a wrong (Z, Y, X), a lost id map or a result on the wrong
device shows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FUNCTIONS = ("fill_label_holes", "calculate_extents", "measure_labels", "measure_labels uint16", "measure_labels float32",
             "label_components", "expand_labels", "distance_transform", "relabel_image_stardist", "relabel_image_stardist3D")
CALLS = ("device tensor", "numpy + device", "host tensor + device", "unsupported dtype")
# where the result lives: "input" = a tensor where the input tensor lives, "device" = a tensor on the device `device=` names, "numpy"
PLACE = {
    "fill_label_holes": {"device tensor": "input", "numpy + device": "numpy", "host tensor + device": "input", "unsupported dtype": "input"},
    "calculate_extents": {"device tensor": "numpy", "unsupported dtype": "numpy"},                          # it has no device=
    "measure_labels": {"device tensor": "numpy", "numpy + device": "numpy", "host tensor + device": "numpy", "unsupported dtype": "numpy"},
    "label_components": {"device tensor": "input", "numpy + device": "numpy", "host tensor + device": "device", "unsupported dtype": "input"},
    "expand_labels": {"device tensor": "input", "numpy + device": "numpy", "host tensor + device": "device", "unsupported dtype": "input"},
    "distance_transform": {"device tensor": "input", "numpy + device": "numpy", "host tensor + device": "device", "unsupported dtype": "input"},
    "relabel_image_stardist": {"device tensor": "input", "numpy + device": "numpy", "host tensor + device": "device"},
    "relabel_image_stardist3D": {"device tensor": "input", "numpy + device": "numpy", "host tensor + device": "device"},
}
# the dtype of the fourth call: none of the function's kernels takes it (distance_transform takes every dtype: float32 is no label dtype)
SUPPORTED = {"label_components": "int32"}                                 # of the other three calls; int64 elsewhere, and for huge ids
UNSUPPORTED = {"fill_label_holes": "uint16", "calculate_extents": "uint16", "measure_labels": "uint16", "label_components": "int64",
               "expand_labels": "float32", "distance_transform": "float32"}


HUGE = np.array([0, 2 ** 40 + 5, 2 ** 40 + 9])                             # the huge ids of objects 1 and 2, in the same order


def image(nd, huge, name=""):
    a = np.zeros((6, 7), np.int64)
    a[1:5, 1:5], a[1:5, 5:7], a[3, 2] = 1, 2, 0
    if nd == 3:
        a = np.stack([a, a, a])
        a[0, 3, 2] = a[2, 3, 2] = 1                                         # the hole is closed along z too
    if huge:
        a = HUGE[a] if not name.startswith("relabel") else np.where(a > 0, a + 10 ** 6, 0)
    return a


def intensity(shape, dtype):
    return ((np.arange(int(np.prod(shape))).reshape(shape) * 37) % 251).astype(dtype)      # whole numbers: every float sum is exact


def run(name, x, nd, **dev):
    from stardist_amd import utils
    from stardist_amd.geometry import relabel_image_stardist, relabel_image_stardist3D
    from stardist_amd.rays3d import Rays_GoldenSpiral
    if name.startswith("measure_labels"):
        img = intensity(tuple(x.shape), name.split()[1]) if " " in name else None
        return utils.measure_labels(x, img, **dev)
    if name == "calculate_extents":
        return utils.calculate_extents(x)
    if name == "distance_transform":
        return utils.distance_transform(x, (1.5, 1.0, 0.5)[3 - nd:], return_indices=True, **dev)
    if name == "expand_labels":
        return utils.expand_labels(x, 1.5, (1.5, 1.0, 0.5)[3 - nd:], **dev)
    if name == "relabel_image_stardist":
        return relabel_image_stardist(x, 8, **dev)
    if name == "relabel_image_stardist3D":
        return relabel_image_stardist3D(x, Rays_GoldenSpiral(8), **dev)
    return getattr(utils, name)(x, **dev)


def parts(result):
    """the arrays of a result, in a fixed order"""
    if isinstance(result, dict):
        return [result[k] for k in sorted(result)]
    return list(result) if isinstance(result, tuple) else [result]


_HOST = {}


def host(name, nd, huge, dtype):
    """the host route's result for this input, computed once"""
    key = (name, nd, huge, dtype)
    if key not in _HOST and huge and name in ("fill_label_holes", "calculate_extents"):
        # their host code cannot take such ids (find_objects): the result on the small ids, renamed in the same ascending order
        small = host(name, nd, False, dtype)
        _HOST[key] = HUGE[small] if name == "fill_label_holes" else small
    if key not in _HOST:
        _HOST[key] = run(name, image(nd, huge, name).astype(dtype), nd)
    return _HOST[key]


def check(torch, name, nd, huge, call, device="cuda:0"):
    fn = name.split()[0]
    if nd != (3 if fn == "relabel_image_stardist3D" else 2) and fn.startswith("relabel"):
        return 0
    if call not in PLACE[fn]:
        return 0
    dtype = UNSUPPORTED[fn] if call == "unsupported dtype" else ("int64" if huge else SUPPORTED.get(fn, "int64"))
    if call == "unsupported dtype" and huge:
        return 0                                                            # ids of 2^40 need int64
    a = image(nd, huge, name).astype(dtype)
    want = host(name, nd, huge, dtype)
    if call == "numpy + device":
        x, got = a, run(name, a.copy(), nd, device=device)
    elif call == "host tensor + device":
        x = torch.from_numpy(a.copy())
        got = run(name, x, nd, device=device)
    else:
        x = torch.as_tensor(a.copy(), device=device)
        got = run(name, x, nd)
    place = PLACE[fn][call]
    if fn.startswith("relabel") and huge and call == "host tensor + device":
        place = "input"                                                     # section 3p, exception 8: through the host function, not moved
    assert len(parts(got)) == len(parts(want)), (name, nd, huge, call)
    for g, w in zip(parts(got), parts(want)):
        what = (name, nd, huge, call)
        if place == "numpy":
            assert isinstance(g, np.ndarray) and g.dtype == w.dtype, what
            value = g
        else:
            assert isinstance(g, torch.Tensor) and str(g.dtype) == "torch." + w.dtype.name, what
            assert g.device == (x.device if place == "input" else torch.device(device)), what
            value = g.cpu().numpy()
        assert value.shape == w.shape and np.array_equal(value, w, equal_nan=True), what
    return 1


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.mark.parametrize("name", FUNCTIONS)
def test_route_value_kind_and_place(torch, name):
    done = sum(check(torch, name, nd, huge, call) for nd in (2, 3) for huge in (False, True) for call in CALLS)
    fn = name.split()[0]
    assert done == (2 if fn.startswith("relabel") else 4) * len(PLACE[fn]) - (0 if fn not in UNSUPPORTED else 2)


def test_the_host_results_have_objects_and_a_filled_hole():
    for nd in (2, 3):
        a = image(nd, False)
        filled = host("fill_label_holes", nd, False, "int64")
        assert (filled != a).sum() == 1 and filled.dtype == np.int64
        assert host("measure_labels uint16", nd, False, "int64")["label"].tolist() == [1, 2]
        assert host("measure_labels", nd, True, "int64")["label"].tolist() == [2 ** 40 + 5, 2 ** 40 + 9]
        assert host("label_components", nd, False, "int32").max() == 2      # the hole is background
        assert (host("expand_labels", nd, True, "int64") == 2 ** 40 + 5).sum() > (a == 1).sum()
    assert set(np.unique(host("relabel_image_stardist", 2, False, "int64"))) == {0, 1, 2}
    assert set(np.unique(host("relabel_image_stardist3D", 3, False, "int64"))) >= {1, 2}


@pytest.mark.parametrize("dtype", ["float32", "int32"])
def test_relabel_refuses_a_dtype_it_does_not_take_on_the_device_too(torch, dtype):
    from stardist_amd.geometry import relabel_image_stardist
    bad = torch.as_tensor(image(2, False).astype(dtype), device="cuda") * (1 if dtype == "float32" else -1)
    with pytest.raises(ValueError, match="non-negative integers"):
        relabel_image_stardist(bad, 8)


def test_a_tensor_on_the_second_device_is_processed_and_returned_there(torch):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    for name in FUNCTIONS:
        for nd in (2, 3):
            check(torch, name, nd, False, "device tensor", device="cuda:1")
            check(torch, name, nd, True, "device tensor", device="cuda:1")
            check(torch, name, nd, False, "host tensor + device", device="cuda:1")
