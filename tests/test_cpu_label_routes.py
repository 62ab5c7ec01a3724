"""CPU: the routing table of the label-image functions, pinned: for every row of a written-out matrix of
(function, input kind, dtype, number of axes, device=, variant) which half ran and with what, and what came back.

The device halves (`_X_device`, and the relabel functions' `_star_representation_device`) are replaced by fakes that record (function,
input kind, dtype, shape, device argument) and return a stand-in a caller can recognise; the relabel functions' host natives are replaced
by recorders too, so every row runs without a device.  An outcome is (calls, result): `calls` what the fakes recorded, `result` the kind,
dtype and place of what the public function returned -- a string where a device half's stand-in came back as it was -- or the name of the
exception.  A ValueError row asserts besides that nothing had run.  TABLE is literal data: it was produced by `outcome` on the commit
before the functions moved out of stardist_amd.utils (with PATCHED naming that module) and must not follow the code.

Rows that need a device (a device tensor in; a host tensor that `device=` moves; the relabel functions' upload, which happens before
their seam) are in tests/test_gpu_label_routes.py."""
import importlib

import numpy as np
import pytest

PATCHED = "stardist_amd.label_ops"                                         # the module whose device halves the fakes replace

BASE = np.array([[0, 1, 1, 0], [0, 1, 2, 2], [0, 0, 2, 0]])                # (3, 4); the volume is two such planes, (2, 3, 4)


def make(kind, dtype, nd, variant):
    a = BASE if nd == 2 else (np.stack([BASE, BASE]) if nd == 3 else (BASE[0] if nd == 1 else np.stack([BASE, BASE])[None]))
    if variant == "negative":
        a = np.where(a == 2, -2, a)
    if variant == "sparse":                                                # an id that would be compacted: 10 ** 6 > 4 * size + 1024
        a = np.where(a == 2, 10 ** 6, a)
    a = (a != 0) if dtype == "bool" else a.astype(dtype)
    if kind == "list":
        return a.tolist()
    if kind == "tensor":
        import torch
        return torch.from_numpy(a.copy())
    return a


def kind_of(x):
    return "numpy" if isinstance(x, np.ndarray) else ("tensor" if type(x).__module__.startswith("torch") else type(x).__name__)


def describe(x):
    """kind, dtype and place of a result"""
    if x is None or isinstance(x, str):
        return x
    if isinstance(x, (tuple, list)):
        return tuple(describe(v) for v in x)
    if isinstance(x, dict):
        return ("dict",) + tuple(describe(x[k]) for k in ("label", "min_intensity") if k in x)
    if isinstance(x, np.ndarray):
        return ("numpy", x.dtype.name)
    if type(x).__module__.startswith("torch"):
        return ("tensor", str(x.dtype)[6:], x.device.type)
    return (type(x).__name__, x)


class Fakes:
    """the halves' stand-ins; `calls` is what they recorded"""

    def __init__(self, monkeypatch):
        import torch
        from stardist_amd.geometry import geom2d, geom3d
        self.calls = []
        mod = importlib.import_module(PATCHED)
        note = lambda fn, x, device: self.calls.append((fn, kind_of(x), str(x.dtype).replace("torch.", ""), tuple(x.shape), device))

        def fill(lbl_img, device=None):
            note("fill_label_holes", lbl_img, device)
            return "filled on the device"

        def boxes(t):
            note("calculate_extents", t, None)
            return np.array([[5, 7]])

        def measure(lbl, img, C, device):
            note("measure_labels", lbl, device)
            if img is not None:
                note("measure_labels image", img, device)
            raw = {"label": torch.tensor([77]), "area": torch.tensor([3]), "bbox": torch.zeros((1, 2 * lbl.ndim), dtype=torch.int64),
                   "csum": torch.zeros((1, lbl.ndim), dtype=torch.int64)}
            if img is not None:
                raw.update(sum=torch.zeros((1, C), dtype=torch.int64), sum2=torch.zeros((1, C), dtype=torch.int64),
                           min=torch.zeros((1, C), dtype=torch.int64), max=torch.zeros((1, C), dtype=torch.int64))
            return raw

        def components(img, connectivity, background, device):
            note("label_components", img, device)
            return torch.full(tuple(img.shape), 7, dtype=torch.int32), torch.tensor(3, dtype=torch.int32)

        def expand(lbl, distance, szyx, device):
            note("expand_labels", lbl, device)
            return "expanded on the device"

        def transform(img, szyx, max_distance, return_distances, return_indices, device):
            note("distance_transform", img, device)
            return (torch.full(tuple(img.shape), 2.5, dtype=torch.float64) if return_distances else None,
                    torch.zeros((len(img.shape),) + tuple(img.shape), dtype=torch.int32) if return_indices else None)

        def star_device(img, rays):
            note("relabel device", img, None)
            raise RuntimeError("the relabel functions' device half needs a device")

        def star_dist(lbl, n_rays, **kw):
            note("relabel_image_stardist host", lbl, None)
            return np.ones(tuple(lbl.shape) + (n_rays,), np.float32)

        def star_dist3D(lbl, rays, **kw):
            note("relabel_image_stardist3D host", lbl, None)
            return np.ones(tuple(lbl.shape) + (len(rays),), np.float32)

        for name, fn in (("_fill_label_holes_device", fill), ("_label_boxes_device", boxes), ("_measure_raw_device", measure),
                         ("_label_components_device", components), ("_expand_labels_device", expand),
                         ("_distance_transform_device", transform)):
            assert callable(getattr(mod, name))
            monkeypatch.setattr(mod, name, fn)
        monkeypatch.setattr(geom2d, "_star_representation_device", star_device)
        monkeypatch.setattr(geom2d, "star_dist", star_dist)
        monkeypatch.setattr(geom2d, "polygons_to_label", lambda dist, points, shape: np.zeros(shape, np.int32))
        monkeypatch.setattr(geom3d, "star_dist3D", star_dist3D)
        monkeypatch.setattr(geom3d, "polyhedron_to_label", lambda dist, points, rays, shape, labels=None, verbose=False: np.zeros(shape, np.uint16))


def call(function, x, device, variant):
    from stardist_amd import utils
    from stardist_amd.geometry import relabel_image_stardist, relabel_image_stardist3D
    dev = {} if device == "absent" else {"device": device}
    if function == "fill_label_holes":
        return utils.fill_label_holes(x, **dev, **({"structure": np.ones((3,) * np.ndim(x))} if variant == "kwargs" else {}))
    if function == "calculate_extents":
        return utils.calculate_extents([np.asarray(x), np.asarray(x)] if variant == "sequence" else x)
    if function == "measure_labels":
        img = None
        if variant.startswith("img:"):
            img = np.ones(np.shape(x) + ((2,) if variant.endswith("+c") else ()), variant[4:].replace("+c", ""))
        return utils.measure_labels(x, img, as_tensors=variant == "as_tensors", **dev)
    if function == "label_components":
        return utils.label_components(x, background=0.5 if variant == "background 0.5" else 0, return_num=variant == "return_num", **dev)
    if function == "expand_labels":
        return utils.expand_labels(x, 0 if variant == "distance 0" else 2, (1.0, np.nan) if variant == "bad spacing" else 1, **dev)
    if function == "distance_transform":
        return utils.distance_transform(x, return_indices=variant == "indices", max_distance=-1.0 if variant == "bad bound" else None, **dev)
    if function == "relabel_image_stardist":
        return relabel_image_stardist(x, 8, **dev, **({"grid": (1, 1)} if variant == "kwargs" else {}))
    if function == "relabel_image_stardist3D":
        from stardist_amd.rays3d import Rays_GoldenSpiral
        return relabel_image_stardist3D(x, Rays_GoldenSpiral(8), **dev, **({"grid": (1, 1, 1)} if variant == "kwargs" else {}))
    raise KeyError(function)


def outcome(row, monkeypatch):
    function, kind, dtype, nd, device, variant = row
    fakes = Fakes(monkeypatch)
    x = make(kind, dtype, nd, variant)
    try:
        result = describe(call(function, x, device, variant))
    except ValueError:
        result = "ValueError"
    return tuple(fakes.calls), result


# (function, input kind, dtype, axes, device=, variant), (what the fakes recorded, what came back)
TABLE = [
    (('fill_label_holes', 'numpy', 'uint8', 2, None, ''), ((), ('numpy', 'uint8'))),
    (('fill_label_holes', 'numpy', 'uint8', 2, 'cuda', ''), ((('fill_label_holes', 'numpy', 'uint8', (3, 4), 'cuda'),), 'filled on the device')),
    (('fill_label_holes', 'tensor', 'uint8', 2, None, ''), ((), ('tensor', 'uint8', 'cpu'))),
    (('fill_label_holes', 'tensor', 'uint8', 2, 'cuda', ''), ((('fill_label_holes', 'tensor', 'uint8', (3, 4), 'cuda'),), 'filled on the device')),
    (('fill_label_holes', 'numpy', 'int8', 2, None, ''), ((), ('numpy', 'int8'))),
    (('fill_label_holes', 'numpy', 'int8', 2, 'cuda', ''), ((('fill_label_holes', 'numpy', 'int8', (3, 4), 'cuda'),), 'filled on the device')),
    (('fill_label_holes', 'tensor', 'int8', 2, None, ''), ((), ('tensor', 'int8', 'cpu'))),
    (('fill_label_holes', 'tensor', 'int8', 2, 'cuda', ''), ((('fill_label_holes', 'tensor', 'int8', (3, 4), 'cuda'),), 'filled on the device')),
    (('fill_label_holes', 'numpy', 'uint16', 2, None, ''), ((), ('numpy', 'uint16'))),
    (('fill_label_holes', 'numpy', 'uint16', 2, 'cuda', ''), ((('fill_label_holes', 'numpy', 'uint16', (3, 4), 'cuda'),), 'filled on the device')),
    (('fill_label_holes', 'tensor', 'uint16', 2, None, ''), ((), ('tensor', 'uint16', 'cpu'))),
    (('fill_label_holes', 'tensor', 'uint16', 2, 'cuda', ''), ((), ('tensor', 'uint16', 'cpu'))),
    (('fill_label_holes', 'numpy', 'int16', 2, None, ''), ((), ('numpy', 'int16'))),
    (('fill_label_holes', 'numpy', 'int16', 2, 'cuda', ''), ((('fill_label_holes', 'numpy', 'int16', (3, 4), 'cuda'),), 'filled on the device')),
    (('fill_label_holes', 'tensor', 'int16', 2, None, ''), ((), ('tensor', 'int16', 'cpu'))),
    (('fill_label_holes', 'tensor', 'int16', 2, 'cuda', ''), ((('fill_label_holes', 'tensor', 'int16', (3, 4), 'cuda'),), 'filled on the device')),
    (('fill_label_holes', 'numpy', 'int32', 2, None, ''), ((), ('numpy', 'int32'))),
    (('fill_label_holes', 'numpy', 'int32', 2, 'cuda', ''), ((('fill_label_holes', 'numpy', 'int32', (3, 4), 'cuda'),), 'filled on the device')),
    (('fill_label_holes', 'tensor', 'int32', 2, None, ''), ((), ('tensor', 'int32', 'cpu'))),
    (('fill_label_holes', 'tensor', 'int32', 2, 'cuda', ''), ((('fill_label_holes', 'tensor', 'int32', (3, 4), 'cuda'),), 'filled on the device')),
    (('fill_label_holes', 'numpy', 'int64', 2, None, ''), ((), ('numpy', 'int64'))),
    (('fill_label_holes', 'numpy', 'int64', 2, 'cuda', ''), ((('fill_label_holes', 'numpy', 'int64', (3, 4), 'cuda'),), 'filled on the device')),
    (('fill_label_holes', 'list', 'int64', 2, None, ''), ((), ('numpy', 'int64'))),
    (('fill_label_holes', 'list', 'int64', 2, 'cuda', ''), ((('fill_label_holes', 'numpy', 'int64', (3, 4), 'cuda'),), 'filled on the device')),
    (('fill_label_holes', 'tensor', 'int64', 2, None, ''), ((), ('tensor', 'int64', 'cpu'))),
    (('fill_label_holes', 'tensor', 'int64', 2, 'cuda', ''), ((('fill_label_holes', 'tensor', 'int64', (3, 4), 'cuda'),), 'filled on the device')),
    (('fill_label_holes', 'numpy', 'bool', 2, None, ''), ((), ('numpy', 'bool'))),
    (('fill_label_holes', 'numpy', 'bool', 2, 'cuda', ''), ((), ('numpy', 'bool'))),
    (('fill_label_holes', 'list', 'bool', 2, None, ''), ((), ('numpy', 'bool'))),
    (('fill_label_holes', 'list', 'bool', 2, 'cuda', ''), ((), ('numpy', 'bool'))),
    (('fill_label_holes', 'tensor', 'bool', 2, None, ''), ((), ('tensor', 'bool', 'cpu'))),
    (('fill_label_holes', 'tensor', 'bool', 2, 'cuda', ''), ((), ('tensor', 'bool', 'cpu'))),
    (('fill_label_holes', 'numpy', 'int64', 3, None, ''), ((), ('numpy', 'int64'))),
    (('fill_label_holes', 'numpy', 'int64', 3, 'cuda', ''), ((('fill_label_holes', 'numpy', 'int64', (2, 3, 4), 'cuda'),), 'filled on the device')),
    (('fill_label_holes', 'list', 'int64', 3, None, ''), ((), ('numpy', 'int64'))),
    (('fill_label_holes', 'list', 'int64', 3, 'cuda', ''), ((('fill_label_holes', 'numpy', 'int64', (2, 3, 4), 'cuda'),), 'filled on the device')),
    (('fill_label_holes', 'tensor', 'int64', 3, None, ''), ((), ('tensor', 'int64', 'cpu'))),
    (('fill_label_holes', 'tensor', 'int64', 3, 'cuda', ''), ((('fill_label_holes', 'tensor', 'int64', (2, 3, 4), 'cuda'),), 'filled on the device')),
    (('fill_label_holes', 'numpy', 'int64', 2, None, 'kwargs'), ((), ('numpy', 'int64'))),
    (('fill_label_holes', 'numpy', 'int64', 2, 'cuda', 'kwargs'), ((), ('numpy', 'int64'))),
    (('fill_label_holes', 'list', 'int64', 2, None, 'kwargs'), ((), ('numpy', 'int64'))),
    (('fill_label_holes', 'list', 'int64', 2, 'cuda', 'kwargs'), ((), ('numpy', 'int64'))),
    (('fill_label_holes', 'tensor', 'int64', 2, None, 'kwargs'), ((), ('tensor', 'int64', 'cpu'))),
    (('fill_label_holes', 'tensor', 'int64', 2, 'cuda', 'kwargs'), ((), ('tensor', 'int64', 'cpu'))),
    (('calculate_extents', 'numpy', 'int32', 1, 'absent', ''), ((), 'ValueError')),
    (('calculate_extents', 'numpy', 'uint8', 1, 'absent', ''), ((), 'ValueError')),
    (('calculate_extents', 'numpy', 'int32', 2, 'absent', ''), ((), ('numpy', 'float64'))),
    (('calculate_extents', 'numpy', 'uint8', 2, 'absent', ''), ((), ('numpy', 'float64'))),
    (('calculate_extents', 'numpy', 'int32', 3, 'absent', ''), ((), ('numpy', 'float64'))),
    (('calculate_extents', 'numpy', 'uint8', 3, 'absent', ''), ((), ('numpy', 'float64'))),
    (('calculate_extents', 'numpy', 'int32', 4, 'absent', ''), ((), ('numpy', 'float64'))),
    (('calculate_extents', 'numpy', 'uint8', 4, 'absent', ''), ((), ('numpy', 'float64'))),
    (('calculate_extents', 'list', 'int64', 2, 'absent', 'sequence'), ((), ('numpy', 'float64'))),
    (('calculate_extents', 'list', 'int64', 3, 'absent', 'sequence'), ((), ('numpy', 'float64'))),
    (('measure_labels', 'numpy', 'uint8', 2, None, ''), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'uint8', 2, 'cuda', ''), ((('measure_labels', 'numpy', 'uint8', (3, 4), 'cuda'),), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'uint8', 2, None, ''), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'uint8', 2, 'cuda', ''), ((('measure_labels', 'tensor', 'uint8', (3, 4), 'cuda'),), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'int32', 2, None, ''), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'int32', 2, 'cuda', ''), ((('measure_labels', 'numpy', 'int32', (3, 4), 'cuda'),), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'int32', 2, None, ''), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'int32', 2, 'cuda', ''), ((('measure_labels', 'tensor', 'int32', (3, 4), 'cuda'),), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'int64', 2, None, ''), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'int64', 2, 'cuda', ''), ((('measure_labels', 'numpy', 'int64', (3, 4), 'cuda'),), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'list', 'int64', 2, None, ''), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'list', 'int64', 2, 'cuda', ''), ((('measure_labels', 'numpy', 'int64', (3, 4), 'cuda'),), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'int64', 2, None, ''), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'int64', 2, 'cuda', ''), ((('measure_labels', 'tensor', 'int64', (3, 4), 'cuda'),), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'bool', 2, None, ''), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'bool', 2, 'cuda', ''), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'list', 'bool', 2, None, ''), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'list', 'bool', 2, 'cuda', ''), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'bool', 2, None, ''), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'bool', 2, 'cuda', ''), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'float32', 2, None, ''), ((), 'ValueError')),
    (('measure_labels', 'numpy', 'float32', 2, 'cuda', ''), ((), 'ValueError')),
    (('measure_labels', 'tensor', 'float32', 2, None, ''), ((), 'ValueError')),
    (('measure_labels', 'tensor', 'float32', 2, 'cuda', ''), ((), 'ValueError')),
    (('measure_labels', 'numpy', 'int64', 3, None, ''), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'int64', 3, 'cuda', ''), ((('measure_labels', 'numpy', 'int64', (2, 3, 4), 'cuda'),), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'list', 'int64', 3, None, ''), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'list', 'int64', 3, 'cuda', ''), ((('measure_labels', 'numpy', 'int64', (2, 3, 4), 'cuda'),), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'int64', 3, None, ''), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'int64', 3, 'cuda', ''), ((('measure_labels', 'tensor', 'int64', (2, 3, 4), 'cuda'),), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'int64', 1, None, ''), ((), 'ValueError')),
    (('measure_labels', 'numpy', 'int64', 1, 'cuda', ''), ((), 'ValueError')),
    (('measure_labels', 'list', 'int64', 1, None, ''), ((), 'ValueError')),
    (('measure_labels', 'list', 'int64', 1, 'cuda', ''), ((), 'ValueError')),
    (('measure_labels', 'tensor', 'int64', 1, None, ''), ((), 'ValueError')),
    (('measure_labels', 'tensor', 'int64', 1, 'cuda', ''), ((), 'ValueError')),
    (('measure_labels', 'numpy', 'int64', 2, None, 'img:uint8'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'int64', 2, 'cuda', 'img:uint8'), ((('measure_labels', 'numpy', 'int64', (3, 4), 'cuda'), ('measure_labels image', 'numpy', 'uint8', (3, 4), 'cuda')), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'list', 'int64', 2, None, 'img:uint8'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'list', 'int64', 2, 'cuda', 'img:uint8'), ((('measure_labels', 'numpy', 'int64', (3, 4), 'cuda'), ('measure_labels image', 'numpy', 'uint8', (3, 4), 'cuda')), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'int64', 2, None, 'img:uint8'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'int64', 2, 'cuda', 'img:uint8'), ((('measure_labels', 'tensor', 'int64', (3, 4), 'cuda'), ('measure_labels image', 'numpy', 'uint8', (3, 4), 'cuda')), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'int64', 2, None, 'img:uint16'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'int64', 2, 'cuda', 'img:uint16'), ((('measure_labels', 'numpy', 'int64', (3, 4), 'cuda'), ('measure_labels image', 'numpy', 'uint16', (3, 4), 'cuda')), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'list', 'int64', 2, None, 'img:uint16'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'list', 'int64', 2, 'cuda', 'img:uint16'), ((('measure_labels', 'numpy', 'int64', (3, 4), 'cuda'), ('measure_labels image', 'numpy', 'uint16', (3, 4), 'cuda')), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'int64', 2, None, 'img:uint16'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'int64', 2, 'cuda', 'img:uint16'), ((('measure_labels', 'tensor', 'int64', (3, 4), 'cuda'), ('measure_labels image', 'numpy', 'uint16', (3, 4), 'cuda')), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'int64', 2, None, 'img:float32'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'float32')))),
    (('measure_labels', 'numpy', 'int64', 2, 'cuda', 'img:float32'), ((('measure_labels', 'numpy', 'int64', (3, 4), 'cuda'), ('measure_labels image', 'numpy', 'float32', (3, 4), 'cuda')), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'list', 'int64', 2, None, 'img:float32'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'float32')))),
    (('measure_labels', 'list', 'int64', 2, 'cuda', 'img:float32'), ((('measure_labels', 'numpy', 'int64', (3, 4), 'cuda'), ('measure_labels image', 'numpy', 'float32', (3, 4), 'cuda')), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'int64', 2, None, 'img:float32'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'float32')))),
    (('measure_labels', 'tensor', 'int64', 2, 'cuda', 'img:float32'), ((('measure_labels', 'tensor', 'int64', (3, 4), 'cuda'), ('measure_labels image', 'numpy', 'float32', (3, 4), 'cuda')), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'int64', 2, None, 'img:float64'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'float64')))),
    (('measure_labels', 'numpy', 'int64', 2, 'cuda', 'img:float64'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'float64')))),
    (('measure_labels', 'list', 'int64', 2, None, 'img:float64'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'float64')))),
    (('measure_labels', 'list', 'int64', 2, 'cuda', 'img:float64'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'float64')))),
    (('measure_labels', 'tensor', 'int64', 2, None, 'img:float64'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'float64')))),
    (('measure_labels', 'tensor', 'int64', 2, 'cuda', 'img:float64'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'float64')))),
    (('measure_labels', 'numpy', 'int64', 2, None, 'img:int32'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'int64', 2, 'cuda', 'img:int32'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'list', 'int64', 2, None, 'img:int32'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'list', 'int64', 2, 'cuda', 'img:int32'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'int64', 2, None, 'img:int32'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'int64', 2, 'cuda', 'img:int32'), ((), ('dict', ('numpy', 'int64'), ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'int64', 2, None, 'img:uint16+c'), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'int64', 2, 'cuda', 'img:uint16+c'), ((('measure_labels', 'numpy', 'int64', (3, 4), 'cuda'), ('measure_labels image', 'numpy', 'uint16', (3, 4, 2), 'cuda')), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'list', 'int64', 2, None, 'img:uint16+c'), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'list', 'int64', 2, 'cuda', 'img:uint16+c'), ((('measure_labels', 'numpy', 'int64', (3, 4), 'cuda'), ('measure_labels image', 'numpy', 'uint16', (3, 4, 2), 'cuda')), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'int64', 2, None, 'img:uint16+c'), ((), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'tensor', 'int64', 2, 'cuda', 'img:uint16+c'), ((('measure_labels', 'tensor', 'int64', (3, 4), 'cuda'), ('measure_labels image', 'numpy', 'uint16', (3, 4, 2), 'cuda')), ('dict', ('numpy', 'int64')))),
    (('measure_labels', 'numpy', 'int64', 2, None, 'as_tensors'), ((), ('dict', ('tensor', 'int64', 'cpu')))),
    (('measure_labels', 'numpy', 'int64', 2, 'cuda', 'as_tensors'), ((('measure_labels', 'numpy', 'int64', (3, 4), 'cuda'),), ('dict', ('tensor', 'int64', 'cpu')))),
    (('measure_labels', 'list', 'int64', 2, None, 'as_tensors'), ((), ('dict', ('tensor', 'int64', 'cpu')))),
    (('measure_labels', 'list', 'int64', 2, 'cuda', 'as_tensors'), ((('measure_labels', 'numpy', 'int64', (3, 4), 'cuda'),), ('dict', ('tensor', 'int64', 'cpu')))),
    (('measure_labels', 'tensor', 'int64', 2, None, 'as_tensors'), ((), ('dict', ('tensor', 'int64', 'cpu')))),
    (('measure_labels', 'tensor', 'int64', 2, 'cuda', 'as_tensors'), ((('measure_labels', 'tensor', 'int64', (3, 4), 'cuda'),), ('dict', ('tensor', 'int64', 'cpu')))),
    (('label_components', 'numpy', 'bool', 2, None, ''), ((), ('numpy', 'int32'))),
    (('label_components', 'numpy', 'bool', 2, 'cuda', ''), ((('label_components', 'numpy', 'bool', (3, 4), 'cuda'),), ('numpy', 'int32'))),
    (('label_components', 'list', 'bool', 2, None, ''), ((), ('numpy', 'int32'))),
    (('label_components', 'list', 'bool', 2, 'cuda', ''), ((('label_components', 'numpy', 'bool', (3, 4), 'cuda'),), ('numpy', 'int32'))),
    (('label_components', 'tensor', 'bool', 2, None, ''), ((), ('tensor', 'int32', 'cpu'))),
    (('label_components', 'tensor', 'bool', 2, 'cuda', ''), ((('label_components', 'tensor', 'bool', (3, 4), 'cuda'),), ('tensor', 'int32', 'cpu'))),
    (('label_components', 'numpy', 'uint8', 2, None, ''), ((), ('numpy', 'int32'))),
    (('label_components', 'numpy', 'uint8', 2, 'cuda', ''), ((('label_components', 'numpy', 'uint8', (3, 4), 'cuda'),), ('numpy', 'int32'))),
    (('label_components', 'tensor', 'uint8', 2, None, ''), ((), ('tensor', 'int32', 'cpu'))),
    (('label_components', 'tensor', 'uint8', 2, 'cuda', ''), ((('label_components', 'tensor', 'uint8', (3, 4), 'cuda'),), ('tensor', 'int32', 'cpu'))),
    (('label_components', 'numpy', 'uint16', 2, None, ''), ((), ('numpy', 'int32'))),
    (('label_components', 'numpy', 'uint16', 2, 'cuda', ''), ((('label_components', 'numpy', 'uint16', (3, 4), 'cuda'),), ('numpy', 'int32'))),
    (('label_components', 'tensor', 'uint16', 2, None, ''), ((), ('tensor', 'int32', 'cpu'))),
    (('label_components', 'tensor', 'uint16', 2, 'cuda', ''), ((('label_components', 'tensor', 'uint16', (3, 4), 'cuda'),), ('tensor', 'int32', 'cpu'))),
    (('label_components', 'numpy', 'int32', 2, None, ''), ((), ('numpy', 'int32'))),
    (('label_components', 'numpy', 'int32', 2, 'cuda', ''), ((('label_components', 'numpy', 'int32', (3, 4), 'cuda'),), ('numpy', 'int32'))),
    (('label_components', 'tensor', 'int32', 2, None, ''), ((), ('tensor', 'int32', 'cpu'))),
    (('label_components', 'tensor', 'int32', 2, 'cuda', ''), ((('label_components', 'tensor', 'int32', (3, 4), 'cuda'),), ('tensor', 'int32', 'cpu'))),
    (('label_components', 'numpy', 'int64', 2, None, ''), ((), ('numpy', 'int32'))),
    (('label_components', 'numpy', 'int64', 2, 'cuda', ''), ((), ('numpy', 'int32'))),
    (('label_components', 'list', 'int64', 2, None, ''), ((), ('numpy', 'int32'))),
    (('label_components', 'list', 'int64', 2, 'cuda', ''), ((), ('numpy', 'int32'))),
    (('label_components', 'tensor', 'int64', 2, None, ''), ((), ('tensor', 'int32', 'cpu'))),
    (('label_components', 'numpy', 'int8', 2, None, ''), ((), ('numpy', 'int32'))),
    (('label_components', 'numpy', 'int8', 2, 'cuda', ''), ((), ('numpy', 'int32'))),
    (('label_components', 'tensor', 'int8', 2, None, ''), ((), ('tensor', 'int32', 'cpu'))),
    (('label_components', 'numpy', 'float32', 2, None, ''), ((), ('numpy', 'int32'))),
    (('label_components', 'numpy', 'float32', 2, 'cuda', ''), ((), ('numpy', 'int32'))),
    (('label_components', 'tensor', 'float32', 2, None, ''), ((), ('tensor', 'int32', 'cpu'))),
    (('label_components', 'numpy', 'bool', 3, None, ''), ((), ('numpy', 'int32'))),
    (('label_components', 'numpy', 'bool', 3, 'cuda', ''), ((('label_components', 'numpy', 'bool', (2, 3, 4), 'cuda'),), ('numpy', 'int32'))),
    (('label_components', 'list', 'bool', 3, None, ''), ((), ('numpy', 'int32'))),
    (('label_components', 'list', 'bool', 3, 'cuda', ''), ((('label_components', 'numpy', 'bool', (2, 3, 4), 'cuda'),), ('numpy', 'int32'))),
    (('label_components', 'tensor', 'bool', 3, None, ''), ((), ('tensor', 'int32', 'cpu'))),
    (('label_components', 'tensor', 'bool', 3, 'cuda', ''), ((('label_components', 'tensor', 'bool', (2, 3, 4), 'cuda'),), ('tensor', 'int32', 'cpu'))),
    (('label_components', 'numpy', 'bool', 1, None, ''), ((), 'ValueError')),
    (('label_components', 'numpy', 'bool', 1, 'cuda', ''), ((), 'ValueError')),
    (('label_components', 'list', 'bool', 1, None, ''), ((), 'ValueError')),
    (('label_components', 'list', 'bool', 1, 'cuda', ''), ((), 'ValueError')),
    (('label_components', 'tensor', 'bool', 1, None, ''), ((), 'ValueError')),
    (('label_components', 'tensor', 'bool', 1, 'cuda', ''), ((), 'ValueError')),
    (('label_components', 'numpy', 'uint8', 2, None, 'return_num'), ((), (('numpy', 'int32'), ('int', 2)))),
    (('label_components', 'numpy', 'uint8', 2, 'cuda', 'return_num'), ((('label_components', 'numpy', 'uint8', (3, 4), 'cuda'),), (('numpy', 'int32'), ('int', 3)))),
    (('label_components', 'tensor', 'uint8', 2, None, 'return_num'), ((), (('tensor', 'int32', 'cpu'), ('int', 2)))),
    (('label_components', 'tensor', 'uint8', 2, 'cuda', 'return_num'), ((('label_components', 'tensor', 'uint8', (3, 4), 'cuda'),), (('tensor', 'int32', 'cpu'), ('int', 3)))),
    (('label_components', 'numpy', 'uint8', 2, None, 'background 0.5'), ((), ('numpy', 'int32'))),
    (('label_components', 'numpy', 'uint8', 2, 'cuda', 'background 0.5'), ((), ('numpy', 'int32'))),
    (('label_components', 'tensor', 'uint8', 2, None, 'background 0.5'), ((), ('tensor', 'int32', 'cpu'))),
    (('expand_labels', 'numpy', 'uint8', 2, None, ''), ((), ('numpy', 'uint8'))),
    (('expand_labels', 'numpy', 'uint8', 2, 'cuda', ''), ((('expand_labels', 'numpy', 'uint8', (3, 4), 'cuda'),), 'expanded on the device')),
    (('expand_labels', 'tensor', 'uint8', 2, None, ''), ((), ('tensor', 'uint8', 'cpu'))),
    (('expand_labels', 'tensor', 'uint8', 2, 'cuda', ''), ((('expand_labels', 'tensor', 'uint8', (3, 4), 'cuda'),), 'expanded on the device')),
    (('expand_labels', 'numpy', 'uint16', 2, None, ''), ((), ('numpy', 'uint16'))),
    (('expand_labels', 'numpy', 'uint16', 2, 'cuda', ''), ((('expand_labels', 'numpy', 'uint16', (3, 4), 'cuda'),), 'expanded on the device')),
    (('expand_labels', 'tensor', 'uint16', 2, None, ''), ((), ('tensor', 'uint16', 'cpu'))),
    (('expand_labels', 'numpy', 'int8', 2, None, ''), ((), ('numpy', 'int8'))),
    (('expand_labels', 'numpy', 'int8', 2, 'cuda', ''), ((('expand_labels', 'numpy', 'int8', (3, 4), 'cuda'),), 'expanded on the device')),
    (('expand_labels', 'tensor', 'int8', 2, None, ''), ((), ('tensor', 'int8', 'cpu'))),
    (('expand_labels', 'tensor', 'int8', 2, 'cuda', ''), ((('expand_labels', 'tensor', 'int8', (3, 4), 'cuda'),), 'expanded on the device')),
    (('expand_labels', 'numpy', 'int32', 2, None, ''), ((), ('numpy', 'int32'))),
    (('expand_labels', 'numpy', 'int32', 2, 'cuda', ''), ((('expand_labels', 'numpy', 'int32', (3, 4), 'cuda'),), 'expanded on the device')),
    (('expand_labels', 'tensor', 'int32', 2, None, ''), ((), ('tensor', 'int32', 'cpu'))),
    (('expand_labels', 'tensor', 'int32', 2, 'cuda', ''), ((('expand_labels', 'tensor', 'int32', (3, 4), 'cuda'),), 'expanded on the device')),
    (('expand_labels', 'numpy', 'int64', 2, None, ''), ((), ('numpy', 'int64'))),
    (('expand_labels', 'numpy', 'int64', 2, 'cuda', ''), ((('expand_labels', 'numpy', 'int64', (3, 4), 'cuda'),), 'expanded on the device')),
    (('expand_labels', 'list', 'int64', 2, None, ''), ((), ('numpy', 'int64'))),
    (('expand_labels', 'list', 'int64', 2, 'cuda', ''), ((('expand_labels', 'numpy', 'int64', (3, 4), 'cuda'),), 'expanded on the device')),
    (('expand_labels', 'tensor', 'int64', 2, None, ''), ((), ('tensor', 'int64', 'cpu'))),
    (('expand_labels', 'tensor', 'int64', 2, 'cuda', ''), ((('expand_labels', 'tensor', 'int64', (3, 4), 'cuda'),), 'expanded on the device')),
    (('expand_labels', 'numpy', 'bool', 2, None, ''), ((), ('numpy', 'bool'))),
    (('expand_labels', 'numpy', 'bool', 2, 'cuda', ''), ((), ('numpy', 'bool'))),
    (('expand_labels', 'list', 'bool', 2, None, ''), ((), ('numpy', 'bool'))),
    (('expand_labels', 'list', 'bool', 2, 'cuda', ''), ((), ('numpy', 'bool'))),
    (('expand_labels', 'tensor', 'bool', 2, None, ''), ((), ('tensor', 'bool', 'cpu'))),
    (('expand_labels', 'numpy', 'float32', 2, None, ''), ((), ('numpy', 'float32'))),
    (('expand_labels', 'numpy', 'float32', 2, 'cuda', ''), ((), ('numpy', 'float32'))),
    (('expand_labels', 'tensor', 'float32', 2, None, ''), ((), ('tensor', 'float32', 'cpu'))),
    (('expand_labels', 'numpy', 'int64', 3, None, ''), ((), ('numpy', 'int64'))),
    (('expand_labels', 'numpy', 'int64', 3, 'cuda', ''), ((('expand_labels', 'numpy', 'int64', (2, 3, 4), 'cuda'),), 'expanded on the device')),
    (('expand_labels', 'list', 'int64', 3, None, ''), ((), ('numpy', 'int64'))),
    (('expand_labels', 'list', 'int64', 3, 'cuda', ''), ((('expand_labels', 'numpy', 'int64', (2, 3, 4), 'cuda'),), 'expanded on the device')),
    (('expand_labels', 'tensor', 'int64', 3, None, ''), ((), ('tensor', 'int64', 'cpu'))),
    (('expand_labels', 'tensor', 'int64', 3, 'cuda', ''), ((('expand_labels', 'tensor', 'int64', (2, 3, 4), 'cuda'),), 'expanded on the device')),
    (('expand_labels', 'numpy', 'int64', 1, None, ''), ((), 'ValueError')),
    (('expand_labels', 'numpy', 'int64', 1, 'cuda', ''), ((), 'ValueError')),
    (('expand_labels', 'list', 'int64', 1, None, ''), ((), 'ValueError')),
    (('expand_labels', 'list', 'int64', 1, 'cuda', ''), ((), 'ValueError')),
    (('expand_labels', 'tensor', 'int64', 1, None, ''), ((), 'ValueError')),
    (('expand_labels', 'tensor', 'int64', 1, 'cuda', ''), ((), 'ValueError')),
    (('expand_labels', 'numpy', 'int64', 2, None, 'negative'), ((), ('numpy', 'int64'))),
    (('expand_labels', 'numpy', 'int64', 2, 'cuda', 'negative'), ((), ('numpy', 'int64'))),
    (('expand_labels', 'list', 'int64', 2, None, 'negative'), ((), ('numpy', 'int64'))),
    (('expand_labels', 'list', 'int64', 2, 'cuda', 'negative'), ((), ('numpy', 'int64'))),
    (('expand_labels', 'tensor', 'int64', 2, None, 'negative'), ((), ('tensor', 'int64', 'cpu'))),
    (('expand_labels', 'numpy', 'int64', 2, None, 'distance 0'), ((), ('numpy', 'int64'))),
    (('expand_labels', 'numpy', 'int64', 2, 'cuda', 'distance 0'), ((), ('numpy', 'int64'))),
    (('expand_labels', 'list', 'int64', 2, None, 'distance 0'), ((), ('numpy', 'int64'))),
    (('expand_labels', 'list', 'int64', 2, 'cuda', 'distance 0'), ((), ('numpy', 'int64'))),
    (('expand_labels', 'tensor', 'int64', 2, None, 'distance 0'), ((), ('tensor', 'int64', 'cpu'))),
    (('expand_labels', 'tensor', 'int64', 2, 'cuda', 'distance 0'), ((), ('tensor', 'int64', 'cpu'))),
    (('expand_labels', 'numpy', 'int64', 2, None, 'bad spacing'), ((), 'ValueError')),
    (('expand_labels', 'numpy', 'int64', 2, 'cuda', 'bad spacing'), ((), 'ValueError')),
    (('expand_labels', 'list', 'int64', 2, None, 'bad spacing'), ((), 'ValueError')),
    (('expand_labels', 'list', 'int64', 2, 'cuda', 'bad spacing'), ((), 'ValueError')),
    (('expand_labels', 'tensor', 'int64', 2, None, 'bad spacing'), ((), 'ValueError')),
    (('expand_labels', 'tensor', 'int64', 2, 'cuda', 'bad spacing'), ((), 'ValueError')),
    (('distance_transform', 'numpy', 'uint8', 2, None, ''), ((), ('numpy', 'float64'))),
    (('distance_transform', 'numpy', 'uint8', 2, 'cuda', ''), ((('distance_transform', 'numpy', 'uint8', (3, 4), 'cuda'),), ('numpy', 'float64'))),
    (('distance_transform', 'tensor', 'uint8', 2, None, ''), ((), ('tensor', 'float64', 'cpu'))),
    (('distance_transform', 'tensor', 'uint8', 2, 'cuda', ''), ((('distance_transform', 'tensor', 'uint8', (3, 4), 'cuda'),), ('tensor', 'float64', 'cpu'))),
    (('distance_transform', 'numpy', 'bool', 2, None, ''), ((), ('numpy', 'float64'))),
    (('distance_transform', 'numpy', 'bool', 2, 'cuda', ''), ((('distance_transform', 'numpy', 'bool', (3, 4), 'cuda'),), ('numpy', 'float64'))),
    (('distance_transform', 'list', 'bool', 2, None, ''), ((), ('numpy', 'float64'))),
    (('distance_transform', 'list', 'bool', 2, 'cuda', ''), ((('distance_transform', 'numpy', 'bool', (3, 4), 'cuda'),), ('numpy', 'float64'))),
    (('distance_transform', 'tensor', 'bool', 2, None, ''), ((), ('tensor', 'float64', 'cpu'))),
    (('distance_transform', 'tensor', 'bool', 2, 'cuda', ''), ((('distance_transform', 'tensor', 'bool', (3, 4), 'cuda'),), ('tensor', 'float64', 'cpu'))),
    (('distance_transform', 'numpy', 'int32', 2, None, ''), ((), ('numpy', 'float64'))),
    (('distance_transform', 'numpy', 'int32', 2, 'cuda', ''), ((('distance_transform', 'numpy', 'int32', (3, 4), 'cuda'),), ('numpy', 'float64'))),
    (('distance_transform', 'tensor', 'int32', 2, None, ''), ((), ('tensor', 'float64', 'cpu'))),
    (('distance_transform', 'tensor', 'int32', 2, 'cuda', ''), ((('distance_transform', 'tensor', 'int32', (3, 4), 'cuda'),), ('tensor', 'float64', 'cpu'))),
    (('distance_transform', 'numpy', 'int64', 2, None, ''), ((), ('numpy', 'float64'))),
    (('distance_transform', 'numpy', 'int64', 2, 'cuda', ''), ((('distance_transform', 'numpy', 'int64', (3, 4), 'cuda'),), ('numpy', 'float64'))),
    (('distance_transform', 'list', 'int64', 2, None, ''), ((), ('numpy', 'float64'))),
    (('distance_transform', 'list', 'int64', 2, 'cuda', ''), ((('distance_transform', 'numpy', 'int64', (3, 4), 'cuda'),), ('numpy', 'float64'))),
    (('distance_transform', 'tensor', 'int64', 2, None, ''), ((), ('tensor', 'float64', 'cpu'))),
    (('distance_transform', 'tensor', 'int64', 2, 'cuda', ''), ((('distance_transform', 'tensor', 'int64', (3, 4), 'cuda'),), ('tensor', 'float64', 'cpu'))),
    (('distance_transform', 'numpy', 'float32', 2, None, ''), ((), ('numpy', 'float64'))),
    (('distance_transform', 'numpy', 'float32', 2, 'cuda', ''), ((('distance_transform', 'numpy', 'float32', (3, 4), 'cuda'),), ('numpy', 'float64'))),
    (('distance_transform', 'tensor', 'float32', 2, None, ''), ((), ('tensor', 'float64', 'cpu'))),
    (('distance_transform', 'tensor', 'float32', 2, 'cuda', ''), ((('distance_transform', 'tensor', 'float32', (3, 4), 'cuda'),), ('tensor', 'float64', 'cpu'))),
    (('distance_transform', 'numpy', 'int64', 3, None, ''), ((), ('numpy', 'float64'))),
    (('distance_transform', 'numpy', 'int64', 3, 'cuda', ''), ((('distance_transform', 'numpy', 'int64', (2, 3, 4), 'cuda'),), ('numpy', 'float64'))),
    (('distance_transform', 'list', 'int64', 3, None, ''), ((), ('numpy', 'float64'))),
    (('distance_transform', 'list', 'int64', 3, 'cuda', ''), ((('distance_transform', 'numpy', 'int64', (2, 3, 4), 'cuda'),), ('numpy', 'float64'))),
    (('distance_transform', 'tensor', 'int64', 3, None, ''), ((), ('tensor', 'float64', 'cpu'))),
    (('distance_transform', 'tensor', 'int64', 3, 'cuda', ''), ((('distance_transform', 'tensor', 'int64', (2, 3, 4), 'cuda'),), ('tensor', 'float64', 'cpu'))),
    (('distance_transform', 'numpy', 'int64', 1, None, ''), ((), 'ValueError')),
    (('distance_transform', 'numpy', 'int64', 1, 'cuda', ''), ((), 'ValueError')),
    (('distance_transform', 'list', 'int64', 1, None, ''), ((), 'ValueError')),
    (('distance_transform', 'list', 'int64', 1, 'cuda', ''), ((), 'ValueError')),
    (('distance_transform', 'tensor', 'int64', 1, None, ''), ((), 'ValueError')),
    (('distance_transform', 'tensor', 'int64', 1, 'cuda', ''), ((), 'ValueError')),
    (('distance_transform', 'numpy', 'int64', 2, None, 'indices'), ((), (('numpy', 'float64'), ('numpy', 'int32')))),
    (('distance_transform', 'numpy', 'int64', 2, 'cuda', 'indices'), ((('distance_transform', 'numpy', 'int64', (3, 4), 'cuda'),), (('numpy', 'float64'), ('numpy', 'int32')))),
    (('distance_transform', 'list', 'int64', 2, None, 'indices'), ((), (('numpy', 'float64'), ('numpy', 'int32')))),
    (('distance_transform', 'list', 'int64', 2, 'cuda', 'indices'), ((('distance_transform', 'numpy', 'int64', (3, 4), 'cuda'),), (('numpy', 'float64'), ('numpy', 'int32')))),
    (('distance_transform', 'tensor', 'int64', 2, None, 'indices'), ((), (('tensor', 'float64', 'cpu'), ('tensor', 'int32', 'cpu')))),
    (('distance_transform', 'tensor', 'int64', 2, 'cuda', 'indices'), ((('distance_transform', 'tensor', 'int64', (3, 4), 'cuda'),), (('tensor', 'float64', 'cpu'), ('tensor', 'int32', 'cpu')))),
    (('distance_transform', 'numpy', 'int64', 2, None, 'bad bound'), ((), 'ValueError')),
    (('distance_transform', 'numpy', 'int64', 2, 'cuda', 'bad bound'), ((), 'ValueError')),
    (('distance_transform', 'list', 'int64', 2, None, 'bad bound'), ((), 'ValueError')),
    (('distance_transform', 'list', 'int64', 2, 'cuda', 'bad bound'), ((), 'ValueError')),
    (('distance_transform', 'tensor', 'int64', 2, None, 'bad bound'), ((), 'ValueError')),
    (('distance_transform', 'tensor', 'int64', 2, 'cuda', 'bad bound'), ((), 'ValueError')),
    (('relabel_image_stardist', 'numpy', 'uint8', 2, None, ''), ((('relabel_image_stardist host', 'numpy', 'uint8', (3, 4), None),), ('numpy', 'int32'))),
    (('relabel_image_stardist', 'tensor', 'uint8', 2, None, ''), ((('relabel_image_stardist host', 'numpy', 'uint8', (3, 4), None),), ('tensor', 'int32', 'cpu'))),
    (('relabel_image_stardist', 'numpy', 'uint16', 2, None, ''), ((('relabel_image_stardist host', 'numpy', 'uint16', (3, 4), None),), ('numpy', 'int32'))),
    (('relabel_image_stardist', 'numpy', 'int32', 2, None, ''), ((('relabel_image_stardist host', 'numpy', 'int32', (3, 4), None),), ('numpy', 'int32'))),
    (('relabel_image_stardist', 'tensor', 'int32', 2, None, ''), ((('relabel_image_stardist host', 'numpy', 'int32', (3, 4), None),), ('tensor', 'int32', 'cpu'))),
    (('relabel_image_stardist', 'numpy', 'int64', 2, None, ''), ((('relabel_image_stardist host', 'numpy', 'int64', (3, 4), None),), ('numpy', 'int32'))),
    (('relabel_image_stardist', 'list', 'int64', 2, None, ''), ((('relabel_image_stardist host', 'numpy', 'int64', (3, 4), None),), ('numpy', 'int32'))),
    (('relabel_image_stardist', 'tensor', 'int64', 2, None, ''), ((('relabel_image_stardist host', 'numpy', 'int64', (3, 4), None),), ('tensor', 'int32', 'cpu'))),
    (('relabel_image_stardist', 'numpy', 'float32', 2, None, ''), ((), 'ValueError')),
    (('relabel_image_stardist', 'numpy', 'float32', 2, 'cuda', ''), ((), 'ValueError')),
    (('relabel_image_stardist', 'tensor', 'float32', 2, None, ''), ((), 'ValueError')),
    (('relabel_image_stardist', 'tensor', 'float32', 2, 'cuda', ''), ((), 'ValueError')),
    (('relabel_image_stardist', 'numpy', 'bool', 2, None, ''), ((), 'ValueError')),
    (('relabel_image_stardist', 'numpy', 'bool', 2, 'cuda', ''), ((), 'ValueError')),
    (('relabel_image_stardist', 'list', 'bool', 2, None, ''), ((), 'ValueError')),
    (('relabel_image_stardist', 'list', 'bool', 2, 'cuda', ''), ((), 'ValueError')),
    (('relabel_image_stardist', 'tensor', 'bool', 2, None, ''), ((), 'ValueError')),
    (('relabel_image_stardist', 'tensor', 'bool', 2, 'cuda', ''), ((), 'ValueError')),
    (('relabel_image_stardist', 'numpy', 'int64', 3, None, ''), ((), 'ValueError')),
    (('relabel_image_stardist', 'numpy', 'int64', 3, 'cuda', ''), ((), 'ValueError')),
    (('relabel_image_stardist', 'list', 'int64', 3, None, ''), ((), 'ValueError')),
    (('relabel_image_stardist', 'list', 'int64', 3, 'cuda', ''), ((), 'ValueError')),
    (('relabel_image_stardist', 'tensor', 'int64', 3, None, ''), ((), 'ValueError')),
    (('relabel_image_stardist', 'tensor', 'int64', 3, 'cuda', ''), ((), 'ValueError')),
    (('relabel_image_stardist', 'numpy', 'int64', 2, None, 'kwargs'), ((('relabel_image_stardist host', 'numpy', 'int64', (3, 4), None),), ('numpy', 'int32'))),
    (('relabel_image_stardist', 'numpy', 'int64', 2, 'cuda', 'kwargs'), ((('relabel_image_stardist host', 'numpy', 'int64', (3, 4), None),), ('numpy', 'int32'))),
    (('relabel_image_stardist', 'list', 'int64', 2, None, 'kwargs'), ((('relabel_image_stardist host', 'numpy', 'int64', (3, 4), None),), ('numpy', 'int32'))),
    (('relabel_image_stardist', 'list', 'int64', 2, 'cuda', 'kwargs'), ((('relabel_image_stardist host', 'numpy', 'int64', (3, 4), None),), ('numpy', 'int32'))),
    (('relabel_image_stardist', 'tensor', 'int64', 2, None, 'kwargs'), ((('relabel_image_stardist host', 'numpy', 'int64', (3, 4), None),), ('tensor', 'int32', 'cpu'))),
    (('relabel_image_stardist', 'tensor', 'int64', 2, 'cuda', 'kwargs'), ((('relabel_image_stardist host', 'numpy', 'int64', (3, 4), None),), ('tensor', 'int32', 'cpu'))),
    (('relabel_image_stardist', 'numpy', 'int64', 2, None, 'sparse'), ((('relabel_image_stardist host', 'numpy', 'int64', (3, 4), None),), ('numpy', 'int32'))),
    (('relabel_image_stardist', 'numpy', 'int64', 2, 'cuda', 'sparse'), ((('relabel_image_stardist host', 'numpy', 'int64', (3, 4), None),), ('numpy', 'int32'))),
    (('relabel_image_stardist', 'list', 'int64', 2, None, 'sparse'), ((('relabel_image_stardist host', 'numpy', 'int64', (3, 4), None),), ('numpy', 'int32'))),
    (('relabel_image_stardist', 'list', 'int64', 2, 'cuda', 'sparse'), ((('relabel_image_stardist host', 'numpy', 'int64', (3, 4), None),), ('numpy', 'int32'))),
    (('relabel_image_stardist', 'tensor', 'int64', 2, None, 'sparse'), ((('relabel_image_stardist host', 'numpy', 'int64', (3, 4), None),), ('tensor', 'int32', 'cpu'))),
    (('relabel_image_stardist', 'tensor', 'int64', 2, 'cuda', 'sparse'), ((('relabel_image_stardist host', 'numpy', 'int64', (3, 4), None),), ('tensor', 'int32', 'cpu'))),
    (('relabel_image_stardist', 'numpy', 'int64', 2, None, 'negative'), ((), 'ValueError')),
    (('relabel_image_stardist', 'numpy', 'int64', 2, 'cuda', 'negative'), ((), 'ValueError')),
    (('relabel_image_stardist', 'list', 'int64', 2, None, 'negative'), ((), 'ValueError')),
    (('relabel_image_stardist', 'list', 'int64', 2, 'cuda', 'negative'), ((), 'ValueError')),
    (('relabel_image_stardist', 'tensor', 'int64', 2, None, 'negative'), ((), 'ValueError')),
    (('relabel_image_stardist', 'tensor', 'int64', 2, 'cuda', 'negative'), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'numpy', 'uint8', 3, None, ''), ((('relabel_image_stardist3D host', 'numpy', 'uint8', (2, 3, 4), None),), ('numpy', 'uint16'))),
    (('relabel_image_stardist3D', 'tensor', 'uint8', 3, None, ''), ((('relabel_image_stardist3D host', 'numpy', 'uint8', (2, 3, 4), None),), ('tensor', 'uint16', 'cpu'))),
    (('relabel_image_stardist3D', 'numpy', 'uint16', 3, None, ''), ((('relabel_image_stardist3D host', 'numpy', 'uint16', (2, 3, 4), None),), ('numpy', 'uint16'))),
    (('relabel_image_stardist3D', 'numpy', 'int32', 3, None, ''), ((('relabel_image_stardist3D host', 'numpy', 'int32', (2, 3, 4), None),), ('numpy', 'uint16'))),
    (('relabel_image_stardist3D', 'tensor', 'int32', 3, None, ''), ((('relabel_image_stardist3D host', 'numpy', 'int32', (2, 3, 4), None),), ('tensor', 'uint16', 'cpu'))),
    (('relabel_image_stardist3D', 'numpy', 'int64', 3, None, ''), ((('relabel_image_stardist3D host', 'numpy', 'int64', (2, 3, 4), None),), ('numpy', 'uint16'))),
    (('relabel_image_stardist3D', 'list', 'int64', 3, None, ''), ((('relabel_image_stardist3D host', 'numpy', 'int64', (2, 3, 4), None),), ('numpy', 'uint16'))),
    (('relabel_image_stardist3D', 'tensor', 'int64', 3, None, ''), ((('relabel_image_stardist3D host', 'numpy', 'int64', (2, 3, 4), None),), ('tensor', 'uint16', 'cpu'))),
    (('relabel_image_stardist3D', 'numpy', 'float32', 3, None, ''), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'numpy', 'float32', 3, 'cuda', ''), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'tensor', 'float32', 3, None, ''), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'tensor', 'float32', 3, 'cuda', ''), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'numpy', 'bool', 3, None, ''), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'numpy', 'bool', 3, 'cuda', ''), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'list', 'bool', 3, None, ''), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'list', 'bool', 3, 'cuda', ''), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'tensor', 'bool', 3, None, ''), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'tensor', 'bool', 3, 'cuda', ''), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'numpy', 'int64', 2, None, ''), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'numpy', 'int64', 2, 'cuda', ''), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'list', 'int64', 2, None, ''), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'list', 'int64', 2, 'cuda', ''), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'tensor', 'int64', 2, None, ''), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'tensor', 'int64', 2, 'cuda', ''), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'numpy', 'int64', 3, None, 'kwargs'), ((('relabel_image_stardist3D host', 'numpy', 'int64', (2, 3, 4), None),), ('numpy', 'uint16'))),
    (('relabel_image_stardist3D', 'numpy', 'int64', 3, 'cuda', 'kwargs'), ((('relabel_image_stardist3D host', 'numpy', 'int64', (2, 3, 4), None),), ('numpy', 'uint16'))),
    (('relabel_image_stardist3D', 'list', 'int64', 3, None, 'kwargs'), ((('relabel_image_stardist3D host', 'numpy', 'int64', (2, 3, 4), None),), ('numpy', 'uint16'))),
    (('relabel_image_stardist3D', 'list', 'int64', 3, 'cuda', 'kwargs'), ((('relabel_image_stardist3D host', 'numpy', 'int64', (2, 3, 4), None),), ('numpy', 'uint16'))),
    (('relabel_image_stardist3D', 'tensor', 'int64', 3, None, 'kwargs'), ((('relabel_image_stardist3D host', 'numpy', 'int64', (2, 3, 4), None),), ('tensor', 'uint16', 'cpu'))),
    (('relabel_image_stardist3D', 'tensor', 'int64', 3, 'cuda', 'kwargs'), ((('relabel_image_stardist3D host', 'numpy', 'int64', (2, 3, 4), None),), ('tensor', 'uint16', 'cpu'))),
    (('relabel_image_stardist3D', 'numpy', 'int64', 3, None, 'sparse'), ((('relabel_image_stardist3D host', 'numpy', 'int64', (2, 3, 4), None),), ('numpy', 'uint16'))),
    (('relabel_image_stardist3D', 'numpy', 'int64', 3, 'cuda', 'sparse'), ((('relabel_image_stardist3D host', 'numpy', 'int64', (2, 3, 4), None),), ('numpy', 'uint16'))),
    (('relabel_image_stardist3D', 'list', 'int64', 3, None, 'sparse'), ((('relabel_image_stardist3D host', 'numpy', 'int64', (2, 3, 4), None),), ('numpy', 'uint16'))),
    (('relabel_image_stardist3D', 'list', 'int64', 3, 'cuda', 'sparse'), ((('relabel_image_stardist3D host', 'numpy', 'int64', (2, 3, 4), None),), ('numpy', 'uint16'))),
    (('relabel_image_stardist3D', 'tensor', 'int64', 3, None, 'sparse'), ((('relabel_image_stardist3D host', 'numpy', 'int64', (2, 3, 4), None),), ('tensor', 'uint16', 'cpu'))),
    (('relabel_image_stardist3D', 'tensor', 'int64', 3, 'cuda', 'sparse'), ((('relabel_image_stardist3D host', 'numpy', 'int64', (2, 3, 4), None),), ('tensor', 'uint16', 'cpu'))),
    (('relabel_image_stardist3D', 'numpy', 'int64', 3, None, 'negative'), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'numpy', 'int64', 3, 'cuda', 'negative'), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'list', 'int64', 3, None, 'negative'), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'list', 'int64', 3, 'cuda', 'negative'), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'tensor', 'int64', 3, None, 'negative'), ((), 'ValueError')),
    (('relabel_image_stardist3D', 'tensor', 'int64', 3, 'cuda', 'negative'), ((), 'ValueError')),
]


@pytest.mark.parametrize("row,want", TABLE, ids=["-".join(str(v) for v in row) for row, _ in TABLE])
def test_route(row, want, monkeypatch):
    got = outcome(row, monkeypatch)
    assert got == want
    if want[1] == "ValueError":
        assert got[0] == ()                                                 # raised before any half ran


def test_the_matrix_covers_every_function_kind_and_device():
    rows = [row for row, _ in TABLE]
    functions = {"fill_label_holes", "calculate_extents", "measure_labels", "label_components", "expand_labels", "distance_transform",
                 "relabel_image_stardist", "relabel_image_stardist3D"}
    assert {r[0] for r in rows} == functions
    for fn in functions:
        mine = [r for r in rows if r[0] == fn]
        assert {r[3] for r in mine} >= {2, 3}, fn
        if fn != "calculate_extents":                                       # it has no device= and takes no host tensor
            assert {r[1] for r in mine} == {"numpy", "list", "tensor"} and {r[4] for r in mine} >= {None, "cuda"}, fn
    assert any(w == "ValueError" for _, (_, w) in TABLE) and any(c for _, (c, _) in TABLE)
