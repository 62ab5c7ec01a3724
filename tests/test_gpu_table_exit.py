"""GPU: the table functions' device routes through the one exit (stardist_amd._route.table_exit): measure_labels with every keyword at
once on device tensors, label_contacts and point_neighbors, numpy out and as_tensors=True, against the host route by the existing
rules -- == for integer images, libm_close for orientation and the 3D equivalent_diameter, tests/_measure_cases.check_float_columns
for the float sums -- and one read-back call per numpy-out call.  Cases: tests/_table_exit_cases.py (67 x 131 and 9 x 33 x 70: every
kernel family runs and the labels present are a strict subset of 0 .. top, so the rows are selected)."""
import numpy as np
import pytest

import _measure_cases as M
import _table_exit_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture
def reads(monkeypatch):
    """the names of the read-back calls (utils.to_host, utils.to_host_many), in order"""
    from stardist_amd import utils
    seen = []
    for name in ("to_host", "to_host_many"):
        monkeypatch.setattr(utils, name, (lambda real, name: lambda *a: seen.append(name) or real(*a))(getattr(utils, name), name))
    return seen


def on_device(torch):
    return lambda a: torch.as_tensor(a, device="cuda")


@pytest.mark.parametrize("name", T.MEASURE_GPU)
def test_measure_labels_with_every_keyword(torch, reads, name):
    want = T.host(name)
    lbl = T.call(name)[1][0]
    assert len(want["label"]) < int(lbl.max())                              # a strict subset of 0 .. top
    got = T.run(name, convert=on_device(torch))
    assert reads == ["to_host_many"] and all(isinstance(v, np.ndarray) for v in got.values())
    T.same_table(got, want, libm=T.LIBM)
    del reads[:]
    got = T.run(name, convert=on_device(torch), as_tensors=True)
    assert reads == [] and all(isinstance(v, torch.Tensor) and v.is_cuda for v in got.values())
    T.same_table(got, want, libm=T.LIBM)
    got = T.run(name, device="cuda")                                        # numpy in
    assert reads == ["to_host_many"]
    T.same_table(got, want, libm=T.LIBM)


def test_measure_labels_of_a_float_image(torch, reads):
    """the float sums differ from the host's by the order of the additions: sum, mean and std within the derived bounds of
    check_float_columns, every other column as for integer images"""
    want = T.host("measure_2d_f32")
    loose = ("sum_intensity", "mean_intensity", "std_intensity")
    for more in ({}, {"as_tensors": True}):
        del reads[:]
        got = T.run("measure_2d_f32", convert=on_device(torch), **more)
        assert reads == ([] if more else ["to_host_many"])
        got = {k: v.cpu().numpy() if more else v for k, v in got.items()}
        assert list(got) == list(want)
        M.check_float_columns("2d_f32_random", got)
        tight = [k for k in want if k not in loose]
        T.same_table({k: got[k] for k in tight}, {k: want[k] for k in tight}, libm=T.LIBM)
        assert all(got[k].dtype == want[k].dtype and got[k].shape == want[k].shape for k in loose)


@pytest.mark.parametrize("name", ("measure_no_pixels", "measure_background"))
def test_empty_tables(torch, reads, name):
    want = T.host(name)
    T.same_table(T.run(name, convert=on_device(torch)), want)
    assert len(reads) <= 1
    got = T.run(name, convert=on_device(torch), as_tensors=True)
    assert all(v.is_cuda for v in got.values())
    T.same_table(got, want)


@pytest.mark.parametrize("name", ("contacts", "points_k", "points_radius", "points_count"))
def test_label_contacts_and_point_neighbors(torch, reads, name):
    want = T.host(name)
    got = T.run(name, convert=on_device(torch))
    assert reads == ["to_host_many"] and all(isinstance(v, np.ndarray) for v in got.values())
    T.same_table(got, want)
    del reads[:]
    got = T.run(name, convert=on_device(torch), as_tensors=True)
    assert reads == [] and all(isinstance(v, torch.Tensor) and v.is_cuda for v in got.values())
    T.same_table(got, want)
