"""CPU: the native calls of one training step are a fixed sequence.
tests/golden/training_call_trace.json holds, for batch 2 of a 2D U-Net, a 3D U-Net and a 3D ResNet, every call that train_loss /
train_loss3d and loss.backward() make through N.dcall (name, integer and float arguments, which arguments are pointers and which
None), and the calls of the same forward pass under torch.no_grad() (validation).  It was recorded (tests/golden/
make_training_call_trace.py) when the 2D and 3D layers were two separate sets with 2D adjoint kernels of their own; the one layer set
of today must launch the same kernels in the same order with the same arguments.  The only difference allowed is written out below:
the 2D max-pool and up-sampling adjoints now go through the 3D entry points with D = 1."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["unet2d", "unet3d", "resnet3d"]


def _expected(call):
    """the recorded call as it is issued today"""
    name, a = call
    if name == "sd_maxpool_adjoint_ndhwc_device":          # (x, gout, C, B, H, W, py, px, gin) -> (x, gout, C, B, 1, H, W, 1, py, px, gin)
        return ["sd_maxpool3d_adjoint_ndhwc_device", a[:4] + [1] + a[4:6] + [1] + a[6:]]
    if name == "sd_upcat_adjoint_ndhwc_device":            # (gcat, c0, up0, c1, B, H, W, g0, g1) -> (gcat, c0, up0, c1, B, 1, H, W, g0, g1)
        return ["sd_upcat3d_adjoint_ndhwc_device", a[:5] + [1] + a[5:]]
    return call


@pytest.fixture(scope="module")
def traces():
    from stardist_amd.build import build_lib
    build_lib(verbose=False)
    spec = importlib.util.spec_from_file_location("make_training_call_trace", os.path.join(HERE, "golden", "make_training_call_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(HERE, "golden", "training_call_trace.json")) as fh:
        want = json.load(fh)
    # through JSON as the stored ones: tuples and lists, ints and bools compare as they were written
    return want, json.loads(json.dumps(mod.record_traces()))


def test_fixture_is_the_recorded_one(traces):
    want, _ = traces
    assert sorted(want) == sorted(CASES + [c + "_nograd" for c in CASES])
    assert [len(want[c]) for c in CASES] == [115, 91, 93]
    count = lambda name: sum(c[0] == name for c in want["unet2d"])
    assert (count("sd_conv3_ndhwc_device"), count("sd_conv_wgrad_ndhwc_device"), count("sd_relu_mask_device"), count("sd_maxpool_ndhwc_device"),
            count("sd_maxpool_adjoint_ndhwc_device"), count("sd_upcat_adjoint_ndhwc_device"), count("sd_convg_ndhwc_device")) == (66, 18, 17, 4, 4, 3, 2)


@pytest.mark.parametrize("grad", [True, False], ids=["backward", "nograd"])
@pytest.mark.parametrize("case", CASES)
def test_same_calls_in_the_same_order(traces, case, grad):
    want, got = traces
    key = case if grad else case + "_nograd"
    exp = [_expected(c) for c in want[key]]
    assert len(got[key]) == len(exp)
    for i, (g, w) in enumerate(zip(got[key], exp)):
        assert g == w, (key, i, g, w)


def test_only_the_2d_adjoints_are_mapped(traces):
    want, _ = traces
    for key, calls in want.items():
        mapped = [c for c in calls if _expected(c) != c]
        assert len(mapped) == (7 if key == "unet2d" else 0), key
