"""CPU: the native calls of an inference pass are a fixed sequence.
tests/golden/inference_call_trace.json holds, for whole StarDistNet.forward passes of 2D U-Nets (default, grid, 48 filters, batch norm,
multi-class), a 3D U-Net and a 3D ResNet in every convolution mode, with and without split16 activations, every call made through
N.dcall (name, integer and float arguments, which arguments are pointers and which None), and the per-module state a pass leaves
behind (_sd_split_out, _sd_consumers, the replan request).  It was recorded (tests/golden/make_inference_call_trace.py) when
_hand_conv was one function in models/unet.py; the classify / plan / launch dispatcher of models/native_layers.py must launch the
same kernels in the same order with the same arguments.  No difference is allowed."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ["f16x3+split16", "f16x3", "bf16x6", "hand"]
CASES = (["unet2d/%s/%s" % (m, p) for m in MODES for p in ("dense", "sparse", "lazy")]
         + ["%s/%s/dense" % (c, m) for c in ("unet2d_grid", "unet2d_48", "unet2d_bn", "unet2d_cls", "unet3d", "resnet3d") for m in MODES]
         + ["unet2d_pinned/f16x3+split16/dense", "unet2d_range/f16x3+split16/dense"])


@pytest.fixture(scope="module")
def traces():
    from stardist_amd.build import build_lib
    build_lib(verbose=False)
    spec = importlib.util.spec_from_file_location("make_inference_call_trace", os.path.join(HERE, "golden", "make_inference_call_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(HERE, "golden", "inference_call_trace.json")) as fh:
        want = json.load(fh)
    saved = {k: os.environ.pop(k, None) for k in ("STARDIST_AMD_CONV", "STARDIST_AMD_SPLIT16", "STARDIST_AMD_LAZY_FEATURES")}
    try:
        # through JSON as the stored ones: tuples and lists, ints and bools compare as they were written
        return want, json.loads(json.dumps(mod.record_traces()))
    finally:
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def test_fixture_is_the_recorded_one(traces):
    want, _ = traces
    assert sorted(want) == sorted(CASES)
    names = lambda key: [c[0] for c in want[key]["calls"]]
    count = lambda key, name: names(key).count(name)
    # every entry-point shape of the 3x3 family is in the recording, and the general kernel, the pooling forms and the heads
    k = "unet2d/f16x3+split16/dense"
    assert len(want[k]["calls"]) == 20 and (count(k, "sd_conv3_c1x32_split16_device"), count(k, "sd_conv3_f16x3_fmt_ndhwc_device"),
                                            count(k, "sd_maxpool_split16_ndhwc_device")) == (1, 14, 3)
    assert names(k)[-2:] == ["sd_dot_combine_device", "sd_head_rows_device"] and len(want[k]["state"]["split_out"]) == 14
    assert want["unet2d/f16x3+split16/lazy"]["calls"][-2][1][14:17] == [None, 1, 0]          # the features layer without its store
    assert (count("unet2d/f16x3/dense", "sd_conv3_f16x3_res_ndhwc_device"), count("unet2d/f16x3/dense", "sd_conv3_f16x3_dot_ndhwc_device")) == (13, 1)
    assert count("unet2d/bf16x6/dense", "sd_conv3_bf16x6_res_ndhwc_device") == 14 and count("unet2d/hand/dense", "sd_conv3_res_ndhwc_device") == 15
    assert (count("unet2d_48/f16x3/dense", "sd_upcat_ndhwc_device"), count("unet2d_48/f16x3/dense", "sd_convg_ndhwc_device")) == (1, 6)
    assert count("resnet3d/f16x3/dense", "sd_convg_ndhwc_device") == 6 and count("unet2d_cls/f16x3/dense", "sd_convg_ndhwc_device") == 1
    # the pinned consumer unpacks, runs on the bf16x6 entry, clears its producer's mark and asks for the pass to be repeated
    p = want["unet2d_pinned/f16x3+split16/dense"]
    i = names("unet2d_pinned/f16x3+split16/dense").index("sd_split16_unpack_device")
    assert p["calls"][i + 1][0] == "sd_conv3_bf16x6_res_ndhwc_device" and p["state"]["replan"] is True
    assert "backbone.down.2.1.0" not in p["state"]["split_out"] and "backbone.down.2.1.0" in want[k]["state"]["split_out"]
    assert p["state"]["consumers"]["backbone.down.2.1.0"] == ["backbone.middle.0.0", "backbone.up.0.0.0"]
    # weights beyond the fp16 range: that layer alone on the bf16x6 entry
    assert count("unet2d_range/f16x3+split16/dense", "sd_conv3_bf16x6_res_ndhwc_device") == 1
    assert all(not want[c]["state"]["replan"] for c in CASES if not c.startswith(("unet2d_pinned", "unet2d_range")))


@pytest.mark.parametrize("case", CASES)
def test_same_calls_in_the_same_order(traces, case):
    want, got = traces
    assert len(got[case]["calls"]) == len(want[case]["calls"])
    for i, (g, w) in enumerate(zip(got[case]["calls"], want[case]["calls"])):
        assert g == w, (case, i, g, w)


@pytest.mark.parametrize("case", CASES)
def test_same_state_after_the_pass(traces, case):
    want, got = traces
    assert got[case]["state"] == want[case]["state"]
