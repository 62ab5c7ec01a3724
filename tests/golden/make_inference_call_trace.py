"""The native calls of whole inference passes, recorded without a GPU: N.dcall is replaced by a recorder, the "is this tensor on the
device" predicate of stardist_amd/models/native_layers.py answers yes, and StarDistNet.forward runs on CPU tensors under
torch.no_grad() (the outputs are uninitialised memory; the shapes, the kernel forms and therefore the calls are not).  Only the host
packing functions of the built library are used.

record_traces() returns {"<case>/<mode>/<pass>": {"calls": [[name, [argument, ...]], ...], "state": {...}}} for models built with
seed=0 on device="cpu":
  unet2d         default Config2D(n_rays=32), 64x64; passes dense, sparse (sparse_head=True) and lazy (sparse_head=True with
                 net.lazy_features_min_bytes = 0: the store-less features layer; the row path behind it is not part of the forward)
  unet2d_grid    grid=(2, 2)
  unet2d_48      unet_n_filter_base=48 (the up levels through sd_upcat_ndhwc_device and the general kernel)
  unet2d_bn      unet_batch_norm=True, net.eval()
  unet2d_cls     n_classes=2
  unet3d         Config3D(n_rays=16, grid=(1, 2, 2)), 16x32x32
  resnet3d       the same with backbone="resnet"
each under force_conv_mode "f16x3" with force_split16(True) ("f16x3+split16") and force_split16(False) ("f16x3"), "bf16x6" and "hand",
every pass on a model of its own.  Two stateful cases on the default 2D net, "f16x3+split16":
  unet2d_pinned  backbone.middle[0]'s convolution carries _sd_force_form = "bf16x6": it unpacks the pooled split16 tensor, its producer's
                 _sd_split_out is cleared and split16_replan() is true after the pass
  unet2d_range   backbone.down[1][1]'s kernel is filled with 1e5 (beyond the fp16 range): the layer takes the bf16x6 entry
An argument is "P" for a pointer, null for None and the number itself otherwise.  "state" holds what StarDistBase._net_forward relies on
after the pass: the names of the convolutions with _sd_split_out set, per producer the names of its _sd_consumers, and split16_replan().
Every whole-network pass could be recorded; nothing is traced layer by layer.

usage: python tests/golden/make_inference_call_trace.py   -> tests/golden/inference_call_trace.json
The committed file was written at commit e7a90ff (_hand_conv still one function in models/unet.py; recorded there by deleting the
is_cuda checks from the functions' source text, as the dispatch test of that commit did); tests/test_cpu_inference_calls.py holds
the classify / plan / launch dispatcher of today against it, so it is regenerated only by a change that means to alter the launch
sequence."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "inference_call_trace.json")
MODES = [("f16x3+split16", "f16x3", True), ("f16x3", "f16x3", False), ("bf16x6", "bf16x6", True), ("hand", "hand", True)]


def _cases():
    """(case, model factory, input shape, passes); a pass = (name, sparse_head, function preparing the net)"""
    from stardist_amd.models import Config2D, Config3D, StarDist2D, StarDist3D
    dense = ("dense", False, None)

    def lazy(net):
        net.lazy_features_min_bytes = 0
    m2 = lambda **kw: (lambda: StarDist2D(Config2D(n_rays=32, **kw), basedir=None, device="cpu", seed=0))
    m3 = lambda **kw: (lambda: StarDist3D(Config3D(n_rays=16, grid=(1, 2, 2), **kw), basedir=None, device="cpu", seed=0))
    yield "unet2d", m2(), (64, 64), [dense, ("sparse", True, None), ("lazy", True, lazy)]
    yield "unet2d_grid", m2(grid=(2, 2)), (64, 64), [dense]
    yield "unet2d_48", m2(unet_n_filter_base=48), (64, 64), [dense]
    yield "unet2d_bn", m2(unet_batch_norm=True), (64, 64), [dense]
    yield "unet2d_cls", m2(n_classes=2), (64, 64), [dense]
    yield "unet3d", m3(), (16, 32, 32), [dense]
    yield "resnet3d", m3(backbone="resnet"), (16, 32, 32), [dense]

    def pinned(net):
        net.backbone.middle[0][0].__dict__["_sd_force_form"] = "bf16x6"

    def out_of_range(net):
        net.backbone.down[1][1][0].weight.fill_(1e5)
    yield "unet2d_pinned", m2(), (64, 64), [("dense", False, pinned)]
    yield "unet2d_range", m2(), (64, 64), [("dense", False, out_of_range)]


def _state(net, NL):
    names = {m: n for n, m in net.named_modules()}
    convs = [m for m in names if "_sd_split_out" in m.__dict__ or "_sd_consumers" in m.__dict__]
    return {"split_out": sorted(names[m] for m in convs if m.__dict__.get("_sd_split_out")),
            "consumers": {names[m]: sorted(names[c] for c in m.__dict__["_sd_consumers"]) for m in convs if m.__dict__.get("_sd_consumers")},
            "replan": bool(NL.split16_replan())}


def record_traces():
    import torch
    from stardist_amd.lib import _native as N
    from stardist_amd.models import native_layers as NL
    calls = []

    def rec(t, name, *args):
        calls.append([name, ["P" if isinstance(a, ctypes.c_void_p) else a for a in args]])
    saved = N.dcall, NL._on_device, NL._flag_ptr
    N.dcall, NL._on_device, NL._flag_ptr = rec, (lambda t: True), (lambda conv, device: 12345)
    try:
        traces = {}
        for case, make, shape, passes in _cases():
            for key, mode, split in (MODES if case not in ("unet2d_pinned", "unet2d_range") else MODES[:1]):
                for pname, sparse, prepare in passes:
                    net = make().net.eval()
                    with torch.no_grad(), NL.force_conv_mode(mode), NL.force_split16(split):
                        if prepare is not None:
                            prepare(net)
                        NL.split16_replan(False)
                        del calls[:]
                        net(torch.zeros((1, 1) + shape), sparse_head=sparse)
                        traces["%s/%s/%s" % (case, key, pname)] = {"calls": list(calls), "state": _state(net, NL)}
                        NL.split16_replan(False)
        return traces
    finally:
        N.dcall, NL._on_device, NL._flag_ptr = saved


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    traces = record_traces()
    with open(OUT, "w") as fh:
        fh.write("{\n" + ",\n".join(json.dumps(k) + ': {"state": ' + json.dumps(v["state"], sort_keys=True) + ', "calls": [\n'
                                   + ",\n".join(json.dumps(c) for c in v["calls"]) + "\n]}" for k, v in traces.items()) + "\n}\n")
    for k, v in traces.items():
        print(k, len(v["calls"]))
