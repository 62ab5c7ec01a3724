"""The native calls of one training step, recorded without a GPU: N.dcall is replaced by a recorder and train_loss / train_loss3d plus
loss.backward() run on CPU tensors (the outputs are uninitialised memory; the shapes, and therefore the calls, are not).  Only the host
packing functions of the built library are used.

record_traces() returns {case: [[name, [argument, ...]], ...]} for batch 2 of
  unet2d   Config2D(n_rays=32, grid=(2, 2)), 64x64
  unet3d   Config3D(n_rays=16, grid=(1, 2, 2)), 16x32x32
  resnet3d the same with backbone="resnet"
each with gradients (forward + backward) and as `<case>_nograd` under torch.no_grad() (the validation path).  An argument is "P" for a
pointer, null for None and the number itself otherwise.

usage: python tests/golden/make_training_call_trace.py   -> tests/golden/training_call_trace.json
The committed file was written at commit 02fb628 (the 2D and 3D layer sets still separate); tests/test_cpu_training_calls.py holds the
layer set of today against it, so it is regenerated only by a change that means to alter the launch sequence."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "training_call_trace.json")
BATCH = 2


def _cases():
    from stardist_amd.models import Config2D, Config3D, StarDist2D, StarDist3D
    from stardist_amd.training import train_loss
    from stardist_amd.training3d import train_loss3d
    yield ("unet2d", StarDist2D(Config2D(n_rays=32, grid=(2, 2), train_patch_size=(64, 64)), basedir=None, device="cpu", seed=0),
           train_loss, (64, 64))
    for bb in ("unet", "resnet"):
        yield (bb + "3d", StarDist3D(Config3D(n_rays=16, grid=(1, 2, 2), backbone=bb, train_patch_size=(16, 32, 32)), basedir=None,
                                     device="cpu", seed=0), train_loss3d, (16, 32, 32))


def record_traces():
    import torch
    from stardist_amd.lib import _native as N
    calls = []

    def rec(t, name, *args):
        calls.append([name, ["P" if isinstance(a, ctypes.c_void_p) else a for a in args]])
    real, N.dcall = N.dcall, rec
    try:
        traces = {}
        for case, model, loss_fn, shape in _cases():
            cfg = model.config
            sub = tuple(s // g for s, g in zip(shape, cfg.grid))
            x = torch.zeros((BATCH,) + shape + (1,))
            pt, dtm = torch.zeros((BATCH,) + sub), torch.zeros((BATCH,) + sub + (cfg.n_rays + 1,))
            for p in model.net.parameters():
                p.requires_grad_(True)
            del calls[:]
            loss_fn(model.net, cfg, x, pt, dtm)[0].backward()
            traces[case] = list(calls)
            del calls[:]
            with torch.no_grad():
                loss_fn(model.net, cfg, x, pt, dtm)
            traces[case + "_nograd"] = list(calls)
        return traces
    finally:
        N.dcall = real


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    traces = record_traces()
    with open(OUT, "w") as fh:
        fh.write("{\n" + ",\n".join(json.dumps(k) + ": [\n" + ",\n".join(json.dumps(c) for c in v) + "\n]" for k, v in traces.items()) + "\n}\n")
    for k, v in traces.items():
        print(k, len(v))
