"""Phase profile of one bound-slot sweep on the device (tools/beam_phase_profile.hip: clip_beam.h compiled with clock stamps at its
phase boundaries), on the pairs of tools/time_clip_latency.py.
    python tools/beam_phase_profile.py build [extra hipcc flags]     compile tools/bin/libbeam_phase[_TAG].so (no GPU needed)
    python tools/beam_phase_profile.py [n ...]                        run: n pairs per launch (default 1 64 16384)
BEAM_PHASE_TAG=NAME selects tools/bin/libbeam_phase_NAME.so (a variant built with extra flags)."""
import ctypes
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TAG = os.environ.get("BEAM_PHASE_TAG", "")
LIB = os.path.join(HERE, "bin", "libbeam_phase%s.so" % ("_" + TAG if TAG else ""))
PHASES = ["prepare both polygons (AddPath; the probe's own, not part of the NMS kernel)", "reset + merged local-minima list",
          "insert_local_minima_into_ael", "pop_scanbeam", "process_horizontals (bottom of the beam)", "build_intersect_list (TopX of every edge + bubble sort)",
          "fixup order + intersect_edges of the list", "top of scan-beam: maxima / horizontal successors / Curr", "top of scan-beam: process_horizontals",
          "top of scan-beam: intermediate vertices (UpdateEdgeIntoAEL)", "after the last beam"]


def build(extra):
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-I" + os.path.join(ROOT, "include")] + extra + \
          [os.path.join(HERE, "beam_phase_profile.hip"), "-o", LIB]
    print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)


def run(ns):
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from _clip_pairs import R, make_pairs
    lib = ctypes.CDLL(LIB)
    vp = ctypes.c_void_p
    lib.beam_phase_profile.argtypes = [vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_longlong, vp, vp, vp, vp]
    rows = lib.beam_phase_rows(); rec = lib.beam_phase_prep_bytes()
    dev = torch.device("cuda:0")
    P = make_pairs()
    print("library %s" % os.path.relpath(LIB, ROOT))
    for n in ns:
        T = [torch.from_numpy(np.ascontiguousarray(a[:n])).to(dev) for a in P]
        prep = torch.zeros(2 * n * rec, dtype=torch.uint8, device=dev)
        tw = torch.zeros(n, dtype=torch.int64, device=dev); fl = torch.zeros(n, dtype=torch.int32, device=dev)
        prof = torch.zeros(n * rows, dtype=torch.int64, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = 1e9
        for rep in range(3):
            e0.record()
            rc = lib.beam_phase_profile(T[0].data_ptr(), T[1].data_ptr(), T[2].data_ptr(), T[3].data_ptr(), n, R, prep.data_ptr(), prep.numel(),
                                        tw.data_ptr(), fl.data_ptr(), prof.data_ptr(), torch.cuda.current_stream().cuda_stream)
            e1.record(); e1.synchronize()
            if rc < 0:
                raise SystemExit("beam_phase_profile failed: %d" % rc)
            best = min(best, e0.elapsed_time(e1))
        pr = prof.cpu().numpy().reshape(n, rows).astype(np.float64)
        total = pr[:, rows - 1]; stamps = pr[:, rows - 2]; ph = pr[:, :len(PHASES)]
        slow = int(np.argmax(total))
        print("\nn = %d pairs, %d bytes of LDS per pair: launch %.3f ms with stamps; slowest lane %.0f ticks = %.2f GHz x launch time; %.0f stamps per lane (mean), flagged pairs %d"
              % (n, rc, best, total[slow], total[slow] / best * 1e-6, stamps.mean(), int((fl.cpu().numpy() != 0).sum())))
        print("   share of a lane's ticks (mean over lanes | slowest lane); the rest is the stamps themselves")
        for k, name in enumerate(PHASES):
            print("   %5.1f %% | %5.1f %%  %9.0f ticks  %s" % (100 * ph[:, k].sum() / total.sum(), 100 * ph[slow, k] / total[slow], ph[:, k].mean(), name))
        print("   %5.1f %% | %5.1f %%  in the stamps" % (100 * (1 - ph.sum() / total.sum()), 100 * (1 - ph[slow].sum() / total[slow])))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build(sys.argv[2:])
    else:
        run([int(a) for a in sys.argv[1:]] or [1, 64, 16384])
