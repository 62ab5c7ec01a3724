"""Record what the 2D NMS gives on the scene of tests/test_gpu_beam_families.py (keep flags, pair counts; default and nms2d_strict) as JSON:
    python tools/record_nms2d_scene_golden.py OUT.json [TEST_FILE]
Run at the commit whose results are to be pinned (the test file may be given from another checkout: only its scene and its runner are
used, the library is the one of the tree this script lies in)."""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
test_file = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "test_gpu_beam_families.py")
spec = importlib.util.spec_from_file_location("scene", test_file)
scene = importlib.util.module_from_spec(spec)
spec.loader.exec_module(scene)
out = {"default": scene.run_nms_scene(0), "strict": scene.run_nms_scene(1)}
with open(sys.argv[1], "w") as fh:
    json.dump(out, fh, indent=1)
print({k: {a: b for a, b in v.items() if a != "keep_bits"} for k, v in out.items()})
