"""tests/golden/uniform_batch.json: what compress_batch() of 21 equal 40 x 52 frames at one quality gave BEFORE the mixed batch existed - the
sha256 of every stream and the call's tic_last_batch_input_path / tic_last_batch_zero_copy figures.  Run on the parent commit of the mixed-batch
change (needs an MI355X); --lib names that commit's library when the tree has moved on:
    python tests/golden/gen/make_goldens_uniform_batch.py [--lib path/to/libtinyimgcodec_hip.so]
tests/test_compress_batch_mixed_gpu.py::test_uniform_call_untouched compares."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "uniform_batch.json"))
args = ap.parse_args()
os.environ.pop("TIC_TEST_HOOKS", None)
from tinyimgcodec_amd import _native as N  # noqa: E402

if args.lib:  # an older library: bind what it exports
    N.LIB_PATH = os.path.abspath(args.lib)
    older = C.CDLL(N.LIB_PATH)
    for name in [k for k in N.SIGNATURES if not hasattr(older, k)]:
        del N.SIGNATURES[name]
import tinyimgcodec_amd as T  # noqa: E402

n, h, w, q, seed = 21, 40, 52, 50, 5200
frames = [np.random.default_rng(seed + i).integers(0, 256, (h, w), dtype=np.uint8) for i in range(n)]
ctx = T.Context(0)
L = N.load()
streams = T.compress_batch(frames, q, ctx=ctx)
assert streams == [T.compress(f, q, ctx=ctx) for f in frames]
d, s, z = C.c_int(-1), C.c_int(-1), C.c_int(-1)
assert L.tic_last_batch_input_path(ctx.handle, C.byref(d), C.byref(s)) == 0 and L.tic_last_batch_zero_copy(ctx.handle, C.byref(z)) == 0
gold = {"n": n, "h": h, "w": w, "quality": q, "seed": seed, "sha256": [hashlib.sha256(b).hexdigest() for b in streams],
        "direct_frames": d.value, "staged_frames": s.value, "zero_copy": z.value, "library": L.tic_version().decode()}
with open(args.out, "w") as f:
    json.dump(gold, f, indent=0, sort_keys=True)
    f.write("\n")
print("wrote", args.out, gold["direct_frames"], gold["staged_frames"], gold["zero_copy"])
