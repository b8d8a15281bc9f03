"""Records tests/golden/encoder_errors.json: (return code, tic_last_error text) of every row of tests/encoder_error_rows.py, from the
library given with --lib (default: the product library of this tree).  The table pins what the argument checks of the encoder entry
points answered BEFORE they were folded onto shared helpers, so it is recorded from a build of the commit before that change, on a GPU:
    python tests/golden/gen/make_goldens_encoder_errors.py --lib <parent build>/libtinyimgcodec_hip.so"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from tinyimgcodec_amd import _native as N  # noqa: E402

import encoder_error_rows as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=N.LIB_PATH)
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "encoder_errors.json"))
args = ap.parse_args()
L = C.CDLL(args.lib)
for name, (res, argtypes) in N.SIGNATURES.items():
    fn = getattr(L, name)
    fn.restype, fn.argtypes = res, argtypes
handle = L.tic_create(0)
assert handle, L.tic_last_error(None).decode()
env = R.Env(L, handle)
table = R.play(env)
env.close()
L.tic_destroy(handle)
with open(args.out, "w") as f:
    json.dump({"async_slots": R.ASYNC_SLOTS, "rows": table}, f, indent=1, sort_keys=True)
    f.write("\n")
print("%d rows -> %s" % (len(table), args.out))
