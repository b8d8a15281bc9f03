#!/usr/bin/env python3
"""Golden fixture for the damaged-stream corpus (tests/damaged_streams.py builds the streams): what the UNMODIFIED reference's
decompress() (codec.py:167-189) makes of every entry, in the build container (same import recipe as make_goldens_r3.py: stand-ins for the
two absent pure-container packages on the path, the reference imported, only its outputs stored).

    python tests/golden/gen/make_goldens_damaged.py     ->  tests/golden/damaged_streams.json

Per entry: name, base, kind, params (for value_flip with the block and scan position), the stream's length and sha256, and either the
geometry and sha256 of the pixels the reference returned or the class name of the exception it raised.  No stream bytes and no images:
tests/test_damaged_streams_cpu.py ties the regenerated corpus to the digests.  A few minutes (0.3 s per 256 x 256 stream).
"""
import json
import os
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLD))
sys.path.insert(0, os.path.join(HERE, "standins"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import tinyimgcodec as ref  # noqa: E402  (the unmodified reference)

import damaged_streams as D  # noqa: E402
from oracle import pyoracle as O  # noqa: E402


def outcome(data):
    try:
        px = ref.decompress(data)
    except Exception as e:  # noqa: BLE001
        return {"raises": type(e).__name__}
    assert px.dtype == np.uint8 and px.ndim == 2
    return {"h": int(px.shape[0]), "w": int(px.shape[1]), "pixels_sha256": D.px_sha(px)}


def main():
    t0 = time.perf_counter()
    bases = D.base_streams(O)
    clean = {}
    for base, s in bases.items():  # the clean streams are the reference's own, and decode to its pixels
        h, w, q, _ = D.BASES[base]
        assert ref.compress(D.base_frame(base), q) == s, base
        clean[base] = dict(outcome(s), bytes=len(s), sha256=D.sha(s))
        assert (clean[base]["h"], clean[base]["w"]) == (h, w)
    entries = D.corpus(O, bases)
    D.check_census(D.census(entries))
    records = []
    for k, (name, base, kind, params, s) in enumerate(entries):
        rec = {"name": name, "base": base, "kind": kind, "params": params, "bytes": len(s), "sha256": D.sha(s)}
        rec.update(outcome(s))
        records.append(rec)
        if k % 50 == 0:
            print("%4d / %d  %6.1f s  %s" % (k, len(entries), time.perf_counter() - t0, name), flush=True)
    meta = {"generator": "tests/golden/gen/make_goldens_damaged.py", "clean": clean, "entries": records}
    with open(D.FIXTURE, "w") as f:
        json.dump(meta, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    raised = sorted({r["raises"] for r in records if "raises" in r})
    print("wrote damaged_streams.json: %d entries, %d bytes, exceptions %s, %.0f s" % (len(records), os.path.getsize(D.FIXTURE), raised, time.perf_counter() - t0))


if __name__ == "__main__":
    main()
