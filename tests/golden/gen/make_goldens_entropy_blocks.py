#!/usr/bin/env python3
"""Golden fixture for the entropy encoder on BUILT coefficients (tests/entropy_blocks.py builds the frames; no transform made them): what
the UNMODIFIED reference's compress() writes for each, in the build container (same import recipe as make_goldens_inverse.py: stand-ins
on the path, the reference imported, only the reference's outputs stored).

    python tests/golden/gen/make_goldens_entropy_blocks.py     ->  tests/golden/entropy_blocks.json

compress() takes an image; for the duration of one call its encode() (codec.py:26-43, looked up in the module at call time, codec.py:134)
is replaced by a function that returns the built dictionary {"height", "width", "quality", "dc", "ac"}; every line that entropy codes it
(codec.py:133-164, huffman.py) is the reference's own.  Per frame: the default-table stream's length and sha256, or the class of the
exception compress() raised; the same for compress(..., auto_generate_huffman_table=True); the frame's census (asserted here).  The
default-table stream must equal oracle.pyoracle.entropy_encode byte for byte, and its length 16 + the census's payload rounded up.
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
import tinyimgcodec.codec as ref_codec  # noqa: E402

import entropy_blocks as EB  # noqa: E402
from oracle import pyoracle as O  # noqa: E402


def reference_streams(fr):
    """(default-table result, own-table result) of the reference for one built frame: bytes, or the exception's class name."""
    dc, ac = EB.dc_ac(fr["zz"])
    built = {"height": fr["h"], "width": fr["w"], "quality": fr["quality"], "dc": dc, "ac": ac}
    original = ref_codec.encode
    out = []
    for adaptive in (False, True):
        ref_codec.encode = lambda image, quality: {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in built.items()}
        try:
            out.append(ref.compress(None, fr["quality"], adaptive) if adaptive else ref.compress(None, fr["quality"]))
        except Exception as e:  # noqa: BLE001  (whatever the reference does is the record)
            out.append(type(e).__name__)
        finally:
            ref_codec.encode = original
    return out


def record(res):
    return {"raises": res} if isinstance(res, str) else {"bytes": len(res), "sha256": EB.sha(res)}


def main():
    t0 = time.perf_counter()
    L = EB.Lengths(O.dump_tables())
    frames = EB.build_frames(L)
    meta = {"generator": "tests/golden/gen/make_goldens_entropy_blocks.py", "frames": {}}
    for name, fr in frames.items():
        c = EB.census(name, fr, L)
        default, adaptive = reference_streams(fr)
        dc, ac = EB.dc_ac(fr["zz"])
        if isinstance(default, str):
            assert default == "KeyError" and EB.expected_len(c) is None, (name, default)
            try:
                O.entropy_encode(dc, ac, fr["h"], fr["w"], fr["quality"])
                raise AssertionError("the oracle encodes " + name)
            except O.OracleError:
                pass
        else:
            assert len(default) == EB.expected_len(c), (name, len(default), c)
            assert default == O.entropy_encode(dc, ac, fr["h"], fr["w"], fr["quality"]), name
        if fr["family"] == "dense_max":
            assert len(default) == 16 + (EB.MAX_BLOCK_BITS * c["blocks"] + 7) // 8, name
        if name.startswith("zeros"):
            assert len(default) == 16 + (6 * c["blocks"] + 7) // 8, name
        meta["frames"][name] = {"family": fr["family"], "h": fr["h"], "w": fr["w"], "quality": fr["quality"], "coeffs_sha256": EB.coeff_sha(fr["zz"]),
                                "stream": record(default), "adaptive": record(adaptive), "census": c}
        print("%-34s %6.1f s  %s  adaptive %s" % (name, time.perf_counter() - t0, default if isinstance(default, str) else len(default),
                                               adaptive if isinstance(adaptive, str) else len(adaptive)), flush=True)
    assert {e["family"] for e in meta["frames"].values()} == set(EB.FAMILIES)
    with open(EB.FIXTURE, "w") as f:
        json.dump(meta, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("wrote entropy_blocks.json: %d frames, %d bytes, %.0f s" % (len(frames), os.path.getsize(EB.FIXTURE), time.perf_counter() - t0))


if __name__ == "__main__":
    main()
