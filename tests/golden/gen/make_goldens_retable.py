#!/usr/bin/env python3
"""Golden fixture for lossless re-tabling (retable_adaptive / retable_default) over the damaged default-table corpus
(tests/damaged_streams.py builds the streams): what the UNMODIFIED reference's reader followed by its writer makes of every entry, in
the build container (same import recipe as make_goldens_damaged.py: stand-ins on the path, the reference imported, only its outputs stored).

    python tests/golden/gen/make_goldens_retable.py     ->  tests/golden/retable_damaged.json

The reader: decompress() (codec.py:167-189) with decode() - looked up in the module at call time, codec.py:189 - replaced for the call by a
function that keeps its argument: the dictionary {"height", "width", "quality", "scaled_dct", "dc", "ac"} the reference read from the stream.
The writer: compress() (codec.py:133-164) with encode() replaced for the call by a function that returns that dictionary (the device of
make_goldens_entropy_blocks.py), once with the default tables and once with auto_generate_huffman_table=True.  Every line that reads or
writes a bit is the reference's own.

Per entry: name, the input's length and sha256 (tests/golden/damaged_streams.json's), and for both re-writes the length and sha256, or the
class name of the exception.  A scaled_dct entry has no re-write by definition (the flag word has room for one family): it is recorded as
{"scaled_dct": true}.  No stream bytes.  The default re-write must equal oracle.pyoracle.entropy_encode of the same dictionary.
About 2.5 minutes.
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

import damaged_streams as D  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

FIXTURE = os.path.join(GOLD, "retable_damaged.json")


def read(data):
    """The dictionary the reference's decompress() hands to decode()."""
    kept = []
    original = ref_codec.decode
    ref_codec.decode = lambda info: kept.append(info)
    try:
        ref.decompress(data)
    finally:
        ref_codec.decode = original
    (info,) = kept
    return info


def write(info, adaptive):
    """The reference's stream of that dictionary: bytes, or the exception's class name."""
    original = ref_codec.encode
    ref_codec.encode = lambda image, quality: {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in info.items()}
    try:
        return ref.compress(None, info["quality"], adaptive)
    except Exception as e:  # noqa: BLE001  (whatever the reference does is the record)
        return type(e).__name__
    finally:
        ref_codec.encode = original


def record(res):
    return {"raises": res} if isinstance(res, str) else {"bytes": len(res), "sha256": D.sha(res)}


def main():
    t0 = time.perf_counter()
    entries = D.corpus(O, D.base_streams(O))
    with open(D.FIXTURE) as f:
        damaged = {e["name"]: e for e in json.load(f)["entries"]}
    assert [e[0] for e in entries] == list(damaged) or sorted(e[0] for e in entries) == sorted(damaged)
    records, wide, scaled, raised = [], [], 0, []
    for k, (name, base, kind, params, s) in enumerate(entries):
        assert (len(s), D.sha(s)) == (damaged[name]["bytes"], damaged[name]["sha256"]), name
        rec = {"name": name, "bytes": len(s), "sha256": D.sha(s)}
        try:
            info = read(s)
        except Exception as e:  # noqa: BLE001
            rec["read_raises"] = type(e).__name__
            raised.append(name)
            records.append(rec)
            continue
        run = np.cumsum(info["dc"].astype(np.int64))
        if run.size and (run.min() < -32768 or run.max() > 32767):
            wide.append(name)
            rec["dc_outside_int16"] = True
        if info["scaled_dct"]:
            scaled += 1
            rec["scaled_dct"] = True
        else:
            default, adaptive = write(info, False), write(info, True)
            if not isinstance(default, str):  # the canonical default-table stream of these coefficients
                assert default == O.entropy_encode(info["dc"].astype(np.int32), info["ac"].astype(np.int32), info["height"], info["width"], info["quality"]), name
            if isinstance(default, str) or isinstance(adaptive, str):
                raised.append(name)
            rec["default"] = record(default)
            rec["adaptive"] = record(adaptive)
        records.append(rec)
        if k % 50 == 0:
            print("%4d / %d  %6.1f s  %s" % (k, len(entries), time.perf_counter() - t0, name), flush=True)
    meta = {"generator": "tests/golden/gen/make_goldens_retable.py", "entries": records}
    with open(FIXTURE, "w") as f:
        json.dump(meta, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("wrote retable_damaged.json: %d entries (%d scaled_dct, %d with an exception %s, %d with a running DC outside int16 %s), %d bytes, %.0f s"
          % (len(records), scaled, len(raised), raised[:5], len(wide), wide[:5], os.path.getsize(FIXTURE), time.perf_counter() - t0))


if __name__ == "__main__":
    main()
