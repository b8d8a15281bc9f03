#!/usr/bin/env python3
"""Golden fixture for requantisation (requantize_zz / requantize / requantized_sizes / requantize_to_size): what the UNMODIFIED reference
computes, in the build container (same import recipe as make_goldens_retable.py: stand-ins on the path, the reference imported, only its
outputs stored).

    python tests/golden/gen/make_goldens_requantize.py     ->  tests/golden/requantize.json

The stage: the reference's own block_quantize(block_quantize(c, q1, inverse=True), q2) (utils.py:48-53) on 8 x 8 blocks in natural order.

Part 1, "pairs": the built corpus of tests/requantize_common.py at every pair of RC.pairs().  Per pair the sha256 of the reference's result
in zig-zag order as little-endian int32 (whole corpus, and its Latin part alone), the count of results outside int16 (the same two), the
count of exact ties (c f1 / f2 in rational arithmetic ends in one half) and the count of elements at which the rational mutant and the
round-half-away mutant of RC differ from the reference.  RC.model - plain numpy - must equal the reference everywhere.

Part 2, "streams": six small images compressed by the reference at three qualities; each stream read by the reference's reader (decode()
replaced for the call, the device of make_goldens_retable.py), its dictionary requantised by the reference's block_quantize at five
target qualities and DPCM'd again, and written by the reference's own compress() (encode() replaced for the call) with the default tables and
with the image's own: length and sha256, or the class name of the exception.  The default-table stream must equal
oracle.pyoracle.entropy_encode of the same arrays.  Part 3, "size_tables": len() of the default-table stream for q = 1..99 of two of them
(-1 where the reference raises).  No stream bytes, no coefficients.  About one minute.
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
from tinyimgcodec.constants import ZIGZAG_ORDER  # noqa: E402
from tinyimgcodec.utils import block_quantize  # noqa: E402

import requantize_common as RC  # noqa: E402
from oracle import pyoracle as O  # noqa: E402


def ref_requantize(zz, q1, q2):
    """The reference's stage on zz16 rows -> int64 [n, 64] in zig-zag order."""
    nat = np.zeros(zz.shape, np.int32)
    nat[:, ZIGZAG_ORDER] = zz  # as decode(), codec.py:58
    out = block_quantize(block_quantize(nat.reshape(-1, 8, 8), q1, inverse=True), q2)
    return out.reshape(-1, 64)[:, ZIGZAG_ORDER].astype(np.int64)  # as encode(), codec.py:32-33


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
    return {"raises": res} if isinstance(res, str) else {"bytes": len(res), "sha256": RC.sha(res)}


def requantized(info, q2):
    """The reader's dictionary at quality q2: cumsum, the reference's stage, DPCM again."""
    n = info["dc"].shape[0]
    zz = np.zeros((n, 64), np.int32)
    zz[:, 0] = np.cumsum(info["dc"])
    zz[:, 1:] = info["ac"]
    r = ref_requantize(zz, info["quality"], q2)
    dc = r[:, 0].copy()
    dc[1:] = np.diff(r[:, 0])
    return {"height": info["height"], "width": info["width"], "quality": q2, "scaled_dct": False, "dc": dc.astype(np.int32),
            "ac": r[:, 1:].astype(np.int32)}, zz


def main():
    t0 = time.perf_counter()
    assert list(ZIGZAG_ORDER) == list(RC.ZIGZAG)
    zz = RC.corpus()
    RC.check_corpus(zz)
    pair_recs, totals = [], {"ties": 0, "rational_differs": 0, "away_differs": 0, "pairs_outside_latin": 0}
    for q1, q2 in RC.pairs():
        r = ref_requantize(zz, q1, q2)
        assert np.array_equal(r, RC.model(zz, q1, q2)), (q1, q2)
        if q1 == q2:
            assert np.array_equal(r, zz), (q1, q2)  # identity
        rat, tie = RC.model_rational(zz, q1, q2)
        rec = {"from": q1, "to": q2, "sha256": RC.digest(r), "sha256_latin": RC.digest(r[:RC.N_LATIN]), "outside_int16": RC.outside_int16(r),
               "outside_int16_latin": RC.outside_int16(r[:RC.N_LATIN]), "ties": int(tie.sum()), "rational_differs": int((rat != r).sum()),
               "away_differs": int((RC.model(zz, q1, q2, "away") != r).sum())}
        for k in ("ties", "rational_differs", "away_differs"):
            totals[k] += rec[k]
        totals["pairs_outside_latin"] += rec["outside_int16_latin"] > 0
        pair_recs.append(rec)
    by = {(p["from"], p["to"]): p for p in pair_recs}
    assert by[(50, 25)]["ties"] > 0 and totals["rational_differs"] > 0 and totals["away_differs"] > 0, totals
    print("pairs: %d, %r, %.1f s" % (len(pair_recs), totals, time.perf_counter() - t0), flush=True)

    stream_recs, tables = [], {}
    for name, img in RC.images().items():
        for q1 in RC.STREAM_Q_FROM:
            s = ref.compress(img, q1)
            assert s == O.compress(img, q1), (name, q1)
            info = read(s)
            rec = {"image": name, "h": int(img.shape[0]), "w": int(img.shape[1]), "from": q1, "bytes": len(s), "sha256": RC.sha(s), "to": {}}
            for q2 in RC.STREAM_Q_TO:
                info2, zz_in = requantized(info, q2)
                mine = RC.requantized_info(zz_in, info, q2)
                assert np.array_equal(mine["dc"], info2["dc"]) and np.array_equal(mine["ac"], info2["ac"])
                default, adaptive = write(info2, False), write(info2, True)
                if not isinstance(default, str):
                    assert default == O.entropy_encode(info2["dc"], info2["ac"], info2["height"], info2["width"], q2), (name, q1, q2)
                if q2 == q1:
                    assert default == s, (name, q1)
                rec["to"][str(q2)] = {"default": record(default), "adaptive": record(adaptive)}
            stream_recs.append(rec)
            if (name, q1) in RC.SIZE_TABLES:
                sizes = [0]  # index = quality
                for q2 in range(1, 100):
                    res = write(requantized(info, q2)[0], False)
                    sizes.append(-1 if isinstance(res, str) else len(res))
                tables["%s@%d" % (name, q1)] = sizes
        print("%s  %.1f s" % (name, time.perf_counter() - t0), flush=True)
    assert len(tables) == len(RC.SIZE_TABLES)
    meta = {"generator": "tests/golden/gen/make_goldens_requantize.py", "numpy": np.__version__, "corpus_sha256": RC.digest(zz), "totals": totals,
            "pairs": pair_recs, "streams": stream_recs, "size_tables": tables}
    with open(RC.FIXTURE, "w") as f:
        json.dump(meta, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("wrote requantize.json: %d pairs, %d streams, %d bytes, %.0f s" % (len(pair_recs), len(stream_recs), os.path.getsize(RC.FIXTURE), time.perf_counter() - t0))


if __name__ == "__main__":
    main()
