#!/usr/bin/env python3
"""Golden fixture for the device decoder of per-image table streams on HAND-BUILT tables (tests/adaptive_tables.py builds the tables and
the coefficients): what the UNMODIFIED reference writes for each case, with the import recipe of make_goldens_adaptive.py (stand-ins for
the two absent pure-container packages on the path, the reference imported from its read-only tree, only its outputs stored).

    python tests/golden/gen/make_goldens_adaptive_tables.py [--skip-longcode]     ->  tests/golden/adaptive_tables.json

Per case the reference's own make_header(buf, info, table) is given the table as its dict of bidicts and its encode_huffman writes the
payload, exactly as compress() strings them together (codec.py:136-164); decode(info) of the same coefficients gives the pixels the stream
holds (the reference's decompress() misreads the flag of such a stream, see make_goldens_adaptive.py).  Where every code of the table is at
most 16 bits the reference's read_huffman_table / decode_huffman / decode_run_length are run on a BitBuffer positioned behind the 16
header bytes and must return the table and the coefficients.  max_table repeats symbols under distinct codes, which no bidict holds:
adaptive_tables.write_stream alone writes it, the reference's encode_huffman confirms its payload bits, and the entry says so.  Every stream must equal adaptive_tables.write_stream's byte for byte, and
adaptive_tables.decode_model must read it back.  The rounds_* tables are the reference's calc_huffman_table of their coefficients and are
stored (codes only).  Stored besides: the census, the visibility figures (bars asserted) and stitch_model's range, range count and
changed[] - for the rounds_* cases asserted to settle where adaptive_tables.SETTLES says - and, once, stitch_model's list for the whole
long-code fixture of adaptive_streams.json (first 0 at round 280, the trace recorded in profiles/adaptive_decode.txt section 4; some
three minutes - --skip-longcode keeps the entry of the existing file).
"""
import argparse
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
from bidict import bidict  # noqa: E402
from tinyimgcodec.bitbuffer import BitBuffer  # noqa: E402
from tinyimgcodec.codec import make_header, read_huffman_table  # noqa: E402
from tinyimgcodec.constants import AC, DC  # noqa: E402
from tinyimgcodec.huffman import calc_huffman_table, decode_huffman, decode_run_length, encode_huffman, encode_run_length  # noqa: E402

import adaptive_tables as AT  # noqa: E402
import inverse_edges as IE  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

INLINE_MAX = 4096


def dc_ac(zz):
    zz = np.asarray(zz, np.int32)
    dc = zz[:, 0].copy()
    dc[1:] = np.diff(dc)
    return dc, np.ascontiguousarray(zz[:, 1:])


def bidicts(table):
    return {DC: bidict((cat, code) for cat, code in table["DC"]), AC: bidict((sym, code) for sym, code in table["AC"])}


def reference_table(zz):
    """calc_huffman_table (huffman.py:101-108) of the coefficients, in the table's own order."""
    dc, ac = dc_ac(zz)
    rle = [y for row in ac for y in encode_run_length(row)]
    t = calc_huffman_table(dc, rle)
    return {"DC": [(int(k), v) for k, v in t[DC].items()], "AC": [((int(k[0]), int(k[1])), v) for k, v in t[AC].items()]}


def reference_stream(table, zz, h, w, q):
    dc, ac = dc_ac(zz)
    t = bidicts(table)
    buf = BitBuffer()
    make_header(buf, {"height": h, "width": w, "quality": q}, t)
    for i in range(len(dc)):
        encode_huffman(buf, dc[i : i + 1], dc_ac=DC, category_codeword=t)
        encode_huffman(buf, encode_run_length(ac[i]), dc_ac=AC, category_codeword=t)
    return buf.to_bytes()


def reference_reads_back(stream, table, zz):
    """read_huffman_table, decode_huffman and decode_run_length of the reference behind the 16 header bytes."""
    dc, ac = dc_ac(zz)
    buf = BitBuffer.from_bytes(stream)
    buf.seek(128)
    t = read_huffman_table(buf)
    assert [(int(k), v) for k, v in t[DC].items()] == table["DC"] and [((int(k[0]), int(k[1])), v) for k, v in t[AC].items()] == table["AC"]
    for i in range(len(dc)):
        assert decode_huffman(buf, 1, DC, t)[0] == dc[i], i
        row = decode_run_length(decode_huffman(buf, dc_ac=AC, category_codeword=t))
        assert len(row) <= 63 and list(row) == ac[i, : len(row)].tolist() and not ac[i, len(row):].any(), i
    return True


def reference_writes_the_payload(table, zz, h, w, q, s):
    """max_table: 256 AC entries over 20 symbols.  The reference's table is a dict of bidicts, one code per symbol, so make_header cannot be
    given it; given the entry write_stream codes each symbol with (the last), the reference's encode_huffman writes the same payload."""
    t = bidicts(table)
    assert len(t[AC]) < len(table["AC"]) == 256 and all(dict(table["AC"])[y] == code for y, code in t[AC].items())
    r = reference_stream({"DC": table["DC"], "AC": list(t[AC].items())}, zz, h, w, q)
    n = AT.symbol_starts(table, zz)[1]
    p, pr = AT.parse(s)[4], AT.parse(r)[4]
    assert p != pr and AT.bit_string(s)[p : p + n] == AT.bit_string(r)[pr : pr + n] and len(s) * 8 - (p + n) < 8 and len(r) * 8 - (pr + n) < 8
    return True


def pixels(zz, h, w, q):
    dc, ac = dc_ac(zz)
    return ref.decode({"height": h, "width": w, "quality": q, "scaled_dct": False, "dc": dc, "ac": ac})


def make_case(name, case, ie):
    t0 = time.perf_counter()
    table, zz, h, w = case["table"], case["zz"], case["h"], case["w"]
    e = {"height": h, "width": w, "blocks": int(len(zz)), "qualities": case["qualities"], "well_formed": case["well_formed"],
         "coeffs_sha256": AT.sha(np.ascontiguousarray(zz, dtype="<i2").tobytes()), "streams": {}}
    first = None
    for q in case["qualities"]:
        if first is not None:
            s = AT.with_quality(first, q)
        elif name == "max_table":
            s = first = AT.write_stream(table, zz, h, w, q)
            e["reference_wrote_it"] = False
            e["reference_wrote_the_payload"] = reference_writes_the_payload(table, zz, h, w, q, s)
        else:
            s = first = reference_stream(table, zz, h, w, q)
            assert s == AT.write_stream(table, zz, h, w, q), name
        if name == "damaged_chain":
            s, e["flipped_bit"] = AT.damage(s)
        e["streams"]["q%d" % q] = {"bytes": len(s), "sha256": AT.sha(s)}
        if case["well_formed"]:
            e["streams"]["q%d" % q]["decoded_sha256"] = AT.sha(np.ascontiguousarray(pixels(zz, h, w, q)).tobytes())
    s = AT.stream_of(name, case)
    assert AT.sha(s) == e["streams"]["q%d" % case["qualities"][0]]["sha256"], name
    if len(s) <= INLINE_MAX:
        e["stream"] = s.hex()
    if name == "too_wide":
        e["reference_wrote_it"] = True
        e["census"] = AT.census(name, case)
    else:
        if case["well_formed"]:
            assert np.array_equal(AT.decode_model(s), zz), name
        e["reference_reads_back"] = False
        if max(len(code) for _, code in table["DC"] + table["AC"]) <= 16 and name != "damaged_chain":
            e["reference_reads_back"] = reference_reads_back(s, table, zz)
        e["census"] = AT.census(name, case, s)
    if name.startswith("rounds_"):
        e["table"] = AT.table_to_json(table)
        AT.check_settles(name, e["census"]["changed"])
    if name in AT.VALUE_CASES:
        e["visibility"] = {}
        for part in AT.parts_of(name):
            v = e["visibility"][part] = AT.visibility(ie, O, case, part)
            AT.check_bars(name, v, part)
    print("%s: %d blocks, %d bytes, changed %s, %.0f s" % (name, len(zz), len(s), e["census"].get("changed"), time.perf_counter() - t0), flush=True)
    return e


def longcode_model():
    zz = AT.longcode_coeffs()
    table = reference_table(zz)
    s = AT.write_stream(table, zz, 8, 8 * len(zz), 50)
    with open(os.path.join(GOLD, "adaptive_streams.json")) as f:
        lc = json.load(f)["longcode"]
    assert (len(s), AT.sha(s)) == (lc["bytes"], lc["sha256"])
    rb, nr, changed = AT.stitch_model(s)
    assert changed.index(0) == 280 and changed[1:4] == [7891, 7169, 6913] and changed[-4:] == [512, 409, 153, 0], changed
    return {"bytes": len(s), "sha256": AT.sha(s), "range_bits": rb, "nranges": nr, "changed": changed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-longcode", action="store_true")
    args = ap.parse_args()
    t0 = time.perf_counter()
    O.build()
    ie = IE.Fixture()
    out = os.path.join(GOLD, "adaptive_tables.json")
    tables = {name: reference_table(AT.rounds_coeffs(name)) for name in AT.ROUNDS}
    cases = AT.build_cases(tables)
    res = {"generator": "tests/golden/gen/make_goldens_adaptive_tables.py", "numpy": np.__version__, "cases": {}}
    for name, case in cases.items():
        res["cases"][name] = make_case(name, case, ie)
    if args.skip_longcode:
        with open(out) as f:
            res["longcode_model"] = json.load(f)["longcode_model"]
    else:
        res["longcode_model"] = longcode_model()
    with open(out, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote adaptive_tables.json, %.0f s" % (time.perf_counter() - t0))


if __name__ == "__main__":
    main()
