#!/usr/bin/env python3
"""Golden fixture for the corpus of damaged per-image-table streams (tests/damaged_adaptive.py builds the streams and states the
decoder's contract as decode_strict): what the UNMODIFIED reference makes of every entry it can be asked about, with the import recipe
of make_goldens_damaged.py (stand-ins for the two absent pure-container packages on the path, the reference imported from its read-only
tree, only its outputs stored).

    python tests/golden/gen/make_goldens_damaged_adaptive.py     ->  tests/golden/damaged_adaptive.json

The reference's decompress() reads the flag word little-endian (codec.py:119) and so never reads the table it wrote.  Two facts give an
expectation all the same:
  the twin     a stream with its flag word rewritten as struct.pack("<I", 1 << 31) IS read by the unmodified decompress(), table and all;
               on the image bases whose codes are at most 16 bits its pixels are decode(encode(img, q)) bit for bit (asserted, "twin_equals_decode")
  the reader   read_huffman_table, then per block decode_huffman / decode_run_length behind the 16 header bytes.  CLEAN: no call raised,
               no block had more than 63 entries, buf.tell() never passed 8 * len; else the exception's class name, "over_63" or "past_end"
Both only for tables IN REACH (damaged_adaptive.reach): every code 1..16 bits (read_huffman_code stops behind 16; a code of length zero
that is not the EOB makes decode_huffman's loop spin and allocate for ever), distinct symbols and codes (a bidict holds one of each).

Everything that touches the reference runs in a CHILD process with an address-space limit and a time limit: first the tables and clean
streams of the image bases (compress(..., auto_generate_huffman_table=True)), then per entry the reader, the twin's decompress() where
decode_strict decodes an in-reach entry, and decode() of decode_strict's coefficients where it decodes one out of reach (marked
"model").  The parent never imports the reference.  It asserts (tests/test_damaged_adaptive_cpu.py asserts the same from the stored
fields, damaged_adaptive.consistency):
  in reach      decode_strict decodes if and only if the reader was clean, and then to equal coefficients; the exceptions are the
                classes where the product is stricter by design, counted by name, at most 3 % of the in-reach entries
  out of reach  the share of decoded entries (bases other than twolevel256q90, incomplete, all_long) that are out of reach is recorded
                and bounded (damaged_adaptive.OUT_OF_REACH_MAX_PERCENT)
  population    kind x outcome class is stored; every class of decode_strict has 3 entries at least; 150 entries at least decode to
                pixels other than their base's
  the model     adaptive_tables.decode_model, where the table passes the strict checks and has no code of length zero, agrees with
                decode_strict (it looks at the DC range behind the last block, decode_strict as the DC runs)
  the oracle    inverse_edges.pixels_block_idct of decode_strict's coefficients gives the stored pixels of every decoded entry

Per entry the fixture holds a row [name, bytes, sha256, outcome, reach, reader]: outcome a class name or [h, w, pixels sha256, "twin" |
"model"]; the 590 exhaustive table flips of lenna64 carry 0 for name and sha256 (the name is lenna64/table_flip/bit<128 + ordinal>, one
digest over their digests stands in "lenna64_table_flips_sha256").  No stream bytes and no images.
"""
import json
import multiprocessing
import os
import pickle
import subprocess
import sys
import tempfile
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLD))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import adaptive_tables as AT  # noqa: E402
import damaged_adaptive as DA  # noqa: E402

CHILD_ADDRESS_SPACE = 6 << 30
CHILD_SECONDS = 3600
WORKERS = 8


def coef_sha(zz):
    return DA.sha(np.ascontiguousarray(zz, dtype="<i4").tobytes())


# ---------------------------------------------------------------------------------------------------------------------------------
# the child: everything that touches the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def child_import():
    import resource

    resource.setrlimit(resource.RLIMIT_AS, (CHILD_ADDRESS_SPACE, CHILD_ADDRESS_SPACE))
    sys.path.insert(0, os.path.join(HERE, "standins"))
    sys.path.insert(0, "/root/reference")
    import tinyimgcodec as ref  # the unmodified reference

    return ref


def child_bases(ref, _):
    out = {}
    for base, (h, w, q, frame) in DA.BASES.items():
        if frame is None:
            continue
        img = DA.base_frame(base)
        s = ref.compress(img, q, auto_generate_huffman_table=True)
        px = ref.decode(dict(ref.encode(img, q), scaled_dct=False))
        tw = ref.decompress(DA.twin(s))
        out[base] = {"stream": s, "pixels_sha256": DA.px_sha(px), "twin_equals_decode": bool(np.array_equal(px, tw))}
    return out


def reader(stream, n):
    """The reference's reader, step by step -> (what it did, int64 [n, 64] with the DC integrated when clean)."""
    from tinyimgcodec.bitbuffer import BitBuffer
    from tinyimgcodec.codec import read_huffman_table
    from tinyimgcodec.constants import AC, DC
    from tinyimgcodec.huffman import decode_huffman, decode_run_length

    total = 8 * len(stream)
    buf = BitBuffer.from_bytes(stream)
    buf.seek(128)
    try:
        t = read_huffman_table(buf)
    except Exception as e:  # noqa: BLE001
        return type(e).__name__, None
    if buf.tell() > total:
        return "past_end", None
    zz = np.zeros((n, 64), np.int64)
    for i in range(n):
        try:
            zz[i, 0] = decode_huffman(buf, 1, DC, t)[0]
            row = decode_run_length(decode_huffman(buf, dc_ac=AC, category_codeword=t))
        except Exception as e:  # noqa: BLE001
            return type(e).__name__, None
        if len(row) > 63:
            return "over_63", None
        if buf.tell() > total:
            return "past_end", None
        zz[i, 1 : 1 + len(row)] = row
    zz[:, 0] = np.cumsum(zz[:, 0])
    return "clean", zz


_REF = None


def child_entry(job):
    ref = _REF
    s, (h, w, q) = job["stream"], job["hwq"]
    out = {"reader": "not_run"}
    if job["reach"] == "in":
        status, zz = reader(s, AT.blocks_of(h, w))
        out["reader"] = status
        if zz is not None:
            out["reader_coef_sha"] = coef_sha(zz)
        if job["zz"] is not None:
            px = ref.decompress(DA.twin(s))
            out["pixels"] = [int(px.shape[0]), int(px.shape[1]), DA.px_sha(px), "twin"]
    elif job["zz"] is not None:
        zz = job["zz"].astype(np.int32)
        dc = zz[:, 0].copy()
        dc[1:] = np.diff(dc)
        px = ref.decode({"height": h, "width": w, "quality": q, "scaled_dct": False, "dc": dc, "ac": np.ascontiguousarray(zz[:, 1:])})
        out["pixels"] = [int(px.shape[0]), int(px.shape[1]), DA.px_sha(px), "model"]
    if job["model"]:  # (not the reference: adaptive_tables.decode_model, here for the worker pool's sake)
        try:
            out["model"] = coef_sha(AT.decode_model(s))
        except AT.NoCode:
            out["model"] = "no_code"
        except ValueError as e:
            out["model"] = {"stream truncated": "truncated", "block of more than 63 AC coefficients": "over_63", "DC outside int16": "dc_range"}[str(e)]
    return out


def child_entries(ref, jobs):
    global _REF
    _REF = ref
    with multiprocessing.get_context("fork").Pool(min(WORKERS, os.cpu_count() or 1)) as pool:
        return pool.map(child_entry, jobs, chunksize=4)


def child_main(stage, src, dst):
    ref = child_import()
    with open(src, "rb") as f:
        payload = pickle.load(f)
    res = {"bases": child_bases, "entries": child_entries}[stage](ref, payload)
    with open(dst, "wb") as f:
        pickle.dump(res, f)


def ask_child(stage, payload):
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "in.pickle"), os.path.join(tmp, "out.pickle")
        with open(src, "wb") as f:
            pickle.dump(payload, f)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", stage, src, dst], check=True, timeout=CHILD_SECONDS)
        with open(dst, "rb") as f:
            return pickle.load(f)


# ---------------------------------------------------------------------------------------------------------------------------------
# the parent
# ---------------------------------------------------------------------------------------------------------------------------------
def main():
    import inverse_edges as IE
    from oracle import pyoracle as O

    t0 = time.perf_counter()
    O.build()
    ie = IE.Fixture()
    made = ask_child("bases", None)
    tables = {b: AT.parse(m["stream"])[3] for b, m in made.items()}
    bases = DA.base_streams(O, None, tables)
    tables_fx = AT.load_fixture()["cases"]
    info = {}
    for base, s in bases.items():
        h, w, q, frame = DA.BASES[base]
        hh, ww, qq, table, first = AT.parse(s)
        assert (hh, ww, qq) == (h, w, q), base
        lens = [len(code) for _, code in table["DC"] + table["AC"]]
        rb = AT.range_rule(len(s), first, AT.blocks_of(h, w))
        e = info[base] = {"bytes": len(s), "sha256": DA.sha(s), "h": h, "w": w, "q": q, "table_bits": first - 128, "payload_bits": len(s) * 8 - first,
                          "longest_code": max(lens), "range_bits": rb, "ranges": (len(s) * 8 - first + rb - 1) // rb}
        if frame is not None:
            assert s == made[base]["stream"], base  # the reference's own compress(..., auto_generate_huffman_table=True)
            e.update(table=AT.table_to_json(table), pixels_sha256=made[base]["pixels_sha256"], twin_equals_decode=made[base]["twin_equals_decode"])
            assert e["twin_equals_decode"] == (max(lens) <= 16), (base, max(lens))
        else:
            ref_e = tables_fx[base]["streams"]["q%d" % q]
            assert (len(s), DA.sha(s)) == (ref_e["bytes"], ref_e["sha256"]), base  # (written by the reference: make_goldens_adaptive_tables.py)
            e["pixels_sha256"] = ref_e["decoded_sha256"]
        print("%-15s %6d B, table %5d bits, longest code %2d, %4d ranges of %d bits" % (base, len(s), e["table_bits"], e["longest_code"], e["ranges"], rb), flush=True)
    assert info["lenna64"]["table_bits"] == 590 and info["noise64"]["longest_code"] > AT.K and info["twolevel256q90"]["longest_code"] > 16
    assert info["noise256"]["ranges"] == 512 and info["twolevel256"]["ranges"] == 513
    assert info["noise256"]["payload_bits"] >= 1 << 18 and info["twolevel256"]["payload_bits"] >= 1 << 18

    entries = DA.corpus(O, None, bases)
    DA.check_population(entries)
    jobs, strict = [], []
    for name, base, kind, params, s in entries:
        cls, zz = DA.outcome_class(s)
        strict.append((cls, zz))
        clean_table = cls not in DA.TABLE_CLASSES and s[12:16] == b"\x80\0\0\0"  # (decode_model asks for exactly this flag word)
        if clean_table:
            table = DA.read_table(s)[0]
            clean_table = min(len(code) for _, code in table["DC"] + table["AC"]) > 0
        h, w, q = DA.header(s)[:3] if len(s) >= 16 else (0, 0, 0)
        jobs.append({"stream": s, "hwq": (h, w, q), "reach": DA.reach(s), "zz": zz, "model": clean_table})
    print("%d entries, decode_strict done, %.0f s" % (len(entries), time.perf_counter() - t0), flush=True)
    got = ask_child("entries", jobs)
    print("the reference done, %.0f s" % (time.perf_counter() - t0), flush=True)

    rows, digests = [], []
    for (name, base, kind, params, s), job, (cls, zz), g in zip(entries, jobs, strict, got):
        if job["model"]:  # decode_model against decode_strict
            want = coef_sha(zz) if cls is None else cls
            assert g["model"] == want or (cls == "dc_range" and len(g["model"]) < 16), (name, cls, g["model"])
        if cls is None:
            outcome = g["pixels"]
            q = job["hwq"][2]
            px = IE.pixels_block_idct(ie, O, zz.astype(np.int64), job["hwq"][0], job["hwq"][1], q, 0)
            assert [int(px.shape[0]), int(px.shape[1]), DA.px_sha(px)] == outcome[:3], ("the oracle's inverse stage differs from the reference's", name)
            if job["reach"] == "in":
                assert g["reader"] == "clean" and g["reader_coef_sha"] == coef_sha(zz), (name, g)
        else:
            outcome = cls
        exhaustive = base == "lenna64" and kind == "table_flip"
        if exhaustive:
            digests.append(DA.sha(s))
        rows.append([0 if exhaustive else name, len(s), 0 if exhaustive else DA.sha(s), outcome, job["reach"], g["reader"]])
    fx = {"generator": "tests/golden/gen/make_goldens_damaged_adaptive.py", "numpy": np.__version__, "bases": info, "entries": rows,
          "lenna64_table_flips_sha256": DA.family_sha(digests)}
    rec = DA.records(fx)
    assert list(rec) == [e[0] for e in entries]
    fx["figures"] = DA.consistency([e[:3] for e in entries], rec, {b: info[b]["pixels_sha256"] for b in info})
    head = json.dumps({k: v for k, v in fx.items() if k != "entries"}, sort_keys=True, separators=(",", ":"))
    text = head[:-1] + ',"entries":[\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]}\n"
    assert json.loads(text) == json.loads(json.dumps(fx))
    with open(DA.FIXTURE, "w") as f:
        f.write(text)
    f = fx["figures"]
    print(json.dumps({k: v for k, v in f.items() if k != "census"}, indent=1))
    for kind in DA.KINDS:
        print("%-11s %s" % (kind, f["census"][kind]))
    assert len(text) < DA.MAX_FIXTURE_BYTES, len(text)
    print("wrote damaged_adaptive.json: %d entries, %d bytes, %.0f s" % (len(rows), len(text), time.perf_counter() - t0))


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--child":
        child_main(*sys.argv[2:])
    else:
        main()
