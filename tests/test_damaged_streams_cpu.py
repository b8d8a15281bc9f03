"""The damaged-stream corpus (tests/damaged_streams.py) on the CPU: the generator reproduces the fixture's streams and meets the census
conditions; the value flips leave the chain of block starts alone and a DC flip moves every later block; the ORACLE gives what the
unmodified reference gave for every entry (tests/golden/damaged_streams.json, written by tests/golden/gen/make_goldens_damaged.py:
472 more reference results the oracle is pinned on); and the product's host decoder, built with AddressSanitizer + UBSan, decodes every
entry to the oracle's pixels from exact-size heap buffers (tests/native/damaged_selftest.cpp)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import damaged_streams as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The entries whose tails go through tic::entropy_decode_tail: a DC flip per base (the clean chain, a changed running DC), cut tails
# (the last block starts, and the stream ends inside it) and flips inside the last 2,048 bits.
TAIL_ENTRIES = ("noise64/value_flip/dc0", "noise40x72/value_flip/dc0", "ragged17x33/value_flip/dc0", "lenna64/value_flip/dc0", "noise256/value_flip/dc0",
                "twolevel256/value_flip/dc0", "noise64/cut/one_short", "noise256/cut/tail0", "noise64/flip1/tail0", "twolevel256/flip1/last_bit")


@pytest.fixture(scope="module")
def fixture():
    return D.load_fixture()


@pytest.fixture(scope="module")
def entries(oracle):
    return D.corpus(oracle)


def test_generator_reproduces_the_fixture(oracle, entries, fixture):
    """Same names in the same order, every stream's length and sha256; the clean bases too.  The census conditions hold: at least 400
    entries, every kind on every base it applies to, at least half of them offered to the device decoder (block floor at 1)."""
    recs = fixture["entries"]
    assert [e[0] for e in entries] == [r["name"] for r in recs]
    for (name, base, kind, params, s), r in zip(entries, recs):
        assert (base, kind, params, len(s), D.sha(s)) == (r["base"], r["kind"], r["params"], r["bytes"], r["sha256"]), name
    for base, s in D.base_streams(oracle).items():
        c = fixture["clean"][base]
        assert (len(s), D.sha(s)) == (c["bytes"], c["sha256"]) and (c["h"], c["w"]) == D.BASES[base][:2], base
    c = D.census(entries)
    D.check_census(c)
    assert c["entries"] == len(recs) >= D.MIN_ENTRIES
    # nothing the product treats differently from the reference on purpose
    for name, base, kind, params, s in entries:
        h, w, q, flag = D.header(s)
        assert len(s) >= 16 and flag in (0, D.SCALED) and 1 <= q <= (62 if flag else 99) and h >= 1 and w >= 1, name
    # (value_flip records carry the block and the scan position)
    assert all({"block", "scan"} <= set(r["params"]) for r in recs if r["kind"] == "value_flip")


def test_value_flips_keep_the_chain_and_a_dc_flip_moves_every_later_block(oracle, entries):
    """By construction a value flip changes no code length: the walker finds every block of the damaged stream where the clean stream
    has it (so a device decoder has nothing to flag and finishes the stream itself).  The AC flips change their own block's pixels and
    no other block's; a DC flip changes the pixels of its block and of EVERY later block (the running sum)."""
    tables = D.Tables(oracle.dump_tables())
    bases = D.base_streams(oracle)
    clean_walk = {b: D.walk(tables, s) for b, s in bases.items()}
    clean_px = {b: oracle.decompress(s) for b, s in bases.items()}
    seen = 0
    for name, base, kind, params, s in entries:
        if kind != "value_flip":
            continue
        seen += 1
        blocks, end = D.walk(tables, s)
        assert D.starts(blocks) == D.starts(clean_walk[base][0]) and end == clean_walk[base][1], name
        h, w = D.BASES[base][:2]
        bw = (w + 7) // 8
        px = oracle.decompress(s)
        changed = [not np.array_equal(px[8 * (b // bw):8 * (b // bw) + 8, 8 * (b % bw):8 * (b % bw) + 8],
                                      clean_px[base][8 * (b // bw):8 * (b // bw) + 8, 8 * (b % bw):8 * (b % bw) + 8]) for b in range(D.nblocks(h, w))]
        if params["scan"] == 0:
            assert params["block"] < max(1, D.nblocks(h, w) // 4), name
            assert changed == [b >= params["block"] for b in range(len(changed))], (name, [b for b, c in enumerate(changed) if not c])
        else:
            assert changed == [b == params["block"] for b in range(len(changed))], name
    assert seen == 5 * len(D.BASES)


def test_oracle_gives_the_references_result_for_every_entry(oracle, entries, fixture):
    """Digest or exception: where the reference raised (struct.error / ValueError, as in test_oracle_golden.py::test_decoder_edges_round3)
    the oracle reports an error, everywhere else it decodes to the reference's geometry and pixels."""
    wrong = []
    for (name, base, kind, params, s), r in zip(entries, fixture["entries"]):
        if "raises" in r:
            assert r["raises"] in ("error", "ValueError"), name
            with pytest.raises(oracle.OracleError):
                oracle.decompress(s)
            continue
        try:
            px = oracle.decompress(s)
        except oracle.OracleError as e:
            wrong.append((name, "OracleError %d" % e.code))
            continue
        if px.shape != (r["h"], r["w"]) or D.px_sha(px) != r["pixels_sha256"]:
            wrong.append((name, px.shape))
    assert not wrong, wrong
    for base, s in D.base_streams(oracle).items():
        assert D.px_sha(oracle.decompress(s)) == fixture["clean"][base]["pixels_sha256"], base


def tail_cases(oracle, entries):
    """(entry index, first block, bit position, running DC) for every block that starts in the last 2,048 bits of the TAIL_ENTRIES, found
    by the walker: the strict walk of a damaged stream ends at the first thing an encoder does not write, and every block start up to
    there - the block it ends in included - is one any decoder arrives at."""
    tables = D.Tables(oracle.dump_tables())
    index = {e[0]: k for k, e in enumerate(entries)}
    out = []
    for name in TAIL_ENTRIES:
        s = entries[index[name]][4]
        blocks, _ = D.walk(tables, s, partial=True)
        mine = [(index[name], b, blk["start"], blk["dc_before"]) for b, blk in enumerate(blocks) if len(s) * 8 - D.TAIL_BITS <= blk["start"] < len(s) * 8]
        assert mine, name
        out += mine
    return out


def test_host_decoder_under_sanitizers(oracle, entries, tmp_path):
    """tests/native/damaged_selftest.cpp with AddressSanitizer + UBSan: tic::parse_header and tic::entropy_decode on every entry (an
    exact-size heap copy), pixels formed with the oracle's inverse stage, equal to tico_decompress's; tic::entropy_decode_tail from
    every block start in the last 2,048 bits of ten entries equal to the tail of the whole decode."""
    if shutil.which("g++") is None or shutil.which("gcc") is None:
        pytest.skip("no host compiler")
    tails = tail_cases(oracle, entries)
    assert len({t[0] for t in tails}) == 10
    path = tmp_path / "corpus.bin"
    with open(path, "wb") as f:
        f.write(b"TICD" + struct.pack("<I", len(entries)))
        for e in entries:
            f.write(struct.pack("<I", len(e[4])) + e[4])
        f.write(struct.pack("<I", len(tails)))
        for t in tails:
            f.write(struct.pack("<IIIi", *t))
    exe, obj = tmp_path / "damaged_selftest", tmp_path / "tic_oracle.o"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run(["gcc", "-c", *flags, "-o", str(obj), os.path.join(ROOT, "oracle", "tic_oracle.c")], check=True)
    subprocess.run(["g++", "-std=c++17", *flags, "-o", str(exe), os.path.join(ROOT, "tests", "native", "damaged_selftest.cpp"),
                    os.path.join(ROOT, "tinyimgcodec_amd", "csrc", "tic_entropy.cpp"), str(obj), "-lm", "-lpthread"], check=True)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("damaged_selftest ok %d " % (len(entries) + len(tails))) in r.stdout, r.stdout
    print(r.stdout.strip())
