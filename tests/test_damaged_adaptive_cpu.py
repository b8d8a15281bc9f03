"""tests/golden/damaged_adaptive.json on the CPU: the seeded corpus of damaged per-image-table streams (tests/damaged_adaptive.py) is the
one the fixture was made from; decode_strict - the documented contract of tic_decompress_adaptive in plain Python - and the oracle's
inverse stage reproduce EVERY stored outcome (all 1,100 entries, not a sample: some 20 s); the fixture is consistent with what the
unmodified reference's reader did (tests/golden/gen/make_goldens_damaged_adaptive.py asserts the same while it writes it); and the host
half of the decoder, compiled stand-alone with AddressSanitizer + UBSan, gives the fixture's outcome for every entry and builds only
look-up tables that name entries of their table.  tests/test_damaged_adaptive_gpu.py runs the same entries through every device route."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import adaptive_tables as AT
import damaged_adaptive as DA
import inverse_edges as IE

FX = DA.load_fixture()
REC = DA.records(FX)


@pytest.fixture(scope="module")
def bases(oracle):
    return DA.base_streams(oracle, FX)


@pytest.fixture(scope="module")
def corpus(oracle, bases):
    return DA.corpus(oracle, FX, bases)


@pytest.fixture(scope="module")
def decoded(corpus):
    """name -> (class, None) or (None, coefficients): decode_strict of every entry, once."""
    return {name: DA.outcome_class(s) for name, base, kind, params, s in corpus}


def test_the_bases_are_the_references_streams(bases):
    """write_stream with the stored table and the oracle's coefficients gives the stream the reference's compress(...,
    auto_generate_huffman_table=True) wrote (the hand-built bases: the stream of tests/golden/adaptive_tables.json), with the figures
    the corpus was specified on."""
    assert list(bases) == list(DA.BASES) and set(bases) == set(FX["bases"])
    for base, s in bases.items():
        e = FX["bases"][base]
        h, w, q, table, first = AT.parse(s)
        assert (len(s), DA.sha(s)) == (e["bytes"], e["sha256"]) and (h, w, q) == (e["h"], e["w"], e["q"]) == DA.BASES[base][:3], base
        assert len(s) <= DA.MAX_BASE_BYTES and first - 128 == e["table_bits"] and len(s) * 8 - first == e["payload_bits"], base
        assert max(len(code) for _, code in table["DC"] + table["AC"]) == e["longest_code"], base
        assert AT.range_rule(len(s), first, AT.blocks_of(h, w)) == e["range_bits"], base
    f = {b: (e["bytes"], e["table_bits"], e["longest_code"], e["ranges"]) for b, e in FX["bases"].items()}
    assert f["lenna64"] == (472, 590, 9, 12) and f["noise64"] == (1814, 703, 12, 33) and f["ragged17x33"][:2] == (313, 518) and FX["bases"]["ragged17x33"]["range_bits"] == 256
    assert f["noise256"] == (35896, 832, 15, 512) and f["twolevel256"] == (36947, 790, 15, 513) and f["twolevel256q90"][::2] == (47940, 17)
    assert FX["bases"]["noise256"]["payload_bits"] == 286208 and FX["bases"]["twolevel256"]["payload_bits"] == 294658
    # the flag-swapped twin of a base is decode(encode()) for the unmodified decompress() wherever no code is longer than 16 bits
    assert {b: e.get("twin_equals_decode") for b, e in FX["bases"].items() if "table" in e} == {
        "lenna64": True, "noise64": True, "ragged17x33": True, "noise256": True, "twolevel256": True, "twolevel256q90": False}


def test_the_corpus_is_the_fixtures(corpus):
    """Names, lengths and digests; the conditions on its size; every kind on every base and every variant somewhere."""
    assert [e[0] for e in corpus] == list(REC) and len(corpus) <= DA.MAX_ENTRIES
    assert os.path.getsize(DA.FIXTURE) < DA.MAX_FIXTURE_BYTES
    flips = []
    for name, base, kind, params, s in corpus:
        r = REC[name]
        assert len(s) == r["bytes"], name
        if r["sha256"] is None:
            assert base == "lenna64" and kind == "table_flip"
            flips.append(DA.sha(s))
        else:
            assert DA.sha(s) == r["sha256"], name
    assert len(flips) == FX["bases"]["lenna64"]["table_bits"] == 590 and DA.family_sha(flips) == FX["lenna64_table_flips_sha256"]
    DA.check_population(corpus)
    for base in DA.BASES:  # the samples are stratified: every field of the table on every base
        assert {p["field"] for n, b, k, p, s in corpus if b == base and k == "table_flip"} == set(DA.FIELDS), base
    assert sum(k == "table_flip" for n, b, k, p, s in corpus) == 590 + 7 * DA.SAMPLE


def test_decode_strict_reproduces_every_outcome(corpus, decoded, oracle):
    """Every entry, not a sample: the class of the refusal, or the geometry and the pixels - decode_strict's coefficients through the
    oracle's divisors and inverse transform (inverse_edges.pixels_block_idct) - that the fixture holds from the reference."""
    ie = IE.Fixture()
    wrong = []
    for name, base, kind, params, s in corpus:
        cls, zz = decoded[name]
        if cls is None:
            h, w, q = DA.header(s)[:3]
            px = IE.pixels_block_idct(ie, oracle, zz.astype(np.int64), h, w, q, 0)
            got = (h, w, DA.px_sha(px))
        else:
            got = cls
        if got != REC[name]["outcome"]:
            wrong.append((name, got if cls else got[:2], REC[name]["outcome"]))
    assert not wrong, (wrong[:10], len(wrong))


def test_the_fixture_is_consistent_with_the_references_reader(corpus):
    """damaged_adaptive.consistency, from the stored fields alone: in reach of the reference's reader decode_strict decodes exactly
    where the reader was clean (the generator compared the coefficients), but for the classes where the product is stricter by design -
    named, counted, at most 3 % -; nothing out of reach was handed to the reader; the out-of-reach share of the decoded entries is the
    measured one and under its bound; every class has three entries, 150 entries decode to other pixels than their base's."""
    figs = DA.consistency([e[:3] for e in corpus], REC, {b: e["pixels_sha256"] for b, e in FX["bases"].items()})
    print({k: v for k, v in figs.items() if k != "census"})
    for kind in DA.KINDS:
        print("%-11s %s" % (kind, figs["census"][kind]))
    assert figs == FX["figures"]
    assert set(figs["stricter_in_reach"]) <= set(DA.STRICTER)
    assert (figs["decoded_counted_out_of_reach"], figs["decoded_counted"]) == (83, 204)  # 40.7 %: the 25 % first asked for do not hold (71 of the 83 are flips of lenna64 that repeat a symbol)
    assert all(r["reach"] == "in" or r["reach"].split(":")[1] in ("header", "table_truncated", "zero_length", "long_code", "repeated_symbol", "repeated_code") for r in REC.values())
    assert all(r["reach"] != "in" for n, r in REC.items() if n.startswith("twolevel256q90/") and r["reach"] != "out:header")


def test_the_lengths_kept_and_the_give_up_classes(corpus, decoded, bases):
    """What the GPU test relies on: a value flip and a table swap that keeps every length leave the chain of block starts the clean
    stream's (walked here with the entry's own table); entries of the classes the device decoder's give-up bits stand for exist on
    bases the device routes take."""
    for name, base, kind, params, s in corpus:
        if kind == "value_flip" or (kind == "table_swap" and params["keeps_lengths"]):
            clean = bases[base]
            n = AT.blocks_of(*DA.header(clean)[:2])
            a = DA.walk(clean, *AT.parse(clean)[3:5], n)
            b = DA.walk(s, *AT.parse(s)[3:5], n, partial=True)
            shift = AT.parse(s)[4] - AT.parse(clean)[4]
            assert [x["start"] + shift for x in a[0][: len(b[0])]] == [x["start"] for x in b[0]], name
            if kind == "value_flip":
                assert decoded[name][0] is None and REC[name]["outcome"][2] != FX["bases"][base]["pixels_sha256"], name
    for cls in ("no_code", "over_63", "truncated", "dc_range"):
        assert any(decoded[n][0] == cls for n, b, k, p, s in corpus if b in ("noise256", "twolevel256")), cls


def test_host_half_of_the_decoder_under_sanitizers(corpus, decoded, tmp_path):
    """tests/native/damaged_adaptive_selftest.cpp: tic_adaptive.cpp and tic_entropy.cpp compiled as HOST code with AddressSanitizer +
    UBSan, a stand-alone program (nothing is loaded into Python under a sanitizer).  It runs adaptive_parse_table, adaptive_decode,
    adaptive_dec_tab_buildable and adaptive_dec_tab_build on exact-size heap copies of every entry: the parser refuses exactly the
    entries of the table classes, the decoder those and the payload classes, and gives decode_strict's coefficients (which
    test_decode_strict_reproduces_every_outcome ties to the fixture's pixels) for every other one; every look-up table built names only
    entries of its table and has nlong within the arrays."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    if not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        pytest.skip("hip/hip_runtime.h is absent: tic_adaptive.h includes it")
    path = tmp_path / "entries.bin"
    counts = [0, 0, 0]
    with open(path, "wb") as f:
        f.write(b"TICD" + struct.pack("<I", len(corpus)))
        for name, base, kind, params, s in corpus:
            cls, zz = decoded[name]
            assert cls == (REC[name]["outcome"] if isinstance(REC[name]["outcome"], str) else None), name
            f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<I", len(s)) + s)
            outcome = 2 if cls is None else 0 if cls in DA.TABLE_CLASSES else 1
            counts[outcome] += 1
            f.write(bytes([outcome]))
            if cls is None:
                f.write(struct.pack("<I", len(zz)) + np.ascontiguousarray(zz, dtype="<i2").tobytes())
    exe = tmp_path / "damaged_adaptive_selftest"
    csrc = os.path.join(root, "tinyimgcodec_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(rocm, "include"), "-o", str(exe), os.path.join(root, "tests", "native", "damaged_adaptive_selftest.cpp"),
                    os.path.join(csrc, "tic_adaptive.cpp"), os.path.join(csrc, "tic_entropy.cpp")], check=True)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = "damaged_adaptive_selftest ok %d entries: %d table refusals, %d payload refusals, %d decoded;" % ((len(corpus),) + tuple(counts))
    assert want in r.stdout and not r.stderr, r.stdout + r.stderr
    print(r.stdout.strip())
