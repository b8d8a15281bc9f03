"""tests/golden/adaptive_tables.json on the CPU: the streams tests/adaptive_tables.py writes for its hand-built tables are the ones the
unmodified reference wrote (tests/golden/gen/make_goldens_adaptive_tables.py), its bit-serial model reads them back, the cases reach the
decoder states they were built for (the census, from the tables and coefficients alone), a wrong coefficient would change a pixel
(visibility, with the oracle's inverse stage), the model of the device decoder's look-up tables agrees with the dict look-up on every code
and on the windows no code starts, and the model of the stitch gives the recorded exits moved per round.
tests/test_adaptive_tables_gpu.py runs the same streams through the device decoder and compares its trace with those lists."""
import json
import os

import numpy as np
import pytest

import adaptive_tables as AT
import inverse_edges as IE

FX = AT.load_fixture()
CASES = list(FX["cases"])
ROUNDS = [n for n in CASES if n.startswith("rounds_")]


@pytest.fixture(scope="module")
def cases():
    return AT.build_cases(AT.fixture_tables(FX))


@pytest.fixture(scope="module")
def streams(cases):
    return {name: AT.stream_of(name, c) for name, c in cases.items()}


def test_the_builder_makes_the_cases_of_the_fixture(cases):
    assert sorted(cases) == sorted(CASES) and FX["generator"] == "tests/golden/gen/make_goldens_adaptive_tables.py"
    assert set(ROUNDS) == set(AT.ROUNDS) == set(AT.SETTLES) and set(AT.VALUE_CASES) <= set(CASES)
    assert {"max_table", "max_distinct_table", "too_wide", "damaged_chain"} <= set(CASES)
    for name, c in cases.items():
        e = FX["cases"][name]
        assert (c["h"], c["w"], len(c["zz"]), c["qualities"], c["well_formed"]) == (e["height"], e["width"], e["blocks"], e["qualities"], e["well_formed"]), name
        assert AT.blocks_of(c["h"], c["w"]) == len(c["zz"]) and c["zz"].dtype == np.int16, name
        assert AT.sha(np.ascontiguousarray(c["zz"], dtype="<i2").tobytes()) == e["coeffs_sha256"], name
        assert c["qualities"] == (list(AT.QUALITIES) if name in AT.VALUE_CASES else [50]), name


def test_the_long_code_coefficients_are_the_fixtures():
    """longcode_coeffs(33) is the array of adaptive_streams.json: the rounds_* cases are that recipe with fewer symbol kinds."""
    with open(os.path.join(AT.GOLDEN, "adaptive_streams.json")) as f:
        e = json.load(f)["longcode"]
    zz = AT.longcode_coeffs()
    assert zz.shape[0] == e["blocks"] and AT.sha(np.ascontiguousarray(zz.astype("<i2")).tobytes()) == e["coeffs_sha256"]
    m = FX["longcode_model"]
    assert (m["bytes"], m["sha256"]) == (e["bytes"], e["sha256"])
    # profiles/adaptive_decode.txt section 4, recorded on an MI355X: 7,891, 7,169, 6,913 ... 512, 409, 153, 0, settled in launch 280
    assert m["changed"][:4] == [1, 7891, 7169, 6913] and m["changed"][-4:] == [512, 409, 153, 0] and m["changed"].index(0) == 280 == len(m["changed"]) - 1
    assert m["range_bits"] == 675


@pytest.mark.parametrize("name", CASES)
def test_write_stream_reproduces_the_references_stream(cases, streams, name):
    e, c = FX["cases"][name], cases[name]
    assert len(streams[name]) < (1 << 20), name  # (a GPU test of it takes seconds)
    for q in c["qualities"]:
        s = AT.with_quality(streams[name], q)
        if q == c["qualities"][-1]:
            assert s == AT.stream_of(name, c, q)  # (the header's quality field is all that differs)
        assert (len(s), AT.sha(s)) == (e["streams"]["q%d" % q]["bytes"], e["streams"]["q%d" % q]["sha256"]), (name, q)
    if "stream" in e:
        assert bytes.fromhex(e["stream"]) == streams[name]
    assert ("stream" in e) == (len(streams[name]) <= 4096), name
    if name == "too_wide":
        assert e["reference_wrote_it"] is True and len(streams[name]) == e["streams"]["q50"]["bytes"]
    # max_table repeats symbols, which the reference's table (a bidict) cannot hold: write_stream alone wrote it, the reference its payload
    assert e.get("reference_wrote_it", True) == (name != "max_table") and e.get("reference_wrote_the_payload", False) == (name == "max_table")
    if name == "damaged_chain":
        clean = AT.write_stream(c["table"], c["zz"], c["h"], c["w"], 50)
        diff = [i for i in range(len(clean)) if clean[i] != streams[name][i]]
        assert diff == [e["flipped_bit"] >> 3] and clean[diff[0]] ^ streams[name][diff[0]] == 0x80 >> (e["flipped_bit"] & 7)
        assert e["flipped_bit"] >= e["census"]["payload_bit"]


@pytest.mark.parametrize("name", CASES)
def test_decode_model_reads_the_coefficients_back(cases, streams, name):
    """The plain reference of the operation.  (The fixture says where the reference's own reader - codes up to 16 bits - read the same.)"""
    c = cases[name]
    if name == "damaged_chain":
        with pytest.raises(AT.NoCode):
            AT.decode_model(streams[name])
        return
    h, w, q, table, payload_bit = AT.parse(streams[name])
    assert (h, w, q, table) == (c["h"], c["w"], c["qualities"][0], c["table"]) and payload_bit == FX["cases"][name]["census"]["payload_bit"]
    assert np.array_equal(AT.decode_model(streams[name]), c["zz"]), name
    short = max(len(code) for _, code in table["DC"] + table["AC"]) <= 16
    assert FX["cases"][name].get("reference_reads_back", False) == short, name


@pytest.mark.parametrize("name", CASES)
def test_census(cases, streams, name):
    """What each family promises (asserted inside census()): the residues, nlong == 256, symbols of exactly 64 bits, a table of
    kAdaptMaxTableBytes, windows without a code in round 0 - and the figures are the fixture's."""
    c = AT.census(name, cases[name], None if name == "too_wide" or name in ROUNDS else streams[name])
    print(name, c)
    want = FX["cases"][name]["census"]
    if name in ROUNDS:  # (the stitch of these cases: test_stitch_model_gives_the_recorded_rounds)
        want = {k: v for k, v in want.items() if k in c}
    assert json.loads(json.dumps(c)) == want, name


def test_max_table_is_exactly_max_table_bytes(cases):
    """kAdaptMaxTableBytes, the length the library sizes its head buffers on, is reached by a prefix code whose size-0 symbols repeat
    (max_table: 20,874 bits end in byte 2,610, the payload starts inside it); no table with distinct symbols is longer than 2,370 bytes
    (max_distinct_table: the longest such less one bit)."""
    c = AT.census("max_table", cases["max_table"])
    assert AT.MAX_TABLE_BYTES == 2610 and AT.MAX_DISTINCT_TABLE_BITS == 18960
    assert c["table_bits"] == 20874 and c["table_bytes"] == 2610 and c["payload_bit"] % 8 == 2 and c["max_symbol_bits"] == 64
    assert (c["ac_entries"], c["distinct_ac_symbols"]) == (256, 20)
    c = AT.census("max_distinct_table", cases["max_distinct_table"])
    assert c["table_bits"] == 18959 and c["table_bytes"] == 2370 and c["payload_bit"] % 8 == 7 and c["max_symbol_bits"] == 64


@pytest.mark.parametrize("name", AT.VALUE_CASES)
def test_visibility(cases, oracle, name):
    """A wrong sign, halved magnitude, dropped top bit, position moved on by one or magnitude less one (sizes 1 .. 4) of any AC coefficient
    changes a pixel of the oracle's under at least one header quality.  The symbols of sizes 11 .. 15 (widest_*: one to a block, the
    least magnitudes of their size) are held to sign and top bit; the blocks of the maximal length saturate and are left out."""
    ie = IE.Fixture()
    for part in AT.parts_of(name):
        v = AT.visibility(ie, oracle, cases[name], part)
        print(name, part, {k: "%d / %d" % tuple(x) for k, x in v.items()})
        assert v == FX["cases"][name]["visibility"][part], (name, part)
        AT.check_bars(name, v, part)


def tails(rng):
    return [0, (1 << 64) - 1] + [int(rng.integers(0, 1 << 62)) << 2 | int(rng.integers(0, 4)) for _ in range(6)]


@pytest.mark.parametrize("name", CASES)
def test_lookup_model_agrees_with_the_dict_lookup(cases, name):
    """Every code of every table followed by all-zero, all-one and seeded tails is found with its length and symbol; seeded windows, and
    every window that starts like a code cut short by a bit or with its last bit flipped, give what the growing-prefix look-up gives -
    "none" exactly where no code is a prefix."""
    if name == "too_wide":
        return  # (65 bits: no window holds it; the parser refuses the table)
    table = cases[name]["table"]
    lut = AT.lut_model(table)
    rng = np.random.default_rng(77)
    nones = 0
    for key in ("DC", "AC"):
        inverse = {code: (sym if key == "DC" else (sym[0] << 4) | sym[1]) for sym, code in table[key]}

        def by_dict(win):
            bits = format(win, "064b")
            for n in range(1, 65):
                if bits[:n] in inverse:
                    return n, inverse[bits[:n]]
            return None

        for code, sym in inverse.items():
            n, c = len(code), int(code, 2)
            for t in tails(rng):
                win = (c << (64 - n)) | (t >> n if n < 64 else 0)
                assert AT.lookup_model(lut[key], win) == (n, sym) == by_dict(win), (name, key, code)
                for other in (((c ^ 1) << (64 - n)) | (t >> n if n < 64 else 0), ((c >> 1) << (65 - n)) | (t >> (n - 1)) if n > 1 else t):
                    got = AT.lookup_model(lut[key], other)
                    assert got == by_dict(other), (name, key, code)
                    nones += got is None
        for t in tails(rng) * 8:
            assert AT.lookup_model(lut[key], t) == by_dict(t), (name, key, t)
    c = AT.census(name, cases[name])
    assert (nones > 0) == (min(c["kraft"]) < 1.0), (name, nones, c["kraft"])


@pytest.mark.parametrize("name", ROUNDS)
def test_stitch_model_gives_the_recorded_rounds(streams, name):
    """The exits moved per round of the shortened long-code arrays, and that each settles in the stretch of rounds it was chosen for."""
    want = FX["cases"][name]["census"]
    rb, nr, changed = AT.stitch_model(streams[name])
    print(name, rb, nr, changed)
    assert (rb, nr, changed) == (want["range_bits"], want["nranges"], want["changed"]), name
    AT.check_settles(name, changed)


def test_the_rounds_cases_have_the_figures_of_k_25_26_and_29():
    """Blocks, bytes, ranges and changed[] of the long-code recipe cut to its last 25, 26 and 29 symbol kinds, and the stretch of rounds
    the fourth case (27 kinds, 7,160 blocks) settles in."""
    figs = {n: (e["blocks"], e["streams"]["q50"]["bytes"], e["census"]["nranges"], e["census"]["changed"]) for n, e in FX["cases"].items() if n in ROUNDS}
    assert figs["rounds_few"] == (3121, 131880, 1562, [1, 675, 281, 25, 0])
    assert figs["rounds_early"] == (5049, 213325, 2527, [1, 30, 0])
    assert figs["rounds_late"][:3] == (21386, 903317, 10705) and figs["rounds_late"][3].index(0) == 42
    assert 10 <= figs["rounds_mid"][3].index(0) <= 18


def test_host_half_of_the_decoder_under_sanitizers(cases, streams, tmp_path):
    """tests/native/adaptive_host_selftest.cpp: tic_adaptive.cpp (adaptive_parse_table, adaptive_decode, adaptive_dec_tab_build) and
    tic_entropy.cpp compiled as HOST code with AddressSanitizer + UBSan - the parser of an embedded table from untrusted bytes and the
    builder of the look-up table device lanes index, which only tests marked gpu reached.  Per case the program gets the stream,
    decode_model's coefficients (or that it raises) and lut_model's tables, works on exact-size heap copies and checks (a) adaptive_decode
    against the model, (b) the parsed and built tables against lut_model, and adaptive_dec_tab_buildable against the build, (c) on boundary
    and max_table every single-bit flip of the table region and every cut from 16 bytes to the payload's first byte: parser and decoder
    agree about the table, a table that parses is a prefix code (brute force), a built look-up table names only its entries.
    too_wide is the one case where the product refuses what the model reads: a symbol of 65 bits with its value, beyond the 64 the
    header documents - written as an error, with no tables."""
    import shutil
    import struct
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    if not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        pytest.skip("hip/hip_runtime.h is absent: tic_adaptive.h includes it")
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(b"TICA" + struct.pack("<I", len(cases)))
        for name, c in cases.items():
            s = streams[name]
            f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<I", len(s)) + s)
            refused = name == "too_wide"
            try:
                zz = AT.decode_model(s)
            except ValueError:  # (NoCode is one)
                zz = None
            assert (zz is None) == (name == "damaged_chain"), name
            if zz is None or refused:
                f.write(b"\0")
            else:
                f.write(b"\1" + struct.pack("<I", len(zz)) + np.ascontiguousarray(zz, dtype="<i2").tobytes())
            if refused:
                f.write(b"\0")
            else:
                lut = AT.lut_model(AT.parse(s)[3])
                f.write(b"\1")
                for key in ("DC", "AC"):
                    t = lut[key]
                    f.write(np.array([0 if e is None else (e[0] << 8) | e[1] for e in t["prim"]], "<u2").tobytes())
                    f.write(struct.pack("<I", len(t["codes"])) + np.array(t["codes"], "<u8").tobytes() + np.array([(n << 8) | y for n, y in t["ls"]], "<u2").tobytes())
            f.write(b"\1" if name in ("boundary", "max_table") else b"\0")
    exe = tmp_path / "adaptive_host_selftest"
    csrc = os.path.join(root, "tinyimgcodec_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(rocm, "include"), "-o", str(exe), os.path.join(root, "tests", "native", "adaptive_host_selftest.cpp"),
                    os.path.join(csrc, "tic_adaptive.cpp"), os.path.join(csrc, "tic_entropy.cpp"), "-lpthread"], check=True)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("adaptive_host_selftest ok %d cases" % len(cases)) in r.stdout and not r.stderr, r.stdout + r.stderr
    print(r.stdout.strip())
