"""The integer encoder's arithmetic at its edges - everything that needs no GPU.

Fixture: tests/golden/scaled_blocks.npz / .json, made by tests/golden/gen/make_goldens_scaled_blocks.py from the unmodified reference: built
8 x 8 blocks (tests/scaled_blocks.py: peak, line1023, word, dcswing) in frames 72 pixels wide, and per frame and setting the reference's
coefficients, stream and decoded pixels.  The one frame whose blocks leave the code table at `best` is pinned on the model there, and on the
reference at the other three settings.

What the tests establish, in this order: the corpus is what the search builds and every block has the property it is named for; the plain
model of tests/scaled_blocks.py equals the reference on every reference-pinned frame (this licenses the model); every mutant of the model
is told from the reference by some block; the ranges tic_scaled_math.h documents hold; the host build of tic_scaled_math.h, under
sanitizers, reproduces the fixture; the host entropy stage gives the reference's streams."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import tinyimgcodec_amd as T

import scaled_blocks as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = S.SETTINGS


@pytest.fixture(scope="module")
def fx():
    return S.Fixture()


@pytest.fixture(scope="module")
def pinned(fx):
    """Per setting (blocks uint8 [n, 64], d [n, u, v] of the model, the REFERENCE's coefficients in natural order [n, u, v]) over every
    reference-pinned frame, fillers included."""
    out = []
    for s in SETTINGS:
        names = [n for n in fx.frames if fx.entry(n, s)["pinned_by"] == "reference"]
        blocks = np.concatenate([S.frame_blocks(fx.pixels(n)) for n in names])
        zz = np.concatenate([fx.zz(n, s) for n in names]).astype(np.int64)
        nat = np.empty_like(zz)
        nat[:, S.ZIGZAG] = zz
        out.append((blocks, S.predct(blocks), nat.reshape(-1, 8, 8)))
    return out


def test_corpus_is_what_the_search_builds(fx):
    """The search has no random choice that is not seeded: built again, it gives the fixture's pixels, notes and tables.  The frames are
    72 pixels wide, the full ones 8 block rows high, and only the no-code frame is pinned on the model, at `best` only."""
    families, notes, info = S.build_corpus()
    frames = S.arrange(families, notes)
    assert sorted(f[0] for f in frames) == sorted(fx.frames)
    for name, family, img, frame_notes in frames:
        e = fx.frames[name]
        assert np.array_equal(fx.pixels(name), img), name
        assert (e["family"], e["h"], e["w"], e["blocks"], e["notes"]) == (family, img.shape[0], S.FRAME_W, len(frame_notes), frame_notes), name
        assert e["h"] <= 8 * S.FRAME_ROWS and e["h"] % 8 == 0
        assert (S.frame_blocks(img)[e["blocks"]:] == S.FILL).all()
        for s in SETTINGS:
            assert fx.entry(name, s)["pinned_by"] == ("model" if (family, s) == ("nocode", "best") else "reference"), (name, s)
    for k, v in info.items():
        assert fx.info[k] == v, k
    assert fx.info["blocks"] == {fam: len(b) for fam, b in families.items()}
    assert sum(1 for e in fx.frames.values() if e["h"] == 64) >= 4  # (the frames launch of the GPU tests takes these)


def test_every_block_has_the_property_it_is_named_for(fx):
    """By the model, on the fixture's pixels.  peak: d at its position is the recorded peak, no single flip of a pixel gains, and the
    tables hold (1, 1) +12,869 / -12,871, (1, 2) +12,371 and (2, 1) +12,369.  line1023: (1, 1) quantises to exactly
    +-1023 / +-1024 at best and the four other positions reach the largest coefficient the corpus knows for them.  word: d is the recorded
    value and every mutant the block claims quantises it differently; both signs occur about equally.  dcswing: flat 0 beside flat 255
    gives the largest DC difference 8-bit pixels can, 1020 at best (508 - -512), category 10."""
    pos, neg = np.array(fx.info["peak_pos"]), np.array(fx.info["peak_neg"])
    blocks, notes = fx.family_blocks("peak")
    assert len(blocks) == 128
    d = S.predct(blocks)
    for k, note in enumerate(notes):
        u, v, pol = k // 16, k // 2 % 8, 1 if k % 2 == 0 else -1
        assert (note["u"], note["v"]) == (u, v) and d[k, u, v] == note["d"] == (pos if pol > 0 else neg)[u, v]
        flips = np.repeat(blocks[k][None], 64, 0)
        flips[np.arange(64), np.arange(64)] ^= 255
        assert set(np.unique(blocks[k])) <= {0, 255} and (S.d_at(flips, u, v) * pol <= note["d"] * pol).all(), (u, v, pol)
    assert (pos[1, 1], pos[1, 2], pos[2, 1], neg[1, 1]) == (12869, 12371, 12369, -12871)
    assert fx.info["peak_max"] == max(pos.max(), -neg.min()) == 12871
    recip, half = S.table(0)
    qmax = np.abs(S.quantise(np.stack([pos, neg]), recip, half)).max(0)
    assert (qmax[0, 1], qmax[0, 2], qmax[1, 1]) == (932, 986, 1073)
    assert sorted(zip(*np.nonzero(qmax > 1023))) == [(1, 1)]  # the only position that leaves the code table
    blocks, notes = fx.family_blocks("line1023")
    q = S.quantise(S.predct(blocks), recip, half)
    assert [int(q[k, 1, 1]) for k in range(4)] == [1023, -1023, 1024, -1024] == [n["q_best"] for n in notes[:4]]
    assert [(n["u"], n["v"]) for n in notes[4:]] == [(0, 1)] * 2 + [(0, 2)] * 2 + [(1, 0)] * 2 + [(1, 2)] * 2
    for k, n in enumerate(notes[4:], 4):
        assert n["d"] == (pos if n["d"] > 0 else neg)[n["u"], n["v"]]  # the peak of its polarity, hence the largest coefficient of it
        assert int(q[k, n["u"], n["v"]]) == n["q_best"] == S.quantise(n["d"], recip[n["u"], n["v"]], half[n["u"], n["v"]])
    assert max(abs(n["q_best"]) for n in notes[4:] if (n["u"], n["v"]) == (0, 1)) == qmax[0, 1]
    assert np.abs(q[:2].reshape(2, 64)[:, 1:]).max() == 1023 and np.abs(q[4:].reshape(-1, 64)[:, 1:]).max() == 986
    blocks, notes = fx.family_blocks("word")
    assert len(blocks) == fx.info["blocks"]["word"]
    d = S.predct(blocks)
    claimed = set()
    for k, n in enumerate(notes):
        u, v = n["u"], n["v"]
        assert d[k, u, v] == n["d"] and n["kills"], (k, n)
        for kill in n["kills"]:
            setting, kind = kill.split(":")
            qf = SETTINGS.index(setting)
            r, h = S.table(qf)
            mr, mh = S.word_mutant(qf, u, v, kind)
            assert S.quantise(n["d"], r[u, v], h[u, v]) != S.quantise(n["d"], mr[u, v], mh[u, v]), (k, n, kill)
            claimed.add((qf, u, v, kind))
    assert len(claimed) == 4 * 256 - len(fx.info["unseparable_words"])
    signs = [np.sign(n["d"]) for n in notes]
    assert abs(signs.count(1) - signs.count(-1)) <= 1 + signs.count(0)
    frame = fx.frames["dcswing_0"]
    dc = {s: np.diff(fx.zz("dcswing_0", s)[:, 0].astype(np.int64), prepend=0) for s in SETTINGS}
    assert frame["blocks"] == 9 and [n["d"] for n in frame["notes"]] == [-8192, 8128] * 3 + [-8192, 8128, -8192]
    assert dc["best"].tolist() == [-512] + [1020, -1020] * 4 and 512 <= 1020 <= 1023  # category 10
    assert [int(np.abs(dc[s]).max()) for s in SETTINGS] == [1020, 510, 255, 127]
    assert S.quantise(pos[0, 0], recip[0, 0], half[0, 0]) - S.quantise(neg[0, 0], recip[0, 0], half[0, 0]) == 1020


def test_model_equals_the_reference_on_every_pinned_frame(fx):
    """model == fixture coefficients for every reference-pinned frame and setting - what licenses the model - and the model-pinned entry
    is the model's, has no stream, and holds exactly the built blocks with an |AC| above 1023."""
    n_ref = 0
    for name, s in fx.cases():
        e = fx.entry(name, s)
        want = S.model(S.frame_blocks(fx.pixels(name)), SETTINGS.index(s))
        assert np.array_equal(fx.zz(name, s), want) and fx.zz(name, s).dtype == np.int16 and S.sha(fx.zz(name, s)) == e["zz_sha256"], (name, s)
        assert e["max_abs_ac"] == np.abs(want[:, 1:]).max()
        if e["pinned_by"] == "reference":
            n_ref += 1
            assert e["max_abs_ac"] <= 1023 and e["bytes"] == 16 + e["payload_bits"] // 8 + 1 == len(fx.stream(name, s))
        else:
            assert (name, s) == ("nocode_0", "best") and fx.stream(name, s) is None
            big = np.abs(want[:, 1:]).max(1) > 1023
            assert big[: fx.frames[name]["blocks"]].all() and not big[fx.frames[name]["blocks"]:].any() and big.sum() == 4
    assert n_ref == 4 * len(fx.frames) - 1


def test_every_mutant_of_the_model_is_told_from_the_reference(fx, pinned):
    """Against the REFERENCE's coefficients of the reference-pinned frames, at the mutant's setting (every setting for a mutant of the
    transform): each multiplier (181 twice, 98, 139, 334) +-1 in the row pass only and in the column pass only; each of the four >> 8 as a
    division truncating toward zero, per pass; (Q + 1) >> 1 as half-divisor; rounded reciprocals; a quantiser that floors the signed sum;
    and the 4 x 256 single-word mutants (reciprocal +-1, half-divisor +-1).  A single-word mutant may survive only if no value in
    0..peak(u, v) - the peak taken from the fixture's own peak blocks - quantises differently under it; the survivors are printed and
    must be exactly the four words of (`low`, 7, 7), whose peak 510 quantises to 0 under the word and under its mutants.

    Not mutants: the int16 truncations behind either pass.  The ranges test below shows why no 8-bit block can tell them from no
    truncation at all: nothing in front of them leaves int16."""
    peaks, _ = fx.family_blocks("peak")
    top = np.abs(S.predct(peaks)).max(0)
    assert top.shape == (8, 8) and top[7, 7] == 510
    survivors, unseparable, counts = [], [], []
    for qf, (blocks, d, ref) in enumerate(pinned):
        recip, half = S.table(qf)
        assert np.array_equal(S.quantise(d, recip, half), ref)
        for name, row, col in S.transform_mutants():
            killed = int((S.quantise(S.predct(blocks, row, col), recip, half) != ref).any(axis=(1, 2)).sum())
            counts.append(killed)
            assert killed, (SETTINGS[qf], name)
        for name, mr, mh, floor in S.table_mutants(qf):
            killed = int((S.quantise(d, mr, mh, floor) != ref).any(axis=(1, 2)).sum())
            counts.append(killed)
            assert killed, (SETTINGS[qf], name)
        for u in range(8):
            for v in range(8):
                for kind in S.WORD_KINDS:
                    mr, mh = S.word_mutant(qf, u, v, kind)
                    tag = "%s:%d,%d:%s" % (SETTINGS[qf], u, v, kind)
                    if not (S.quantise(d[:, u, v], mr[u, v], mh[u, v]) != ref[:, u, v]).any():
                        survivors.append(tag)
                    if not S.separating_values(qf, u, v, kind, int(top[u, v])).any():
                        unseparable.append(tag)
    print("transform and whole-table mutants: %d, each told apart by at least %d blocks" % (len(counts), min(counts)))
    print("surviving single-word mutants (%d of 1024): %s" % (len(survivors), ", ".join(survivors)))
    assert survivors == unseparable == ["low:7,7:" + k for k in S.WORD_KINDS] == fx.info["unseparable_words"]
    assert len(S.transform_mutants()) == 2 * (5 * 2 + 4)


def test_documented_ranges_hold(fx):
    """The figures in tic_scaled_math.h's header - the row pass's maximum in output 0 and elsewhere, the column pass's maximum - are
    read from the header and bound what the search finds: the row maxima over all 256 rows of extreme pixels (exhaustive: 1024, 1282,
    1232, 1089, 1020, 728, 510, 255) and the peak tables.  All lie below 32,768, so neither int16 truncation ever changes a value on
    8-bit input: a kernel that truncated elsewhere, or not at all, cannot be told apart by pixels, and the truncations are not counted
    among the mutants.  The products the header names stay below 2^31."""
    text = open(os.path.join(ROOT, "tinyimgcodec_amd", "csrc", "tic_scaled_math.h")).read()
    m = re.search(r"= ([\d,]+) in output 0 and ([\d,]+) elsewhere [^,]*, a column pass ([\d,]+) at \(1, 1\)", " ".join(text.replace("//", " ").split()))
    assert m, "the header's range comment has changed its wording"
    row0, row_rest, col = (int(g.replace(",", "")) for g in m.groups())
    rows = S.row_maxima()
    assert rows == fx.info["row_maxima"] == [1024, 1282, 1232, 1089, 1020, 728, 510, 255]
    assert rows[0] <= row0 and max(rows[1:]) <= row_rest < 32768
    assert fx.info["peak_max"] <= col < 32768
    every = fx.all_blocks()
    r = S.row_pass(every)
    assert np.abs(r).max() <= row_rest and np.abs(S.predct(every)).max() <= col
    # the same without any truncation: nothing changes
    px = every.reshape(-1, 8, 8).astype(np.int64) - 128
    assert np.array_equal(S.fdct8(S.fdct8(px).transpose(0, 2, 1)).transpose(0, 2, 1), S.predct(every))
    assert col * 334 < 2 ** 31 and (60 + col) * 6553 < 2 ** 31 and int(S.table(0)[0].max()) == 6553 and int(S.table(0)[1].max()) == 60


def test_sanitized_host_build_reproduces_the_fixture(fx, tmp_path):
    """tic_scaled_math.h compiled for the host as a stand-alone program under ASan / UBSan (tests/native/scaled_selftest.cpp, as
    tests/test_scaled_encode_cpu.py runs it): the whole corpus at every setting, the model-pinned frame included - there the program has to
    agree with the model."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = tmp_path / "scaled_selftest"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "scaled_selftest.cpp")], check=True)
    blocks = fx.all_blocks()
    for qf, s in enumerate(SETTINGS):
        fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
        fin.write_bytes(struct.pack("<ii", len(blocks), qf) + np.ascontiguousarray(blocks).tobytes())
        r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "scaled_selftest ok" in r.stdout, r.stdout + r.stderr
        zz = np.fromfile(str(fout), np.int16).reshape(-1, 64)
        want = np.concatenate([fx.zz(n, s) for n in fx.frames])
        assert np.array_equal(zz, want), (s, int((zz != want).sum()))


def test_host_entropy_stage_gives_the_reference_streams(fx, oracle):
    """entropy_encode_scaled on the fixture's coefficients = the fixture's streams, byte for byte - |AC| = 1023 and a DC difference of
    1020 included; the frame with |AC| = 1024 and 1072 / 1073 is refused.  The oracle decodes every stream to the reference's pixels."""
    for name, s in fx.cases():
        e, fr = fx.entry(name, s), fx.frames[name]
        if e["pinned_by"] == "model":
            with pytest.raises(KeyError):
                T.entropy_encode_scaled(fx.zz(name, s), fr["h"], fr["w"], s)
            continue
        got = T.entropy_encode_scaled(fx.zz(name, s), fr["h"], fr["w"], s)
        assert got == fx.stream(name, s) and S.sha(np.frombuffer(got, np.uint8)) == e["sha256"], (name, s)
        dec = oracle.decompress(got)
        assert dec.shape == (fr["h"], fr["w"]) and S.sha(dec) == e["dec_sha256"], (name, s)
    assert fx.entry("line1023_0", "best")["max_abs_ac"] == 1023
