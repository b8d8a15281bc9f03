"""encode() / compress() of integer images outside 0..255 without a GPU: the corpus of tests/wide_blocks.py against its fixture
(tests/golden/wide_blocks.npz / .json, written by the unmodified reference), the oracle and the host entropy coders against the fixture,
and the proof that the corpus can tell a wrong kernel: plain numpy mutants of the transform, each of which has to differ from the
fixture on every frame of the family built for it.  The census lines are printed (pytest -s shows them)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N
from tinyimgcodec_amd import codec as TC

import wide_blocks as WB
from conftest import ROOT


@pytest.fixture(scope="module")
def fx():
    return WB.Fixture()


def test_the_builder_reproduces_every_input(fx):
    frames = WB.frames()
    assert list(frames) == list(fx.entries)
    for name, f in frames.items():
        e = fx.entries[name]
        assert f.img.dtype == np.int32 and f.img.shape == (e["h"], e["w"]) and f.quality == e["quality"] and f.family == e["family"], name
        assert WB.sha(f.img) == e["sha256"], name
        n = -(-e["h"] // 8) * -(-e["w"] // 8)
        assert fx.dc(name).shape == (n,) and fx.ac(name).shape == (n, 63) and fx.dc(name).dtype == fx.ac(name).dtype == np.int32, name
    assert max(e["h"] * e["w"] for e in fx.entries.values()) == 64 * 512


def test_every_family_reaches_its_edge(fx):
    """What the families are for, read off the frames and the fixture."""
    frames = WB.frames()
    fam = {k: [frames[n] for n in fx.names(k)] for k in WB.FAMILIES}
    for k, v in fam.items():
        print("census %-9s %s" % (k, {a: b for a, b in fx.census[k].items() if not isinstance(b, dict)}))
        assert len(v) == fx.census[k]["frames"] > 0
    # geometry: the shapes of the table, three qualities each; tiles_x up to 4, more than one workgroup, a last tile of one block
    shapes = {f.img.shape for f in fam["geometry"]}
    assert shapes == set(WB.GEOMETRY_SHAPES) and len(fam["geometry"]) == 3 * len(shapes)
    tiles = {(h, w): (-(-(-(-w // 8)) // 8), -(-h // 8)) for (h, w) in shapes}  # (tiles_x, block rows)
    assert tiles[(72, 136)] == (3, 9) and tiles[(40, 200)] == (4, 5) and tiles[(264, 8)] == (1, 33) and tiles[(8, 264)] == (5, 1)
    assert all(np.abs(f.img).max() > 30000 for f in fam["geometry"] if f.img.size >= 64)
    # reflect: every pair of short axes, distinct magnitudes above 1,000
    assert {f.img.shape for f in fam["reflect"]} == set(WB.REFLECT_SHAPES)
    for f in fam["reflect"]:
        assert np.abs(f.img).min() > 1000 and len(np.unique(np.abs(f.img))) == f.img.size, f.name
    # magnitude: the amplitudes are reached, and beyond int16 the coefficients leave it too
    for f in fam["magnitude"]:
        k = int(re.match(r"mag_k(\d+)_", f.name).group(1))
        assert 2 ** (k - 1) <= np.abs(f.img.astype(np.int64)).max() <= 2 ** k, f.name
    assert fx.census["magnitude"]["max_abs_ac"] > 2 ** 24 and np.abs(fx.ac("mag_k31_sym_q10").astype(np.int64)).max() > 2 ** 24
    # extremes: pixels whose `- 128` wraps, the flat frame and the pair of the issue
    assert fx.census["extremes"]["pixels_that_wrap"] > 0
    assert int(fx.dc("ext_flat_min_q10")[0]) == 214748352
    assert fx.dc(WB.PAIR_FRAME).tolist() == [2147483519, 129]
    # ties: every block of every frame is a tie, and the reference rounds both ways, unlike half-even
    for (u, v) in WB.TIE_POSITIONS:
        c = fx.census["ties"]["%d%d" % (u, v)]
        print("census ties (%d, %d): %s" % (u, v, c))
        assert c["up"] + c["down"] == 512 and c["up"] >= 100 and c["down"] >= 100 and c["unlike_half_even"] > 0
        assert (WB.tie_exact_twice(u, v, frames["tie_%d%d_q50" % (u, v)].img) % 2 != 0).all()
    # float qualities, and the streams on both sides of the code tables' ends
    assert sorted({f.quality for f in fam["floatq"]}) == list(WB.FLOAT_QUALITIES) and len(fam["floatq"]) == 8
    s = fx.census["streams"]["streams"]
    for name, c in s.items():
        print("census streams %-20s %s" % (name, c))
    assert s["str_ramp_q50"]["max_abs_running_dc"] == 46000 and s["str_ramp_q50"]["max_abs_dc_diff"] == 2000 and s["str_ramp_q50"]["result"] == "86 bytes"
    assert s["str_dc2047_q50"]["max_abs_dc_diff"] == 2047 and s["str_dc2048_q50"]["max_abs_dc_diff"] == 2048
    assert s["str_ac1023_q50"]["max_abs_ac"] == 1023 and s["str_ac1024_q50"]["max_abs_ac"] == 1024
    assert sorted(fx.dc("str_dc2047_q50").tolist()) == [-2047, 0, 2047] and sorted(fx.dc("str_dc2048_q50").tolist()) == [-2048, 0, 2048]
    assert {int(fx.ac(n).min()) for n in ("str_ac1023_q50",)} == {-1023} and int(fx.ac("str_ac1024_q50").max()) == 1024
    assert [fx.stream(n) for n in ("str_dc2048_q50", "str_ac1024_q50")] == ["KeyError", "KeyError"]
    assert all(isinstance(fx.stream(n), bytes) for n in fx.names("streams") if n not in ("str_dc2048_q50", "str_ac1024_q50"))
    assert s["str_12bit_q50"]["max_abs_ac"] < 1024 and frames["str_12bit_q50"].img.max() > 255


def test_the_oracle_equals_the_fixture_on_every_frame(fx, oracle):
    bad = []
    for name, f in WB.frames().items():
        dc, ac = oracle.encode_wide(f.img, f.quality)
        diff = WB.first_difference(dc, ac, fx.dc(name), fx.ac(name))
        if diff:
            bad.append("%s: %s" % (name, diff))
    assert not bad, "\n".join(bad)


def test_the_oracle_takes_strided_int32_rows(fx, oracle):
    """tico_encode_i32's stride, and its float-quality twin, behind pyoracle.encode_wide: a view with padded rows."""
    for name in ("geo_9x65_q50", "fq_geo_9x65_q33p3"):
        f = WB.frames()[name]
        buf = np.full((f.img.shape[0], f.img.shape[1] + 5), WB.I32_MAX, np.int32)
        buf[:, : f.img.shape[1]] = f.img
        L = oracle.lib()
        dc, ac = np.zeros(fx.dc(name).shape, np.int32), np.zeros(fx.ac(name).shape, np.int32)
        if isinstance(f.quality, float):
            L.tico_encode_i32_f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_ssize_t, C.c_double, C.c_void_p, C.c_void_p]
            rc = L.tico_encode_i32_f(buf.ctypes.data, f.img.shape[0], f.img.shape[1], buf.shape[1], f.quality, dc.ctypes.data, ac.ctypes.data)
        else:
            rc = L.tico_encode_i32(buf.ctypes.data_as(C.POINTER(C.c_int32)), f.img.shape[0], f.img.shape[1], buf.shape[1], f.quality,
                                   dc.ctypes.data_as(C.POINTER(C.c_int32)), ac.ctypes.data_as(C.POINTER(C.c_int32)))
        assert rc == 0 and WB.first_difference(dc, ac, fx.dc(name), fx.ac(name)) is None, name


def test_the_entropy_coders_write_the_reference_streams(fx, oracle):
    """The oracle's coder and the library's coder of int32 differences (tic_entropy_encode_dpcm, behind compress() of a wide image), fed the
    fixture's dc / ac: the reference's bytes, and an error exactly where the reference raised KeyError."""
    for name in fx.names("streams"):
        e, want = fx.entries[name], fx.stream(name)
        if isinstance(want, bytes):
            assert oracle.entropy_encode(fx.dc(name), fx.ac(name), e["h"], e["w"], e["quality"]) == want, name
            assert TC._entropy_encode_dpcm(fx.dc(name), fx.ac(name), e["h"], e["w"], e["quality"]) == want, name
        else:
            assert want == "KeyError"
            with pytest.raises(oracle.OracleError):
                oracle.entropy_encode(fx.dc(name), fx.ac(name), e["h"], e["w"], e["quality"])
            with pytest.raises(KeyError):
                TC._entropy_encode_dpcm(fx.dc(name), fx.ac(name), e["h"], e["w"], e["quality"])


def test_the_dpcm_coder_agrees_with_the_zz16_coder_where_both_apply(fx):
    """Where the running DC fits int16 and everything has a code, entropy_encode of the zz16 layout and the coder of the differences write
    the same stream; where it does not fit, only the latter writes one."""
    for name in fx.names("streams"):
        e, want = fx.entries[name], fx.stream(name)
        run = np.cumsum(fx.dc(name).astype(np.int64))
        if not isinstance(want, bytes) or np.abs(run).max() > 32767:
            continue
        zz = np.concatenate([run[:, None], fx.ac(name)], axis=1).astype(np.int16)
        assert T.entropy_encode(zz, e["h"], e["w"], e["quality"]) == want, name
    assert np.abs(np.cumsum(fx.dc("str_ramp_q50").astype(np.int64))).max() > 32767 and isinstance(fx.stream("str_ramp_q50"), bytes)


def test_the_wide_header_is_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "tinyimgcodec_hip_wide.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(tic_\w+)\s*\(", text))
    assert declared == set(N.WIDE_SIGNATURES) == {"tic_entropy_encode_dpcm"}
    for other in (N.SIGNATURES, N.RATE_ADAPTIVE_SIGNATURES, N.TRANSCODE_SIGNATURES, N.TRANSCODE_BATCH_SIGNATURES):
        assert not declared & set(other)
    for path in (N.LIB_PATH, N.HOOKS_LIB_PATH):
        assert hasattr(C.CDLL(path), "tic_entropy_encode_dpcm"), path
    L = N.load()
    assert L.tic_entropy_encode_dpcm.argtypes == N.WIDE_SIGNATURES["tic_entropy_encode_dpcm"][1]
    out, n, z = np.zeros(64, np.uint8), C.c_size_t(7), np.zeros(64, np.int32)
    assert L.tic_entropy_encode_dpcm(None, None, 8, 8, 50, out.ctypes.data, out.size, C.byref(n)) == N.TIC_E_ARG
    assert L.tic_entropy_encode_dpcm(z.ctypes.data, z.ctypes.data, 8, 8, 50, None, 64, C.byref(n)) == N.TIC_E_ARG
    assert L.tic_entropy_encode_dpcm(z.ctypes.data, z.ctypes.data, 8, 8, 100, out.ctypes.data, out.size, C.byref(n)) == N.TIC_E_QUALITY
    assert L.tic_entropy_encode_dpcm(z.ctypes.data, z.ctypes.data, 8, 8, 50, out.ctypes.data, 16, C.byref(n)) == N.TIC_E_SPACE
    assert n.value == 7 and not out[16:].any()
    assert L.tic_entropy_encode_dpcm(None, None, 0, 8, 50, out.ctypes.data, out.size, C.byref(n)) == N.TIC_OK and n.value == 16


# ---- the corpus can tell a wrong kernel ---------------------------------------------------------------------------------------------

def _mutant_census(fx, oracle, label, names, **switch):
    """Per frame the number of blocks in which the mutant differs from the fixture; the unmutated model must equal the fixture there (so
    that the mutation is what differs).  Every count has to be positive."""
    frames = WB.frames()
    counts = {}
    for name in names:
        f = frames[name]
        dc, ac = WB.model(f.img, f.quality, oracle.dct8)
        assert WB.first_difference(dc, ac, fx.dc(name), fx.ac(name)) is None, "the unmutated model differs on %s" % name
        mdc, mac = WB.model(f.img, f.quality, oracle.dct8, **switch)
        counts[name] = int(WB.differing_blocks(mdc, mac, fx.dc(name), fx.ac(name)).size)
    print("mutant %-28s %s" % (label, counts))
    assert counts and all(c > 0 for c in counts.values()), (label, {n: c for n, c in counts.items() if c == 0})
    return counts


def test_mutant_float_subtraction_of_128(fx, oracle):
    """`(double)pixel - 128.0` instead of int32's wrapping subtraction, on the frames of the extremes family that hold a pixel in
    INT32_MIN .. INT32_MIN + 127 (the others - INT32_MIN + 128 and INT32_MAX alone - are its first non-wrapping neighbours: no mutant of
    the subtraction can differ there, and this one must not)."""
    frames = WB.frames()
    wraps = [n for n in fx.names("extremes") if (frames[n].img.astype(np.int64) - 128 < WB.I32_MIN).any()]
    rest = [n for n in fx.names("extremes") if n not in wraps]
    assert len(wraps) >= 7 and "ext_flat_min_q10" in wraps and "ext_flat_min127_q10" in wraps and "ext_flat_min128_q10" in rest
    _mutant_census(fx, oracle, "float subtraction of 128", wraps, float_sub=True)
    for name in rest:
        f = frames[name]
        assert WB.first_difference(*WB.model(f.img, f.quality, oracle.dct8, float_sub=True), fx.dc(name), fx.ac(name)) is None, name


def test_mutant_single_bounce_reflection(fx, oracle):
    """One reflection at the edge, on the reflect frames with an axis of 2..4 samples (np.pad bounces twice and more there).  An axis of one
    sample has nothing to tell apart - every index reads that sample - so 1 x 1, 1 x 5.. and 5.. x 1 are not in this list; an axis of 5..7
    needs a single bounce only."""
    names = [n for n in fx.names("reflect") if any(2 <= d <= 4 for d in WB.frames()[n].img.shape)]
    assert len(names) == 49 - 16  # of the 7 x 7 shapes, all but those with both axes in {1, 5, 6, 7}
    _mutant_census(fx, oracle, "single-bounce reflection", names, single_bounce=True)


def test_mutant_unwrapped_dc_difference(fx, oracle):
    _mutant_census(fx, oracle, "unwrapped DC difference", [WB.PAIR_FRAME], wide_diff=True)


def test_mutant_tiles_x_taken_as_one(fx, oracle):
    names = [n for n in fx.names("geometry") if n.startswith(("geo_72x136_", "geo_40x200_"))]
    assert len(names) == 6
    counts = _mutant_census(fx, oracle, "tiles_x taken as 1", names, tiles_x_one=True)
    assert counts["geo_72x136_q50"] >= 9 * 8 and counts["geo_40x200_q50"] >= 5 * 16  # every block beyond the first tile of its row, almost surely


def test_mutant_matrix_dct_on_the_ties(fx, oracle):
    """D @ X @ D.T and np.round - a transform as exact as the reference's, in another operation order - against the reference on exact
    ties.  On the 512 flat blocks it must disagree on at least a quarter, the reference itself rounding at least 100 up and 100 down; on the
    other three positions it has to disagree somewhere."""
    frames = WB.frames()
    f = frames["tie_00_q50"]
    dc, ac = WB.model(f.img, 50, oracle.dct8)
    assert WB.first_difference(dc, ac, fx.dc(f.name), fx.ac(f.name)) is None
    mdc, mac = WB.model(f.img, 50, oracle.dct8, matrix_dct=True)
    got, want = np.cumsum(mdc), np.cumsum(fx.dc(f.name).astype(np.int64))
    odd = WB.tie_odds()
    up, down = int((2 * want > odd).sum()), int((2 * want < odd).sum())
    differ = int((got != want).sum())
    print("mutant matrix-product DCT on tie_00: differs on %d of 512 flat blocks; the reference rounds %d up, %d down" % (differ, up, down))
    assert up + down == 512 and up >= 100 and down >= 100
    assert (up, down) == (fx.census["ties"]["00"]["up"], fx.census["ties"]["00"]["down"])
    assert differ >= 128
    assert (np.abs(2 * got - odd) == 1).all()  # (the mutant rounds every tie to a neighbour: it is wrong only in the direction)
    _mutant_census(fx, oracle, "matrix-product DCT", ["tie_04_q50", "tie_40_q50", "tie_44_q50"], matrix_dct=True)
