"""entropy_decode (a stream's coefficients) and lossless re-tabling on the GPU: the fused decoder's phase 1 with a coefficient sink
(tinyimgcodec_amd/csrc/tic_entropy_dec_gpu.hip dec_decode_coef_kernel), decode_on_device's coefficient sink, the adaptive reader's front
half, and the two re-writes, through the C-ABI of include/tinyimgcodec_hip_transcode.h and the Python mirror.

Every expectation is a fixture made by the unmodified reference or the pinned oracle: the built coefficients of tests/decoder_streams.py
and tests/entropy_blocks.py (tied to their fixtures' digests), lenna.npz, benchmark_set.json / adaptive_streams.json, the damaged corpora
(damaged_streams.json, retable_damaged.json, damaged_adaptive.json).  Comparisons are array_equal or sha256.  Besides the values every
test asserts the PATH where one is due: a reader that goes wrong quietly hands over to the host - right coefficients, and a device
reader that does not work.  Run with `-m gpu` on an MI355X."""
import ctypes as C
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import damaged_adaptive as DA
import damaged_streams as D
import decoder_streams as DS
import entropy_blocks as EB
import test_decoder_streams_gpu as TD  # check_path, state, SECOND_RUN, FORCED: the rules of the pixel route, not restated

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N
from conftest import GOLDEN, rand_frame

pytestmark = pytest.mark.gpu

FX = TD.FX
NAMES = TD.NAMES
TAIL = 64  # sentinel bytes behind every output buffer
SCALED = 1 << 30


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def lengths(oracle):
    return EB.Lengths(oracle.dump_tables())


@pytest.fixture(scope="module")
def built(oracle, lengths):
    """name -> frame (with its coefficients, tied to the fixture's coeffs_sha256), (name, variant key) -> stream, tied as well."""
    frames = DS.build_frames(lengths)
    assert sorted(frames) == sorted(NAMES) and len(NAMES) == 26
    streams = {}
    for name, fr in frames.items():
        assert EB.sha(np.ascontiguousarray(fr["zz"], dtype="<i4").tobytes()) == FX[name]["coeffs_sha256"], name
        payload = DS.payload_stream(oracle, fr)
        for variant in fr["variants"]:
            s = DS.with_header(payload, fr, variant)
            rec = FX[name]["streams"][DS.key(variant)]
            assert (len(s), EB.sha(s)) == (rec["bytes"], rec["sha256"]), (name, variant)
            streams[name, DS.key(variant)] = s
    return frames, streams


def c_decode(L, handle, s, n, adaptive=False):
    """tic_entropy_decode[_adaptive] into n * 128 bytes of 0xA5 with a sentinel behind them -> (rc, int16 [n, 64], (h, w, quality, flag))."""
    buf = np.frombuffer(bytes(s), np.uint8)
    out = np.full(n * 128 + TAIL, 0xA5, np.uint8)
    h, w, q, flag = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_uint32(0)
    if adaptive:
        rc = L.tic_entropy_decode_adaptive(handle, buf.ctypes.data, buf.size, out.ctypes.data, n, C.byref(h), C.byref(w), C.byref(q))
    else:
        rc = L.tic_entropy_decode(handle, buf.ctypes.data, buf.size, out.ctypes.data, n, C.byref(h), C.byref(w), C.byref(q), C.byref(flag))
    assert (out[n * 128:] == 0xA5).all(), "bytes behind the caller's buffer were written"
    if rc != N.TIC_OK:
        assert (out == 0xA5).all(), "a failing call wrote into its buffer"
    return rc, out[: n * 128].view(np.int16).reshape(n, 64), (h.value, w.value, q.value, flag.value)


def check_built(L, ctx, name, key, frames, streams, what):
    """One built stream through tic_entropy_decode: the built coefficients and the header's fields, or TIC_E_RANGE for the twins."""
    fr, s = frames[name], streams[name, key]
    flag, q = [v for v in fr["variants"] if DS.key(v) == key][0]
    rc, zz, head = c_decode(L, ctx.handle, s, DS.N)
    if DS.is_twin(name):
        assert rc == N.TIC_E_RANGE and "running DC" in L.tic_last_error(ctx.handle).decode(), (what, name, key, rc)
        with pytest.raises(ValueError):
            T.entropy_decode(s, ctx=ctx)
        return
    assert rc == N.TIC_OK, (what, name, key, rc, L.tic_last_error(ctx.handle).decode())
    assert head == (DS.H, DS.W, q, SCALED if flag else 0), (what, name, key, head)
    if not np.array_equal(zz, fr["zz"]):
        bad = np.argwhere(zz != fr["zz"])
        pytest.fail("%s, %s %s: %d coefficients differ, the first in block %d at scan position %d: %d instead of %d"
                    % (what, name, key, len(bad), bad[0][0], bad[0][1], zz[tuple(bad[0])], fr["zz"][tuple(bad[0])]))


# ---- the built frames: 2,145 blocks - eight full workgroups, one of 97 lanes, a wave of 33 ----------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_built_frames_default_route(name, ctx, built):
    """Every header variant through tic_entropy_decode: the built coefficients from the device reader, in one run at the range the rule
    gives or in two with the longest - path, give-up, range and tries as tic_decompress's (tests/test_decoder_streams_gpu.py)."""
    L = N.load()
    frames, streams = built
    rule = FX[name]["census"]["range_rule"]
    for variant in frames[name]["variants"]:
        key = DS.key(variant)
        check_built(L, ctx, name, key, frames, streams, "default route")
        path, giveup, r, tries = TD.state(L, ctx.handle)
        print("%-22s %-4s -> path %d, giveup %d, range %d bits (rule %d), tries %d" % (name, key, path, giveup, r, rule, tries))
        TD.check_path(name, path, giveup, "tic_entropy_decode")
        if path == 1:
            assert (r, tries) == ((2016, 2) if rule in TD.SECOND_RUN.get(name, ()) else (rule, 1)), (name, key, r, tries)


@pytest.mark.parametrize("name", NAMES)
def test_built_frames_host_route(name, ctx, built, monkeypatch):
    """TIC_DECODE_HOST=1: the host reader, path 2, the same coefficients (and the same refusal of the twins)."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_HOST", "1")
    frames, streams = built
    for variant in frames[name]["variants"]:
        check_built(L, ctx, name, DS.key(variant), frames, streams, "host route")
        assert L.tic_last_decode_path(ctx.handle) == 2, (name, variant)
        assert L.tic_last_decode_giveup(ctx.handle) == 0, (name, variant)


def forced_set(L, ctx, built, forced, what):
    frames, streams = built
    for name in TD.FORCED:
        key = TD.plain_key(name)
        check_built(L, ctx, name, key, frames, streams, what)
        path, giveup, r, tries = TD.state(L, ctx.handle)
        print("%s: %-16s -> path %d, giveup %d, range %d bits, tries %d" % (what, name, path, giveup, r, tries))
        assert (path, giveup) == (1, 0), (what, name, path, giveup)
        first = forced if forced else FX[name]["census"]["range_rule"]
        assert (r, tries) in ((first, 1), (2016, 2)), (what, name, r, tries)
        assert (tries == 2) == (first in TD.SECOND_RUN.get(name, ())), (what, name, r, tries)


@pytest.mark.parametrize("forced", [288, 2016])
def test_forced_ranges(forced, ctx, built, monkeypatch):
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_RANGE", str(forced))
    forced_set(L, ctx, built, forced, "forced range %d" % forced)


def test_flat_grid(ctx, built, monkeypatch):
    """TIC_DECODE_FLAT_GRID=0: the sums in front of a workgroup by look-back."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_FLAT_GRID", "0")
    forced_set(L, ctx, built, 0, "look-back sums")


def test_the_frames_reach_both_windows_of_the_new_kernel():
    """By the size rule of the launcher (stream bits / blocks <= 240: the 2,048-word window); the scaled flag makes no third kernel."""
    seen = {e["census"]["bits_per_block"] <= 240 for n, e in FX.items() if not DS.is_twin(n)}
    assert seen == {True, False}


# ---- block-count edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(256, 256), (8, 8200), (8, 8712)], ids=lambda s: "%dx%d" % s)
def test_block_count_edges(shape, ctx, oracle):
    """1,024 blocks (every workgroup full), 1,025 (one lane in the last workgroup), 1,089 (a wave with one block): seeded noise, the
    oracle's stream, the oracle's coefficients; the device route with nothing flagged."""
    L = N.load()
    h, w = shape
    n = ((h + 7) // 8) * ((w + 7) // 8)
    assert n in (1024, 1025, 1089)
    img = rand_frame(7000 + w, h, w)
    s = oracle.compress(img, 50)
    rc, zz, head = c_decode(L, ctx.handle, s, n)
    assert rc == N.TIC_OK and head == (h, w, 50, 0), (rc, head, L.tic_last_error(ctx.handle).decode())
    assert np.array_equal(zz, oracle.encode_zz16(img, 50))
    assert (L.tic_last_decode_path(ctx.handle), L.tic_last_decode_giveup(ctx.handle)) == (1, 0)


def test_frames_without_blocks(ctx):
    """TIC_OK with nothing written for the decode calls, TIC_E_ARG for tic_retable_adaptive (as tic_compress_adaptive); the Python
    dictionary is what the reference's reader makes of such a header: empty dc and ac, which decode() turns into an empty image."""
    L = N.load()
    for h, w in ((0, 0), (0, 8), (8, 0)):
        s = struct.pack("<IIII", h, w, 50, 0)
        rc, _, head = c_decode(L, ctx.handle, s, 0)
        assert rc == N.TIC_OK and head == (h, w, 50, 0)
        info = T.entropy_decode(s, ctx=ctx)
        assert info["dc"].shape == (0,) and info["ac"].shape == (0, 63) and T.decode(info, ctx=ctx).shape == (h, w)
        buf, out, n = np.frombuffer(s, np.uint8), np.zeros(64, np.uint8), C.c_size_t(0)
        assert L.tic_retable_adaptive(ctx.handle, buf.ctypes.data, buf.size, out.ctypes.data, out.size, C.byref(n)) == N.TIC_E_ARG
        assert (out == 0).all()


# ---- the reference's own dictionary ------------------------------------------------------------------------------------------------------
def test_the_references_dictionary(ctx):
    lenna = np.load(os.path.join(GOLDEN, "lenna.npz"))
    info = T.entropy_decode(lenna["q50_bs"].tobytes(), ctx=ctx)
    assert (info["height"], info["width"], info["quality"], info["scaled_dct"]) == (512, 512, 50, False)
    assert info["dc"].dtype == np.int32 and np.array_equal(info["dc"], lenna["q50_dc"])
    assert info["ac"].dtype == np.int16 and info["ac"].shape == (4096, 63) and np.array_equal(info["ac"], lenna["q50_ac"])
    assert sorted(info) == ["ac", "dc", "height", "quality", "scaled_dct", "width"]
    for q in (10, 50, 90):
        s = lenna["q%d_bs" % q].tobytes()
        assert np.array_equal(T.decode(T.entropy_decode(s, ctx=ctx), ctx=ctx), lenna["q%d_dec" % q]), q
        zz, hdr = T.entropy_decode_zz(s, ctx=ctx)
        assert zz.shape == (4096, 64) and zz.dtype == np.int16 and hdr == {"height": 512, "width": 512, "quality": q, "scaled_dct": False}
        assert T.entropy_encode(zz, 512, 512, q) == s  # the mirror of entropy_encode


# ---- the entropy_blocks fixture: 123 built frames ----------------------------------------------------------------------------------------
def adaptive_device_eligible(s):
    """tic_api.hip adaptive_device_takes with the size line out of the way: no code of length zero."""
    table = DA.read_table(s)[0]
    return min(len(code) for _, code in table["DC"] + table["AC"]) > 0


def test_entropy_blocks_frames(ctx, lengths, monkeypatch):
    """Streams from entropy_encode / entropy_encode_adaptive of the built coefficients, tied to the fixture first.  Each re-write is the
    fixture's stream of the other family (KeyError where the reference has no default code); both readers return the built coefficients.
    The frames of 2,145 blocks take the device readers (the adaptive reader's line lowered with TIC_DECODE_MIN_BITS), the strips the host's."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_MIN_BITS", "0")
    fx = EB.load_fixture()["frames"]
    frames = EB.build_frames(lengths)
    assert set(frames) == set(fx) and len(frames) == 123
    big = 0
    for name, fr in frames.items():
        e, zz, h, w, q = fx[name], fr["zz"], fr["h"], fr["w"], fr["quality"]
        assert EB.coeff_sha(zz) == e["coeffs_sha256"], name
        n = zz.shape[0]
        default = adaptive = None
        if "raises" not in e["stream"]:
            default = T.entropy_encode(zz, h, w, q)
            assert EB.sha(default) == e["stream"]["sha256"], name
        if "raises" not in e["adaptive"]:
            adaptive = T.entropy_encode_adaptive(zz, h, w, q, ctx=ctx)
            assert EB.sha(adaptive) == e["adaptive"]["sha256"], name
        big += n == EB.BASE_N
        if default is not None:
            got, hdr = T.entropy_decode_zz(default, ctx=ctx)
            assert np.array_equal(got, zz) and hdr == {"height": h, "width": w, "quality": q, "scaled_dct": False}, name
            path, giveup = L.tic_last_decode_path(ctx.handle), L.tic_last_decode_giveup(ctx.handle)
            if n == EB.BASE_N:
                TD.check_path(name if name in TD.MAY_HAND_OVER else "", path, giveup, "entropy_decode of " + name)
            else:
                assert (path, giveup) == (2, 0), (name, path, giveup)
            if adaptive is not None:
                assert EB.sha(T.retable_adaptive(default, ctx=ctx)) == e["adaptive"]["sha256"], name
            else:
                with pytest.raises(OverflowError):
                    T.retable_adaptive(default, ctx=ctx)
        if adaptive is not None:
            info = T.entropy_decode_adaptive(adaptive, ctx=ctx)
            path, giveup = L.tic_last_decode_path(ctx.handle), L.tic_last_decode_giveup(ctx.handle)
            assert np.array_equal(np.cumsum(info["dc"], dtype=np.int64), zz[:, 0]) and np.array_equal(info["ac"], zz[:, 1:]), name
            if n == EB.BASE_N and adaptive_device_eligible(adaptive):
                assert (path, giveup) == (1, 0), ("the adaptive device reader handed over", name, path, giveup)
            elif n != EB.BASE_N:
                assert (path, giveup) == (2, 0), (name, path, giveup)
            if default is not None:
                assert EB.sha(T.retable_default(adaptive, ctx=ctx)) == e["stream"]["sha256"], name
            else:
                assert e["stream"]["raises"] == "KeyError", name
                with pytest.raises(KeyError):
                    T.retable_default(adaptive, ctx=ctx)
    assert big == 57


# ---- the benchmark set: 49 images x 6 qualities -----------------------------------------------------------------------------------------
def benchmark_jobs():
    pixels = np.load(os.path.join(GOLDEN, "benchmark_set.npz"))["pixels"]
    with open(os.path.join(GOLDEN, "benchmark_set.json")) as f:
        default = {(e["image"], e["quality"]): e for e in json.load(f)["entries"]}
    with open(os.path.join(GOLDEN, "adaptive_streams.json")) as f:
        adaptive = {(e["image"], e["quality"]): e for e in json.load(f)["benchmark"]}
    assert sorted(default) == sorted(adaptive) and len(default) == 294
    return pixels, default, adaptive


def retable_both_ways(L, ctx, pixels, default, adaptive, keys, lowered):
    for k in keys:
        s = T.compress(pixels[k[0] - 1], k[1], ctx=ctx)
        assert (len(s), D.sha(s)) == (default[k]["bytes"], default[k]["sha256"]), k
        ra = T.retable_adaptive(s, ctx=ctx)
        assert (L.tic_last_decode_path(ctx.handle), L.tic_last_decode_giveup(ctx.handle)) == (1, 0), ("retable_adaptive", k)
        assert (len(ra), D.sha(ra)) == (adaptive[k]["bytes"], adaptive[k]["sha256"]), k
        rd = T.retable_default(ra, ctx=ctx)
        if lowered:
            assert (L.tic_last_decode_path(ctx.handle), L.tic_last_decode_giveup(ctx.handle)) == (1, 0), ("retable_default", k)
        assert D.sha(rd) == default[k]["sha256"], k


def test_benchmark_set_both_ways(ctx, monkeypatch):
    """retable_adaptive(compress(img, q)) is the reference's stream with the image's own tables, retable_default of that the reference's
    default stream again; the device reader in both directions (the adaptive reader's line lowered: its streams at q = 5 are 4 KB)."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_MIN_BITS", "0")
    pixels, default, adaptive = benchmark_jobs()
    retable_both_ways(L, ctx, pixels, default, adaptive, sorted(default), True)


def test_ten_benchmark_retablings(ctx):
    """Ten of them without a hook (what the shipped library runs too): the default-table reader on the device."""
    pixels, default, adaptive = benchmark_jobs()
    retable_both_ways(N.load(), ctx, pixels, default, adaptive, sorted(default)[::30][:10], False)


# ---- the damaged default-table corpus: all 472 entries -----------------------------------------------------------------------------------
def test_damaged_default_corpus(ctx, oracle, monkeypatch):
    """decode(entropy_decode(s)) is the reference's decompress(s) for every entry (TIC_DECODE_MIN_BLOCKS=1: the small bases reach the
    device reader); both re-writes are the reference's reader followed by its writer (retable_damaged.json), and the re-written stream
    decodes to the same pixels.  The two scaled_dct entries are refused."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_MIN_BLOCKS", "1")
    rec = {r["name"]: r for r in D.load_fixture()["entries"]}
    with open(os.path.join(GOLDEN, "retable_damaged.json")) as f:
        rt = {r["name"]: r for r in json.load(f)["entries"]}
    entries = D.corpus(oracle)
    assert len(entries) == 472 and [e[0] for e in entries] == list(rec) == list(rt)
    on_device = rewritten = 0
    for name, base, kind, params, s in entries:
        assert D.sha(s) == rec[name]["sha256"] == rt[name]["sha256"], name
        want = (rec[name]["h"], rec[name]["w"], rec[name]["pixels_sha256"])
        px = T.decode(T.entropy_decode(s, ctx=ctx), ctx=ctx)
        path, giveup = L.tic_last_decode_path(ctx.handle), L.tic_last_decode_giveup(ctx.handle)
        assert not (path == 1 and giveup != 0), (name, path, giveup)
        on_device += path == 1
        assert (px.shape[0], px.shape[1], D.px_sha(px)) == want, ("decode(entropy_decode(s))", name, path, giveup)
        if rt[name].get("scaled_dct"):
            with pytest.raises(ValueError):
                T.retable_adaptive(s, ctx=ctx)
            continue
        ra = T.retable_adaptive(s, ctx=ctx)
        assert (len(ra), D.sha(ra)) == (rt[name]["adaptive"]["bytes"], rt[name]["adaptive"]["sha256"]), ("retable_adaptive", name)
        rd = T.retable_default(ra, ctx=ctx)
        assert (len(rd), D.sha(rd)) == (rt[name]["default"]["bytes"], rt[name]["default"]["sha256"]), ("retable_default", name)
        px = T.decompress_adaptive(ra, ctx=ctx)
        assert (px.shape[0], px.shape[1], D.px_sha(px)) == want, ("decompress_adaptive(retable_adaptive(s))", name)
        rewritten += 1
    print("%d entries, %d read by the device reader, %d re-written both ways" % (len(entries), on_device, rewritten))
    assert rewritten == 470 and on_device >= 100


# ---- the damaged adaptive corpus: 1,100 entries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lowered", [False, True], ids=["default_route", "device_line_lowered"])
def test_damaged_adaptive_corpus(lowered, ctx, oracle, monkeypatch):
    """entropy_decode_adaptive raises ValueError exactly where the fixture's contract refuses; elsewhere decode() of its dictionary gives
    the fixture's pixels."""
    L = N.load()
    if lowered:
        assert L.tic_build_has_test_hooks() == 1
        monkeypatch.setenv("TIC_DECODE_MIN_BLOCKS", "1")
        monkeypatch.setenv("TIC_DECODE_MIN_BITS", "0")
    fx = DA.load_fixture()
    rec = DA.records(fx)
    entries = DA.corpus(oracle, fx, DA.base_streams(oracle, fx))
    assert [e[0] for e in entries] == list(rec) and len(entries) == 1100
    wrong, on_device = [], 0
    for name, base, kind, params, s in entries:
        o = rec[name]["outcome"]
        try:
            info = T.entropy_decode_adaptive(s, ctx=ctx)
        except ValueError:
            got = "refused"
        else:
            px = T.decode(info, ctx=ctx)
            got = [px.shape[0], px.shape[1], DA.px_sha(px)]
            on_device += L.tic_last_decode_path(ctx.handle) == 1
        if (got == "refused") != isinstance(o, str) or (got != "refused" and list(o) != got):
            wrong.append((name, got if got == "refused" else got[:2], o if isinstance(o, str) else list(o)[:2]))
    print("%d entries, %d wrong, %d decoded entries read by the device reader" % (len(entries), len(wrong), on_device))
    assert not wrong, (wrong[:10], len(wrong))
    if lowered:
        assert on_device >= 150


# ---- stream and coefficients resident --------------------------------------------------------------------------------------------------
class Resident:
    """A stream buffer and a coefficient buffer in device memory, 0xCD where the reader must not write."""

    def __init__(self, ctx, L, max_stream, nblocks):
        self.ctx, self.L, self.n = ctx, L, nblocks
        self.d_s, self.d_zz = C.c_void_p(), C.c_void_p()
        self.bytes = nblocks * 128 + TAIL
        ctx.check(L.tic_dev_alloc(ctx.handle, max_stream + 64, C.byref(self.d_s)))
        ctx.check(L.tic_dev_alloc(ctx.handle, self.bytes, C.byref(self.d_zz)))

    def load(self, s, offset):
        buf = np.frombuffer(bytes(s), np.uint8)
        self.ctx.check(self.L.tic_memcpy_h2d(self.ctx.handle, C.c_void_p(self.d_s.value + offset), buf.ctypes.data, buf.size))
        self.ctx.check(self.L.tic_memset_dev(self.ctx.handle, self.d_zz, 0xCD, self.bytes))
        return C.c_void_p(self.d_s.value + offset), buf.size

    def rows(self):
        host = np.empty(self.bytes, np.uint8)
        self.ctx.check(self.L.tic_memcpy_d2h(self.ctx.handle, host.ctypes.data, self.d_zz, host.size))
        return host

    def free(self):
        self.L.tic_dev_free(self.ctx.handle, self.d_s)
        self.L.tic_dev_free(self.ctx.handle, self.d_zz)


def test_device_resident_form(ctx, built):
    """tic_entropy_decode_dev: the stream at a 4-byte aligned and at an odd device address, the rows in the caller's buffer with nothing
    behind them written; a buffer one block short gives TIC_E_SPACE and stays untouched; the timed form leaves the same rows."""
    L = N.load()
    frames, streams = built
    jobs = [("pairs", "q50"), ("long_codes", "q99"), ("dense_max", TD.plain_key("dense_max")), ("spikes_flat_one", "q50"), ("pairs", "s0")]
    rs = Resident(ctx, L, max(len(streams[j]) for j in jobs), DS.N)
    try:
        for name, key in jobs:
            for offset in (0, 4, 1, 3):
                d_s, n = rs.load(streams[name, key], offset)
                h, w, q, flag = C.c_int(), C.c_int(), C.c_int(), C.c_uint32()
                rc = L.tic_entropy_decode_dev(ctx.handle, d_s, n, rs.d_zz, DS.N, C.byref(h), C.byref(w), C.byref(q), C.byref(flag))
                assert rc == N.TIC_OK, (name, key, offset, rc, L.tic_last_error(ctx.handle).decode())
                assert (h.value, w.value) == (DS.H, DS.W) and (flag.value != 0) == key.startswith("s")
                assert (L.tic_last_decode_path(ctx.handle), L.tic_last_decode_giveup(ctx.handle)) == (1, 0), (name, key, offset)
                host = rs.rows()
                assert (host[DS.N * 128:] == 0xCD).all(), "bytes behind the caller's buffer were written"
                assert np.array_equal(host[: DS.N * 128].view(np.int16).reshape(DS.N, 64), frames[name]["zz"]), (name, key, offset)
            d_s, n = rs.load(streams[name, key], 0)
            rc = L.tic_entropy_decode_dev(ctx.handle, d_s, n, rs.d_zz, DS.N - 1, None, None, None, None)
            assert rc == N.TIC_E_SPACE and (rs.rows() == 0xCD).all(), (name, key, rc)
            ms = C.c_float(-1)
            rc = L.tic_entropy_decode_dev_timed(ctx.handle, d_s, n, rs.d_zz, DS.N, 1, 2, C.byref(ms))
            assert rc == N.TIC_OK and ms.value > 0, (name, key, rc, L.tic_last_error(ctx.handle).decode())
            host = rs.rows()
            assert (host[DS.N * 128:] == 0xCD).all()
            assert np.array_equal(host[: DS.N * 128].view(np.int16).reshape(DS.N, 64), frames[name]["zz"]), (name, key, "timed")
        rc = L.tic_entropy_decode_dev_timed(ctx.handle, C.c_void_p(rs.d_s.value + 1), 4096, rs.d_zz, DS.N, 1, 1, C.byref(ms))
        assert rc == N.TIC_E_ARG  # the device route only: an odd address goes through a copy
    finally:
        rs.free()


# ---- context state ----------------------------------------------------------------------------------------------------------------------
def state_jobs(oracle, built):
    """What the state tests call: a 512 x 512 noise stream (dense), a built 264 x 520 frame (small), their adaptive twins and every
    expectation, from the oracle and the built coefficients."""
    frames, streams = built
    img = rand_frame(512512, 512, 512)
    big = oracle.compress(img, 90)
    small, small_zz = streams["pairs", "q50"], frames["pairs"]["zz"]
    return {"img": img, "big": big, "big_zz": oracle.encode_zz16(img, 90), "small": small, "small_zz": small_zz,
            "twin": streams["dc_bounds_pos_over", TD.plain_key("dc_bounds_pos_over")]}


def new_calls(c, J, big_first=True):
    """Every new call, a dense one then a small one: exact."""
    order = ("big", "small") if big_first else ("small", "big")
    for which in order:
        s, zz = J[which], J[which + "_zz"]
        q = 90 if which == "big" else 50
        h, w = (512, 512) if which == "big" else (DS.H, DS.W)
        got, hdr = T.entropy_decode_zz(s, ctx=c)
        assert np.array_equal(got, zz) and (hdr["height"], hdr["width"]) == (h, w), which
        ra = T.retable_adaptive(s, ctx=c)
        assert ra == T.entropy_encode_adaptive(zz, h, w, q, ctx=c), which  # (that encoder is pinned on the reference by its own tests)
        info = T.entropy_decode_adaptive(ra, ctx=c)
        assert np.array_equal(np.cumsum(info["dc"], dtype=np.int64), zz[:, 0]) and np.array_equal(info["ac"], zz[:, 1:]), which
        assert T.retable_default(ra, ctx=c) == bytes(s), which


def own_errors(c, J):
    """Each new call's own errors, each followed by a good call."""
    L = N.load()
    with pytest.raises(ValueError):
        T.entropy_decode_zz(J["twin"], ctx=c)  # a running DC outside int16
    with pytest.raises(ValueError):
        T.retable_adaptive(J["twin"], ctx=c)
    out = np.zeros(64, np.uint8)
    n = C.c_size_t(0)
    buf = np.frombuffer(bytes(J["small"]), np.uint8)
    assert L.tic_retable_adaptive(c.handle, buf.ctypes.data, buf.size, out.ctypes.data, out.size, C.byref(n)) == N.TIC_E_SPACE
    assert n.value > 64 and (out == 0).all()
    ra = T.retable_adaptive(J["small"], ctx=c)
    assert n.value == len(ra)
    cut = ra[: len(ra) // 2]
    with pytest.raises(ValueError):
        T.entropy_decode_adaptive(cut, ctx=c)
    with pytest.raises(ValueError):
        T.retable_default(cut, ctx=c)
    abuf = np.frombuffer(ra, np.uint8)
    n = C.c_size_t(0)
    assert L.tic_retable_default(c.handle, abuf.ctypes.data, abuf.size, out.ctypes.data, out.size, C.byref(n)) == N.TIC_E_SPACE
    assert n.value == len(J["small"]) and (out == 0).all()
    rc, _, _ = c_decode(L, c.handle, J["small"], DS.N - 1)
    assert rc == N.TIC_E_SPACE
    new_calls(c, J, big_first=False)


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0xA5], ids=lambda b: "0x%02X" % b)
def test_fresh_context_under_poisoned_allocation(byte, oracle, built, monkeypatch):
    """TIC_POISON: every buffer the new calls use comes straight out of a poisoned allocation; then tic_test_poison and the calls again."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_POISON", "0x%02X" % byte)
    J = state_jobs(oracle, built)
    c = T.Context(0)
    try:
        new_calls(c, J, big_first=False)
        new_calls(c, J)  # dirty, then small
        c.check(L.tic_test_poison(c.handle, byte ^ 0x5A))
        new_calls(c, J)
        own_errors(c, J)
    finally:
        c.close()


def test_interleaved_with_the_other_calls(oracle, built):
    """The new calls between tic_decompress, tic_compress and tic_compress_adaptive on one context: everybody's result stays exact."""
    J = state_jobs(oracle, built)
    c = T.Context(0)
    try:
        for _ in range(2):
            assert T.compress(J["img"], 90, ctx=c) == J["big"]
            new_calls(c, J)
            assert np.array_equal(T.decompress(J["big"], ctx=c), oracle.decompress(J["big"]))
            ra = T.compress_adaptive(J["img"], 90, ctx=c)
            assert T.retable_default(ra, ctx=c) == J["big"] and T.retable_adaptive(J["big"], ctx=c) == ra
            assert T.compress(J["img"], 90, ctx=c) == J["big"]
            own_errors(c, J)
            assert np.array_equal(T.decompress_adaptive(ra, ctx=c), oracle.decompress(J["big"]))
    finally:
        c.close()


def test_the_header_guess_is_left_alone(oracle, built):
    """tic_decompress_dev's guess streak: what tic_last_decode_guess reads over a run of equal frames is the same with new calls -
    of another geometry - in between."""
    L = N.load()
    J = state_jobs(oracle, built)

    def run(between):
        c = T.Context(0)
        rs = Resident(c, L, len(J["big"]), 4096)
        d_o = C.c_void_p()
        c.check(L.tic_dev_alloc(c.handle, 512 * 512, C.byref(d_o)))
        seen = []
        try:
            d_s, n = rs.load(J["big"], 0)
            for _ in range(5):
                assert L.tic_decompress_dev(c.handle, d_s, n, d_o, 512, 512 * 512, None, None) == N.TIC_OK
                seen.append(L.tic_last_decode_guess(c.handle))
                if between:
                    new_calls(c, J, big_first=False)
                    rc = L.tic_entropy_decode_dev(c.handle, d_s, n, rs.d_zz, 4096, None, None, None, None)
                    assert rc == N.TIC_OK
        finally:
            L.tic_dev_free(c.handle, d_o)
            rs.free()
            c.close()
        return seen

    plain, mixed = run(False), run(True)
    print("tic_last_decode_guess over five equal frames: %s; with the new calls in between: %s" % (plain, mixed))
    assert plain == mixed and 1 in plain


# ---- the library that ships ------------------------------------------------------------------------------------------------------------
def test_on_the_shipped_library():
    """The built frames' default route and ten benchmark re-tablings once more in a fresh process on the library that ships
    (TIC_TEST_HOOKS=0: no hooks compiled in)."""
    assert os.environ.get("TIC_TEST_HOOKS") == "1" and N.load().tic_build_has_test_hooks() == 1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    env["TIC_TEST_HOOKS"] = "0"
    code = ("import sys; sys.path.insert(0, %r); import tinyimgcodec_amd._native as N; assert N.load().tic_build_has_test_hooks() == 0; "
            "import pytest; sys.exit(pytest.main([%r, '-m', 'gpu', '-q', '-x', '-p', 'no:cacheprovider', '-k', "
            "'test_built_frames_default_route or test_ten_benchmark or test_block_count or test_the_references']))" % (root, os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail
