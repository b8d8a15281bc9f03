"""Damaged default-table streams through every decoder route: tests/damaged_streams.py builds ONE seeded corpus (flipped bits, value
flips that keep every code length, cuts, appended garbage, tails of ones and zeros, deleted and inserted bytes, headers of another
geometry or quality, the scaled flag), tests/golden/damaged_streams.json holds what the UNMODIFIED reference's decompress() made of every
entry - pixels for all of them: it swallows a block's exception (codec.py:178-186) and reads on behind the data's end (huffman.py:66-98).
The fixture is the expectation on every route; neither the oracle nor the host route is asked.  tests/test_damaged_streams_cpu.py pins
the corpus, the oracle and the host decoder on the same fixture without a GPU.

The device decoder's rule is "anything unusual on the true chain raises a flag and the host decodes": it is wrong without notice when it
does not flag damage the reference reacts to, or when it finishes a still-valid chain with other pixels than the reference's.  The value
flips are the second case made certain: the chain is the clean stream's, so the device decoder must finish them itself (path 1, nothing
flagged), with the changed coefficient and, for a DC, the changed sum in every later block, across its workgroups.

Census of test_single_call's first run (TIC_DECODE_MIN_BLOCKS=1), kind x what became of the entry; "gave up" by give-up bit
(include/tinyimgcodec_hip.h, tic_last_decode_giveup), an entry counted under every bit it raised; "second run" = two or more runs:

    kind         entries  not eligible  device finished  gave up: 16  gave up: 32  second run
    flip1             77            25               46            0            6          11
    flip3             36            12                9            0           15          18
    value_flip        30            10               20            0            0           0
    cut               59            33               26            0            0           0
    garbage           30            10               20            0            0           2
    ones_tail         18             6                3            9            0          10
    zeros_tail        18             6                0           12            0          12
    delete            48            16               28            0            4           4
    insert            60            20               11            0           29          29
    geometry          70            24               46            0            0           0
    quality           24             8               16            0            0           0
    flag_scaled        2             1                1            0            0           0
    all              472           171              226           21           54          86

Give-up bits the corpus reached as a decode's last word: 16 (tails of ones and zeros) and 32 (flips, deleted and inserted bytes), both
incidents on the true chain; 86 entries took more than one run (a first run that flags anything is repeated with the blocks of the last
2,048 bits left to the host, one that met a range without a synchronisation point - bit 4 - at 2,016 bits: tic_api.hip
decode_on_device), 11 of them finished by the device decoder then.  Not reached: 1 (an incident in the first range), 2 (trace overflow), 4 as the last word, 8, 64 (no
block produced), 128 (a look-back that timed out), 256 (a block behind the stream's end: every cut stream was finished by the device
decoder and the host's tail decode) and 512 (a running DC outside int16: tests/test_decoder_streams_gpu.py has the twins for it).

Run with `-m gpu` on an MI355X."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import damaged_streams as D

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = 64            # sentinel bytes behind every output buffer
FILL = 0xAB
HEADER_KINDS = ("geometry", "quality")
RESIDENT_BASES = ("noise256", "twolevel256", "noise64", "lenna64")
SHIPPED_BASES = ("noise256", "twolevel256")
FX = D.load_fixture()
REC = {r["name"]: r for r in FX["entries"]}


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus(oracle):
    """The entries, tied to the fixture's digests, and the clean base streams."""
    entries = D.corpus(oracle)
    assert [e[0] for e in entries] == [r["name"] for r in FX["entries"]]
    for name, base, kind, params, s in entries:
        assert (len(s), D.sha(s)) == (REC[name]["bytes"], REC[name]["sha256"]), name
    bases = D.base_streams(oracle)
    for b, s in bases.items():
        assert D.sha(s) == FX["clean"][b]["sha256"], b
    return entries, bases


def expected(rec):
    """What the reference gave: (h, w, digest of the pixels), or the exception's class name."""
    return rec["raises"] if "raises" in rec else (rec["h"], rec["w"], rec["pixels_sha256"])


def outcome_of(px):
    return (px.shape[0], px.shape[1], D.px_sha(px))


def single_call(ctx, s):
    """One stream through T.decompress -> (outcome as expected() writes it, path, giveup, tries)."""
    L = N.load()
    try:
        got = outcome_of(T.decompress(s, ctx=ctx))
    except (N.NativeError, ValueError, struct.error) as e:
        got = type(e).__name__
    r, tries = C.c_int(), C.c_int()
    assert L.tic_last_decode_range(ctx.handle, C.byref(r), C.byref(tries)) == N.TIC_OK
    return got, L.tic_last_decode_path(ctx.handle), L.tic_last_decode_giveup(ctx.handle), tries.value


def census_table(rows):
    """rows: (kind, eligible, path, giveup, tries) -> the table of the module docstring."""
    bits = sorted({1 << k for r in rows for k in range(12) if r[3] >> k & 1})
    head = ["kind", "entries", "not eligible", "device finished"] + ["gave up: %d" % b for b in bits] + ["second run"]
    lines = [head]
    for kind in D.KINDS + ("all",):
        mine = [r for r in rows if kind in (r[0], "all")]
        lines.append([kind, len(mine), sum(not r[1] for r in mine), sum(r[1] and r[2] == 1 for r in mine)]
                     + [sum(r[1] and r[2] != 1 and bool(r[3] & b) for r in mine) for b in bits] + [sum(r[1] and r[4] >= 2 for r in mine)])
    width = [max(len(str(l[k])) for l in lines) for k in range(len(head))]
    return "\n".join("  ".join(str(c).ljust(width[k]) if k == 0 else str(c).rjust(width[k]) for k, c in enumerate(l)) for l in lines)


# ---- tic_decompress ---------------------------------------------------------------------------------------------------------------------
def test_single_call(ctx, corpus, monkeypatch):
    """Every entry through T.decompress three times: with TIC_DECODE_MIN_BLOCKS=1 (the small bases reach the device decoder), with
    TIC_DECODE_HOST=1 and with TIC_DECODE_SERIAL=1.  Every run gives the fixture's result.  On the first run every value flip on a base
    the device decoder takes ends on path 1 with nothing flagged - its pixels are the device decoder's -, and no entry that ended on
    path 1 carries a give-up bit.  The census table of the first run is printed (and copied into the module docstring)."""
    entries, bases = corpus
    assert N.load().tic_build_has_test_hooks() == 1
    for hook in ("TIC_DECODE_MIN_BLOCKS", "TIC_DECODE_HOST", "TIC_DECODE_SERIAL"):
        monkeypatch.setenv(hook, "1")
        rows, wrong = [], []
        for name, base, kind, params, s in entries:
            got, path, giveup, tries = single_call(ctx, s)
            if got != expected(REC[name]):
                wrong.append((name, got, path, giveup, tries))
            rows.append((kind, D.device_eligible(s), path, giveup, tries))
            if hook == "TIC_DECODE_MIN_BLOCKS":
                assert not (path == 1 and giveup != 0), (name, path, giveup)
                if kind == "value_flip" and D.device_eligible(bases[base]):
                    assert (path, giveup) == (1, 0), ("the device decoder handed over a stream whose chain is the clean one", name, path, giveup, tries)
            else:
                assert path == 2, (hook, name, path)
        monkeypatch.delenv(hook)
        print("\n%s=1: %d entries, %d wrong" % (hook, len(entries), len(wrong)))
        if hook == "TIC_DECODE_MIN_BLOCKS":
            print(census_table(rows))
        assert not wrong, (hook, wrong[:10], len(wrong))


# ---- tic_decompress_batch ---------------------------------------------------------------------------------------------------------------
def run_batch(L, handle, jobs):
    """jobs: [(name, stream, expected outcome)] -> rc; every output buffer caps[i] + TAIL bytes of FILL; checks sentinels, geometry, pixels."""
    n = len(jobs)
    bufs = [np.frombuffer(s, np.uint8) for _, s, _ in jobs]
    caps = [D.header(s)[0] * D.header(s)[1] for _, s, _ in jobs]
    outs = [np.full(c + TAIL, FILL, np.uint8) for c in caps]
    hs, ws = (C.c_int * n)(*[-1] * n), (C.c_int * n)(*[-1] * n)
    rc = L.tic_decompress_batch(handle, (C.c_void_p * n)(*[b.ctypes.data for b in bufs]), (C.c_size_t * n)(*[b.size for b in bufs]), n,
                                (C.c_void_p * n)(*[o.ctypes.data for o in outs]), (C.c_size_t * n)(*caps), hs, ws)
    return rc, outs, caps, hs, ws


def test_batch(ctx, corpus, monkeypatch):
    """The whole corpus through tic_decompress_batch at the C-ABI, every third frame a clean base stream, with the default chunking and
    in chunks of seven frames (TIC_DBATCH_CHUNK, the hook of this call), both with TIC_DECODE_MIN_BLOCKS=1 so that the small bases are
    offered to the batch kernels.  Every frame has the fixture's geometry and pixels - the clean frames too, whatever their neighbours
    are -, every sentinel behind a buffer is intact, and every frame is accounted for.  Entries the reference refuses at the header go
    in a call of their own, which returns the documented error with nothing decoded ("headers are checked before any work")."""
    entries, bases = corpus
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    clean = [("clean/" + b, s, (FX["clean"][b]["h"], FX["clean"][b]["w"], FX["clean"][b]["pixels_sha256"])) for b, s in bases.items()]
    refused = [(name, s, expected(REC[name])) for name, base, kind, params, s in entries if "raises" in REC[name]]
    assert all(kind == "cut" and len(s) < 19 for name, base, kind, params, s in entries if "raises" in REC[name])
    jobs, k = [], 0
    for name, base, kind, params, s in entries:
        if "raises" in REC[name]:
            continue
        jobs.append((name, s, expected(REC[name])))
        if len(jobs) % 3 == 2:
            jobs.append(clean[k % len(clean)])
            k += 1
    assert sum(j[0].startswith("clean/") for j in jobs) * 3 >= len(jobs) - 2
    monkeypatch.setenv("TIC_DECODE_MIN_BLOCKS", "1")
    for chunk in (None, "7"):
        if chunk:
            monkeypatch.setenv("TIC_DBATCH_CHUNK", chunk)
        rc, outs, caps, hs, ws = run_batch(L, ctx.handle, jobs)
        assert rc == N.TIC_OK, (chunk, rc, L.tic_last_error(ctx.handle).decode())
        v = [C.c_int() for _ in range(4)]
        assert L.tic_last_decompress_batch(ctx.handle, *[C.byref(x) for x in v]) == N.TIC_OK
        batch_frames, single_frames, chunks, direct = (x.value for x in v)
        print("\nchunk %s: %d frames -> batch_frames %d, single_frames %d, chunks %d, direct_frames %d" % (chunk or "default", len(jobs), batch_frames, single_frames, chunks, direct))
        wrong = []
        for i, (name, s, want) in enumerate(jobs):
            assert (outs[i][caps[i]:] == FILL).all(), ("bytes behind the caller's buffer were written", chunk, name)
            got = (hs[i], ws[i], D.sha(outs[i][:caps[i]].tobytes()))
            if got != want:
                wrong.append((i, name, got[:2]))
        assert not wrong, (chunk, wrong[:10], len(wrong))
        assert batch_frames + single_frames == len(jobs), (chunk, batch_frames, single_frames, len(jobs))
        if chunk:
            assert chunks >= (batch_frames + 6) // 7 and batch_frames > 0, (chunks, batch_frames)
    if refused:  # the header's contract: the first bad frame's error, nothing decoded
        mixed = jobs[:2] + refused + jobs[2:4]
        rc, outs, caps, hs, ws = run_batch(L, ctx.handle, mixed)
        assert rc == N.TIC_E_STREAM, rc
        assert all((o == FILL).all() for o in outs)


# ---- tic_decompress_dev and its asynchronous form ----------------------------------------------------------------------------------------
class Surface:
    """A stream buffer and a pixel buffer in device memory, FILL everywhere the decoder must not write."""

    def __init__(self, ctx, L, max_stream, nbytes):
        self.ctx, self.L, self.bytes = ctx, L, nbytes + TAIL
        self.d_s, self.d_o = C.c_void_p(), C.c_void_p()
        ctx.check(L.tic_dev_alloc(ctx.handle, max_stream + 64, C.byref(self.d_s)))
        ctx.check(L.tic_dev_alloc(ctx.handle, self.bytes, C.byref(self.d_o)))

    def load(self, s):
        buf = np.frombuffer(s, np.uint8)
        self.ctx.check(self.L.tic_memcpy_h2d(self.ctx.handle, self.d_s, buf.ctypes.data, buf.size))
        self.ctx.check(self.L.tic_memset_dev(self.ctx.handle, self.d_o, FILL, self.bytes))
        return buf.size

    def pixels(self, h, w, stride, what):
        """The h x w window, rows `stride` apart; everything between and behind the rows must still be FILL."""
        host = np.empty(self.bytes, np.uint8)
        self.ctx.check(self.L.tic_memcpy_d2h(self.ctx.handle, host.ctypes.data, self.d_o, host.size))
        rows = host[: h * stride].reshape(h, stride)
        assert (rows[:, w:] == FILL).all() and (host[h * stride:] == FILL).all(), ("bytes outside the window were written", what)
        return np.ascontiguousarray(rows[:, :w])

    def free(self):
        self.L.tic_dev_free(self.ctx.handle, self.d_s)
        self.L.tic_dev_free(self.ctx.handle, self.d_o)


def resident_subset(entries):
    sub = [e for e in entries if e[1] in RESIDENT_BASES]
    assert {e[2] for e in sub} == set(D.KINDS)
    return sub


def declared(s):
    h, w = D.header(s)[:2]
    return h, w, w + 24


def test_resident_and_async(corpus, monkeypatch):
    """Every kind on the 256 x 256 and 64 x 64 bases through tic_decompress_dev with out_stride = w + 24 into a sentinel-filled buffer
    sized for the largest declared geometry, behind two clean streams of the base's header (a guess is armed), and through
    tic_decompress_dev_async with four tickets open, collected out of order.  The rows carry the fixture's pixels and everything between
    and behind them is sentinel.  A geometry or quality entry decoded behind two clean streams never has its guess held (+1); where the
    clean streams armed one and the entry is long enough to be launched on it, tic_last_decode_guess is -1."""
    entries, bases = corpus
    sub = resident_subset(entries)
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_MIN_BLOCKS", "1")
    ctx2 = T.Context(0)
    biggest = max(declared(e[4])[0] * declared(e[4])[2] for e in sub)
    longest = max(len(e[4]) for e in sub)
    surfaces = [Surface(ctx2, L, longest, biggest) for _ in range(4)]

    def sync(sf, s):
        h, w, stride = declared(s)
        n = sf.load(s)
        hh, ww = C.c_int(), C.c_int()
        rc = L.tic_decompress_dev(ctx2.handle, sf.d_s, n, sf.d_o, stride, h * stride, C.byref(hh), C.byref(ww))
        assert rc == N.TIC_OK, (rc, L.tic_last_error(ctx2.handle).decode())
        return hh.value, ww.value

    def arm(base):
        """Two clean streams of the base -> True when the device decoder finished both (their header is cached, a guess comes next)."""
        paths = []
        for _ in range(2):
            assert sync(surfaces[0], bases[base]) == D.BASES[base][:2]
            paths.append(L.tic_last_decode_path(ctx2.handle))
        return paths == [1, 1]

    def check(sf, name, kind, s, hw, armed, what, guess_is_this_calls=True):
        h, w, stride = declared(s)
        want = expected(REC[name])
        assert hw == (h, w) == want[:2], (what, name, hw)
        px = sf.pixels(h, w, stride, (what, name))
        assert D.px_sha(px) == want[2], (what, name, "path %d, giveup %d, guess %d" % (L.tic_last_decode_path(ctx2.handle), L.tic_last_decode_giveup(ctx2.handle), L.tic_last_decode_guess(ctx2.handle)))
        if kind in HEADER_KINDS and guess_is_this_calls:
            guess = L.tic_last_decode_guess(ctx2.handle)
            assert guess != 1, (what, name, guess)
            if armed and D.device_eligible(s):
                assert guess == -1, (what, name, guess)

    try:
        # ---- synchronous: the entries of a base behind two clean streams; every header entry behind two of its own
        guesses = {}
        for base in RESIDENT_BASES:
            armed = arm(base)
            for name, b, kind, params, s in sub:
                if b != base:
                    continue
                if kind in HEADER_KINDS:
                    armed = arm(base)
                hw = sync(surfaces[1], s)
                g = L.tic_last_decode_guess(ctx2.handle)
                guesses[kind, g] = guesses.get((kind, g), 0) + 1
                check(surfaces[1], name, kind, s, hw, armed, "tic_decompress_dev")
        print("\ntic_decompress_dev: (kind, guess) -> entries: %s" % sorted(guesses.items()))
        # ---- asynchronous: groups of four tickets behind two clean streams, collected out of order
        guesses = {}
        for base in RESIDENT_BASES:
            mine = [e for e in sub if e[1] == base]
            for at in range(0, len(mine), 4):
                group = mine[at:at + 4]
                armed = arm(base)
                tickets = []
                for k, (name, b, kind, params, s) in enumerate(group):
                    h, w, stride = declared(s)
                    n = surfaces[k].load(s)
                    t = C.c_longlong(-1)
                    ctx2.check(L.tic_decompress_dev_async(ctx2.handle, surfaces[k].d_s, n, surfaces[k].d_o, stride, h * stride, C.byref(t)))
                    tickets.append(t.value)
                for k in [k for k in (2, 0, 3, 1) if k < len(group)]:
                    name, b, kind, params, s = group[k]
                    hh, ww = C.c_int(), C.c_int()
                    rc = L.tic_decompress_async_result(ctx2.handle, tickets[k], 1, C.byref(hh), C.byref(ww))
                    assert rc == N.TIC_OK, (name, rc, L.tic_last_error(ctx2.handle).decode())
                    # (hooks build: the ticket's fate is in tic_last_error.  A ticket that was not launched ran synchronously when it was
                    #  opened, and tic_last_decode_guess has been overwritten by the tickets collected since)
                    launched = " launched 1," in L.tic_last_error(ctx2.handle).decode()
                    g = L.tic_last_decode_guess(ctx2.handle) if launched else "not launched"
                    guesses[kind, g] = guesses.get((kind, g), 0) + 1
                    check(surfaces[k], name, kind, s, (hh.value, ww.value), armed, "tic_decompress_dev_async", launched)
        print("tic_decompress_dev_async: (kind, guess) -> entries: %s" % sorted(guesses.items(), key=str))
        assert any(guesses.get((kind, -1)) for kind in HEADER_KINDS), "no geometry or quality entry was launched on a guess"
    finally:
        for sf in surfaces:
            sf.free()
        ctx2.close()


# ---- the library that ships ------------------------------------------------------------------------------------------------------------
def shipped_child():
    """Runs in the fresh process of test_shipped_library: the 256 x 256 entries through decompress and decompress_batch of the library
    without hooks."""
    from oracle import pyoracle
    assert N.load().tic_build_has_test_hooks() == 0 and not [k for k in os.environ if k.startswith("TIC_") and k != "TIC_TEST_HOOKS"]
    entries = [e for e in D.corpus(pyoracle) if e[1] in SHIPPED_BASES]
    assert {e[2] for e in entries} == set(D.KINDS) - {"flag_scaled"}
    ctx = T.Context(0)
    L = N.load()
    on_device = 0
    for name, base, kind, params, s in entries:
        got, path, giveup, tries = single_call(ctx, s)
        assert got == expected(REC[name]), ("decompress", name, got, path, giveup, tries)
        assert not (path == 1 and giveup != 0), (name, path, giveup)
        if kind == "value_flip":
            assert (path, giveup) == (1, 0), (name, path, giveup)
        on_device += path == 1
    outs = T.decompress_batch([e[4] for e in entries], ctx=ctx)
    for (name, base, kind, params, s), px in zip(entries, outs):
        assert outcome_of(px) == expected(REC[name]), ("decompress_batch", name)
    v = [C.c_int() for _ in range(4)]
    assert L.tic_last_decompress_batch(ctx.handle, *[C.byref(x) for x in v]) == N.TIC_OK
    assert v[0].value + v[1].value == len(entries)
    ctx.close()
    print("shipped library ok: %d entries, %d finished by the device decoder; batch_frames %d, single_frames %d" % (len(entries), on_device, v[0].value, v[1].value))


def test_shipped_library():
    """The 256 x 256 entries, all kinds, through decompress and decompress_batch in ONE fresh process that loads the library that ships
    (no hooks compiled in) and sets no TIC_* variable."""
    assert os.environ.get("TIC_TEST_HOOKS") == "1" and N.load().tic_build_has_test_hooks() == 1
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    env["TIC_TEST_HOOKS"] = "0"
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_damaged_streams_gpu as M; M.shipped_child()" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "shipped library ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
