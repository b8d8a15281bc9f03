"""Damaged per-image-table streams through every decoder route: tests/damaged_adaptive.py builds ONE seeded corpus (every bit of one
table region and stratified samples of seven more, exchanged symbols and codes, value flips that keep every code length, payload flips
at range and workgroup seams, cuts, tails, deleted and inserted bytes, other geometries, qualities and flag words, DC sums that leave
int16 with the chain intact), tests/golden/damaged_adaptive.json holds for every entry the class of the refusal the documented contract
asks for, or the pixels - the unmodified reference's decompress() of the flag-swapped twin where its reader can be asked, its decode() of
the contract's coefficients elsewhere.  The fixture is the expectation on every route; neither the host route nor the oracle is asked.
Every output buffer has 64 sentinel bytes behind it, and a failing call leaves its whole buffer untouched.
tests/test_damaged_adaptive_cpu.py pins the corpus, the contract and the host decoder (under sanitizers) on the same fixture without a GPU.

The device decoder's rule is "anything unusual on the true chain raises a flag and the host decodes": it is wrong without notice when it
finishes a frame the contract refuses, or finishes a still-valid chain with other coefficients than the mutated table gives.  Some 250
entries are of the second kind: the table still parses, every block decodes, to other pixels.

Census of test_single_call_device_route's first run (TIC_DECODE_MIN_BLOCKS=1, TIC_DECODE_MIN_BITS=0); "not eligible": the table is
refused on the host or has a code of length zero; "gave up" by the bits of tic_last_decode_giveup, an entry under every bit it raised:

    kind        entries  not eligible  device finished  gave up: 4  gave up: 8  gave up: 16  gave up: 32
    table_flip      926           591              175           0         160          128            1
    table_swap       24             0                9           0          15           13            0
    value_flip       16             0               16           0           0            0            0
    flip1            22             0               17           0           5            4            0
    flip3             9             0                0           0           9            8            0
    cut              28            15                0           0          13           13            0
    garbage           8             4                4           0           0            0            0
    ones_tail         8             4                0           0           4            4            0
    zeros_tail        8             4                1           0           3            3            0
    delete            8             3                3           0           2            1            0
    insert            8             4                0           0           4            2            0
    geometry         16             0               12           0           4            4            0
    quality           8             0                8           0           0            0            0
    flag              8             6                2           0           0            0            0
    dc_run            3             0                0           0           0            0            3
    all            1100           631              247           0         219          180            4

Every decoded entry (247, 224 of them with other pixels than the base's) was finished by the device decoder; give-up bits 8 (an incident
on the chain), 16 (the chain ends before block N) and 32 (a running DC outside int16) are each some entry's last word; 4 (no fixed point)
is not reached.  DESIGN.md 5.12.1 has the other routes' figures.

Run with `-m gpu` on an MI355X."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_tables as AT
import damaged_adaptive as DA

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = 64            # sentinel bytes behind every output buffer
FILL = 0xAB
RESIDENT_BASES = ("noise256", "twolevel256", "twolevel256q90", "noise64")
SHIPPED_BASES = ("noise256", "twolevel256")
INTACT = ("lenna64", "noise64", "ragged17x33", "incomplete")  # the intact neighbours of a batch, in turn
FX = DA.load_fixture()
REC = DA.records(FX)
GIVEUP_BITS = (4, 8, 16, 32)


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


def tied_corpus(oracle):
    """The entries, tied to the fixture's digests, and the clean base streams."""
    bases = DA.base_streams(oracle, FX)
    for b, s in bases.items():
        assert DA.sha(s) == FX["bases"][b]["sha256"], b
    entries = DA.corpus(oracle, FX, bases)
    assert [e[0] for e in entries] == list(REC)
    flips = []
    for name, base, kind, params, s in entries:
        assert len(s) == REC[name]["bytes"], name
        if REC[name]["sha256"] is None:
            flips.append(DA.sha(s))
        else:
            assert DA.sha(s) == REC[name]["sha256"], name
    assert DA.family_sha(flips) == FX["lenna64_table_flips_sha256"]
    return entries, bases


@pytest.fixture(scope="module")
def corpus(oracle):
    return tied_corpus(oracle)


def expected(name):
    """What the fixture holds: (h, w, digest of the pixels), or "refused" (every class of the contract is TIC_E_STREAM / ValueError)."""
    o = REC[name]["outcome"]
    return "refused" if isinstance(o, str) else o


def clean_outcome(base):
    e = FX["bases"][base]
    return (e["h"], e["w"], e["pixels_sha256"])


def device_eligible(name, s):
    """Whether the device decoder is offered the stream once the size thresholds are out of the way: a table the host parser takes,
    no code of length zero, a block at least."""
    o = REC[name]["outcome"]
    if isinstance(o, str) and o in DA.TABLE_CLASSES:
        return False
    table = DA.read_table(s)[0]
    return AT.blocks_of(*DA.header(s)[:2]) >= 1 and min(len(code) for _, code in table["DC"] + table["AC"]) > 0


def single_call(ctx, s):
    """tic_decompress_adaptive at the C-ABI into h * w + TAIL bytes of FILL -> (outcome as expected() writes it, path, giveup)."""
    L = N.load()
    h, w = DA.header(s)[:2]
    buf = np.frombuffer(s, np.uint8)
    out = np.full(h * w + TAIL, FILL, np.uint8)
    rc = L.tic_decompress_adaptive(ctx.handle, buf.ctypes.data, buf.size, out.ctypes.data, h * w)
    assert (out[h * w:] == FILL).all(), "bytes behind the caller's buffer were written"
    if rc == N.TIC_OK:
        got = (h, w, DA.sha(out[: h * w].tobytes()))
    else:
        assert rc == N.TIC_E_STREAM, (rc, L.tic_last_error(ctx.handle).decode())
        assert (out == FILL).all(), "a failing call wrote into its buffer"
        got = "refused"
    return got, L.tic_last_decode_path(ctx.handle), L.tic_last_decode_giveup(ctx.handle)


def census_table(rows):
    """rows: (kind, eligible, path, giveup) -> the table of DESIGN.md."""
    head = ["kind", "entries", "not eligible", "device finished"] + ["gave up: %d" % b for b in GIVEUP_BITS]
    lines = [head]
    for kind in DA.KINDS + ("all",):
        mine = [r for r in rows if kind in (r[0], "all")]
        lines.append([kind, len(mine), sum(not r[1] for r in mine), sum(r[1] and r[2] == 1 for r in mine)] + [sum(r[1] and r[2] != 1 and bool(r[3] & b) for r in mine) for b in GIVEUP_BITS])
    width = [max(len(str(l[k])) for l in lines) for k in range(len(head))]
    return "\n".join("  ".join(str(c).ljust(width[k]) if k == 0 else str(c).rjust(width[k]) for k, c in enumerate(l)) for l in lines)


def must_finish_on_device(name, kind, params):
    """The chain of block starts is the clean stream's and every block decodes: nothing for the device decoder to flag."""
    return expected(name) != "refused" and (kind == "value_flip" or (kind == "table_swap" and params["keeps_lengths"]))


# ---- tic_decompress_adaptive ------------------------------------------------------------------------------------------------------------
def run_single(ctx, entries, hooks):
    """Every entry through the single call -> rows for the census.  hooks: whether the size thresholds are out of the way (every
    eligible entry is then offered to the device decoder)."""
    rows, wrong = [], []
    for k, (name, base, kind, params, s) in enumerate(entries):
        got, path, giveup = single_call(ctx, s)
        if got != expected(name):
            wrong.append((name, got if got == "refused" else got[:2], REC[name]["outcome"], path, giveup))
        eligible = device_eligible(name, s)
        rows.append((kind, eligible, path, giveup))
        assert not (path == 1 and giveup != 0) and path in (1, 2), (name, path, giveup)
        if hooks:
            assert (path == 2 and giveup == 0) if not eligible else (path == 1 or giveup != 0), (name, eligible, path, giveup)
        if must_finish_on_device(name, kind, params) and (hooks or path == 1 or base in SHIPPED_BASES):
            assert (path, giveup) == (1, 0), ("the device decoder handed over a stream whose chain is the clean one", name, path, giveup)
        if k % 10 == 0:  # ... and the Python call: the same pixels, or ValueError
            if got == "refused":
                with pytest.raises(ValueError):
                    T.decompress_adaptive(s, ctx=ctx)
            else:
                assert DA.px_sha(T.decompress_adaptive(s, ctx=ctx)) == got[2], name
    return rows, wrong


def test_single_call_device_route(ctx, corpus, monkeypatch):
    """Every entry through tic_decompress_adaptive with TIC_DECODE_MIN_BLOCKS=1 and TIC_DECODE_MIN_BITS=0: every stream whose table the
    host parser takes and that has no code of length zero is offered to the device decoder.  Every entry gives the fixture's outcome;
    an entry that ended on path 1 carries no give-up bit, one that was offered and ended on path 2 carries one; the value flips and the
    table swaps that keep every length (where every block still decodes) end on path 1 with nothing flagged - their pixels are the
    device decoder's, looked up in the mutated table.  Give-up bits 8, 16 and 32 are each some entry's last word.  The census is printed."""
    entries, bases = corpus
    assert N.load().tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_MIN_BLOCKS", "1")
    monkeypatch.setenv("TIC_DECODE_MIN_BITS", "0")
    rows, wrong = run_single(ctx, entries, True)
    print("\n%d entries, %d wrong" % (len(entries), len(wrong)))
    print(census_table(rows))
    assert not wrong, (wrong[:10], len(wrong))
    for bit in (8, 16, 32):
        assert any(r[1] and r[2] == 2 and r[3] & bit for r in rows), "no entry's give-up word has bit %d" % bit
    assert sum(must_finish_on_device(n, k, p) for n, b, k, p, s in entries) >= 20
    finished_other = sum(r[2] == 1 and REC[e[0]]["outcome"][2] != FX["bases"][e[1]]["pixels_sha256"] for r, e in zip(rows, entries))
    print("finished by the device decoder with other pixels than the base's: %d" % finished_other)
    assert finished_other >= 150


def test_single_call_host_route(ctx, corpus, monkeypatch):
    """The same with TIC_DECODE_HOST=1: the host's bit-serial decoder alone, path 2 with nothing flagged, the fixture's outcome."""
    entries, bases = corpus
    assert N.load().tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_HOST", "1")
    wrong = []
    for name, base, kind, params, s in entries:
        got, path, giveup = single_call(ctx, s)
        assert (path, giveup) == (2, 0), (name, path, giveup)
        if got != expected(name):
            wrong.append((name, got if got == "refused" else got[:2], REC[name]["outcome"]))
    assert not wrong, (wrong[:10], len(wrong))


# ---- tic_decompress_adaptive_dev ----------------------------------------------------------------------------------------------------------
def test_resident_route(corpus, monkeypatch):
    """Every entry of the 256 x 256 bases and of noise64 through tic_decompress_adaptive_dev, twice: the stream at a 4-byte aligned
    device address (decoded where it lies, read in 32-bit words: the bytes behind `len` up to the next word are 0xFF here and must be
    masked) into a window at an 8-byte aligned address, and at an address off by one (copied first) into a window at an odd one.  The
    window lies in a larger poisoned buffer, rows w + 24 apart: it holds the fixture's pixels and no other byte is written; a failing
    call writes nothing at all."""
    entries, bases = corpus
    sub = [e for e in entries if e[1] in RESIDENT_BASES]
    assert {e[2] for e in sub} == set(DA.KINDS) and {len(e[4]) % 4 for e in sub if e[2] == "cut"} == {0, 1, 2, 3}
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_MIN_BLOCKS", "1")
    monkeypatch.setenv("TIC_DECODE_MIN_BITS", "0")
    ctx2 = T.Context(0)
    y0, margin = 5, 9
    geo = [DA.header(e[4])[:2] for e in sub]
    surface_bytes = max((h + margin) * (w + 24) for h, w in geo)
    stream_bytes = max(len(e[4]) for e in sub) + 16
    d_s, d_o = C.c_void_p(), C.c_void_p()
    ctx2.check(L.tic_dev_alloc(ctx2.handle, stream_bytes, C.byref(d_s)))
    ctx2.check(L.tic_dev_alloc(ctx2.handle, surface_bytes, C.byref(d_o)))
    host = np.empty(surface_bytes, np.uint8)
    paths = {}
    try:
        for (name, base, kind, params, s), (h, w) in zip(sub, geo):
            stride = w + 24
            buf = np.frombuffer(s, np.uint8)
            for off, x0 in ((0, 8), (1, 3)):
                ctx2.check(L.tic_memset_dev(ctx2.handle, d_s, 0xFF, stream_bytes))
                ctx2.check(L.tic_memcpy_h2d(ctx2.handle, C.c_void_p(d_s.value + off), buf.ctypes.data, buf.size))
                ctx2.check(L.tic_memset_dev(ctx2.handle, d_o, FILL, surface_bytes))
                win = C.c_void_p(d_o.value + y0 * stride + x0)
                hh, ww = C.c_int(-1), C.c_int(-1)
                rc = L.tic_decompress_adaptive_dev(ctx2.handle, C.c_void_p(d_s.value + off), buf.size, win, stride, (h - 1) * stride + w, C.byref(hh), C.byref(ww))
                path, giveup = L.tic_last_decode_path(ctx2.handle), L.tic_last_decode_giveup(ctx2.handle)
                ctx2.check(L.tic_memcpy_d2h(ctx2.handle, host.ctypes.data, d_o, host.size))
                want = expected(name)
                what = (name, off, rc, path, giveup)
                if want == "refused":
                    assert rc == N.TIC_E_STREAM and (host == FILL).all(), what
                else:
                    assert rc == N.TIC_OK and (hh.value, ww.value) == (h, w) == want[:2], what
                    rows = host[y0 * stride + x0:][: (h - 1) * stride + w]
                    px = np.stack([rows[r * stride:][:w] for r in range(h)])
                    assert DA.px_sha(px) == want[2], what
                    for r in range(h):
                        rows[r * stride:][:w] = FILL
                    assert (host == FILL).all(), ("bytes outside the window were written",) + what
                    if must_finish_on_device(name, kind, params):
                        assert (path, giveup) == (1, 0), what
                paths[off, path] = paths.get((off, path), 0) + 1
    finally:
        L.tic_dev_free(ctx2.handle, d_s)
        L.tic_dev_free(ctx2.handle, d_o)
        ctx2.close()
    print("\ntic_decompress_adaptive_dev: %d entries; (address offset, path) -> calls: %s" % (len(sub), sorted(paths.items())))
    assert paths.get((0, 1), 0) >= 50 and paths.get((1, 1), 0) >= 50 and paths.get((0, 2), 0) >= 50


# ---- tic_decompress_batch_adaptive ------------------------------------------------------------------------------------------------------
class BatchCall:
    """One tic_decompress_batch_adaptive call at the C-ABI; outs[i] is caps[i] + TAIL bytes of FILL."""

    def __init__(self, ctx, streams):
        L = N.load()
        n = self.n = len(streams)
        self.keep = [np.frombuffer(s, np.uint8) for s in streams]
        self.shapes = [DA.header(s)[:2] for s in streams]
        self.caps = [h * w for h, w in self.shapes]
        self.outs = [np.full(c + TAIL, FILL, np.uint8) for c in self.caps]
        self.hs, self.ws = (C.c_int * n)(*([-7] * n)), (C.c_int * n)(*([-7] * n))
        self.rc = L.tic_decompress_batch_adaptive(ctx.handle, (C.c_void_p * n)(*[b.ctypes.data for b in self.keep]), (C.c_size_t * n)(*[b.size for b in self.keep]), n,
                                                  (C.c_void_p * n)(*[o.ctypes.data for o in self.outs]), (C.c_size_t * n)(*self.caps), self.hs, self.ws)
        self.error = L.tic_last_error(ctx.handle).decode()
        v = [C.c_int(-1) for _ in range(3)]
        assert L.tic_last_decompress_batch_adaptive(ctx.handle, *[C.byref(x) for x in v]) == 0
        self.figures = tuple(x.value for x in v)

    def check(self, jobs, what):
        """jobs: [(name, stream, expected outcome)].  The return code is the first failing frame's; every frame that did not itself fail
        is complete and correct, a failing one's buffer is untouched, hs / ws are filled, no byte behind a capacity is written."""
        bad = [i for i, j in enumerate(jobs) if j[2] == "refused"]
        if bad:
            assert self.rc == N.TIC_E_STREAM and self.error.startswith("frame %d: " % bad[0]), (what, self.rc, self.error, jobs[bad[0]][0])
        else:
            assert self.rc == N.TIC_OK, (what, self.rc, self.error)
        wrong = []
        for i, (name, s, want) in enumerate(jobs):
            assert (self.outs[i][self.caps[i]:] == FILL).all(), ("bytes behind the caller's buffer were written", what, name)
            assert (self.hs[i], self.ws[i]) == self.shapes[i], (what, name, self.hs[i], self.ws[i])
            if want == "refused":
                assert (self.outs[i] == FILL).all(), ("a failing frame's buffer was written", what, name)
            elif (self.shapes[i][0], self.shapes[i][1], DA.sha(self.outs[i][: self.caps[i]].tobytes())) != want:
                wrong.append((i, name))
        assert not wrong, (what, wrong[:10], len(wrong))
        assert self.figures[0] + self.figures[1] == len(jobs), (what, self.figures)


def between_intact(entries, bases, per_call=31):
    """-> calls of at most 64 frames: an intact frame, then every entry with an intact frame behind it."""
    calls, k = [], 0
    for at in range(0, len(entries), per_call):
        jobs = [("clean/" + INTACT[k % 4], bases[INTACT[k % 4]], clean_outcome(INTACT[k % 4]))]
        for name, base, kind, params, s in entries[at:at + per_call]:
            k += 1
            jobs += [(name, s, expected(name)), ("clean/" + INTACT[k % 4], bases[INTACT[k % 4]], clean_outcome(INTACT[k % 4]))]
        assert len(jobs) <= 64
        calls.append(jobs)
    return calls


def run_batches(ctx, entries, bases):
    totals = [0, 0, 0]
    for c, jobs in enumerate(between_intact(entries, bases)):
        call = BatchCall(ctx, [j[1] for j in jobs])
        call.check(jobs, "call %d" % c)
        totals = [a + b for a, b in zip(totals, call.figures)]
    return totals


def test_batch_route(ctx, corpus):
    """Every entry between intact frames through tic_decompress_batch_adaptive at the C-ABI, in calls of at most 64 frames (the batch
    kernels apply no size threshold: every frame with a table that parses and no code of length zero is theirs)."""
    entries, bases = corpus
    totals = run_batches(ctx, entries, bases)
    print("\n%d entries between intact frames: batch_frames %d, single_frames %d, chunks %d" % ((len(entries),) + tuple(totals)))
    assert totals[0] >= len(entries)  # (every intact frame at least, and every entry the kernels finished)


def test_batch_of_many_tables_over_one_payload(ctx, corpus):
    """ONE call of only the table flips and table swaps of lenna64 that still decode: some 140 different tables over the same payload,
    a look-up table per frame, every frame with the fixture's pixels - most of them not the base's."""
    entries, bases = corpus
    jobs = [(n, s, expected(n)) for n, b, k, p, s in entries if b == "lenna64" and k in ("table_flip", "table_swap") and expected(n) != "refused"]
    assert len(jobs) >= 140 and sum(j[2] != clean_outcome("lenna64") for j in jobs) >= 100
    call = BatchCall(ctx, [j[1] for j in jobs])
    print("\n%d frames: batch_frames %d, single_frames %d, chunks %d" % ((len(jobs),) + call.figures))
    call.check(jobs, "tables")
    assert call.figures[0] >= len(jobs) - 8, call.figures  # (a table with a code of length zero is the single call's)


# ---- the library that ships ------------------------------------------------------------------------------------------------------------
def shipped_child():
    """Runs in the fresh process of test_shipped_library: the entries of noise256 and twolevel256 through the single call and the batch
    call of the library without hooks."""
    from oracle import pyoracle
    assert N.load().tic_build_has_test_hooks() == 0 and not [k for k in os.environ if k.startswith("TIC_") and k != "TIC_TEST_HOOKS"]
    entries, bases = tied_corpus(pyoracle)
    entries = [e for e in entries if e[1] in SHIPPED_BASES]
    assert {e[2] for e in entries} == set(DA.KINDS)
    ctx = T.Context(0)
    for b in SHIPPED_BASES:  # the clean streams are the device decoder's in this library
        assert single_call(ctx, bases[b]) == (clean_outcome(b), 1, 0), b
    rows, wrong = run_single(ctx, entries, False)
    assert not wrong, (wrong[:10], len(wrong))
    totals = run_batches(ctx, entries, bases)
    ctx.close()
    print(census_table(rows))
    print("shipped library ok: %d entries, %d finished by the device decoder; batch_frames %d, single_frames %d, chunks %d"
          % ((len(entries), sum(r[2] == 1 for r in rows)) + tuple(totals)))


def test_shipped_library():
    """The entries of noise256 and twolevel256, all kinds, through the single call and the batch call in ONE fresh process that loads the
    library that ships (no hooks compiled in) and sets no TIC_* variable."""
    assert os.environ.get("TIC_TEST_HOOKS") == "1" and N.load().tic_build_has_test_hooks() == 1
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    env["TIC_TEST_HOOKS"] = "0"
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_damaged_adaptive_gpu as M; M.shipped_child()" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "shipped library ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
