"""Batch transcoding on the GPU (include/tinyimgcodec_hip_transcode_batch.h): many streams back to their coefficients, or from one Huffman
table family to the other, in one call - the batch form of the decoder's coefficient sink (tic_entropy_dec_gpu.hip
dec_decode_coef_batch_kernel), the plumbing that keeps a chunk's coefficients on the device between the reader of one family and the
writer of the other (tic_api.hip), and the Python mirror.

Frame i's result is the single call's: every expectation is a fixture made by the unmodified reference or the pinned oracle - the built
coefficients of tests/decoder_streams.py, benchmark_set.json / adaptive_streams.json, the damaged corpora - or the single call itself, which
its own tests pin on those.  Besides the values the tests assert the COUNTERS where they are due: a batch path that goes wrong quietly
hands its frames to the single call - right bytes, and a batch that does not work.  Run with `-m gpu` on an MI355X."""
import ctypes as C
import itertools
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import context_state_common as CS
import damaged_adaptive as DA
import damaged_streams as D
import decoder_streams as DS
import test_decoder_streams_gpu as TD
from test_entropy_decode_gpu import benchmark_jobs, built, ctx, lengths  # noqa: F401 - fixtures (module scope) and the benchmark set's loader

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N
from conftest import GOLDEN, rand_frame

pytestmark = pytest.mark.gpu

FX = TD.FX
NAMES = TD.NAMES
GUARD = 2  # guard blocks of 0x5A5A behind every cap_blocks[i]
TAIL = 64  # sentinel bytes behind every stream buffer


def counters(L, handle):
    v = [C.c_int(-1) for _ in range(3)]
    assert L.tic_last_transcode_batch(handle, *[C.byref(x) for x in v]) == N.TIC_OK
    return tuple(x.value for x in v)


def ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def c_decode_batch(L, handle, streams, nblocks):
    """tic_entropy_decode_batch into buffers of nblocks[i] blocks of 0xA5 with guard blocks of 0x5A5A behind them -> (rc, rcs, [int16 [n, 64]], heads).
    A failing frame must have left its buffer alone, and nobody writes a guard block."""
    n = len(streams)
    bufs = [np.frombuffer(bytes(s), np.uint8) for s in streams]
    outs = []
    for nb in nblocks:
        o = np.full((nb + GUARD) * 64, 0x5A5A, np.uint16)
        o[: nb * 64] = 0xA5A5
        outs.append(o)
    hs, ws, qs, fl = (C.c_int * n)(*[-1] * n), (C.c_int * n)(*[-1] * n), (C.c_int * n)(*[-1] * n), (C.c_uint32 * n)()
    rcs = (C.c_int * n)(*[99] * n)
    rc = L.tic_entropy_decode_batch(handle, ptrs(bufs), (C.c_size_t * n)(*[b.size for b in bufs]), n, ptrs(outs), (C.c_size_t * n)(*nblocks), hs, ws, qs, fl, rcs)
    zz = []
    for i, (o, nb) in enumerate(zip(outs, nblocks)):
        assert (o[nb * 64:] == 0x5A5A).all(), "frame %d: a guard block behind cap_blocks was written" % i
        if rcs[i] != N.TIC_OK:
            assert (o[: nb * 64] == 0xA5A5).all(), "frame %d: a failing frame wrote into its buffer" % i
        zz.append(o[: nb * 64].view(np.int16).reshape(nb, 64))
    return rc, list(rcs), zz, [(hs[i], ws[i], qs[i], fl[i]) for i in range(n)]


def c_retable_batch(L, handle, fn, streams, caps):
    """fn = tic_retable_adaptive_batch / tic_retable_default_batch at the C-ABI -> (rc, rcs, [bytes or None], out_lens); sentinels behind caps[i]."""
    n = len(streams)
    bufs = [np.frombuffer(bytes(s), np.uint8) for s in streams]
    outs = [np.full(c + TAIL, 0xA5, np.uint8) for c in caps]
    olens, rcs = (C.c_size_t * n)(), (C.c_int * n)(*[99] * n)
    rc = fn(handle, ptrs(bufs), (C.c_size_t * n)(*[b.size for b in bufs]), n, ptrs(outs), (C.c_size_t * n)(*caps), olens, rcs)
    res = []
    for i, (o, c) in enumerate(zip(outs, caps)):
        assert (o[c:] == 0xA5).all(), "frame %d: bytes behind the caller's buffer were written" % i
        if rcs[i] != N.TIC_OK:
            assert (o == 0xA5).all(), "frame %d: a failing frame wrote into its buffer" % i
        res.append(o[: olens[i]].tobytes() if rcs[i] == N.TIC_OK else None)
    return rc, list(rcs), res, list(olens)


def first_bad(zz, want):
    bad = np.argwhere(zz != want)
    return "%d coefficients differ, the first in block %d at scan position %d: %d instead of %d" % (len(bad), bad[0][0], bad[0][1], zz[tuple(bad[0])], want[tuple(bad[0])])


# ---- (a) the built frames in ONE call: 2,145 blocks each - eight full workgroups, one of 97 lanes, a last wave of 33 - so every frame's last
# workgroup is partial and the next frame's first row lies directly behind its last one in the chunk's buffer ----------------------------------
@pytest.mark.parametrize("order", ["fixture_order", "reversed"])
def test_built_frames_in_one_call(order, ctx, built):
    L = N.load()
    frames, streams = built
    names = list(NAMES) if order == "fixture_order" else list(reversed(NAMES))
    assert len(names) == 26 and DS.N == 2145
    keys = [TD.plain_key(n) for n in names]
    rc, rcs, zz, heads = c_decode_batch(L, ctx.handle, [streams[n, k] for n, k in zip(names, keys)], [DS.N] * 26)
    twins = [i for i, n in enumerate(names) if DS.is_twin(n)]
    assert len(twins) == 2 and sorted(names[i] for i in twins) == ["dc_bounds_neg_over", "dc_bounds_pos_over"]
    for i, (name, key) in enumerate(zip(names, keys)):
        if i in twins:
            assert rcs[i] == N.TIC_E_RANGE, (name, rcs[i])
            continue
        assert rcs[i] == N.TIC_OK, (name, rcs[i])
        assert heads[i] == (DS.H, DS.W, int(key[1:]), 0), (name, heads[i])
        assert np.array_equal(zz[i], frames[name]["zz"]), "%s (frame %d, between %s and %s): %s" % (
            name, i, names[i - 1] if i else "-", names[i + 1] if i + 1 < 26 else "-", first_bad(zz[i], frames[name]["zz"]))
    for i in twins:  # the neighbours of the frames given up on are complete (checked above) - and are not twins themselves
        for j in (i - 1, i + 1):
            assert 0 <= j < 26 and (j in twins or rcs[j] == N.TIC_OK)
    msg = L.tic_last_error(ctx.handle).decode()
    assert rc == N.TIC_E_RANGE and msg.startswith("frame %d: " % min(twins)) and "running DC" in msg, (rc, msg)
    got = counters(L, ctx.handle)
    print("26 built frames, %s: batch_frames %d, single_frames %d, chunks %d" % (order, *got))
    assert got == (24, 2, 1), got  # what profiles/decoder_streams.txt records for the pixel route


# ---- (b) both windows, from the fixture's lengths alone -------------------------------------------------------------------------------------
def test_both_windows_are_reached(ctx, built):
    """The launcher's rule (stream bits / blocks <= 240 for every frame of the chunk: the 2,048-word window): a chunk of sparse frames only,
    and a chunk that also holds dense_max."""
    L = N.load()
    frames, streams = built
    plain = [n for n in NAMES if not DS.is_twin(n)]
    bits = {n: FX[n]["streams"][TD.plain_key(n)]["bytes"] * 8 // DS.N for n in plain}
    sparse = [n for n in plain if bits[n] <= 240]
    assert len(sparse) >= 10 and "dense_max" in plain and bits["dense_max"] > 240
    for what, names in (("sparse frames only", sparse), ("with dense_max", sparse[:5] + ["dense_max"] + sparse[5:])):
        assert all(bits[n] <= 240 for n in names) == (what == "sparse frames only")
        rc, rcs, zz, _ = c_decode_batch(L, ctx.handle, [streams[n, TD.plain_key(n)] for n in names], [DS.N] * len(names))
        assert rc == N.TIC_OK and set(rcs) == {N.TIC_OK}, (what, rc, rcs, L.tic_last_error(ctx.handle).decode())
        for n, z in zip(names, zz):
            assert np.array_equal(z, frames[n]["zz"]), (what, n, first_bad(z, frames[n]["zz"]))
        got = counters(L, ctx.handle)
        print("%s: %d frames -> batch_frames %d, single_frames %d, chunks %d" % (what, len(names), *got))
        assert got[0] + got[1] == len(names) and got[2] == 1
        # (a chunk runs once: a frame whose own range would be longer than the chunk's may be flagged and take the single call - never dense_max, whose
        #  range is the longest)
        assert got[0] >= len(names) - 1, got


# ---- (c) 1,024 / 1,025 / 1,089 blocks next to each other -------------------------------------------------------------------------------------
EDGE_SHAPES = ((256, 256), (8, 8200), (8, 8712))


@pytest.fixture(scope="module")
def edges(oracle):
    out = []
    for h, w in EDGE_SHAPES:
        img = rand_frame(7000 + w, h, w)
        out.append((oracle.compress(img, 50), oracle.encode_zz16(img, 50), h, w))
    return out


def test_block_count_edges_in_one_chunk(ctx, edges):
    """Every workgroup full / one lane in the last workgroup / a wave with one block, in all six orders: the oracle's coefficients."""
    L = N.load()
    for perm in itertools.permutations(range(3)):
        rc, rcs, zz, heads = c_decode_batch(L, ctx.handle, [edges[k][0] for k in perm], [edges[k][1].shape[0] for k in perm])
        assert rc == N.TIC_OK and rcs == [N.TIC_OK] * 3, (perm, rc, rcs, L.tic_last_error(ctx.handle).decode())
        for i, k in enumerate(perm):
            assert heads[i] == (edges[k][2], edges[k][3], 50, 0), (perm, i, heads[i])
            assert np.array_equal(zz[i], edges[k][1]), (perm, i, first_bad(zz[i], edges[k][1]))
        assert counters(L, ctx.handle) == (3, 0, 1), (perm, counters(L, ctx.handle))
    assert [e[1].shape[0] for e in edges] == [1024, 1025, 1089]


# ---- (d) chunk seams --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seam_jobs(ctx, oracle):
    """Five 256 x 256 frames at five qualities, their coefficients from the oracle, their re-writes from the single calls."""
    jobs = []
    for k, q in enumerate((20, 50, 75, 90, 35)):
        img = rand_frame(8100 + k, 256, 256)
        s = oracle.compress(img, q)
        ra = T.retable_adaptive(s, ctx=ctx)
        assert T.retable_default(ra, ctx=ctx) == bytes(s)
        jobs.append((bytes(s), oracle.encode_zz16(img, q), ra))
    return jobs


def check_seams(L, ctx, jobs, count, want_chunks, what):
    pick = [jobs[i % len(jobs)] for i in range(count)]
    got = T.entropy_decode_zz_batch([p[0] for p in pick], ctx=ctx)
    assert all(np.array_equal(g[0], p[1]) for g, p in zip(got, pick)), what
    assert counters(L, ctx.handle) == (count, 0, want_chunks), (what, "entropy_decode_zz_batch", counters(L, ctx.handle))
    assert T.retable_adaptive_batch([p[0] for p in pick], ctx=ctx) == [p[2] for p in pick], what
    assert counters(L, ctx.handle) == (count, 0, want_chunks), (what, "retable_adaptive_batch", counters(L, ctx.handle))
    assert T.retable_default_batch([p[2] for p in pick], ctx=ctx) == [p[0] for p in pick], what
    assert counters(L, ctx.handle) == (count, 0, want_chunks), (what, "retable_default_batch", counters(L, ctx.handle))


def test_sixty_five_frames_are_two_chunks(ctx, seam_jobs):
    check_seams(N.load(), ctx, seam_jobs, 65, 2, "65 frames")


@pytest.mark.parametrize("chunk", [1, 3])
def test_lowered_chunk_limits(chunk, ctx, seam_jobs, monkeypatch):
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_TBATCH_CHUNK", str(chunk))
    check_seams(L, ctx, seam_jobs, 7, (7 + chunk - 1) // chunk, "chunks of %d" % chunk)


# ---- (e) fallbacks between intact frames ------------------------------------------------------------------------------------------------------
def outcome(fn):
    try:
        return fn()
    except Exception as e:  # noqa: BLE001 - the class is what is compared
        return e


def same(a, b):
    if isinstance(a, Exception) or isinstance(b, Exception):
        return type(a) is type(b)
    if isinstance(a, tuple):
        return np.array_equal(a[0], b[0]) and a[1] == b[1]
    return a == b


def test_fallbacks_between_intact_frames(ctx, built, seam_jobs, oracle):
    L = N.load()
    frames, streams = built
    good = [j[0] for j in seam_jobs]
    small_img = rand_frame(8201, 64, 64)
    odd = {
        "0x16": struct.pack("<IIII", 0, 16, 50, 0),
        "8x8": bytes(oracle.compress(rand_frame(8200, 8, 8), 50)),
        "below the device line": bytes(oracle.compress(small_img, 50)),
        "scaled_dct": bytes(streams["pairs", "s0"]),
        "cut": good[1][: len(good[1]) // 2],
    }
    mixed, where = [], {}
    for k, (what, s) in enumerate(odd.items()):
        mixed += [good[k % len(good)], s]
        where[len(mixed) - 1] = what
    mixed.append(good[0])
    n_good = len(mixed) - len(odd)
    for batch, single in ((T.entropy_decode_zz_batch, T.entropy_decode_zz), (T.retable_adaptive_batch, T.retable_adaptive)):
        want = [outcome(lambda s=s: single(s, ctx=ctx)) for s in mixed]
        got = batch(mixed, ctx=ctx, errors="return")
        b, s_, _ = counters(L, ctx.handle)
        for i, (g, w) in enumerate(zip(got, want)):
            assert same(g, w), (batch.__name__, i, where.get(i, "intact"), type(g), type(w))
            if isinstance(g, Exception):
                assert "frame %d: " % i in str(g), (batch.__name__, i, str(g))
        assert not any(isinstance(w, Exception) for i, w in enumerate(want) if i not in where), batch.__name__
        assert b >= n_good, (batch.__name__, b, s_)  # the intact frames took the batch kernels, whatever lay between them
        failing = [i for i, w in enumerate(want) if isinstance(w, Exception)]
        if failing:
            with pytest.raises(type(want[failing[0]])) as ei:
                batch(mixed, ctx=ctx)
            assert "frame %d: " % failing[0] in str(ei.value), str(ei.value)
        else:
            assert all(same(g, w) for g, w in zip(batch(mixed, ctx=ctx), want))
    # the scaled_dct stream: decoded by the one, refused by the other
    i_scaled = [i for i, w in where.items() if w == "scaled_dct"][0]
    assert np.array_equal(T.entropy_decode_zz_batch(mixed, ctx=ctx, errors="return")[i_scaled][0], frames["pairs"]["zz"])
    assert isinstance(T.retable_adaptive_batch(mixed, ctx=ctx, errors="return")[i_scaled], ValueError)
    # ... and the way back: a header-only stream, an 8 x 8 frame, a small frame, a cut stream between intact adaptive streams
    agood = [j[2] for j in seam_jobs]
    aodd = [struct.pack("<III", 0, 16, 50) + b"\x80\0\0\0", T.compress_adaptive(rand_frame(8200, 8, 8), 50, ctx=ctx), T.compress_adaptive(small_img, 50, ctx=ctx),
            agood[1][: len(agood[1]) // 2]]
    amixed = []
    for k, s in enumerate(aodd):
        amixed += [agood[k % len(agood)], s]
    amixed.append(agood[0])
    want = [outcome(lambda s=s: T.retable_default(s, ctx=ctx)) for s in amixed]
    got = T.retable_default_batch(amixed, ctx=ctx, errors="return")
    assert all(same(g, w) for g, w in zip(got, want)), [(i, type(g), type(w)) for i, (g, w) in enumerate(zip(got, want)) if not same(g, w)]
    assert counters(L, ctx.handle)[0] >= len(amixed) - len(aodd)
    assert isinstance(want[-2], ValueError)  # the cut stream
    failing = [i for i, w in enumerate(want) if isinstance(w, Exception)]
    with pytest.raises(type(want[failing[0]])) as ei:
        T.retable_default_batch(amixed, ctx=ctx)
    assert "frame %d: " % failing[0] in str(ei.value)


def test_retable_cli_also(seam_jobs, tmp_path, capsys):
    """retable_cli IN OUT --also IN OUT ...: several files through one batch call; a file that cannot be rewritten is reported on stderr, the
    others are written, and the exit status is 1."""
    from tinyimgcodec_amd import retable_cli

    paths = []
    for k, data in enumerate([seam_jobs[0][0], seam_jobs[1][0][:9], seam_jobs[2][0]]):  # (the middle one: nine bytes, no header)
        src = tmp_path / ("in%d.img" % k)
        src.write_bytes(data)
        paths.append((str(src), str(tmp_path / ("out%d.img" % k))))
    argv = [paths[0][0], paths[0][1], "--also", paths[1][0], paths[1][1], "--also", paths[2][0], paths[2][1]]
    assert retable_cli.main(argv) == 1
    out, err = capsys.readouterr()
    assert open(paths[0][1], "rb").read() == seam_jobs[0][2] and open(paths[2][1], "rb").read() == seam_jobs[2][2]
    assert not os.path.exists(paths[1][1]) and paths[1][0] in err and "frame 1: " in err and len(err.strip().splitlines()) == 1
    assert out.count(" bytes (") == 2 and paths[0][0] in out and paths[2][0] in out
    # all good, the way back: exit status 0, the inputs' bytes again
    back = [(paths[0][1], str(tmp_path / "back0.img")), (paths[2][1], str(tmp_path / "back2.img"))]
    assert retable_cli.main([back[0][0], back[0][1], "--to", "default", "--also", back[1][0], back[1][1]]) == 0
    assert open(back[0][1], "rb").read() == seam_jobs[0][0] and open(back[1][1], "rb").read() == seam_jobs[2][0]
    capsys.readouterr()


# ---- (f) one frame's caps[i] one byte short, at the C-ABI -------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["adaptive", "default"])
def test_one_buffer_one_byte_short(direction, ctx, seam_jobs):
    L = N.load()
    src = [j[0] if direction == "adaptive" else j[2] for j in seam_jobs]
    want = [j[2] if direction == "adaptive" else j[0] for j in seam_jobs]
    fn = L.tic_retable_adaptive_batch if direction == "adaptive" else L.tic_retable_default_batch
    for short in (0, 2, 4):
        caps = [len(w) + 100 for w in want]
        caps[short] = len(want[short]) - 1
        rc, rcs, res, olens = c_retable_batch(L, ctx.handle, fn, src, caps)
        msg = L.tic_last_error(ctx.handle).decode()
        assert rc == N.TIC_E_SPACE and msg.startswith("frame %d: " % short) and ("%d bytes needed" % len(want[short])) in msg, (rc, msg)
        for i in range(len(src)):
            if i == short:
                assert rcs[i] == N.TIC_E_SPACE and olens[i] == len(want[i]), (direction, short, rcs[i], olens[i])
            else:
                assert rcs[i] == N.TIC_OK and res[i] == want[i], (direction, short, i, rcs[i])
        assert counters(L, ctx.handle) == (len(src), 0, 1), counters(L, ctx.handle)
    # exactly enough is enough
    rc, rcs, res, olens = c_retable_batch(L, ctx.handle, fn, src, [len(w) for w in want])
    assert rc == N.TIC_OK and res == want


# ---- (g) the reference's benchmark set: 49 images x 6 qualities ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bench_streams(ctx):
    pixels, default, adaptive = benchmark_jobs()
    keys = sorted(default)
    streams = {}
    for k in keys:
        s = T.compress(pixels[k[0] - 1], k[1], ctx=ctx)
        assert (len(s), D.sha(s)) == (default[k]["bytes"], default[k]["sha256"]), k
        streams[k] = s
    return keys, streams, default, adaptive


def check_bench(L, ctx, keys, streams, default, adaptive):
    ra = T.retable_adaptive_batch([streams[k] for k in keys], ctx=ctx)
    ca = counters(L, ctx.handle)
    for k, s in zip(keys, ra):
        assert (len(s), D.sha(s)) == (adaptive[k]["bytes"], adaptive[k]["sha256"]), ("retable_adaptive_batch", k)
    rd = T.retable_default_batch(ra, ctx=ctx)
    cd = counters(L, ctx.handle)
    for k, s in zip(keys, rd):
        assert (len(s), D.sha(s)) == (default[k]["bytes"], default[k]["sha256"]), ("retable_default_batch", k)
    return ca, cd


def test_benchmark_set_per_quality(ctx, bench_streams):
    """49 streams of one quality are one chunk: every frame by the batch kernels, both directions."""
    L = N.load()
    keys, streams, default, adaptive = bench_streams
    for q in sorted({k[1] for k in keys}):
        kq = [k for k in keys if k[1] == q]
        assert len(kq) == 49
        ca, cd = check_bench(L, ctx, kq, streams, default, adaptive)
        print("q = %2d: retable_adaptive_batch (batch, single, chunks) = %s, retable_default_batch = %s" % (q, ca, cd))
        assert ca == (49, 0, 1) and cd == (49, 0, 1), (q, ca, cd)


def test_benchmark_set_in_one_call(ctx, bench_streams):
    """All 294 in one call.  Measured on an MI355X: see DESIGN.md 5.13b."""
    L = N.load()
    keys, streams, default, adaptive = bench_streams
    assert len(keys) == 294
    ca, cd = check_bench(L, ctx, keys, streams, default, adaptive)
    print("294 streams: retable_adaptive_batch (batch, single, chunks) = %s, retable_default_batch = %s" % (ca, cd))
    for c in (ca, cd):
        assert c[0] + c[1] == 294 and c[0] >= 280, c  # (the cap keeps the fallback from hiding a dead batch path)


def test_ten_benchmark_streams(ctx, bench_streams):
    """Ten of them without a hook (what the shipped library runs too)."""
    L = N.load()
    keys, streams, default, adaptive = bench_streams
    ca, cd = check_bench(L, ctx, keys[::30][:10], streams, default, adaptive)
    assert ca[0] + ca[1] == 10 and cd[0] + cd[1] == 10 and ca[0] >= 9 and cd[0] >= 9, (ca, cd)


# ---- (h) damaged streams --------------------------------------------------------------------------------------------------------------------------
def test_damaged_default_corpus_through_the_batch(ctx, oracle, seam_jobs, monkeypatch):
    """All 472 entries of damaged_streams.json through retable_adaptive_batch, an intact stream after every third: 470 give the reference's
    reader followed by its writer (retable_damaged.json), the two scaled_dct entries are refused, every intact frame is exact."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_MIN_BLOCKS", "1")
    monkeypatch.setenv("TIC_DECODE_MIN_BITS", "0")
    with open(os.path.join(GOLDEN, "retable_damaged.json")) as f:
        rt = {r["name"]: r for r in json.load(f)["entries"]}
    entries = D.corpus(oracle)
    assert len(entries) == 472 and [e[0] for e in entries] == list(rt)
    batch, tags = [], []
    for i, (name, base, kind, params, s) in enumerate(entries):
        assert D.sha(s) == rt[name]["sha256"], name
        batch.append(bytes(s)), tags.append(name)
        if i % 3 == 2:
            batch.append(seam_jobs[i % 5][0]), tags.append(i % 5)
    got = T.retable_adaptive_batch(batch, ctx=ctx, errors="return")
    b, s_, chunks = counters(L, ctx.handle)
    rewritten = refused = 0
    for tag, g in zip(tags, got):
        if isinstance(tag, int):
            assert g == seam_jobs[tag][2], ("an intact frame between damaged ones", tag)
        elif rt[tag].get("scaled_dct"):
            assert isinstance(g, ValueError), tag
            refused += 1
        else:
            assert not isinstance(g, Exception), (tag, g)
            assert (len(g), D.sha(g)) == (rt[tag]["adaptive"]["bytes"], rt[tag]["adaptive"]["sha256"]), tag
            rewritten += 1
    print("%d frames (472 damaged): batch_frames %d, single_frames %d, chunks %d" % (len(batch), b, s_, chunks))
    intact = sum(isinstance(t, int) for t in tags)
    assert (rewritten, refused) == (470, 2) and b + s_ == len(batch) - refused and b >= intact, (rewritten, refused, b, s_)  # (the intact frames at least)


def test_damaged_adaptive_corpus_through_the_batch(ctx, oracle, seam_jobs, monkeypatch):
    """The 1,100 entries of damaged_adaptive.json through retable_default_batch, an intact stream after every fifth.  Expectations as
    test_damaged_adaptive_corpus derives them for the single reader: ValueError exactly where the fixture's contract refuses; elsewhere the
    re-written stream decodes to the fixture's pixels - or KeyError, where a symbol has no default code, exactly where the single call
    raises it; and every frame is the single call's, byte for byte."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_MIN_BLOCKS", "1")
    monkeypatch.setenv("TIC_DECODE_MIN_BITS", "0")
    fx = DA.load_fixture()
    rec = DA.records(fx)
    entries = DA.corpus(oracle, fx, DA.base_streams(oracle, fx))
    assert [e[0] for e in entries] == list(rec) and len(entries) == 1100
    batch, tags = [], []
    for i, e in enumerate(entries):
        batch.append(bytes(e[4])), tags.append(e[0])
        if i % 5 == 4:
            batch.append(seam_jobs[i % 3][2]), tags.append(i % 3)
    got = T.retable_default_batch(batch, ctx=ctx, errors="return")
    b, s_, chunks = counters(L, ctx.handle)
    wrong, decoded, keyerr = [], 0, 0
    for tag, s, g in zip(tags, batch, got):
        if isinstance(tag, int):
            assert g == seam_jobs[tag][0], ("an intact frame between damaged ones", tag)
            continue
        o = rec[tag]["outcome"]
        w = outcome(lambda: T.retable_default(s, ctx=ctx))
        if not same(g, w):
            wrong.append((tag, "batch", type(g).__name__, "single", type(w).__name__))
        elif isinstance(o, str):
            if not isinstance(g, ValueError):
                wrong.append((tag, "not refused", type(g).__name__))
        elif isinstance(g, KeyError):
            keyerr += 1
        elif isinstance(g, Exception):
            wrong.append((tag, "refused", type(g).__name__))
        else:
            px = T.decompress(g, ctx=ctx)
            decoded += 1
            if [px.shape[0], px.shape[1], DA.px_sha(px)] != list(o):
                wrong.append((tag, "pixels"))
    print("%d frames (1,100 damaged): batch_frames %d, single_frames %d, chunks %d; %d re-written, %d without a default code, %d wrong"
          % (len(batch), b, s_, chunks, decoded, keyerr, len(wrong)))
    assert not wrong, (wrong[:10], len(wrong))
    assert decoded >= 150 and b >= 220  # (the 220 intact frames at least)


# ---- (i) context state -------------------------------------------------------------------------------------------------------------------------
def batch_calls(c, jobs, counts=(12, 2)):
    """A large call followed by a small one, all three entry points: exact."""
    for count in counts:
        pick = [jobs[i % len(jobs)] for i in range(count)]
        got = T.entropy_decode_zz_batch([p[0] for p in pick], ctx=c)
        assert all(np.array_equal(g[0], p[1]) for g, p in zip(got, pick)), count
        assert T.retable_adaptive_batch([p[0] for p in pick], ctx=c) == [p[2] for p in pick], count
        assert T.retable_default_batch([p[2] for p in pick], ctx=c) == [p[0] for p in pick], count
        assert counters(N.load(), c.handle) == (count, 0, 1)


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0xA5], ids=lambda b: "0x%02X" % b)
def test_fresh_context_under_poisoned_allocation(byte, seam_jobs, monkeypatch):
    """TIC_POISON: every buffer the batch calls use comes straight out of a poisoned allocation; then tic_test_poison and the calls again."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_POISON", "0x%02X" % byte)
    c = T.Context(0)
    try:
        batch_calls(c, seam_jobs, counts=(2, 12, 2))
        c.check(L.tic_test_poison(c.handle, byte ^ 0x5A))
        batch_calls(c, seam_jobs)
    finally:
        c.close()


def test_between_single_calls_and_with_a_ticket_open(seam_jobs):
    """A batch call between single transcoding calls, with a decode ticket open on the same context; the single calls' diagnostics are left
    as the last single call set them."""
    L = N.load()
    case = CS.DEV_SMALL[:1]
    c = T.Context(0)
    try:
        for _ in range(2):
            s, zz, ra = seam_jobs[0]
            assert T.retable_adaptive(s, ctx=c) == ra
            tickets = CS.open_decompress_tickets(c, case)
            before = TD.state(L, c.handle)  # (opening a ticket is a decode call of its own)
            batch_calls(c, seam_jobs)
            assert TD.state(L, c.handle) == before, "a batch call changed tic_last_decode_*"
            px = [CS.collect_decompress_ticket(c, t) for t in tickets]
            assert all(np.array_equal(a, b) for a, b in zip(px, CS.exp_pixels(case)))
            assert T.retable_default(ra, ctx=c) == s
            got, _ = T.entropy_decode_zz(s, ctx=c)
            assert np.array_equal(got, zz)
    finally:
        c.close()


# ---- (j) the library that ships -----------------------------------------------------------------------------------------------------------------
def test_on_the_shipped_library():
    """(a), (c) and ten frames of (g) once more in a fresh process on the library that ships (TIC_TEST_HOOKS=0: no hooks compiled in)."""
    assert os.environ.get("TIC_TEST_HOOKS") == "1" and N.load().tic_build_has_test_hooks() == 1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    env["TIC_TEST_HOOKS"] = "0"
    code = ("import sys; sys.path.insert(0, %r); import tinyimgcodec_amd._native as N; assert N.load().tic_build_has_test_hooks() == 0; "
            "import pytest; sys.exit(pytest.main([%r, '-m', 'gpu', '-q', '-x', '-p', 'no:cacheprovider', '-k', "
            "'test_built_frames_in_one_call or test_block_count_edges_in_one_chunk or test_ten_benchmark_streams']))" % (root, os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail
