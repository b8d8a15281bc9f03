"""Mixed batches on the GPU: frames of any sizes and qualities through ONE tic_compress_batch_v call (compress_batch of the Python mirror with shapes
or qualities that differ).  Every stream must be the bytes of oracle.compress (pinned on the reference) and of compress() for that frame, whatever
the order of the frames, the packing kernel, the chunking or the build; the reference's benchmark loop (49 images x 6 qualities) is one call."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

import mixed_batch_common as M

pytestmark = pytest.mark.gpu


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(oracle, ctx):
    """The small set, what the oracle makes of it, and - checked once - that compress() makes the same."""
    frames, qs = M.small_frames()
    want = [oracle.compress(f, q) for f, q in zip(frames, qs)]
    for f, q, s in zip(frames, qs, want):
        assert T.compress(f, q, ctx=ctx) == s, (f.shape, q)
    return frames, qs, want


def orders(n):
    rng = np.random.default_rng(20240607)
    return {"caller": list(range(n)), "reversed": list(range(n))[::-1], "shuffled": [int(i) for i in rng.permutation(n)]}


@pytest.mark.parametrize("chunk", [None, "3"])
@pytest.mark.parametrize("lane", [0, 99])
def test_small_mixed_set(ctx, small, monkeypatch, lane, chunk):
    """Twelve frames from 1 x 1 to 512 x 512 at five qualities in one call, in three orders, with the 8-lane packing kernel (the default) and with the
    lane-per-block kernel allowed up to q = 99 (noise at q = 90 and 99 does not fit its strings: the call lowers the bound and runs again), in one
    chunk and - on this test-hooks build - in chunks of three (four chunks, every slot used; with the lane kernel allowed the chunks of q = 5 .. 50
    keep it).  The bytes depend on none of it, and no frame hides behind the one-by-one fallback."""
    frames, qs, want = small
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    if chunk:
        monkeypatch.setenv("TIC_BATCH_CHUNK", chunk)
    try:
        for name, order in orders(len(frames)).items():
            ctx.check(L.tic_set_entropy_lane_kernel(ctx.handle, lane))
            call = M.VCall(ctx, [frames[i] for i in order], [qs[i] for i in order])
            got = call.streams()
            for k, i in enumerate(order):
                assert got[k] == want[i], (name, lane, chunk, k, i, frames[i].shape, qs[i], len(got[k]), len(want[i]))
            nb, ns, nc, nl = M.figures(ctx)
            assert (nb, ns, nc) == (len(frames), 0, 4 if chunk else 1), (name, nb, ns, nc, nl)
            if not chunk:
                assert nl == len(frames) - M.MERGED_RUNS, nl  # one chunk: the two pairs of equal width and quality are one launch each
        # the Python mirror: a quality per frame
        assert T.compress_batch(frames, qs, ctx=ctx) == want
    finally:
        ctx.check(L.tic_set_entropy_lane_kernel(ctx.handle, 0))


def test_small_mixed_set_on_the_shipped_library(small, tmp_path):
    """The same set through compress_batch() in a fresh process that loads the library that ships (no test hooks, no TIC_* variable)."""
    frames, qs, want = small
    np.savez(tmp_path / "set.npz", **{"f%d" % i: f for i, f in enumerate(frames)}, **{"s%d" % i: np.frombuffer(s, np.uint8) for i, s in enumerate(want)},
             qs=np.array(qs))
    code = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N
assert N.load().tic_build_has_test_hooks() == 0 and N._lib_path() == N.LIB_PATH
z = np.load(sys.argv[1])
qs = [int(q) for q in z["qs"]]
frames = [z["f%d" % i] for i in range(len(qs))]
for order in (list(range(len(qs))), list(range(len(qs)))[::-1]):
    got = T.compress_batch([frames[i] for i in order], [qs[i] for i in order])
    for k, i in enumerate(order):
        assert got[k] == z["s%d" % i].tobytes(), (k, i)
got = T.compress_batch(frames[:5], 50)  # shapes differ, one quality
assert got == [T.compress(f, 50) for f in frames[:5]]
print("mixed batch on the shipped library ok")
'''
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "set.npz")], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "mixed batch on the shipped library ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("lane", [0, 99])
def test_dpcm_restarts_at_every_frame(ctx, oracle, lane):
    """Two one-block frames whose DCs lie far apart (flat 0, flat 255), then noise: a previous DC that leaked from the frame in front - through the
    8-lane kernel's load of the block before the wave's first, or the lane kernel's read 64 coefficients in front of its partition - changes the
    first symbol of the second (or third) stream."""
    frames = [np.zeros((8, 8), np.uint8), np.full((8, 8), 255, np.uint8), np.random.default_rng(77).integers(0, 256, (64, 64), dtype=np.uint8)]
    want = [oracle.compress(f, 50) for f in frames]
    assert want[0] != want[1]
    L = N.load()
    try:
        ctx.check(L.tic_set_entropy_lane_kernel(ctx.handle, lane))
        for order in ([0, 1, 2], [1, 0, 2], [2, 1, 0]):
            call = M.VCall(ctx, [frames[i] for i in order], [50] * 3)
            assert call.streams() == [want[i] for i in order], (lane, order)
            assert M.figures(ctx)[:3] == (3, 0, 1)
            assert [T.compress(frames[i], 50, ctx=ctx) for i in order] == [want[i] for i in order]
    finally:
        ctx.check(L.tic_set_entropy_lane_kernel(ctx.handle, 0))


def test_benchmark_set_in_one_call(ctx):
    """The reference's benchmark loop - 49 images x qualities 90, 80, 50, 20, 10, 5, image outer, quality inner (tests/benchmark.py:12-23 of the
    reference) - as ONE compress call and ONE decompress call: all 294 lengths and sha256 of tests/golden/benchmark_set.json, then its decoded
    pixels.  No frame behind the fallback, and at most chunks + 5 transform launches: six qualities sorted are six runs, a chunk boundary
    splits at most one run each."""
    with open(os.path.join(GOLDEN, "benchmark_set.json")) as f:
        entries = json.load(f)["entries"]
    px = np.load(os.path.join(GOLDEN, "benchmark_set.npz"))["pixels"]
    assert len(entries) == 294 and [(e["image"], e["quality"]) for e in entries[:7]] == [(1, 90), (1, 80), (1, 50), (1, 20), (1, 10), (1, 5), (2, 90)]
    streams = T.compress_batch([px[e["image"] - 1] for e in entries], [e["quality"] for e in entries], ctx=ctx)
    nb, ns, nc, nl = M.figures(ctx)
    print("benchmark set in one call: batch_frames %d single_frames %d chunks %d transform_launches %d" % (nb, ns, nc, nl))
    for e, s in zip(entries, streams):
        assert len(s) == e["bytes"] and sha(s) == e["sha256"], (e["image"], e["quality"])
    assert (nb, ns) == (294, 0) and nl <= nc + 5, (nb, ns, nc, nl)
    images = T.decompress_batch(streams, ctx=ctx)
    for e, im in zip(entries, images):
        assert im.shape == (512, 512) and sha(np.ascontiguousarray(im).tobytes()) == e["decoded_sha256"], (e["image"], e["quality"])


def test_fallback_frames(ctx, oracle, monkeypatch):
    """A frame without blocks (0 x 16: the host's header-only stream) and a 1024 x 1024 frame beyond the chunk's byte budget - lowered to 512 KiB by
    TIC_BATCH_CHUNK_BYTES, with TIC_BATCH_CHUNK=1 - among small frames: the large one is coded alone behind the batch and counts as a single frame,
    every other frame with blocks counts as a batch frame, and all bytes are right."""
    rng = np.random.default_rng(99)
    frames = [rng.integers(0, 256, (16, 24), dtype=np.uint8), np.zeros((0, 16), np.uint8), rng.integers(0, 256, (1024, 1024), dtype=np.uint8),
              rng.integers(0, 256, (33, 8), dtype=np.uint8), np.full((64, 64), 128, np.uint8)]
    qs = [50, 10, 50, 90, 5]
    want = [oracle.compress(f, q) for f, q in zip(frames, qs)]
    assert len(want[1]) == 16
    monkeypatch.setenv("TIC_BATCH_CHUNK", "1")
    monkeypatch.setenv("TIC_BATCH_CHUNK_BYTES", str(512 << 10))
    call = M.VCall(ctx, frames, qs)
    assert call.streams() == want
    assert M.figures(ctx) == (3, 1, 3, 3)
    assert T.compress_batch(frames, qs, ctx=ctx) == want
    monkeypatch.delenv("TIC_BATCH_CHUNK_BYTES")
    call = M.VCall(ctx, frames, qs)  # within the budget the large frame is a batch frame
    assert call.streams() == want and M.figures(ctx) == (4, 0, 4, 4)


def test_errors(ctx, small):
    """Argument checks run before any work and name the first offending frame: nothing is written to any output buffer.  A stream that does not
    fit its buffer and a coefficient without a Huffman code fail the call once the device has found them."""
    frames, qs, want = small
    # a bad quality in the middle of the list (and a worse frame behind it: the FIRST one is reported)
    bad = list(qs)
    bad[5], bad[8] = 100, 0
    call = M.VCall(ctx, frames, bad)
    assert call.rc == N.TIC_E_QUALITY and call.error.startswith("frame 5: ") and "100" in call.error and call.untouched(), (call.rc, call.error)
    # a null frame: sizes given, pixels missing
    L = N.load()
    call = M.VCall(ctx, frames, qs, null_images=(6, 9))
    assert call.rc == N.TIC_E_ARG and call.error.startswith("frame 6: ") and call.untouched(), (call.rc, call.error)
    # null arrays, a negative count, a negative size, a stride below the width
    for name in ("images", "hs", "ws", "strides", "quals", "outs", "caps", "lens"):
        call = M.VCall(ctx, frames, qs, null_arrays=(name,))
        assert call.rc == N.TIC_E_ARG and call.untouched(), (name, call.rc, call.error)
    call = M.VCall(ctx, frames, qs, n=-1)
    assert call.rc == N.TIC_E_ARG and call.untouched(), (call.rc, call.error)
    assert L.tic_compress_batch_v(ctx.handle, None, 0, None, None, None, None, None, None, None) == N.TIC_OK
    call = M.VCall(ctx, frames, qs, strides=[f.shape[1] - (1 if i == 9 else 0) for i, f in enumerate(frames)])
    assert call.rc == N.TIC_E_ARG and call.error.startswith("frame 9: ") and call.untouched(), (call.rc, call.error)
    # caps[i] one byte short: TIC_E_SPACE naming frame i
    for i in (7, 0):
        caps_l = [L.tic_compress_bound(*f.shape) for f in frames]
        caps_l[i] = len(want[i]) - 1
        call = M.VCall(ctx, frames, qs, caps=caps_l)
        assert call.rc == N.TIC_E_SPACE and "frame %d " % i in call.error, (i, call.rc, call.error)
    # a flat 255 frame at q = 99 has a DC without a Huffman code: a late frame fails the call (KeyError in the reference and in the mirror)
    late = frames + [np.full((8, 8), 255, np.uint8)]
    call = M.VCall(ctx, late, qs + [99])
    assert call.rc == N.TIC_E_RANGE, (call.rc, call.error)
    with pytest.raises(KeyError):
        T.compress_batch(late, qs + [99], ctx=ctx)
    with pytest.raises(KeyError):
        T.compress(late[-1], 99, ctx=ctx)
    # the mirror's own checks
    with pytest.raises(ValueError):
        T.compress_batch(frames, qs[:-1], ctx=ctx)
    with pytest.raises(ValueError, match="not supported"):
        T.compress_batch(frames, qs, threads=2, ctx=ctx)
    with pytest.raises(ValueError, match="not supported"):
        T.compress_batch(frames, 50, devices=[0])
    # and the context still works
    assert T.compress_batch(frames, qs, ctx=ctx) == want


def test_uniform_call_untouched(ctx):
    """compress_batch of 21 equal 40 x 52 frames at one quality is the call it was: the bytes and the tic_last_batch_input_path /
    tic_last_batch_zero_copy figures recorded on the parent commit (tests/golden/uniform_batch.json, tests/golden/gen/make_goldens_uniform_batch.py) -
    also right after a mixed call has used the context's slots."""
    with open(os.path.join(GOLDEN, "uniform_batch.json")) as f:
        gold = json.load(f)
    L = N.load()
    frames = [np.random.default_rng(gold["seed"] + i).integers(0, 256, (gold["h"], gold["w"]), dtype=np.uint8) for i in range(gold["n"])]
    assert (gold["n"], gold["h"], gold["w"]) == (21, 40, 52)
    for round_ in range(2):
        got = T.compress_batch(frames, gold["quality"], ctx=ctx)
        d, s, z = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        ctx.check(L.tic_last_batch_input_path(ctx.handle, C.byref(d), C.byref(s)))
        ctx.check(L.tic_last_batch_zero_copy(ctx.handle, C.byref(z)))
        assert [sha(b) for b in got] == gold["sha256"], round_
        assert (d.value, s.value, z.value) == (gold["direct_frames"], gold["staged_frames"], gold["zero_copy"]), (round_, d.value, s.value, z.value)
        T.compress_batch(frames[:3] + [frames[0][:8, :8]], [5, 50, 90, 10], ctx=ctx)  # a mixed call in between


def test_encode_cli_writes_several_files_in_one_call(small, tmp_path, capsys):
    """encode_cli INPUT OUTPUT --also INPUT OUTPUT ...: images of different sizes, one compress_batch() call, a file and two lines each."""
    from tinyimgcodec_amd import encode_cli

    frames, qs, want = small
    pick = [3, 5, 8]
    argv = []
    for k, i in enumerate(pick):
        np.save(tmp_path / ("in%d.npy" % k), frames[i])
        argv += ([] if k == 0 else ["--also"]) + [str(tmp_path / ("in%d.npy" % k)), str(tmp_path / ("out%d.img" % k))]
    assert encode_cli.main(argv + ["--quality", "10"]) == 0
    lines = capsys.readouterr().out.splitlines()
    for k, i in enumerate(pick):
        got = (tmp_path / ("out%d.img" % k)).read_bytes()
        assert got == T.compress(frames[i], 10) and lines[2 * k] == "%d bytes" % len(got), (k, i)
    assert (tmp_path / "out0.img").read_bytes() == want[3] and (tmp_path / "out2.img").read_bytes() == want[8]  # (their quality in the set is 10)
