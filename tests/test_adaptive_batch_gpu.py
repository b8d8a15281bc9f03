"""The adaptive batch encoder on the GPU: frames of any sizes and qualities through ONE tic_compress_batch_adaptive_v call (compress_batch_adaptive
of the Python mirror).  Every stream must be the bytes of the unmodified reference's compress(..., auto_generate_huffman_table=True)
(tests/golden/adaptive_batch.json, adaptive_streams.json) and of compress_adaptive() for that frame, whatever the order of the frames, their
neighbours in a chunk, the chunking or the build."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

import adaptive_batch_common as A
from test_adaptive_gpu import longcode_coeffs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def fxset(ctx):
    """The fixture's frames, the reference's streams, and - checked once - that compress_adaptive() writes the same."""
    entries, frames, qs = A.load_fixture()
    want = []
    for e, f, q in zip(entries, frames, qs):
        s = T.compress_adaptive(f, q, ctx=ctx)
        A.check_stream(s, e)
        want.append(s)
    assert len(want) == 11 and len(want[8]) == 23  # (the flat 32 x 32 frame: one-symbol tables, no payload)
    return entries, frames, qs, want


def caps_of(frames):
    L = N.load()
    return [L.tic_compress_bound(f.shape[0], f.shape[1]) + 4096 for f in frames]


def streams_of(call):
    assert call.rc == 0, (call.rc, call.error)
    out = []
    for i in range(call.n):
        n = call.lens[i]
        assert (call.outs[i][n:] == 0xAB).all(), i  # nothing behind a stream's end
        out.append(call.outs[i][:n].tobytes())
    return out


def orders(n):
    rng = np.random.default_rng(20261019)
    return {"caller": list(range(n)), "reversed": list(range(n))[::-1], "shuffled": [int(i) for i in rng.permutation(n)]}


@pytest.mark.parametrize("chunk", [None, "3"])
def test_fixture_set_in_one_call(ctx, fxset, monkeypatch, chunk):
    """Eleven frames from one block to 513 (255, 256 and 257 blocks among them: one workgroup, one full, two), flat frames without payload and DC
    categories 12-13, in three orders, in one chunk and - on this test-hooks build - in chunks of three (four chunks: every slot is used again).
    Every call is made twice on the one context: counts left in a slot by its previous chunk would show in the second."""
    entries, frames, qs, want = fxset
    assert N.load().tic_build_has_test_hooks() == 1
    if chunk:
        monkeypatch.setenv("TIC_BATCH_CHUNK", chunk)
    for name, order in orders(len(frames)).items():
        for rep in range(2):
            call = A.ACall(ctx, [frames[i] for i in order], [qs[i] for i in order], caps_of([frames[i] for i in order]))
            got = streams_of(call)
            for k, i in enumerate(order):
                A.check_stream(got[k], entries[i])
                assert got[k] == want[i], (name, rep, chunk, k, i)
            assert A.figures(ctx) == (len(frames), 0, 4 if chunk else 1), (name, A.figures(ctx))
    assert T.compress_batch_adaptive(frames, qs, ctx=ctx) == want  # the Python mirror: a quality per frame
    assert T.compress_batch_adaptive(frames[:4], 50, ctx=ctx) == [T.compress_adaptive(f, 50, ctx=ctx) for f in frames[:4]]  # ... and one for all


def test_fixture_set_on_the_shipped_library(fxset, tmp_path):
    """The same set through compress_batch_adaptive() in a fresh process that loads the library that ships (no test hooks, no TIC_* variable)."""
    entries, frames, qs, want = fxset
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
    got = T.compress_batch_adaptive([frames[i] for i in order], [qs[i] for i in order])
    for k, i in enumerate(order):
        assert got[k] == z["s%d" % i].tobytes(), (k, i)
print("adaptive batch on the shipped library ok")
'''
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "set.npz")], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "adaptive batch on the shipped library ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_dpcm_and_keys_restart_at_every_frame(ctx):
    """Two one-block frames whose DCs lie far apart (flat 0, flat 255), then noise, in three orders: a previous DC that leaked from the frame in
    front changes the first symbol of the stream behind.  And one noise frame at the first, a middle and the last position of a chunk of equal
    shapes and qualities (the plan keeps the caller's order among equals): first-occurrence keys counted from the chunk's first block, not the
    frame's, would order equal frequencies differently and change the table."""
    frames = [np.zeros((8, 8), np.uint8), np.full((8, 8), 255, np.uint8), np.random.default_rng(77).integers(0, 256, (64, 64), dtype=np.uint8)]
    want = [T.compress_adaptive(f, 50, ctx=ctx) for f in frames]
    assert want[0] != want[1]
    for order in ([0, 1, 2], [1, 0, 2], [2, 1, 0]):
        assert T.compress_batch_adaptive([frames[i] for i in order], 50, ctx=ctx) == [want[i] for i in order], order
        assert A.figures(ctx) == (3, 0, 1)
    noise = frames[2]
    others = [np.random.default_rng(900 + k).integers(0, 256, (64, 64), dtype=np.uint8) for k in range(2)]
    got = T.compress_batch_adaptive([noise, others[0], noise, others[1], noise], 50, ctx=ctx)
    assert got[0] == got[2] == got[4] == want[2]
    assert got[1] == T.compress_adaptive(others[0], 50, ctx=ctx) and got[3] == T.compress_adaptive(others[1], 50, ctx=ctx)


def test_zero_payload_frame_between_two_noise_frames(ctx, fxset):
    """A flat frame's stream is header and two one-symbol tables: 23 bytes, no payload bit, an area of two 16-byte pieces.  Its neighbours' bytes
    do not change, and it is the fixture's."""
    entries, frames, qs, want = fxset
    a, b = (np.random.default_rng(s).integers(0, 256, (32, 32), dtype=np.uint8) for s in (31, 32))
    got = T.compress_batch_adaptive([a, frames[8], b], 50, ctx=ctx)
    assert got[1] == want[8] and len(got[1]) == 23
    assert got[0] == T.compress_adaptive(a, 50, ctx=ctx) and got[2] == T.compress_adaptive(b, 50, ctx=ctx)
    assert A.figures(ctx) == (3, 0, 1)


def test_coefficient_entry(ctx):
    """Built coefficients reach the kernels through tic_entropy_encode_adaptive_batch: the `longcode` frame of adaptive_streams.json (codes of 29
    bits, 44 with their value bits) between two small frames matches its fixture, the small frames theirs; a DC of -32768 (category 16) is an
    OverflowError that names its frame."""
    with open(os.path.join(GOLDEN, "adaptive_batch.json")) as f:
        ref = json.load(f)["longcode"]
    with open(os.path.join(GOLDEN, ref["file"])) as f:
        e = json.load(f)[ref["key"]]
    zz = longcode_coeffs()
    assert A.sha(np.ascontiguousarray(zz.astype("<i2")).tobytes()) == e["coeffs_sha256"]
    a, b = (np.random.default_rng(s).integers(0, 256, (24, 40), dtype=np.uint8) for s in (41, 42))
    za, zb = T.dctq(a, 50, ctx=ctx), T.dctq(b, 90, ctx=ctx)
    got = T.entropy_encode_adaptive_batch([za, zz, zb], [(24, 40), (e["height"], e["width"]), (24, 40)], [50, e["quality"], 90], ctx=ctx)
    assert A.figures(ctx) == (3, 0, 1)
    assert len(got[1]) == e["bytes"] and got[1][:64].hex() == e["head"] and A.sha(got[1]) == e["sha256"]
    assert got[0] == T.compress_adaptive(a, 50, ctx=ctx) and got[2] == T.compress_adaptive(b, 90, ctx=ctx)
    bad = np.zeros((1, 64), np.int16)
    bad[0, 0] = -32768
    with pytest.raises(OverflowError, match="frame 1:"):
        T.entropy_encode_adaptive_batch([za, bad, zb], [(24, 40), (8, 8), (24, 40)], [50, 50, 90], ctx=ctx)
    assert T.entropy_encode_adaptive_batch([za, zb], [(24, 40), (24, 40)], [50, 90], ctx=ctx) == [got[0], got[2]]  # (the context works on)


def test_capacity(ctx):
    """At the C level, into buffers filled with 0xAB: one frame of three gets a byte less than its stream needs.  The call ends in TIC_E_SPACE, that
    frame's buffer is untouched and its out_lens entry is the need; the other two are complete; nothing is written behind any stream's end."""
    frames = [np.random.default_rng(50 + k).integers(0, 256, s, dtype=np.uint8) for k, s in enumerate(((40, 56), (16, 72), (64, 64)))]
    qs = [75, 50, 20]
    want = [T.compress_adaptive(f, q, ctx=ctx) for f, q in zip(frames, qs)]
    for short in range(3):
        caps = [len(w) + 100 for w in want]
        caps[short] = len(want[short]) - 1
        call = A.ACall(ctx, frames, qs, caps)
        assert call.rc == N.TIC_E_SPACE, (call.rc, call.error)
        for i in range(3):
            assert call.lens[i] == len(want[i])
            if i == short:
                assert call.lens[i] > caps[i] and (call.outs[i] == 0xAB).all()
            else:
                assert call.outs[i][: len(want[i])].tobytes() == want[i] and (call.outs[i][len(want[i]):] == 0xAB).all()
    # exact capacities are enough, and the Python mirror's second call fetches what its first guess left out
    call = A.ACall(ctx, frames, qs, [len(w) for w in want])
    assert streams_of(call) == want


def test_benchmark_set_in_one_call(ctx, monkeypatch):
    """The reference's benchmark loop with its own tables - 49 images x qualities 90, 80, 50, 20, 10, 5 - as ONE call: all 294 lengths and sha256 of
    the `benchmark` entries of adaptive_streams.json, no frame behind the one-by-one route; the same in several chunks (a byte budget of 4 MB:
    sixteen 512 x 512 frames a chunk); six of the streams decode to the pixels of benchmark_set.json."""
    with open(os.path.join(GOLDEN, "adaptive_streams.json")) as f:
        entries = json.load(f)["benchmark"]
    with open(os.path.join(GOLDEN, "benchmark_set.json")) as f:
        decoded = {(e["image"], e["quality"]): e["decoded_sha256"] for e in json.load(f)["entries"]}
    px = np.load(os.path.join(GOLDEN, "benchmark_set.npz"))["pixels"]
    assert len(entries) == 294
    images, qs = [px[e["image"] - 1] for e in entries], [e["quality"] for e in entries]
    streams = T.compress_batch_adaptive(images, qs, ctx=ctx)
    nb, ns, nc = A.figures(ctx)
    print("benchmark set, adaptive, in one call: batch_frames %d single_frames %d chunks %d" % (nb, ns, nc))
    assert (nb, ns) == (294, 0) and nc == 5, (nb, ns, nc)  # 294 frames in chunks of 64
    for e, s in zip(entries, streams):
        assert len(s) == e["bytes"] and A.sha(s) == e["sha256"], (e["image"], e["quality"])
    monkeypatch.setenv("TIC_BATCH_CHUNK_BYTES", str(4 << 20))
    again = T.compress_batch_adaptive(images, qs, ctx=ctx)
    nb, ns, nc = A.figures(ctx)
    assert (nb, ns) == (294, 0) and nc == 19 and again == streams, (nb, ns, nc)
    for k in (0, 5, 100, 151, 200, 293):
        e = entries[k]
        im = T.decompress_adaptive(streams[k], ctx=ctx)
        assert A.sha(np.ascontiguousarray(im).tobytes()) == decoded[(e["image"], e["quality"])], (e["image"], e["quality"])


def test_frames_larger_than_a_chunk_are_coded_behind_the_batch(ctx, fxset, monkeypatch):
    """With a byte budget of 4,096 staged pixels per chunk the four wide frames of the fixture (8 x 2040 ... 7 x 4100) do not fit a chunk: they go
    through tic_compress_adaptive behind the batch, the other seven through the chunks; the bytes are the same.  A wide frame with a short buffer
    is reported like a frame of a chunk: TIC_E_SPACE at the end, its buffer untouched, everything else written."""
    entries, frames, qs, want = fxset
    monkeypatch.setenv("TIC_BATCH_CHUNK_BYTES", "4096")
    call = A.ACall(ctx, frames, qs, caps_of(frames))
    assert streams_of(call) == want
    nb, ns, nc = A.figures(ctx)
    assert (nb, ns) == (7, 4) and nc >= 2, (nb, ns, nc)
    caps = caps_of(frames)
    caps[4] = len(want[4]) - 1  # 8 x 2040: coded alone
    call = A.ACall(ctx, frames, qs, caps)
    assert call.rc == N.TIC_E_SPACE, (call.rc, call.error)
    for i in range(len(frames)):
        assert call.lens[i] == len(want[i])
        if i == 4:
            assert (call.outs[i] == 0xAB).all()
        else:
            assert call.outs[i][: len(want[i])].tobytes() == want[i] and (call.outs[i][len(want[i]):] == 0xAB).all()
    assert T.compress_batch_adaptive(frames, qs, ctx=ctx) == want
