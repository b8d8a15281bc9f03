"""The adaptive batch decoder on the GPU: streams with per-image Huffman tables, of any sizes and qualities, through ONE tic_decompress_batch_adaptive
call (decompress_batch_adaptive of the Python mirror).  Every frame must be the fixtures' pixels (the reference's decode(encode()),
tests/golden/adaptive_batch.json, adaptive_streams.json, benchmark_set.json) and what decompress_adaptive() gives for that stream alone, whatever
its neighbours in a chunk, the chunking, the download route or the build.  Every test checks its streams against the fixtures' sha256 before it
decodes them: a wrong input cannot pass as a right output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

import adaptive_decode_batch_common as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return D.adaptive_streams_fixture()


@pytest.fixture(scope="module")
def fxset(ctx, fx):
    """-> (names, streams, decoded digests): the 11 frames of adaptive_batch.json and every case of adaptive_streams.json except frame_1080p,
    compressed by ONE compress_batch_adaptive and checked against the fixtures' stream digests."""
    entries, frames, qs = D.load_fixture()
    cases = [c for c in fx["cases"] if c["name"] != "frame_1080p"]
    entries = list(entries) + cases
    frames = list(frames) + [D.case_image(c["name"], c["height"], c["width"]) for c in cases]
    qs = list(qs) + [c["quality"] for c in cases]
    assert len(entries) == 11 + 29
    streams = T.compress_batch_adaptive(frames, qs, ctx=ctx)
    for s, e in zip(streams, entries):
        assert len(s) == e["bytes"] and D.sha(s) == e["sha256"], e
    names = ["%s %dx%d q%d" % (e.get("name", e.get("kind")), e["height"], e["width"], e["quality"]) for e in entries]
    return names, streams, [e["decoded_sha256"] for e in entries]


def noise_64x96(fx, ctx, q):
    e = next(c for c in fx["cases"] if c["name"] == "noise" and c["quality"] == q)
    s = T.compress_adaptive(D.case_image("noise", 64, 96), q, ctx=ctx)
    assert len(s) == e["bytes"] and D.sha(s) == e["sha256"]
    return s, e["decoded_sha256"]


def frame_1080p(fx, ctx):
    e = next(c for c in fx["cases"] if c["name"] == "frame_1080p")
    s = T.compress_adaptive(D.case_image(e["name"], e["height"], e["width"]), e["quality"], ctx=ctx)
    assert len(s) == e["bytes"] == 865763 and D.sha(s) == e["sha256"]
    return s, e["decoded_sha256"]


def check_fixture_set(ctx, fxset, chunks):
    names, streams, want = fxset
    taken = sum(D.batch_takes(s) for s in streams)
    assert 2 <= taken < len(streams)  # both kinds are in the set: the flat and one-block frames are the single call's
    for rep in range(2):  # (twice on the one context: what a chunk leaves in the buffers must not show in the next call)
        got = T.decompress_batch_adaptive(streams, ctx=ctx)
        assert len(got) == len(streams)
        for name, px, w in zip(names, got, want):
            assert D.px_sha(px) == w, (name, rep)
        print("figures:", D.figures(ctx), "taken:", taken)
        assert D.figures(ctx) == (taken, len(streams) - taken, chunks(taken)), D.figures(ctx)


def test_fixture_set_in_one_call(ctx, fxset):
    """Forty frames from one block to 513 - flat frames, one-block frames, checkerboards at q = 97..99, sides that are no multiples of 8 - in ONE
    decompress_batch_adaptive: every frame's pixels are the fixture's; the frames whose table has at least two DC and two AC entries (read from
    the stream) are decoded by the batch kernels, the rest - a code of length zero - by the single call."""
    check_fixture_set(ctx, fxset, lambda taken: 1)


def test_benchmark_set_in_one_call(ctx, fx):
    """The 294 streams of the benchmark loop (49 images of 512 x 512 at six qualities; the single call sends the smaller ones to the host's
    decoder): one call, one chunk, every frame by the batch kernels, every frame's pixels the fixture's."""
    pixels = np.load(os.path.join(GOLDEN, "benchmark_set.npz"))["pixels"]
    with open(os.path.join(GOLDEN, "benchmark_set.json")) as f:
        decoded = {(e["image"], e["quality"]): e["decoded_sha256"] for e in json.load(f)["entries"]}
    bench = fx["benchmark"]
    assert len(bench) == 294
    streams = T.compress_batch_adaptive([pixels[e["image"] - 1] for e in bench], [e["quality"] for e in bench], ctx=ctx)
    for s, e in zip(streams, bench):
        assert len(s) == e["bytes"] and D.sha(s) == e["sha256"], e
    got = T.decompress_batch_adaptive(streams, ctx=ctx)
    for px, e in zip(got, bench):
        assert D.px_sha(px) == decoded[(e["image"], e["quality"])], e
    print("figures:", D.figures(ctx), "direct:", D.direct_frames(ctx))
    assert D.figures(ctx) == (294, 0, 1)


def test_fixture_set_in_several_chunks(ctx, fxset, monkeypatch):
    """The same forty frames in chunks of three taken frames (the hooks build's TIC_ADBATCH_CHUNK): same pixels, and as many chunks as the plan
    cuts for that limit - no byte limit is near, so ceil(taken / 3)."""
    assert N.load().tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_ADBATCH_CHUNK", "3")
    check_fixture_set(ctx, fxset, lambda taken: -(-taken // 3))


def test_workgroup_boundaries(ctx, fx):
    """Noise frames of height 8 at q = 50 whose streams have 255, 256, 257 and 513 ranges (one workgroup not full, full, two, three: found through
    tic_adaptive_decode_geometry) between an 8 x 8 frame and the 1080p fixture frame of 32,400 blocks, in two orders: every frame is what
    decompress_adaptive() gives for its stream alone, the 1080p frame the fixture's pixels.  The boundary frames and the 1080p frame are decoded by
    the batch kernels; the 8 x 8 frame is one block - a one-entry DC table, a code of length zero - and so the single call's by the take rule."""
    found = {}
    for target in (255, 256, 257, 513):
        for nblocks in range(2 * target - 12, 2 * target + 3):
            for seed in range(4):
                s = T.compress_adaptive(D.rand_frame(9000 + seed, 8, 8 * nblocks), 50, ctx=ctx)
                if D.geometry(s, nblocks)[1] == target:
                    found[target] = s
                    break
            if target in found:
                break
    assert sorted(found) == [255, 256, 257, 513], sorted(found)
    big, big_sha = frame_1080p(fx, ctx)
    tiny = T.compress_adaptive(D.rand_frame(5, 8, 8), 50, ctx=ctx)
    assert not D.batch_takes(tiny) and all(D.batch_takes(s) for s in found.values()) and D.batch_takes(big)
    batch = [tiny] + [found[t] for t in (255, 256, 257, 513)] + [big]
    alone = [D.px_sha(T.decompress_adaptive(s, ctx=ctx)) for s in batch]
    assert alone[-1] == big_sha
    for order in (list(range(6)), [5, 3, 1, 0, 4, 2]):
        got = T.decompress_batch_adaptive([batch[i] for i in order], ctx=ctx)
        for k, i in enumerate(order):
            assert D.px_sha(got[k]) == alone[i], (order, k, i)
        print("figures:", D.figures(ctx))
        assert D.figures(ctx) == (5, 1, 1)


def test_one_frames_give_up_leaves_its_neighbours_alone(ctx, fx):
    """The long-code stream (146,579 blocks; its chain advances a workgroup per launch) between two 64 x 96 noise streams: its pixels are decode()
    of its coefficients, the neighbours' the fixtures'.  A model of the stitch (tests/adaptive_tables.py stitch_model, its list for this stream in
    tests/golden/adaptive_tables.json) settles it in round 280, far behind the batch's nineteen: it is the single call's frame, with its 512
    rounds, and its neighbours are the batch kernels'."""
    e = fx["longcode"]
    zz = D.longcode_coeffs()
    assert zz.shape[0] == 146579 and D.sha(np.ascontiguousarray(zz.astype("<i2")).tobytes()) == e["coeffs_sha256"]
    s = T.entropy_encode_adaptive(zz, e["height"], e["width"], e["quality"], ctx=ctx)
    assert len(s) == e["bytes"] and D.sha(s) == e["sha256"]
    a, a_sha = noise_64x96(fx, ctx, 50)
    b, b_sha = noise_64x96(fx, ctx, 90)
    got = T.decompress_batch_adaptive([a, s, b], ctx=ctx)
    figs = D.figures(ctx)
    print("figures (batch, single, chunks):", figs, "- the long-code frame went the", "batch's" if figs[0] == 3 else "single call's", "way")
    assert D.px_sha(got[0]) == a_sha and D.px_sha(got[2]) == b_sha
    dc = zz[:, 0].astype(np.int32)
    dc[1:] = np.diff(dc)
    want = T.decode({"height": e["height"], "width": e["width"], "quality": e["quality"], "scaled_dct": False, "dc": dc,
                     "ac": zz[:, 1:].astype(np.int32)}, ctx=ctx)
    assert np.array_equal(got[1], want)
    assert figs == (2, 1, 1)


def damaged(s):
    """(label, stream) of the damage list of tests/test_adaptive_decode_gpu.py: cuts, a bit flipped in the table, bits flipped in the payload,
    garbage behind the end."""
    out = [("cut %d" % c, s[:c]) for c in np.linspace(16, len(s) - 1, 10).astype(int)]
    assert D.batch_takes(s)
    b = bytearray(s)
    b[40] ^= 0x10  # (the table of a noise frame is some hundred bytes long)
    out.append(("table bit", bytes(b)))
    rng = np.random.default_rng(2024)
    for _ in range(20):
        pos = int(rng.integers(len(s) * 8 // 4, len(s) * 8 * 3 // 4))
        b = bytearray(s)
        b[pos >> 3] ^= 0x80 >> (pos & 7)
        out.append(("payload bit %d" % pos, bytes(b)))
    out.append(("garbage", s + rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()))
    return out


def test_damage_inside_a_batch(ctx, fx):
    """The damage list on the 64 x 96 noise stream at q = 90, every damaged stream between intact ones, at the C-ABI with outputs of caps[i] + 64
    sentinel bytes: every frame ends as tic_decompress_adaptive alone ends on that stream (the same pixels, or a failure), the return code is the
    first failing frame's, every intact frame is complete, no byte behind any caps[i] is written - and the Python call raises ValueError naming
    that first frame."""
    s, s_sha = noise_64x96(fx, ctx, 90)
    jobs = damaged(s)
    streams, labels = [s], ["intact"]
    for label, d in jobs:
        streams += [d, s]
        labels += [label, "intact"]
    alone = [D.single(ctx, d) for d in streams]
    first_bad = next(i for i, (rc, _) in enumerate(alone) if rc != 0)
    assert sum(rc != 0 for rc, _ in alone) >= 10 and any(rc == 0 and lab != "intact" for (rc, _), lab in zip(alone, labels))  # both outcomes occur
    call = D.DCall(ctx, streams)
    print("rc:", call.rc, call.error, "figures:", D.figures(ctx))
    assert call.rc == alone[first_bad][0] == N.TIC_E_STREAM and call.error.startswith("frame %d: " % first_bad), (call.rc, call.error, first_bad)
    for i, ((rc, digest), lab) in enumerate(zip(alone, labels)):
        assert call.untouched_behind(i), (i, lab)
        assert (call.hs[i], call.ws[i]) == (64, 96), i
        if rc == 0:
            assert D.px_sha(call.pixels(i)) == digest, (i, lab)
        if lab == "intact":
            assert rc == 0 and digest == s_sha
    figs = D.figures(ctx)
    assert figs[0] + figs[1] == len(streams) and figs[0] >= len(jobs) + 1  # (every intact frame at least by the batch kernels)
    with pytest.raises(ValueError, match="^frame %d: " % first_bad):
        T.decompress_batch_adaptive(streams, ctx=ctx)


def test_both_download_routes(ctx, fx):
    """Dense frames that follow each other in one block (the Python mirror's: 48 frames of 64 x 96, 288 KB) come down in one direct copy; frames
    of width 21 and 2040 in buffers of their own go through the pinned buffer and the copy threads.  The same pixels either way."""
    pairs = [noise_64x96(fx, ctx, q) for q in (5, 50, 90, 99)]
    streams, want = [p[0] for p in pairs] * 12, [p[1] for p in pairs] * 12
    got = T.decompress_batch_adaptive(streams, ctx=ctx)
    assert [D.px_sha(px) for px in got] == want
    print("dense block: figures", D.figures(ctx), "direct", D.direct_frames(ctx))
    assert D.figures(ctx) == (48, 0, 1) and D.direct_frames(ctx) == 48
    call = D.DCall(ctx, streams)  # the same streams into buffers of their own: nothing follows anything
    assert call.rc == 0 and D.direct_frames(ctx) == 0 and D.figures(ctx) == (48, 0, 1)
    assert [D.px_sha(call.pixels(i)) for i in range(48)] == want and all(call.untouched_behind(i) for i in range(48))
    entries, frames, qs = D.load_fixture()
    pick = [i for i, e in enumerate(entries) if (e["height"], e["width"]) in ((13, 21), (8, 2040))]
    assert len(pick) == 2
    odd = [T.compress_adaptive(frames[i], qs[i], ctx=ctx) for i in pick]
    for s, i in zip(odd, pick):
        assert D.sha(s) == entries[i]["sha256"]
    call = D.DCall(ctx, odd + odd)
    assert call.rc == 0 and D.direct_frames(ctx) == 0 and D.figures(ctx) == (4, 0, 1)
    for k in range(4):
        assert D.px_sha(call.pixels(k)) == entries[pick[k % 2]]["decoded_sha256"] and call.untouched_behind(k), k
    got = T.decompress_batch_adaptive(odd + odd, ctx=ctx)  # (one block, but rows of 21 pixels are not the device buffer's rows of 24: pinned too)
    assert [D.px_sha(px) for px in got] == [entries[i]["decoded_sha256"] for i in pick] * 2 and D.direct_frames(ctx) == 0


def test_fixture_set_on_the_shipped_library():
    """test_fixture_set_in_one_call once more in a fresh process that loads the library that ships (TIC_TEST_HOOKS=0: no hooks compiled in)."""
    assert os.environ.get("TIC_TEST_HOOKS") == "1" and N.load().tic_build_has_test_hooks() == 1
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    env["TIC_TEST_HOOKS"] = "0"
    code = ("import sys; sys.path.insert(0, %r); import tinyimgcodec_amd._native as N; assert N.load().tic_build_has_test_hooks() == 0; "
            "import pytest; sys.exit(pytest.main([%r, '-m', 'gpu', '-q', '-x', '-s', '-p', 'no:cacheprovider', '-k', "
            "'test_fixture_set_in_one_call']))" % (ROOT, os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0 and "1 passed" in r.stdout and "failed" not in r.stdout, tail
