"""The device decoder of per-image table streams (tic_adaptive_dec_gpu.hip) on HAND-BUILT tables and on the middle of its rounds protocol:
the streams of tests/adaptive_tables.py (checked against the digests of tests/golden/adaptive_tables.json, which the unmodified reference
wrote) through decompress_adaptive() and decompress_batch_adaptive().  Pixels are the fixture's (the reference's decode() of the built
coefficients); the exits moved per round that the library prints under TIC_DECODE_TRACE are, entry for entry, the lists a plain Python
model of the stitch computed without the library (adaptive_tables.stitch_model, recorded in the fixture)."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

import adaptive_decode_batch_common as D
import adaptive_tables as AT

pytestmark = pytest.mark.gpu

FX = AT.load_fixture()
WELL_FORMED = [n for n, e in FX["cases"].items() if e["well_formed"] and not n.startswith("rounds_")]
ROUNDS = [n for n in FX["cases"] if n.startswith("rounds_")]


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def streams():
    """name -> the stream under the case's first quality, checked against the fixture's digest: a wrong input cannot pass as a right output."""
    out = {}
    for name, c in AT.build_cases(AT.fixture_tables(FX)).items():
        s = AT.stream_of(name, c)
        e = FX["cases"][name]["streams"]["q%d" % c["qualities"][0]]
        assert (len(s), AT.sha(s)) == (e["bytes"], e["sha256"]) and len(s) < (1 << 20), name
        out[name] = s
    return out


@pytest.fixture(scope="module")
def noise(ctx):
    """The two 64 x 96 noise streams of adaptive_streams.json (q = 50 and 90) -> [(stream, pixel digest, stitch_model's changed[])]."""
    fx = D.adaptive_streams_fixture()
    out = []
    for q in (50, 90):
        e = next(c for c in fx["cases"] if c["name"] == "noise" and c["quality"] == q)
        s = T.compress_adaptive(D.case_image("noise", 64, 96), q, ctx=ctx)
        assert len(s) == e["bytes"] and D.sha(s) == e["sha256"]
        out.append((s, e["decoded_sha256"], AT.stitch_model(s)[2]))
    return out


def variants(name, streams):
    """[(stream, pixel digest)] under every header quality of the case."""
    e = FX["cases"][name]
    return [(AT.with_quality(streams[name], q), e["streams"]["q%d" % q]["decoded_sha256"]) for q in e["qualities"]]


def path_of(ctx):
    L = N.load()
    return L.tic_last_decode_path(ctx.handle), L.tic_last_decode_giveup(ctx.handle)


def outcome(stream, ctx):
    try:
        return D.px_sha(T.decompress_adaptive(stream, ctx=ctx))
    except ValueError:
        return "ValueError"


def small_streams_to_the_device(monkeypatch):
    assert N.load().tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_MIN_BLOCKS", "1")
    monkeypatch.setenv("TIC_DECODE_MIN_BITS", "0")


# ---- single call ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WELL_FORMED)
def test_single_call_on_the_device(ctx, streams, monkeypatch, name):
    """Every well-formed family is decoded by the device decoder - a full long list, symbols of exactly 64 bits, a 64-bit code of size 0,
    a 15-bit DC code of category 15, a table of exactly kAdaptMaxTableBytes (its symbols repeat), the longest table of distinct symbols,
    an incomplete code, long codes below the short ones, blocks longer
    than a range - to the pixels the reference's decode() gives for the built coefficients, under every header quality."""
    small_streams_to_the_device(monkeypatch)
    for s, want in variants(name, streams):
        assert outcome(s, ctx) == want, name
        assert path_of(ctx) == (1, 0), (name, path_of(ctx))


@pytest.mark.parametrize("name", WELL_FORMED)
def test_single_call_on_the_host(ctx, streams, monkeypatch, name):
    """The same streams under TIC_DECODE_HOST=1: the same pixels from the host's bit-serial decoder."""
    assert N.load().tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_HOST", "1")
    for s, want in variants(name, streams):
        assert outcome(s, ctx) == want, name
        assert path_of(ctx) == (2, 0), (name, path_of(ctx))


def test_too_wide_and_damaged_chain_end_as_on_the_host(ctx, streams, monkeypatch):
    """too_wide (a symbol of 65 bits with its value) is refused by the one table parser on either route.  damaged_chain (the true chain
    meets a window without a code before block N) ends on the device route as under TIC_DECODE_HOST=1 - on path 2, after a give-up."""
    small_streams_to_the_device(monkeypatch)
    got = {}
    for name in ("too_wide", "damaged_chain"):
        got[name] = outcome(streams[name], ctx), path_of(ctx)
        print(name, got[name])
    assert got["too_wide"][0] == "ValueError" and got["too_wide"][1][0] == 2
    assert got["damaged_chain"][1][0] == 2 and got["damaged_chain"][1][1] != 0
    assert outcome(streams["incomplete"], ctx) == FX["cases"]["incomplete"]["streams"]["q5"]["decoded_sha256"] and path_of(ctx) == (1, 0)  # (the twin without the flipped bit)
    monkeypatch.setenv("TIC_DECODE_HOST", "1")
    for name in ("too_wide", "damaged_chain"):
        assert outcome(streams[name], ctx) == got[name][0], name
        assert path_of(ctx) == (2, 0)
    assert got["damaged_chain"][0] == "ValueError"  # (decode_model: a window without a code - the host decoder's "code without a symbol")


# ---- batch -----------------------------------------------------------------------------------------------------------------------------
def family_set(streams):
    """[(name, stream, digest)]: every well-formed family, each under another of its header qualities."""
    out = []
    for i, name in enumerate(WELL_FORMED):
        v = variants(name, streams)
        out.append((name,) + v[i % len(v)])
    return out


def check_family_set(ctx, streams, chunks):
    jobs = family_set(streams)
    assert len(jobs) == 8 and all(D.batch_takes(s) for _, s, _ in jobs)
    for order in (list(range(len(jobs))), [4, 1, 6, 0, 7, 3, 5, 2]):
        for rep in range(2):  # (twice on the one context: what a chunk leaves in the buffers must not show in the next call)
            got = T.decompress_batch_adaptive([jobs[i][1] for i in order], ctx=ctx)
            for k, i in enumerate(order):
                assert D.px_sha(got[k]) == jobs[i][2], (jobs[i][0], order, rep)
            print("figures:", D.figures(ctx))
            assert D.figures(ctx) == (len(jobs), 0, chunks(len(jobs))), D.figures(ctx)


def test_families_in_one_batch(ctx, streams):
    """All well-formed families through one decompress_batch_adaptive, in two orders and twice on one context: every frame by the batch
    kernels (each workgroup stages ITS frame's tables: a full long list beside an empty one), every frame the fixture's pixels."""
    check_family_set(ctx, streams, lambda n: 1)


def test_families_in_chunks_of_three(ctx, streams, monkeypatch):
    assert N.load().tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_ADBATCH_CHUNK", "3")
    check_family_set(ctx, streams, lambda n: -(-n // 3))


def test_families_in_one_batch_on_the_shipped_library():
    """test_families_in_one_batch once more in a fresh process that loads the library that ships (TIC_TEST_HOOKS=0: no hooks compiled in;
    the batch has no size threshold, so it needs none)."""
    assert os.environ.get("TIC_TEST_HOOKS") == "1" and N.load().tic_build_has_test_hooks() == 1
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    env["TIC_TEST_HOOKS"] = "0"
    code = ("import sys; sys.path.insert(0, %r); import tinyimgcodec_amd._native as N; assert N.load().tic_build_has_test_hooks() == 0; "
            "import pytest; sys.exit(pytest.main([%r, '-m', 'gpu', '-q', '-x', '-s', '-p', 'no:cacheprovider', '-k', "
            "'test_families_in_one_batch and not shipped']))" % (ROOT, os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0 and "1 passed" in r.stdout and "failed" not in r.stdout, tail


@pytest.mark.parametrize("bad", [("too_wide", "damaged_chain"), ("damaged_chain", "too_wide")])
def test_bad_tables_inside_a_batch(ctx, streams, bad):
    """too_wide and damaged_chain between intact frames at the C-ABI, outputs of caps[i] + 64 sentinel bytes: the return code and the
    "frame i: " message are the first failing frame's, the neighbours are complete with the pixels tic_decompress_adaptive alone gives,
    and no byte behind any caps[i] is written.  The figures say how each frame went: the four intact ones by the batch kernels, too_wide
    (its table does not parse: no frame of theirs) and damaged_chain (taken, given up on at the incident) by the single call."""
    jobs = family_set(streams)
    names = [jobs[0][0], bad[0], jobs[1][0], jobs[2][0], bad[1], jobs[3][0]]
    batch = [jobs[0][1], streams[bad[0]], jobs[1][1], jobs[2][1], streams[bad[1]], jobs[3][1]]
    want = [jobs[0][2], None, jobs[1][2], jobs[2][2], None, jobs[3][2]]
    alone = [D.single(ctx, s) for s in batch]
    assert [rc for rc, _ in alone] == [0, N.TIC_E_STREAM, 0, 0, N.TIC_E_STREAM, 0], alone
    call = D.DCall(ctx, batch)
    print("rc:", call.rc, call.error, "figures:", D.figures(ctx))
    assert call.rc == N.TIC_E_STREAM and call.error.startswith("frame 1: "), (call.rc, call.error)
    for i, (name, w) in enumerate(zip(names, want)):
        assert call.untouched_behind(i), (i, name)
        assert (call.hs[i], call.ws[i]) == D.shape_of(batch[i]), (i, name)
        if w is not None:
            assert alone[i][1] == w and D.px_sha(call.pixels(i)) == w, (i, name)
    figs = D.figures(ctx)
    assert figs == (4, 2, 1), figs
    with pytest.raises(ValueError, match="^frame 1: "):
        T.decompress_batch_adaptive(batch, ctx=ctx)


# ---- rounds ----------------------------------------------------------------------------------------------------------------------------
SINGLE_LINE = re.compile(r"adaptive decode: (\d+) blocks, range (\d+), rounds (\d+)\.\.(-?\d+)( and the passes)?, exits moved:((?: \d+)*), give-up (\d+), blocks on the chain (\d+)")
BATCH_LINE = re.compile(r"adaptive batch decode: (\d+) frames, rounds (\d+)\.\.(\d+)( and the passes)?, exits moved in round (\d+): (\d+), frames still moving: (\d+)")


def single_trace(err):
    """-> (range, [exits moved per round, joined over the launches], [(round0, last round, passes)])."""
    lines = [m.groups() for m in SINGLE_LINE.finditer(err)]
    moved = [int(x) for g in lines for x in g[5].split()]
    return {int(g[1]) for g in lines}, moved, [(int(g[2]), int(g[3]), g[4] is not None) for g in lines]


def batch_trace(err):
    """-> [(frames, round0, last round, passes, the round reported, exits moved in it, frames still moving)] per launch."""
    return [(int(g[0]), int(g[1]), int(g[2]), g[3] is not None, int(g[4]), int(g[5]), int(g[6])) for g in (m.groups() for m in BATCH_LINE.finditer(err))]


def launched(changed):
    """The rounds the single call launches for a chain the model settles in round z = len(changed) - 1: three, then sixteen at a time."""
    z = len(changed) - 1
    return 3 if z <= 2 else 3 + 16 * -(-(z - 2) // 16)


def padded(changed, n):
    return (changed + [0] * n)[:n]


@pytest.mark.parametrize("name", ROUNDS)
def test_rounds_of_the_single_call_are_the_models(ctx, streams, monkeypatch, capfd, name):
    """TIC_DECODE_TRACE: the exits moved per round, joined over the launches, equal stitch_model's changed[] entry for entry (and are 0
    behind its first 0, up to the end of the launch of sixteen); the geometry is the model's; path 1, the fixture's pixels."""
    small_streams_to_the_device(monkeypatch)
    monkeypatch.setenv("TIC_DECODE_TRACE", "1")
    e = FX["cases"][name]
    capfd.readouterr()
    got = outcome(streams[name], ctx)
    err = capfd.readouterr().err
    path = path_of(ctx)
    ranges, moved, launches = single_trace(err)
    print(name, "trace:", moved, launches, "model:", e["census"]["changed"])
    assert ranges == {e["census"]["range_bits"]} and D.geometry(streams[name], e["blocks"]) == (e["census"]["range_bits"], e["census"]["nranges"])
    n = launched(e["census"]["changed"])
    assert moved == padded(e["census"]["changed"], n), name
    assert launches[0] == (0, 2, True) and (len(launches) == 1 or launches[-1] == (n, n - 1, True)), launches
    assert path == (1, 0) and got == e["streams"]["q50"]["decoded_sha256"], (name, path)


def check_batch_rounds(ctx, names, batch, want, models, capfd):
    """One decompress_batch_adaptive of `batch` under TIC_DECODE_TRACE against the models' changed[] of its frames."""
    late = [m for m in models if len(m) - 1 > AT.BATCH_ROUNDS - 1]  # frames round 18 still moves: the single call's
    total = [sum(padded(m, AT.BATCH_ROUNDS)[r] for m in models) for r in range(AT.BATCH_ROUNDS)]
    capfd.readouterr()
    got = T.decompress_batch_adaptive(batch, ctx=ctx)
    err = capfd.readouterr().err
    figs = D.figures(ctx)
    lines = batch_trace(err)
    print(names, "figures:", figs, "trace:", lines, single_trace(err)[1])
    for k, (px, w) in enumerate(zip(got, want)):
        assert D.px_sha(px) == w, (names, k)
    assert figs == (len(batch) - len(late), len(late), 1), figs
    F = len(batch)
    if total[2] == 0:  # every frame settles within the three rounds launched with the passes: no round 3 .. 18
        assert lines == [(F, 0, 2, True, 2, 0, 0)], lines
    else:
        assert lines == [(F, 0, 2, True, 2, total[2], sum(m[2] != 0 for m in models if len(m) > 2)),
                         (F, 3, 18, False, 18, total[18], len(late)),
                         (F, 19, 18, True, 18, total[18], len(late))], lines
        assert (total[18] == 0) == (not late)
    # the frame round 18 still moved goes through the single call with all its rounds: the model's again
    moved = single_trace(err)[1]
    assert moved == [x for m in late for x in padded(m, launched(m))], moved


@pytest.mark.parametrize("name", ROUNDS)
def test_rounds_of_a_batch(ctx, streams, noise, monkeypatch, capfd, name):
    """Each rounds_* case between the two 64 x 96 noise streams.  The case that settles by round 2 sees no further round; the others get
    rounds 3 .. 18 and the passes and the inverse transform a second time - over a chunk whose noise frames have settled and whose
    workgroups leave at once while the exit buffers keep alternating; the case beyond round 18 is then the single call's, its neighbours
    stay batch frames.  "exits moved in round 18" is 0 exactly when the model settles by then."""
    assert N.load().tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_TRACE", "1")
    e = FX["cases"][name]
    batch = [noise[0][0], streams[name], noise[1][0]]
    want = [noise[0][1], e["streams"]["q50"]["decoded_sha256"], noise[1][1]]
    check_batch_rounds(ctx, ["noise", name, "noise"], batch, want, [noise[0][2], e["census"]["changed"], noise[1][2]], capfd)


def test_all_rounds_cases_in_one_chunk(ctx, streams, noise, monkeypatch, capfd):
    """The four rounds_* cases and the noise frames in one chunk, in two orders and twice on one context: frames that settle in rounds 2, 4
    and 14 beside one that never does within the nineteen."""
    assert N.load().tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_TRACE", "1")
    pool = [("noise50",) + noise[0]] + [(n, streams[n], FX["cases"][n]["streams"]["q50"]["decoded_sha256"], FX["cases"][n]["census"]["changed"]) for n in ROUNDS]
    pool.append(("noise90",) + noise[1])
    for order in (list(range(6)), [4, 2, 5, 1, 3, 0]):
        for rep in range(2):
            pick = [pool[i] for i in order]
            check_batch_rounds(ctx, [p[0] for p in pick], [p[1] for p in pick], [p[2] for p in pick], [p[3] for p in pick], capfd)
