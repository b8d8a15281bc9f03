"""Requantisation on the GPU (include/tinyimgcodec_hip_requantize.h): requantize_zz on the built corpus at every pair of the fixture,
requantize against the reference's streams, requantized_sizes and requantize_to_size against the reference's size tables, the context as
state, and the shipped library.  Exact results only: every expectation is tests/golden/requantize.json (made by the unmodified reference),
the plain numpy model of tests/requantize_common.py (held to that fixture by tests/test_requantize_cpu.py) or the pinned oracle."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import damaged_streams as D
import requantize_common as RC

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N
from conftest import GOLDEN, rand_frame

pytestmark = pytest.mark.gpu

DAMAGED = ("noise64/flip1/seeded0", "noise64/garbage/seeded1", "noise40x72/cut/at16", "noise40x72/insert/bytes1", "ragged17x33/garbage/ones300",
           "ragged17x33/zeros_tail/seeded0", "lenna64/value_flip/dc1", "lenna64/delete/bytes8", "noise256/flip3/tail", "noise256/garbage/seeded1",
           "twolevel256/ones_tail/seeded0", "twolevel256/cut/in_dc_value")


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return RC.load_fixture()


@pytest.fixture(scope="module")
def corpus(fx):
    zz = RC.corpus()
    assert RC.digest(zz) == fx["corpus_sha256"]
    return zz


class Resident:
    """Device buffers of a test, freed with it."""

    def __init__(self, ctx):
        self.ctx, self.L, self.ptrs = ctx, N.load(), []

    def alloc(self, nbytes):
        p = C.c_void_p()
        self.ctx.check(self.L.tic_dev_alloc(self.ctx.handle, nbytes, C.byref(p)))
        self.ptrs.append(p)
        return p

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        self.ctx.check(self.L.tic_memcpy_h2d(self.ctx.handle, p, arr.ctypes.data, arr.nbytes))
        return p

    def down(self, p, shape, dtype=np.int16):
        out = np.empty(shape, dtype)
        self.ctx.check(self.L.tic_memcpy_d2h(self.ctx.handle, out.ctypes.data, p, out.nbytes))
        return out

    def free(self):
        for p in self.ptrs:
            self.L.tic_dev_free(self.ctx.handle, p)
        self.ptrs = []


def run_jobs(ctx, rs, d_src, src_blocks, jobs, d_out, out_blocks):
    """tic_requantize_zz_v_dev over jobs [(src_block, nblocks, q1, q2)] -> (int16 [sum nblocks, 64], range flags)."""
    n = len(jobs)
    arr = lambda t, k: (t * n)(*[j[k] for j in jobs])  # noqa: E731
    rng = (C.c_int * n)(*([7] * n))
    total = sum(j[1] for j in jobs)
    ctx.check(rs.L.tic_requantize_zz_v_dev(ctx.handle, d_src, src_blocks, n, arr(C.c_size_t, 0), arr(C.c_size_t, 1), arr(C.c_int, 2), arr(C.c_int, 3), d_out,
                                           out_blocks, rng))
    return rs.down(d_out, (total, 64)), list(rng)


def check_result(got, flag, zz, q1, q2, want_outside, want_sha):
    """One job's rows against the fixture's record of the pair: the flag exactly where a result leaves int16; the digest where none does,
    and everywhere else every element that stayed inside int16 against the model."""
    assert flag == (1 if want_outside else 0), (q1, q2, flag, want_outside)
    if not want_outside:
        assert RC.digest(got) == want_sha, (q1, q2)
    else:
        want = RC.model(zz, q1, q2)
        inside = (want >= -32768) & (want <= 32767)
        assert RC.outside_int16(want) == want_outside and np.array_equal(got[inside], want[inside]), (q1, q2)


@pytest.mark.parametrize("part", ["corpus", "latin"])
def test_every_pair_64_jobs_per_launch(part, ctx, fx, corpus):
    """Every pair of the fixture on resident buffers, 64 jobs to a launch, every job reading the same rows: the whole corpus (2,051 blocks)
    and its Latin part alone (2,047: a last chunk of 7 blocks)."""
    zz = corpus if part == "corpus" else corpus[:RC.N_LATIN]
    nb, suffix = zz.shape[0], "" if part == "corpus" else "_latin"
    rs = Resident(ctx)
    try:
        d_src, d_out = rs.up(zz), rs.alloc(64 * nb * 128)
        pairs = fx["pairs"]
        flagged = 0
        for first in range(0, len(pairs), 64):
            chunk = pairs[first:first + 64]
            got, flags = run_jobs(ctx, rs, d_src, nb, [(0, nb, p["from"], p["to"]) for p in chunk], d_out, 64 * nb)
            for k, p in enumerate(chunk):
                check_result(got[k * nb:(k + 1) * nb], flags[k], zz, p["from"], p["to"], p["outside_int16" + suffix], p["sha256" + suffix])
                flagged += flags[k]
        assert flagged == sum(p["outside_int16" + suffix] > 0 for p in pairs) > 0
        assert T.last_requantize(ctx)["store_launches"] == 1  # (the last call's 13 jobs)
    finally:
        rs.free()


def test_job_seams(ctx, corpus):
    """One list whose jobs have different lengths and sources that overlap each other: every seam between two jobs falls somewhere else in a
    chunk of 8 blocks, and a job of one block stands between two long ones."""
    lens = [1, 7, 8, 9, 2047, 1, 63, 64, 65, 127, 128, 129, 255, 257, 2051, 3, 1, 130, 511, 513]
    qs = [(50, 25), (99, 3), (1, 99), (25, 50), (3, 1), (50, 50), (25, 24), (50, 49), (99, 98), (3, 4)]
    jobs = [((k * 37) % (RC.N_CORPUS - n + 1), n, *qs[k % len(qs)]) for k, n in enumerate(lens)]
    total = sum(lens)
    rs = Resident(ctx)
    try:
        d_src, d_out = rs.up(corpus), rs.up(np.full((total + 8, 64), 0x5A5A, np.uint16))
        got, flags = run_jobs(ctx, rs, d_src, RC.N_CORPUS, jobs, d_out, total)
        at = 0
        for (src, n, q1, q2), flag in zip(jobs, flags):
            want = RC.model(corpus[src:src + n], q1, q2)
            inside = (want >= -32768) & (want <= 32767)
            assert flag == (0 if inside.all() else 1), (src, n, q1, q2)
            assert np.array_equal(got[at:at + n][inside], want[inside]), (src, n, q1, q2)
            at += n
        assert (rs.down(d_out, (total + 8, 64), np.uint16)[total:] == 0x5A5A).all()  # nothing behind the last job
        # the refusals that need no launch
        L, one = rs.L, (C.c_size_t * 1)
        rng = (C.c_int * 1)(7)
        call = lambda src, n, q1, q2, out_blocks, d_o=d_out: L.tic_requantize_zz_v_dev(  # noqa: E731
            ctx.handle, d_src, RC.N_CORPUS, 1, one(src), one(n), (C.c_int * 1)(q1), (C.c_int * 1)(q2), d_o, out_blocks, rng)
        assert call(0, 8, 50, 100, 8) == N.TIC_E_QUALITY and call(0, 8, 0, 50, 8) == N.TIC_E_QUALITY
        assert call(0, 9, 50, 25, 8) == N.TIC_E_SPACE and call(RC.N_CORPUS - 7, 8, 50, 25, 8) == N.TIC_E_ARG and call(0, 0, 50, 25, 8) == N.TIC_E_ARG
        assert call(0, 8, 50, 25, 8, d_src) == N.TIC_E_ARG and rng[0] == 7  # source and destination overlap
    finally:
        rs.free()


def test_requantize_zz_host_and_resident(ctx, fx, corpus):
    """The single call: every pair from host buffers (KeyError exactly where the fixture counts a result outside int16); resident, out of
    place and in place, at 2,047 blocks and at one."""
    for p in fx["pairs"]:
        if p["outside_int16"]:
            with pytest.raises(KeyError):
                T.requantize_zz(corpus, p["from"], p["to"], ctx=ctx)
        else:
            assert RC.digest(T.requantize_zz(corpus, p["from"], p["to"], ctx=ctx)) == p["sha256"], (p["from"], p["to"])
    by = {(p["from"], p["to"]): p for p in fx["pairs"]}
    L = N.load()
    rs = Resident(ctx)
    try:
        for q1, q2 in ((50, 25), (99, 3), (25, 99), (1, 99)):
            p = by[(q1, q2)]
            for nb in (RC.N_LATIN, 1):
                zz = corpus[:nb]
                d_a, d_b = rs.up(zz), rs.alloc(nb * 128)
                rc = L.tic_requantize_zz_dev(ctx.handle, d_a, nb, q1, q2, d_b)
                want = RC.model(zz, q1, q2)
                assert rc == (N.TIC_E_RANGE if RC.outside_int16(want) else N.TIC_OK), (q1, q2, nb)
                assert np.array_equal(rs.down(d_a, (nb, 64)), zz)  # the source is left alone
                inside = (want >= -32768) & (want <= 32767)
                assert np.array_equal(rs.down(d_b, (nb, 64))[inside], want[inside])
                if nb == RC.N_LATIN and not p["outside_int16_latin"]:
                    assert RC.digest(rs.down(d_b, (nb, 64))) == p["sha256_latin"]
                assert L.tic_requantize_zz_dev(ctx.handle, d_a, nb, q1, q2, d_a) == rc  # in place
                assert np.array_equal(rs.down(d_a, (nb, 64))[inside], want[inside])
        d_a = rs.up(corpus)
        assert L.tic_requantize_zz_dev(ctx.handle, d_a, 16, 50, 25, C.c_void_p(d_a.value + 128)) == N.TIC_E_ARG  # overlapping, not the same
        assert L.tic_requantize_zz_dev(ctx.handle, d_a, 16, 50, 25, C.c_void_p(d_a.value + 8)) == N.TIC_E_ARG    # not 16-byte aligned
        assert L.tic_requantize_zz_dev(ctx.handle, d_a, 16, 50, 100, d_a) == N.TIC_E_QUALITY
        assert L.tic_requantize_zz_dev(ctx.handle, None, 0, 50, 25, None) == N.TIC_OK
    finally:
        rs.free()


# ---- streams ----------------------------------------------------------------------------------------------------------------------------
def test_requantize_against_the_reference_s_streams(ctx, fx, oracle):
    """Both families, every image x source quality x target quality of the fixture; the host reader's route (frames of at most 64 blocks)."""
    imgs = RC.images()
    for s in fx["streams"]:
        src = T.compress(imgs[s["image"]], s["from"], ctx=ctx)
        assert (len(src), RC.sha(src)) == (s["bytes"], s["sha256"])
        for q, rec in s["to"].items():
            for family, adaptive in (("default", False), ("adaptive", True)):
                out = T.requantize(src, int(q), adaptive=adaptive, ctx=ctx)
                assert (len(out), RC.sha(out)) == (rec[family]["bytes"], rec[family]["sha256"]), (s["image"], s["from"], q, family)
                assert T.last_requantize(ctx) == {"route": 2, "measure_launches": 0, "store_launches": 1, "rounds": 0}
    for name, q1 in RC.SIZE_TABLES:  # KeyError where the reference's writer raises it
        table = fx["size_tables"]["%s@%d" % (name, q1)]
        src = oracle.compress(imgs[name], q1)
        for q in range(1, 100):
            if table[q] < 0:
                with pytest.raises(KeyError):
                    T.requantize(src, q, ctx=ctx)
    empty = T.compress(np.zeros((0, 5), np.uint8), 50, ctx=ctx)
    assert len(empty) == 16 and T.requantize(empty, 7, ctx=ctx) == empty[:8] + (7).to_bytes(4, "little") + empty[12:]


def test_identity_on_the_benchmark_set(ctx):
    """requantize(s, q_of_s) == s for every default-table stream of the benchmark set at quality 50, read by the device reader."""
    pixels = np.load(os.path.join(GOLDEN, "benchmark_set.npz"))["pixels"]
    with open(os.path.join(GOLDEN, "benchmark_set.json")) as f:
        recs = {e["image"]: e for e in json.load(f)["entries"] if e["quality"] == 50}
    assert len(recs) == 49
    for i in range(49):
        s = T.compress(pixels[i], 50, ctx=ctx)
        assert (len(s), RC.sha(s)) == (recs[i + 1]["bytes"], recs[i + 1]["sha256"]), i
        assert T.requantize(s, 50, ctx=ctx) == s, i
        assert T.last_requantize(ctx)["route"] == 1


def composition(ctx, s, q):
    """requantize(s, q) against entropy_encode(requantize_zz(*entropy_decode_zz(s), q)): the same bytes, or KeyError on both sides (the
    reader's ValueError for a running DC outside int16 is requantize()'s KeyError: TIC_E_RANGE either way)."""
    try:
        zz, hdr = T.entropy_decode_zz(s, ctx=ctx)
        want = T.entropy_encode(T.requantize_zz(zz, hdr["quality"], q, ctx=ctx), hdr["height"], hdr["width"], q)
    except (KeyError, ValueError):
        with pytest.raises(KeyError):
            T.requantize(s, q, ctx=ctx)
        return None
    got = T.requantize(s, q, ctx=ctx)
    assert got == want
    return got


def test_composition_on_damaged_streams(ctx, oracle):
    entries = {e[0]: e[4] for e in D.corpus(oracle)}
    rec = {r["name"]: r for r in D.load_fixture()["entries"]}
    done = 0
    for name in DAMAGED:
        s = entries[name]
        assert D.sha(s) == rec[name]["sha256"], name
        q0 = T.parse_header(s)["quality"]
        for q in (max(1, q0 // 3), q0, min(99, q0 + 7)):
            done += composition(ctx, s, q) is not None
    assert done >= 20, done


def test_composition_on_both_sides_of_the_device_reader_s_line(ctx, monkeypatch):
    """1024 x 1024 noise - 16,384 blocks - is read by the device reader; 1016 x 1024 - 16,256 blocks - by the host reader once the reader's
    short-stream line stands where its long-stream line does (TIC_DECODE_MIN_BLOCKS: without the hook the device reader takes frames from
    1,024 blocks on, and the route is then the one tic_entropy_decode takes for the same stream)."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    big, below = rand_frame(1024, 1024, 1024), rand_frame(1016, 1016, 1024)
    s_big, s_below = T.compress(big, 90, ctx=ctx), T.compress(below, 90, ctx=ctx)
    assert composition(ctx, s_big, 40) is not None
    assert T.last_requantize(ctx)["route"] == 1 and L.tic_last_decode_giveup(ctx.handle) == 0
    assert T.requantize(s_big, 90, ctx=ctx) == s_big
    assert composition(ctx, s_below, 40) is not None
    T.entropy_decode_zz(s_below, ctx=ctx)
    path = L.tic_last_decode_path(ctx.handle)
    T.requantize(s_below, 40, ctx=ctx)
    assert T.last_requantize(ctx)["route"] == path
    monkeypatch.setenv("TIC_DECODE_MIN_BLOCKS", "16384")
    assert composition(ctx, s_below, 40) is not None
    assert T.last_requantize(ctx)["route"] == 2
    assert composition(ctx, s_big, 40) is not None
    assert T.last_requantize(ctx)["route"] == 1


# ---- sizes and the search ------------------------------------------------------------------------------------------------------------------
def search_plan(sizes, budget, qmin, qmax, depth):
    """RateSearch (tic_rate_plan.h) over a table of sizes -> (quality or None, rounds): per round qmin (once) and every middle the bisection
    can reach within `depth` steps, then the bisection as far as the known sizes carry."""
    known, lo, hi, rounds = {}, qmin, qmax, 0

    def candidates(lo, hi, d, out):
        if lo >= hi or d == 0:
            return
        mid = (lo + hi + 1) // 2
        if mid not in known:
            out.append(mid)
        candidates(mid, hi, d - 1, out)
        candidates(lo, mid - 1, d - 1, out)

    fits = lambda q: 0 <= known[q] <= budget  # noqa: E731
    while True:
        cand = [] if qmin in known else [qmin]
        candidates(lo, hi, depth, cand)
        if not cand:
            break
        rounds += 1
        for q in cand:
            known[q] = sizes[q]
        if not fits(qmin):
            return None, rounds
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if mid not in known:
                break
            if fits(mid):
                lo = mid
            else:
                hi = mid - 1
        else:
            break
    return lo, rounds


@pytest.mark.parametrize("which", range(len(RC.SIZE_TABLES)))
def test_sizes_and_search(which, ctx, fx, oracle):
    name, q1 = RC.SIZE_TABLES[which]
    table = fx["size_tables"]["%s@%d" % (name, q1)]
    s = oracle.compress(RC.images()[name], q1)
    sizes = T.requantized_sizes(s, range(1, 100), ctx=ctx)
    assert list(sizes) == table[1:]
    assert T.last_requantize(ctx) == {"route": 2, "measure_launches": 2, "store_launches": 0, "rounds": 1}  # 99 qualities: launches of 64 and 35
    assert list(T.requantized_sizes(s, [q1, 5, q1], ctx=ctx)) == [len(s), table[5], len(s)]
    streams = {}
    inside = sorted(v for v in table[1:q1 + 1] if v >= 0)
    budgets = [table[1] - 1, 10 ** 9, table[q1 // 2], table[q1 // 2] - 1, inside[len(inside) // 3], table[q1] - 1]
    for qmax in (None, 99):
        for budget in budgets:
            want, rounds = search_plan(table, budget, 1, q1 if qmax is None else qmax, 3)
            assert want == RC.bisect(table, budget, 1, q1 if qmax is None else qmax)
            if want is None:
                with pytest.raises(ValueError, match="%d bytes at quality 1 exceed" % table[1]):
                    T.requantize_to_size(s, budget, max_quality=qmax, ctx=ctx)
                assert T.last_requantize(ctx) == {"route": 2, "measure_launches": rounds, "store_launches": 0, "rounds": rounds}
                continue
            got, q = T.requantize_to_size(s, budget, max_quality=qmax, ctx=ctx)
            # the stream is read once; a round is one launch of the measuring kernel, the chosen quality one of the store kernel
            assert T.last_requantize(ctx) == {"route": 2, "measure_launches": rounds, "store_launches": 1, "rounds": rounds}, (budget, qmax)
            assert q == want and len(got) == table[q] <= budget, (budget, qmax)
            if q not in streams:
                streams[q] = T.requantize(s, q, ctx=ctx)
            assert got == streams[q]
    assert T.requantize_to_size(s, 10 ** 9, ctx=ctx) == (s, q1)
    if table[99] < 0:  # min_quality itself has no stream
        with pytest.raises(KeyError):
            T.requantize_to_size(s, 10 ** 9, min_quality=99, max_quality=99, ctx=ctx)


def plan_rounds(table, budget, qmin, qmax, depth):
    return search_plan(table, budget, qmin, qmax, depth)[1]


@pytest.mark.parametrize("case", ["bench512", "noise1024", "noise2904"])
def test_many_qualities_per_workgroup(case, ctx, oracle):
    """The measuring kernel where a workgroup takes SEVERAL qualities and a wave several rounds, which the small frames above never reach
    (a frame of one workgroup gives every quality a workgroup of its own):
      bench512   4,096 blocks, 32 workgroups: 64 qualities in a launch are split 32 ways - two per workgroup, and one in the launch of 35;
      noise1024  16,384 blocks, 128 workgroups, the device reader: split 8 - eight qualities per workgroup;
      noise2904  131,769 blocks, the 1,024 workgroups the grid is capped at: no split - one read of the frame, all nine qualities in every
                 workgroup, and waves that stride to a second round of chunks.
    Expected: len(requantize(s, q)) - the store kernel and the default writer, pinned by the tests above -, -1 where it raises KeyError; for
    the benchmark frame also the oracle's stream of the model's coefficients at five qualities.  Then one search on the frame."""
    if case == "bench512":
        img, q1, qs = np.load(os.path.join(GOLDEN, "benchmark_set.npz"))["pixels"][3], 90, list(range(1, 100))
    elif case == "noise1024":
        img, q1, qs = rand_frame(1024, 1024, 1024), 75, list(range(1, 100))
    else:
        img, q1, qs = rand_frame(2904, 2904, 2904), 50, [1, 5, 10, 20, 30, 40, 45, 50, 60]
    s = T.compress(img, q1, ctx=ctx)
    want = []
    for q in qs:
        try:
            want.append(len(T.requantize(s, q, ctx=ctx)))
        except KeyError:
            want.append(-1)
    route = T.last_requantize(ctx)["route"]
    assert route == 1  # (all three are the device reader's)
    got = T.requantized_sizes(s, qs, ctx=ctx)
    assert got.tolist() == want, [(q, g, w) for q, g, w in zip(qs, got.tolist(), want) if g != w][:10]
    assert T.last_requantize(ctx) == {"route": 1, "measure_launches": (len(qs) + 63) // 64, "store_launches": 0, "rounds": 1}
    assert want[qs.index(q1)] == len(s) and min(w for w in want if w >= 0) < len(s) // 2
    if case == "bench512":
        zz = oracle.encode_zz16(img, q1)
        for q in (1, 37, 50, 64, 99):
            info = RC.requantized_info(zz, {"height": 512, "width": 512, "quality": q1}, q)
            try:
                ref = len(oracle.entropy_encode(info["dc"], info["ac"], 512, 512, q))
            except oracle.OracleError:  # a value without a code
                ref = -1
            assert want[q - 1] == ref, q
    table = dict(zip(qs, want))
    full = [0] + [table.get(q, -1) for q in range(1, 100)]
    qmax = q1
    valid = sorted(w for q, w in table.items() if w >= 0 and q <= qmax)
    budget = valid[len(valid) // 2]
    if len(qs) == 99:
        out, q = T.requantize_to_size(s, budget, ctx=ctx)
        n = L_blocks(img)
        rounds = plan_rounds(full, budget, 1, qmax, 3 if n <= 16384 else 2 if n <= 262144 else 1)
        assert T.last_requantize(ctx) == {"route": 1, "measure_launches": rounds, "store_launches": 1, "rounds": rounds}
        assert q == RC.bisect(full, budget, 1, qmax) and len(out) == full[q] <= budget and out == T.requantize(s, q, ctx=ctx)
    else:  # (a table of nine qualities does not carry a bisection over 1..50: the search's own guard - its stream's length against its probe - and the budget)
        out, q = T.requantize_to_size(s, budget, ctx=ctx)
        assert len(out) <= budget and 1 <= q <= qmax and out == T.requantize(s, q, ctx=ctx)


def L_blocks(img):
    return N.load().tic_num_blocks(int(img.shape[0]), int(img.shape[1]))


# ---- the context as state ------------------------------------------------------------------------------------------------------------------
def state_jobs(oracle, fx):
    imgs = RC.images()
    big_img = rand_frame(77, 512, 512)
    J = {"big_img": big_img, "big": oracle.compress(big_img, 90), "small_img": imgs["bench0_64x64"], "small": oracle.compress(imgs["bench0_64x64"], 90)}
    zz_big, hdr = oracle.encode_zz16(big_img, 90), {"height": 512, "width": 512, "quality": 90}
    info = RC.requantized_info(zz_big, hdr, 30)
    J["big_30"] = oracle.entropy_encode(info["dc"], info["ac"], 512, 512, 30)
    J["small_table"] = fx["size_tables"]["bench0_64x64@90"]
    rec = next(s for s in fx["streams"] if s["image"] == "bench0_64x64" and s["from"] == 90)
    J["small_25"] = rec["to"]["25"]
    J["nocode"] = oracle.compress(imgs["bench2_40x72"], 50)
    return J


def new_calls(c, J, big_first=True):
    order = ("big", "small") if big_first else ("small", "big")
    for which in order:
        if which == "big":
            assert T.requantize(J["big"], 30, ctx=c) == J["big_30"]
            assert T.requantized_sizes(J["big"], [30, 90], ctx=c).tolist() == [len(J["big_30"]), len(J["big"])]
            out, q = T.requantize_to_size(J["big"], len(J["big_30"]), ctx=c)
            assert len(out) <= len(J["big_30"]) and q >= 30 and T.requantize(J["big"], q, ctx=c) == out
        else:
            for family in ("default", "adaptive"):
                out = T.requantize(J["small"], 25, adaptive=family == "adaptive", ctx=c)
                assert (len(out), RC.sha(out)) == (J["small_25"][family]["bytes"], J["small_25"][family]["sha256"])
            assert T.requantized_sizes(J["small"], range(1, 100), ctx=c).tolist() == J["small_table"][1:]
            budget = J["small_table"][40]
            out, q = T.requantize_to_size(J["small"], budget, ctx=c)
            assert q == RC.bisect(J["small_table"], budget, 1, 90) and len(out) == J["small_table"][q]


def own_errors(c, J):
    """TIC_E_RANGE from both places it can come from, a refused stream, a short buffer: the next call is exact."""
    with pytest.raises(KeyError):
        T.requantize(J["nocode"], 99, ctx=c)
    with pytest.raises(KeyError):
        T.requantize_zz(np.full((9, 64), 32767, np.int16), 25, 50, ctx=c)  # (twice 32767)
    with pytest.raises(ValueError):
        T.requantize(J["small"][:12] + (1 << 30).to_bytes(4, "little") + J["small"][16:], 25, ctx=c)
    L = N.load()
    out, n = np.zeros(64, np.uint8), C.c_size_t(0)
    buf = np.frombuffer(J["big"], np.uint8)
    assert L.tic_requantize(c.handle, buf.ctypes.data, buf.size, 30, 0, out.ctypes.data, out.size, C.byref(n)) == N.TIC_E_SPACE
    assert n.value == len(J["big_30"]) and (out == 0).all()
    new_calls(c, J, big_first=False)


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0xA5], ids=lambda b: "0x%02X" % b)
def test_fresh_context_under_poisoned_allocation(byte, oracle, fx, monkeypatch):
    """TIC_POISON: every buffer the new calls use comes straight out of a poisoned allocation; a large call then a small one and the
    other way round; tic_test_poison and the calls again; a call after TIC_E_RANGE; and nothing is left allocated behind the context."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_POISON", "0x%02X" % byte)
    J = state_jobs(oracle, fx)
    live = L.tic_test_live_buffers()
    c = T.Context(0)
    try:
        new_calls(c, J, big_first=False)
        new_calls(c, J)
        c.check(L.tic_test_poison(c.handle, byte ^ 0x5A))
        new_calls(c, J)
        own_errors(c, J)
        assert L.tic_test_live_buffers() > live
    finally:
        c.close()
    assert L.tic_test_live_buffers() == live


def test_interleaved_with_the_other_calls(oracle, fx):
    """The new calls between tic_compress and tic_decompress of other geometries on one context: everybody's result stays exact."""
    J = state_jobs(oracle, fx)
    other = rand_frame(5, 200, 328)
    other_s = oracle.compress(other, 75)
    c = T.Context(0)
    try:
        for _ in range(2):
            assert T.compress(other, 75, ctx=c) == other_s
            new_calls(c, J)
            assert np.array_equal(T.decompress(other_s, ctx=c), oracle.decompress(other_s))
            assert T.compress(J["big_img"], 90, ctx=c) == J["big"]
            own_errors(c, J)
            assert np.array_equal(T.decompress(J["big_30"], ctx=c), oracle.decompress(J["big_30"]))
            assert T.compress(other, 75, ctx=c) == other_s
    finally:
        c.close()


# ---- the library that ships ------------------------------------------------------------------------------------------------------------
def test_on_the_shipped_library():
    """The Latin part at every pair, the job seams, the reference's streams and the identity once more in a fresh process on the library
    that ships (TIC_TEST_HOOKS=0: no hooks compiled in)."""
    assert os.environ.get("TIC_TEST_HOOKS") == "1" and N.load().tic_build_has_test_hooks() == 1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    env["TIC_TEST_HOOKS"] = "0"
    code = ("import sys; sys.path.insert(0, %r); import tinyimgcodec_amd._native as N; assert N.load().tic_build_has_test_hooks() == 0; "
            "import pytest; sys.exit(pytest.main([%r, '-m', 'gpu', '-q', '-x', '-p', 'no:cacheprovider', '-k', "
            "'test_every_pair_64_jobs_per_launch and latin or test_job_seams or test_requantize_against or test_identity_on']))"
            % (root, os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail
