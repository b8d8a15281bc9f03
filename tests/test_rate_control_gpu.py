"""Rate control on the GPU: compressed_size / compressed_sizes / compress_to_size and the C-ABI under them, against stream lengths
recorded from the unmodified reference (tests/golden/rate_control.json), the oracle's streams, and a Python replay of the bisection
that is the search's contract."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

from conftest import rand_frame
from test_rate_control_cpu import IMAGES, fixture_image, load_fixture

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return load_fixture()["images"]


def bisect(sizes, budget, qmin, qmax):
    """The contract, replayed on recorded sizes (index q - 1; None = no code): the quality the search must return, or the exception."""
    def fits(q):
        return sizes[q - 1] is not None and sizes[q - 1] <= budget

    if not fits(qmin):
        return KeyError if sizes[qmin - 1] is None else ValueError
    lo, hi = qmin, qmax
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if fits(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


def single_frame_depth(nblocks):
    """The look-ahead of a single-frame search, by the frame's block count (csrc/tic_rate_plan.h; not the batch search's rate_depth)."""
    return 3 if nblocks <= 16384 else 2 if nblocks <= 262144 else 1


def schedule(sizes, budget, qmin, qmax, depth):
    """The documented schedule of tic_compress_to_size, replayed on sizes (index q - 1; None = no code): (probes, host waits).  A round
    probes every middle the bisection can reach within `depth` further steps from where it stands and has not probed yet - the first round
    qmin as well - behind one wait; then the bisection goes as far as the probed sizes carry it.  The stream is one more wait; a qmin
    that does not fit ends the search after the first round, without a stream."""
    def fits(q):
        return sizes[q - 1] is not None and sizes[q - 1] <= budget

    def middles(lo, hi, d, out):
        if lo < hi and d > 0:
            mid = (lo + hi + 1) // 2
            if mid not in probed:
                out.append(mid)
            middles(mid, hi, d - 1, out)
            middles(lo, mid - 1, d - 1, out)

    probed, rounds = set(), 0
    lo, hi = qmin, qmax
    while True:
        cand = [] if rounds else [qmin]
        middles(lo, hi, depth, cand)
        assert len(cand) == len(set(cand))
        if not cand:
            return len(probed), rounds + 1
        probed.update(cand)
        rounds += 1
        if not fits(qmin):
            return len(probed), rounds
        while lo < hi and (lo + hi + 1) // 2 in probed:
            mid = (lo + hi + 1) // 2
            if fits(mid):
                lo = mid
            else:
                hi = mid - 1


class Dev:
    """Device buffers through the C-ABI of library L; freed by close()."""

    def __init__(self, L, handle):
        self.L, self.h, self.ptrs = L, handle, []

    def alloc(self, nbytes, fill=None):
        p = C.c_void_p()
        assert self.L.tic_dev_alloc(self.h, max(nbytes, 16), C.byref(p)) == 0
        self.ptrs.append(p)
        if fill is not None:
            assert self.L.tic_memset_dev(self.h, p, fill, max(nbytes, 16)) == 0
            assert self.L.tic_sync(self.h) == 0
        return p

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        if arr.nbytes:
            assert self.L.tic_memcpy_h2d(self.h, p, arr.ctypes.data, arr.nbytes) == 0
        return p

    def download(self, p, nbytes):
        out = np.empty(nbytes, np.uint8)
        assert self.L.tic_memcpy_d2h(self.h, out.ctypes.data, p, nbytes) == 0
        return out

    def close(self):
        for p in self.ptrs:
            self.L.tic_dev_free(self.h, p)
        self.ptrs = []


@pytest.fixture()
def dev(ctx):
    d = Dev(N.load(), ctx.handle)
    yield d
    d.close()


@pytest.mark.parametrize("name", IMAGES)
def test_compressed_sizes_equal_the_reference(ctx, fx, name):
    """All 99 qualities in one call: the reference's stream length, -1 where the reference raises KeyError."""
    e = fx[name]
    got = T.compressed_sizes(fixture_image(name), range(1, 100), ctx=ctx)
    assert got.dtype == np.int64 and got.shape == (99,)
    want = [-1 if v is None else v for v in e["sizes"]]
    print(name, "q1/q50/q97:", got[0], got[49], got[96])
    assert got.tolist() == want, [(q + 1, int(g), w) for q, (g, w) in enumerate(zip(got, want)) if g != w][:5]
    # any order, repeats
    qs = [97, 3, 3, 50, 99, 1]
    assert T.compressed_sizes(fixture_image(name), qs, ctx=ctx).tolist() == [want[q - 1] for q in qs]


def test_compressed_size_on_ragged_shapes(ctx, oracle):
    """compressed_size == len(compress(...)) == len(oracle.compress(...)) on 40 seeded ragged shapes at seeded qualities."""
    rng = np.random.default_rng(20261017)
    for i in range(40):
        h, w = int(rng.integers(1, 160)), int(rng.integers(1, 200))
        q = int(rng.integers(1, 98))
        if i % 3 == 0:
            img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        elif i % 3 == 1:
            img = (np.add.outer(np.arange(h) * 3, np.arange(w) * 2) % 256).astype(np.uint8)
        else:
            img = np.clip(128 + 60 * np.sin(np.add.outer(np.arange(h) / 7.0, np.arange(w) / 11.0)) + rng.normal(0, 6, (h, w)), 0, 255).astype(np.uint8)
        n = T.compressed_size(img, q, ctx=ctx)
        assert n == len(T.compress(img, q, ctx=ctx)) == len(oracle.compress(img, q)), (i, h, w, q)
    for shape in ((0, 8), (8, 0), (0, 0)):  # no blocks: the header alone, at every quality
        img = np.zeros(shape, np.uint8)
        assert T.compressed_size(img, 50, ctx=ctx) == 16 == len(T.compress(img, 50, ctx=ctx))
        bs, q = T.compress_to_size(img, 16, 5, 80, ctx=ctx)
        assert (bs, q) == (T.compress(img, 80, ctx=ctx), 80)
        with pytest.raises(ValueError, match="16 bytes"):
            T.compress_to_size(img, 15, ctx=ctx)
    with pytest.raises(KeyError):
        T.compressed_size(rand_frame(7, 256, 256), 99, ctx=ctx)


def test_entropy_size_dev_equals_the_packers_length(ctx, dev):
    """tic_entropy_size_dev on the resident coefficients of a 4096^2 frame == the out_len tic_entropy_encode_dev reports for the same
    buffer (two qualities; a ragged frame; and TIC_E_RANGE from both where a coefficient has no code)."""
    L = N.load()
    for seed, h, w, q in ((1234, 4096, 4096, 50), (1234, 4096, 4096, 90), (5, 1083, 1925, 75), (7, 256, 256, 99), (9, 8, 8, 50), (9, 24, 8, 50)):
        img = rand_frame(seed, h, w)
        nb = L.tic_num_blocks(h, w)
        d_img, d_zz = dev.upload(img), dev.alloc(nb * 128 + 16)
        ctx.check(L.tic_dctq_dev(ctx.handle, d_img, h, w, w, q, d_zz, N.KERNEL_AUTO))
        cap = L.tic_compress_bound(h, w)
        d_out = dev.alloc(cap)
        want, got = C.c_size_t(0), C.c_size_t(0)
        rc_enc = L.tic_entropy_encode_dev(ctx.handle, d_zz, h, w, q, d_out, cap, C.byref(want))
        rc = L.tic_entropy_size_dev(ctx.handle, d_zz, h, w, C.byref(got))
        print(h, w, q, "encode_dev:", rc_enc, want.value, "size_dev:", rc, got.value)
        assert rc == rc_enc == (N.TIC_E_RANGE if q == 99 else N.TIC_OK)
        if rc == N.TIC_OK:
            assert got.value == want.value
        dev.close()
    n = C.c_size_t(0)
    assert L.tic_entropy_size_dev(ctx.handle, None, 0, 8, C.byref(n)) == N.TIC_OK and n.value == 16
    assert L.tic_entropy_size_dev(ctx.handle, None, 8, 8, C.byref(n)) == N.TIC_E_ARG
    assert L.tic_entropy_size_dev(ctx.handle, None, 8, 8, None) == N.TIC_E_ARG


@pytest.mark.parametrize("name", IMAGES)
def test_compress_to_size_is_the_bisection(ctx, fx, oracle, name):
    """Budgets drawn from the recorded sizes - size(q), size(q) - 1, size(1) - 1, size(1), 10^9 - over the ranges (1, 99), (20, 60),
    (q, q): the quality of the replayed bisection, the oracle's bytes at that quality, ValueError / KeyError in the failing cases.  On
    these images sizes do not decrease with the quality (asserted), so the result is also the largest fitting quality of the range."""
    sizes = fx[name]["sizes"]
    img = fixture_image(name)
    enc = [s for s in sizes if s is not None]
    assert all(a <= b for a, b in zip(enc, enc[1:])), "recorded sizes decrease somewhere"
    assert all(s is None for s in sizes[len(enc):])
    streams = {}
    cases = 0
    for q in (1, 2, 19, 20, 33, 50, 60, 61, 90, len(enc), 98, 99):
        budgets = [sizes[0] - 1, sizes[0], 10 ** 9]
        if sizes[q - 1] is not None:
            budgets += [sizes[q - 1], sizes[q - 1] - 1]
        for budget in budgets:
            for qmin, qmax in ((1, 99), (20, 60), (q, q)):
                want = bisect(sizes, budget, qmin, qmax)
                cases += 1
                if want is ValueError:
                    with pytest.raises(ValueError, match="%d bytes at quality %d " % (sizes[qmin - 1], qmin)):
                        T.compress_to_size(img, budget, qmin, qmax, ctx=ctx)
                    continue
                if want is KeyError:
                    with pytest.raises(KeyError):
                        T.compress_to_size(img, budget, qmin, qmax, ctx=ctx)
                    continue
                bs, got = T.compress_to_size(img, budget, qmin, qmax, ctx=ctx)
                assert got == want, (name, budget, qmin, qmax, got, want)
                fitting = [k for k in range(qmin, qmax + 1) if sizes[k - 1] is not None and sizes[k - 1] <= budget]
                assert got == max(fitting)
                if got not in streams:
                    streams[got] = oracle.compress(img, got)
                assert bs == streams[got] and len(bs) == sizes[got - 1] <= budget, (name, budget, qmin, qmax, got)
    print(name, cases, "searches,", len(streams), "distinct qualities")
    assert cases >= 150


def search_dev(L, handle, d_img, h, w, budget, qmin, qmax, d_out, cap):
    n, q = C.c_size_t(0), C.c_int(-7)
    rc = L.tic_compress_to_size_dev(handle, d_img, h, w, w, budget, qmin, qmax, d_out, cap, C.byref(n), C.byref(q))
    return rc, n.value, q.value


def check_search_dev(L, handle, oracle, sizes, img):
    """tic_compress_to_size_dev into a sentinel-filled buffer: untouched on every failure, untouched past out_len on success; the host
    waits at most 8 times for the range 1..99, and tic_last_rate_search reports exactly the probes and waits of the replayed schedule."""
    h, w = img.shape
    d = Dev(L, handle)
    try:
        d_img = d.upload(img)
        cap = L.tic_compress_bound(h, w)
        d_out = d.alloc(cap + 64, SENTINEL)
        untouched = np.full(cap + 64, SENTINEL, np.uint8)
        first_null = sizes.index(None) + 1
        failures = ((sizes[0] - 1, 1, 99, cap, N.TIC_E_SPACE, sizes[0]),               # qmin too large: its size is reported
                    (10 ** 9, first_null, 99, cap, N.TIC_E_RANGE, None),                  # qmin has no code
                    (10 ** 9, 60, 20, cap, N.TIC_E_QUALITY, None), (10 ** 9, 0, 50, cap, N.TIC_E_QUALITY, None),
                    (10 ** 9, 1, 100, cap, N.TIC_E_QUALITY, None),
                    (10 ** 9, 1, 99, 15, N.TIC_E_SPACE, None),                            # cap below a header
                    (sizes[49], 1, 99, sizes[49] - 1, N.TIC_E_SPACE, sizes[49]))          # the chosen stream does not fit cap
        depth = single_frame_depth(L.tic_num_blocks(h, w))
        probes, waits = C.c_int(0), C.c_int(0)
        for budget, qmin, qmax, c, want_rc, want_len in failures + ((sizes[0] - 1, 1, 1, cap, N.TIC_E_SPACE, sizes[0]),):
            rc, n, q = search_dev(L, handle, d_img, h, w, budget, qmin, qmax, d_out, c)
            assert rc == want_rc, (budget, qmin, qmax, c, rc)
            assert want_len is None or n == want_len
            assert np.array_equal(d.download(d_out, cap + 64), untouched), (budget, qmin, qmax, c)
            if c == cap and want_rc in (N.TIC_E_SPACE, N.TIC_E_RANGE):  # the failing first probe: its round (qmin and the middles), no stream
                assert L.tic_last_rate_search(handle, C.byref(probes), C.byref(waits)) == 0
                print("budget", budget, "range", qmin, qmax, "fails; probes", probes.value, "host waits", waits.value)
                assert (probes.value, waits.value) == schedule(sizes, budget, qmin, qmax, depth) and waits.value == 1
                if qmin == qmax:
                    assert (probes.value, waits.value) == (1, 1)
        for budget, qmin, qmax, c in ((sizes[49], 1, 99, cap), (sizes[49], 1, 99, sizes[49]), (sizes[29] - 1, 1, 99, cap), (10 ** 9, 1, 99, cap),
                                      (sizes[39], 20, 60, cap), (sizes[0], 1, 1, cap)):
            assert L.tic_memset_dev(handle, d_out, SENTINEL, cap + 64) == 0
            rc, n, q = search_dev(L, handle, d_img, h, w, budget, qmin, qmax, d_out, c)
            want = bisect(sizes, budget, qmin, qmax)
            assert (rc, q, n) == (N.TIC_OK, want, sizes[want - 1]), (budget, qmin, qmax, rc, q, n)
            got = d.download(d_out, cap + 64)
            assert got[:n].tobytes() == oracle.compress(img, q)
            assert np.array_equal(got[n:], untouched[n:]), "bytes behind the stream were written"
            assert L.tic_last_rate_search(handle, C.byref(probes), C.byref(waits)) == 0
            print("budget", budget, "range", qmin, qmax, "-> q", q, n, "bytes; probes", probes.value, "host waits", waits.value)
            assert 1 <= waits.value <= 8 and waits.value <= probes.value + 1 and probes.value <= 99
            if qmin == qmax:
                assert (probes.value, waits.value) == (1, 2)
            assert (probes.value, waits.value) == schedule(sizes, budget, qmin, qmax, depth), (budget, qmin, qmax)
    finally:
        d.close()


def test_search_dev_writes_nothing_it_should_not(ctx, fx, oracle):
    for name in ("lenna", "bench06_crop203x317"):
        check_search_dev(N.load(), ctx.handle, oracle, fx[name]["sizes"], fixture_image(name))


def test_search_dev_waits_on_a_large_frame(ctx, dev):
    """Range 1..99 on a 4096^2 frame (the look-ahead is shallower there): still at most 8 host waits, and the stream is tic_compress_dev's."""
    L = N.load()
    img = rand_frame(1234, 4096, 4096)
    d_img = dev.upload(img)
    cap = L.tic_compress_bound(4096, 4096)
    d_out, d_ref = dev.alloc(cap), dev.alloc(cap)
    qs = (C.c_int * 3)(20, 50, 80)
    sz = (C.c_longlong * 3)()
    ctx.check(L.tic_stream_sizes_dev(ctx.handle, d_img, 4096, 4096, 4096, qs, 3, sz))
    budget = sz[1]
    rc, n, q = search_dev(L, ctx.handle, d_img, 4096, 4096, budget, 1, 99, d_out, cap)
    probes, waits = C.c_int(0), C.c_int(0)
    assert L.tic_last_rate_search(ctx.handle, C.byref(probes), C.byref(waits)) == 0
    print("4096^2: q", q, n, "bytes; probes", probes.value, "host waits", waits.value, "sizes at 20/50/80:", list(sz))
    assert rc == N.TIC_OK and n <= budget and q >= 50 and waits.value <= 8
    want = C.c_size_t(0)
    ctx.check(L.tic_compress_dev(ctx.handle, d_img, 4096, 4096, 4096, q, d_ref, cap, C.byref(want)))
    assert want.value == n and np.array_equal(dev.download(d_out, n), dev.download(d_ref, n))
    if q < 99:  # the next quality does not fit (sizes of noise grow with the quality)
        nxt = (C.c_int * 1)(q + 1)
        ctx.check(L.tic_stream_sizes_dev(ctx.handle, d_img, 4096, 4096, 4096, nxt, 1, sz))
        assert sz[0] < 0 or sz[0] > budget


def test_search_dev_at_depth_two(ctx, dev):
    """A 1024 x 1032 frame has 16512 blocks, just past the 16384 up to which a single-frame search looks three steps ahead - and far below
    the 131072 at which the batch search's rate_depth leaves three: the one size at which the two depths disagree.  Range 1..99, the budget
    its own size at q = 50: the counters are the replay's at depth 2 (not at depth 3) on the sizes of one tic_stream_sizes_dev call, the
    stream is tic_compress_dev's at the quality found."""
    L = N.load()
    h, w = 1024, 1032
    assert L.tic_num_blocks(h, w) == 16512 and single_frame_depth(16512) == 2 and single_frame_depth(16384) == 3
    d_img = dev.upload(rand_frame(1234, h, w))
    cap = L.tic_compress_bound(h, w)
    d_out, d_ref = dev.alloc(cap), dev.alloc(cap)
    qs, sz = (C.c_int * 99)(*range(1, 100)), (C.c_longlong * 99)()
    ctx.check(L.tic_stream_sizes_dev(ctx.handle, d_img, h, w, w, qs, 99, sz))
    sizes = [None if v < 0 else v for v in sz]
    budget = sizes[49]
    want = bisect(sizes, budget, 1, 99)
    rc, n, q = search_dev(L, ctx.handle, d_img, h, w, budget, 1, 99, d_out, cap)
    probes, waits = C.c_int(0), C.c_int(0)
    assert L.tic_last_rate_search(ctx.handle, C.byref(probes), C.byref(waits)) == 0
    two, three = schedule(sizes, budget, 1, 99, 2), schedule(sizes, budget, 1, 99, 3)
    print("1024x1032: q", q, n, "bytes; probes", probes.value, "host waits", waits.value, "replay at depth 2:", two, "at depth 3:", three)
    assert (rc, q, n) == (N.TIC_OK, want, sizes[want - 1])
    assert two != three and (probes.value, waits.value) == two
    ref = C.c_size_t(0)
    ctx.check(L.tic_compress_dev(ctx.handle, d_img, h, w, w, q, d_ref, cap, C.byref(ref)))
    assert ref.value == n and np.array_equal(dev.download(d_out, n), dev.download(d_ref, n))


def test_stream_sizes_dev_produces_no_stream(ctx, dev, fx):
    """The d_out of an earlier tic_compress_dev is unchanged by tic_stream_sizes_dev; its sizes are that call's out_len; a bad quality
    fails with TIC_E_QUALITY before anything runs (the results stay as they were)."""
    L = N.load()
    img = fixture_image("lenna")
    sizes = fx["lenna"]["sizes"]
    d_img = dev.upload(img)
    cap = L.tic_compress_bound(512, 512)
    d_out = dev.alloc(cap, SENTINEL)
    n = C.c_size_t(0)
    ctx.check(L.tic_compress_dev(ctx.handle, d_img, 512, 512, 512, 40, d_out, cap, C.byref(n)))
    before = dev.download(d_out, cap)
    qs = (C.c_int * 5)(40, 1, 99, 97, 40)
    sz = (C.c_longlong * 5)(*([-5] * 5))
    ctx.check(L.tic_stream_sizes_dev(ctx.handle, d_img, 512, 512, 512, qs, 5, sz))
    assert list(sz) == [n.value, sizes[0], -1, sizes[96], n.value] and n.value == sizes[39]
    assert np.array_equal(dev.download(d_out, cap), before)
    for bad in (0, 100, -1):
        qs = (C.c_int * 3)(40, bad, 50)
        sz = (C.c_longlong * 3)(-5, -5, -5)
        assert L.tic_stream_sizes_dev(ctx.handle, d_img, 512, 512, 512, qs, 3, sz) == N.TIC_E_QUALITY
        assert list(sz) == [-5, -5, -5]
    assert L.tic_stream_sizes_dev(ctx.handle, None, 512, 512, 512, qs, 1, sz) == N.TIC_E_ARG
    assert L.tic_stream_sizes_dev(ctx.handle, d_img, 512, 512, 512, None, 1, sz) == N.TIC_E_ARG
    assert L.tic_stream_sizes_dev(ctx.handle, d_img, 512, 512, 512, qs, 0, sz) == N.TIC_OK


def test_cli_max_bytes(ctx, fx, tmp_path, capsys):
    """encode_cli --max-bytes: the bytes of compress_to_size, the chosen quality as a third line; not together with --scaled / --quality."""
    from tinyimgcodec_amd import encode_cli as cli

    img = fixture_image("lenna")
    src, dst = tmp_path / "lenna.npy", tmp_path / "out.img"
    np.save(src, img)
    assert cli.main([str(src), str(dst), "--max-bytes", "20000"]) == 0
    out = capsys.readouterr().out.splitlines()
    bs, q = T.compress_to_size(img, 20000, ctx=ctx)
    assert q == bisect(fx["lenna"]["sizes"], 20000, 1, 99)
    assert dst.read_bytes() == bs
    assert out == [f"{len(bs)} bytes", f"Compression Ratio: {512 * 512 / len(bs)}:1", f"Quality: {q}"]
    assert cli.main([str(src), str(dst), "--max-bytes", "20000", "--min-quality", "10", "--max-quality", "30"]) == 0
    assert capsys.readouterr().out.splitlines()[2] == "Quality: 30" and dst.read_bytes() == T.compress(img, 30, ctx=ctx)
    for extra in (["--scaled", "med"], ["--quality", "50"]):
        with pytest.raises(SystemExit):
            cli.main([str(src), str(dst), "--max-bytes", "20000"] + extra)
    with pytest.raises(SystemExit):
        cli.main([str(src), str(dst), "--min-quality", "10"])
    capsys.readouterr()


def test_shipped_library(fx, oracle):
    """The same through the library that ships (no test hooks compiled in), bound here beside the test-hooks build this process runs:
    all 99 sizes of two fixture images from tic_stream_sizes, and the sentinel / bisection checks of tic_compress_to_size_dev."""
    assert N.load().tic_build_has_test_hooks() == 1
    L = C.CDLL(N.LIB_PATH)
    for fn, (res, args) in N.SIGNATURES.items():
        f = getattr(L, fn)
        f.restype, f.argtypes = res, args
    assert L.tic_build_has_test_hooks() == 0
    handle = L.tic_create(0)
    assert handle, L.tic_last_error(None)
    try:
        for name in ("lenna", "noise256_seed7"):
            img = fixture_image(name)
            sizes = fx[name]["sizes"]
            qs = (C.c_int * 99)(*range(1, 100))
            sz = (C.c_longlong * 99)()
            assert L.tic_stream_sizes(handle, img.ctypes.data, img.shape[0], img.shape[1], img.strides[0], qs, 99, sz) == 0
            assert list(sz) == [-1 if v is None else v for v in sizes]
            check_search_dev(L, handle, oracle, sizes, img)
            out = np.full(sizes[49] + 8, SENTINEL, np.uint8)
            n, q = C.c_size_t(0), C.c_int(0)
            assert L.tic_compress_to_size(handle, img.ctypes.data, img.shape[0], img.shape[1], img.strides[0], sizes[49], 1, 99, out.ctypes.data,
                                          sizes[49], C.byref(n), C.byref(q)) == 0
            assert q.value == bisect(sizes, sizes[49], 1, 99) and out[: n.value].tobytes() == oracle.compress(img, q.value)
            assert (out[n.value:] == SENTINEL).all()
    finally:
        L.tic_destroy(handle)
