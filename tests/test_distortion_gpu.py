"""Rate-distortion on the GPU: rd_points / roundtrip_psnr / compress_to_psnr / roundtrip_sse_scaled and the C-ABI under them, against the
round-trip errors recorded from the unmodified reference (tests/golden/distortion.json), the oracle's round trip (tied to that record by
tests/test_distortion_cpu.py) and a Python replay of the bisection that is the search's contract.  Every comparison is an integer equality
or a float identity.  Each test runs on the test-hooks build and repeats one call on the library that ships."""
import ctypes as C
import math

import numpy as np
import pytest

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

import inverse_edges as IE
from conftest import rand_frame
from distortion_common import SETTINGS, load_distortion, oracle_sums, scaled_image, sums
from test_rate_control_cpu import IMAGES, fixture_image, load_fixture
from test_rate_control_gpu import Dev
from test_rate_control_gpu import bisect as bisect_size
from test_rate_control_gpu import single_frame_depth

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def shipped():
    """(library, context handle) of the build that ships (no test hooks compiled in), bound beside the test-hooks build this process runs."""
    assert N.load().tic_build_has_test_hooks() == 1
    L = C.CDLL(N.LIB_PATH)
    for fn, (res, args) in N.SIGNATURES.items():
        f = getattr(L, fn)
        f.restype, f.argtypes = res, args
    assert L.tic_build_has_test_hooks() == 0
    handle = L.tic_create(0)
    assert handle, L.tic_last_error(None)
    yield L, handle
    L.tic_destroy(handle)


@pytest.fixture(scope="module")
def fx():
    return load_distortion()


@pytest.fixture(scope="module")
def rate():
    return load_fixture()["images"]


def rd_raw(L, handle, img, qs, d_img=None, stride=None):
    """tic_rd_points (host image) or tic_rd_points_dev (d_img, stride) -> three lists."""
    h, w = img.shape
    qa = (C.c_int * len(qs))(*qs)
    sz = (C.c_longlong * len(qs))(*([-5] * len(qs)))
    a, b = (C.c_uint64 * len(qs))(), (C.c_uint64 * len(qs))()
    if d_img is None:
        rc = L.tic_rd_points(handle, img.ctypes.data, h, w, img.strides[0], qa, len(qs), sz, a, b)
    else:
        rc = L.tic_rd_points_dev(handle, d_img, h, w, stride, qa, len(qs), sz, a, b)
    assert rc == N.TIC_OK, (rc, L.tic_last_error(handle).decode())
    return list(sz), list(a), list(b)


def oracle_size(oracle, img, q):
    try:
        return len(oracle.compress(img, q))
    except oracle.OracleError:
        return -1


def bisect_psnr(sse, max_sse, qmin, qmax):
    """The contract, replayed on recorded errors (index q - 1; None = no code): the quality the search must return, or the exception."""
    def meets(q):
        return sse[q - 1] is not None and sse[q - 1] <= max_sse

    if not meets(qmax):
        return KeyError if sse[qmax - 1] is None else ValueError
    lo, hi = qmin, qmax
    while lo < hi:
        mid = (lo + hi) // 2
        if meets(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo


def schedule_psnr(sse, max_sse, qmin, qmax, depth):
    """The documented schedule of tic_compress_to_psnr, replayed on errors (index q - 1; None = no code): (probes, host waits) - the mirror
    of test_rate_control_gpu.schedule.  A round probes every middle the bisection can reach within `depth` further steps and has not
    probed yet - the first round qmax as well - behind one wait; then the bisection goes as far as the probed errors carry it.  The stream
    is one more wait; a qmax that does not meet the bound ends the search after the first round, without a stream."""
    def meets(q):
        return sse[q - 1] is not None and sse[q - 1] <= max_sse

    def middles(lo, hi, d, out):
        if lo < hi and d > 0:
            mid = (lo + hi) // 2
            if mid not in probed:
                out.append(mid)
            middles(lo, mid, d - 1, out)
            middles(mid + 1, hi, d - 1, out)

    probed, rounds = set(), 0
    lo, hi = qmin, qmax
    while True:
        cand = [] if rounds else [qmax]
        middles(lo, hi, depth, cand)
        assert len(cand) == len(set(cand))
        if not cand:
            return len(probed), rounds + 1
        probed.update(cand)
        rounds += 1
        if not meets(qmax):
            return len(probed), rounds
        while lo < hi and (lo + hi) // 2 in probed:
            mid = (lo + hi) // 2
            if meets(mid):
                hi = mid
            else:
                lo = mid + 1


@pytest.mark.parametrize("name", IMAGES)
def test_rd_points_equal_the_fixture(ctx, shipped, fx, rate, oracle, name):
    """All 99 qualities in one call: the reference's stream length and its two error sums; -1 where the reference raises KeyError, with
    the sums the oracle's decode of those coefficients gives."""
    e = fx["images"][name]
    img = fixture_image(name)
    sizes, sse, wrapped = T.rd_points(img, range(1, 100), ctx=ctx)
    assert (sizes.dtype, sse.dtype, wrapped.dtype) == (np.int64, np.uint64, np.uint64) and sizes.shape == sse.shape == wrapped.shape == (99,)
    want_sizes = [-1 if v is None else v for v in rate[name]["sizes"]]
    want = [(e["sse"][q - 1], e["sse_wrapped"][q - 1]) if e["sse"][q - 1] is not None else oracle_sums(oracle, img, q) for q in range(1, 100)]
    print(name, "q1/q50/q99:", [(int(sizes[q]), int(sse[q]), int(wrapped[q])) for q in (0, 49, 98)])
    got = list(zip(sse.tolist(), wrapped.tolist()))
    assert got == want, [(q + 1, g, x) for q, (g, x) in enumerate(zip(got, want)) if g != x][:5]
    assert sizes.tolist() == want_sizes, [(q + 1, int(g), x) for q, (g, x) in enumerate(zip(sizes, want_sizes)) if g != x][:5]
    assert want_sizes[98] == -1 and want[98][0] > 0
    # any order, repeats; and the PSNR of one quality, both arithmetics
    qs = [97, 3, 3, 50, 99, 1]
    s2, a2, b2 = T.rd_points(img, qs, ctx=ctx)
    assert (s2.tolist(), list(zip(a2.tolist(), b2.tolist()))) == ([want_sizes[q - 1] for q in qs], [want[q - 1] for q in qs])
    assert T.roundtrip_psnr(img, 50, ctx=ctx) == T.psnr_from_sse(e["sse"][49], img.size)
    assert T.roundtrip_psnr(img, 50, reference_arithmetic=True, ctx=ctx) == e["psnr_ref"][49]
    with pytest.raises(KeyError):
        T.roundtrip_psnr(img, 99, ctx=ctx)
    L, handle = shipped
    assert rd_raw(L, handle, img, [1, 50, 97, 99]) == ([want_sizes[q - 1] for q in (1, 50, 97, 99)], [want[q - 1][0] for q in (1, 50, 97, 99)],
                                                      [want[q - 1][1] for q in (1, 50, 97, 99)])


def test_ragged_and_tiny_frames(ctx, shipped, oracle):
    """1x1 ... 203x317 crops of the fixture's ragged image, expectations from the oracle's round trip; the 13x21 frame also as a device
    image with row stride 37 (no row 8-byte aligned) and 24 (aligned rows, a last block that is not whole), padding filled with 255: a
    counted padding pixel or an 8-byte load where bytes are due shows in the sums."""
    base = fixture_image("bench06_crop203x317")
    L = N.load()
    qs = [1, 50, 90, 97]
    for h, w in ((1, 1), (7, 9), (8, 8), (13, 21), (64, 72), (203, 317)):
        img = np.ascontiguousarray(base[:h, :w])
        want = [oracle_sums(oracle, img, q) for q in qs]
        sizes, sse, wrapped = T.rd_points(img, qs, ctx=ctx)
        print((h, w), list(zip(sizes.tolist(), sse.tolist())))
        assert list(zip(sse.tolist(), wrapped.tolist())) == want, (h, w)
        assert sizes.tolist() == [oracle_size(oracle, img, q) for q in qs], (h, w)
    img = np.ascontiguousarray(base[:13, :21])
    want = [oracle_sums(oracle, img, q) for q in qs]
    for lib, handle in ((L, ctx.handle), shipped):
        d = Dev(lib, handle)
        try:
            for stride in (37, 24):
                padded = np.full((13, stride), 255, np.uint8)
                padded[:, :21] = img
                got = rd_raw(lib, handle, img, qs, d.upload(padded), stride)
                assert list(zip(got[1], got[2])) == want, stride
                assert got[0] == [oracle_size(oracle, img, q) for q in qs]
        finally:
            d.close()


def test_tile_count_not_a_multiple_of_a_workgroup(ctx, shipped, oracle):
    """72 x 136: 9 block rows of 3 strips of 8 blocks (the last strip holds one block) = 27 strips, four per workgroup: the last
    workgroup has a wave without a strip.  88 x 8: 11 strips of one block."""
    for seed, h, w in ((31, 72, 136), (32, 88, 8)):
        ntiles = ((h + 7) // 8) * (((w + 7) // 8 + 7) // 8)
        assert ntiles % 4 != 0
        img = rand_frame(seed, h, w)
        want = [oracle_sums(oracle, img, q) for q in (5, 60)]
        for lib, handle in ((N.load(), ctx.handle), shipped):
            got = rd_raw(lib, handle, img, [5, 60])
            assert list(zip(got[1], got[2])) == want, (h, w)


def test_flat_and_wide_sums(ctx, shipped, oracle):
    """A flat 128 frame decodes to itself: sums 0, PSNR inf.  2048 x 1024 noise at quality 1: a true sum above 2^32 (asserted on the
    oracle's number first) - 32-bit accumulation anywhere behind a workgroup would show."""
    flat = np.full((40, 56), 128, np.uint8)
    sizes, sse, wrapped = T.rd_points(flat, [1, 50, 97], ctx=ctx)
    assert sse.tolist() == wrapped.tolist() == [0, 0, 0] and (sizes > 16).all()
    assert T.roundtrip_psnr(flat, 50, ctx=ctx) == math.inf == T.roundtrip_psnr(flat, 50, reference_arithmetic=True, ctx=ctx)
    bs, q, p = T.compress_to_psnr(flat, math.inf, 1, 97, ctx=ctx)
    assert (bs, q, p) == (T.compress(flat, 1, ctx=ctx), 1, math.inf)
    img = rand_frame(2026, 2048, 1024)
    want = oracle_sums(oracle, img, 1)
    print("2048 x 1024 noise, q = 1: sse", want[0], "wrapped", want[1])
    assert want[0] > 2 ** 32
    sizes, sse, wrapped = T.rd_points(img, [1], ctx=ctx)
    assert (int(sse[0]), int(wrapped[0])) == want
    assert sizes[0] == len(oracle.compress(img, 1))
    L, handle = shipped
    got = rd_raw(L, handle, img, [1])
    assert (got[1][0], got[2][0]) == want


def distortion_dev(L, handle, d_zz, d_img, h, w, stride, quality, exponent):
    out = (C.c_uint64 * 2)(7, 7)
    rc = L.tic_distortion_dev(handle, d_zz, d_img, h, w, stride, quality, exponent, out)
    return rc, (out[0], out[1])


def test_distortion_dev_alone(ctx, shipped, oracle):
    """tic_distortion_dev on coefficients no encoder made (frames of inverse_edges.npz whose running DC fits int16) against an unrelated
    image: the sums computed from the reference's pixels of those coefficients (the oracle's block route, checked against the fixture's
    digest and crops).  A ragged frame, a non-integral quality through the custom slot, a scaled frame at exponent 3; image rows with a
    stride of their own, padding 255; both device buffers unchanged afterwards."""
    ie = IE.Fixture()
    L = N.load()
    for name in ("ragged_q50", "clip_q10", "scaled_e3", "sparse_q37_5"):
        e = ie.frames[name]
        h, w, q = e["height"], e["width"], e["quality"]
        if name == "sparse_q37_5":  # (4,096 blocks through a Python loop: the top 64 rows of blocks do)
            h = 64
        dc, ac = ie.coeffs(name)
        zz = IE.zz_absolute(dc, ac)[: ((h + 7) // 8) * ((w + 7) // 8)]
        assert np.abs(zz).max() <= 32767
        ref = IE.pixels_block_idct(ie, oracle, zz, h, w, q, e["flag"])
        if h == e["height"]:
            assert ie.matches_reference(name, ref), name
        else:
            assert np.array_equal(ref[:64, :64], ie.crops(name)[0]), name
        scaled = bool(e["flag"] & IE.SCALED)
        assert (name == "scaled_e3") == scaled and (not scaled or q == 3)
        stride = w + 13 if name == "ragged_q50" else w + 8
        orig = np.full((h, stride), 255, np.uint8)
        orig[:, :w] = rand_frame(len(name), h, w)
        want = sums(np.ascontiguousarray(orig[:, :w]), ref)
        zz16 = np.ascontiguousarray(zz.astype(np.int16))
        for lib, handle in ((L, ctx.handle), shipped) if name == "ragged_q50" else ((L, ctx.handle),):  # (the shipped library: one frame)
            d = Dev(lib, handle)
            try:
                d_zz, d_img = d.upload(zz16), d.upload(orig)
                if scaled:
                    quality, exponent = 0, int(q)
                elif float(q) != int(q):
                    assert lib.tic_set_custom_quality(handle, float(q)) == N.TIC_OK
                    quality, exponent = N.QUALITY_CUSTOM, -1
                else:
                    quality, exponent = int(q), -1
                rc, got = distortion_dev(lib, handle, d_zz, d_img, h, w, stride, quality, exponent)
                print(name, (h, w), "stride", stride, "->", rc, got)
                assert rc == N.TIC_OK and got == want, (name, got, want)
                assert np.array_equal(d.download(d_zz, zz16.nbytes), zz16.view(np.uint8).ravel())
                assert np.array_equal(d.download(d_img, orig.nbytes), orig.ravel())
                ms = C.c_float(-1.0)
                assert lib.tic_distortion_dev_timed(handle, d_zz, d_img, h, w, stride, quality, exponent, 1, 2, C.byref(ms)) == N.TIC_OK and ms.value > 0
                # idct_kernel timed the same way writes the reference's pixels, rows cropped to w
                d_px = d.alloc(h * stride, SENTINEL)
                ms = C.c_float(-1.0)
                assert lib.tic_idct_dev_timed(handle, d_zz, d_px, h, w, stride, quality, exponent, 1, 2, C.byref(ms)) == N.TIC_OK and ms.value > 0
                px = d.download(d_px, h * stride).reshape(h, stride)
                assert np.array_equal(px[:, :w], ref) and (px[:, w:] == SENTINEL).all(), name
            finally:
                d.close()
    # arguments
    d = Dev(L, ctx.handle)
    try:
        buf = d.alloc(4096)
        out = (C.c_uint64 * 2)(7, 7)
        assert distortion_dev(L, ctx.handle, None, None, 0, 8, 8, 50, -1) == (N.TIC_OK, (0, 0))
        assert L.tic_distortion_dev(ctx.handle, buf, buf, 8, 8, 8, 50, -1, None) == N.TIC_E_ARG
        for args, want_rc in (((None, buf, 8, 8, 8, 50, -1), N.TIC_E_ARG), ((buf, None, 8, 8, 8, 50, -1), N.TIC_E_ARG),
                              ((buf, buf, -1, 8, 8, 50, -1), N.TIC_E_ARG), ((buf, buf, 8, 8, 7, 50, -1), N.TIC_E_ARG),
                              ((buf, buf, 8, 8, 8, 100, -1), N.TIC_E_QUALITY), ((buf, buf, 8, 8, 8, 50, 63), N.TIC_E_QUALITY)):
            assert L.tic_distortion_dev(ctx.handle, *args, out) == want_rc, args
        assert L.tic_distortion_dev(ctx.handle, buf, buf, 8, 8, 8, 100, 5, out) == N.TIC_OK  # (the quality is ignored on the scaled branch)
    finally:
        d.close()


def search_dev(L, handle, d_img, h, w, max_sse, qmin, qmax, d_out, cap):
    n, q, s = C.c_size_t(0), C.c_int(-7), C.c_uint64(7)
    rc = L.tic_compress_to_psnr_dev(handle, d_img, h, w, w, max_sse, qmin, qmax, d_out, cap, C.byref(n), C.byref(q), C.byref(s))
    return rc, n.value, q.value, s.value


@pytest.mark.parametrize("name", ("lenna", "bench06_crop203x317", "noise256_seed7"))
def test_compress_to_psnr_is_the_bisection(ctx, shipped, fx, rate, name):
    """Targets on, one ulp above and one ulp below the true PSNR of several rows, over 1..97, 1..99 (whose upper end has no code on these
    images: KeyError), a sub-range and (q, q): the quality of the replayed bisection, compress()'s bytes at that quality, psnr_from_sse of
    the recorded error; ValueError naming the PSNR at max_quality when the target is out of reach.  On these images the error does not
    grow with the quality (asserted), so the result is also the smallest quality of the range that meets the target."""
    e = fx["images"][name]
    sse = e["sse"]
    img = fixture_image(name)
    n = img.size
    enc = [s for s in sse if s is not None]
    assert all(a >= b for a, b in zip(enc, enc[1:])), "the recorded error grows somewhere"
    streams = {}
    cases = 0
    for q in (1, 2, 20, 33, 50, 60, 61, 90, 97):
        p = T.psnr_from_sse(sse[q - 1], n)
        for target in (p, math.nextafter(p, math.inf), math.nextafter(p, -math.inf)):
            max_sse = T.max_sse_for_psnr(target, n)
            for qmin, qmax in ((1, 97), (1, 99), (20, 60), (q, q)):
                want = bisect_psnr(sse, max_sse, qmin, qmax)
                cases += 1
                if want is KeyError:
                    with pytest.raises(KeyError):
                        T.compress_to_psnr(img, target, qmin, qmax, ctx=ctx)
                    continue
                if want is ValueError:
                    with pytest.raises(ValueError, match="%s dB at quality %d " % (repr(T.psnr_from_sse(sse[qmax - 1], n)).replace(".", r"\."), qmax)):
                        T.compress_to_psnr(img, target, qmin, qmax, ctx=ctx)
                    continue
                bs, got, psnr = T.compress_to_psnr(img, target, qmin, qmax, ctx=ctx)
                assert got == want, (name, target, qmin, qmax, got, want)
                assert got == min(k for k in range(qmin, qmax + 1) if sse[k - 1] is not None and sse[k - 1] <= max_sse)
                assert psnr == T.psnr_from_sse(sse[got - 1], n) and psnr >= target
                if got not in streams:
                    streams[got] = T.compress(img, got, ctx=ctx)
                assert bs == streams[got] and len(bs) == rate[name]["sizes"][got - 1], (name, target, qmin, qmax, got)
    print(name, cases, "searches,", len(streams), "distinct qualities")
    assert cases == 108 and len(streams) >= 8
    with pytest.raises(ValueError, match="fall short of min_psnr"):
        T.compress_to_psnr(img, math.inf, 1, 97, ctx=ctx)
    L, handle = shipped
    buf = np.empty(L.tic_compress_bound(*img.shape), np.uint8)
    nb, qq, ss = C.c_size_t(0), C.c_int(0), C.c_uint64(0)
    assert L.tic_compress_to_psnr(handle, img.ctypes.data, img.shape[0], img.shape[1], img.strides[0], sse[32], 20, 60, buf.ctypes.data, buf.size,
                                  C.byref(nb), C.byref(qq), C.byref(ss)) == N.TIC_OK
    want = bisect_psnr(sse, sse[32], 20, 60)
    assert (qq.value, ss.value) == (want, sse[want - 1]) and buf[: nb.value].tobytes() == T.compress(img, want, ctx=ctx)


def check_search_dev(L, handle, oracle, sse, sizes, img):
    """tic_compress_to_psnr_dev into a sentinel-filled buffer: untouched on every failure, untouched past out_len on success; quality and
    error reported with TIC_E_SPACE / TIC_E_RANGE; fewer host waits than probes over 1..97, and tic_last_rate_search reports exactly the
    probes and waits of the replayed schedule."""
    h, w = img.shape
    d = Dev(L, handle)
    try:
        d_img = d.upload(img)
        cap = L.tic_compress_bound(h, w)
        d_out = d.alloc(cap + 64, SENTINEL)
        untouched = np.full(cap + 64, SENTINEL, np.uint8)
        failures = ((sse[96] - 1, 1, 97, cap, N.TIC_E_SPACE, 97, sse[96]),       # out of reach: quality and error of qmax are reported
                    (0, 30, 60, cap, N.TIC_E_SPACE, 60, sse[59]),
                    (2 ** 63, 1, 99, cap, N.TIC_E_RANGE, 99, None),              # qmax has no code
                    (2 ** 63, 60, 20, cap, N.TIC_E_QUALITY, -7, 7), (2 ** 63, 0, 50, cap, N.TIC_E_QUALITY, -7, 7),
                    (2 ** 63, 1, 100, cap, N.TIC_E_QUALITY, -7, 7),
                    (2 ** 63, 1, 97, 15, N.TIC_E_SPACE, -7, 7),                  # cap below a header
                    (sse[49], 1, 97, sizes[49] - 1, N.TIC_E_SPACE, None, None))  # the chosen stream does not fit cap
        depth = single_frame_depth(L.tic_num_blocks(h, w))
        probes, waits = C.c_int(0), C.c_int(0)
        for max_sse, qmin, qmax, c, want_rc, want_q, want_sse in failures:
            rc, n, q, s = search_dev(L, handle, d_img, h, w, max_sse, qmin, qmax, d_out, c)
            assert rc == want_rc, (max_sse, qmin, qmax, c, rc)
            if c == cap and want_rc in (N.TIC_E_SPACE, N.TIC_E_RANGE):  # the failing first probe: its round (qmax and the middles), no stream
                assert L.tic_last_rate_search(handle, C.byref(probes), C.byref(waits)) == 0
                print("max_sse", max_sse, "range", qmin, qmax, "fails; probes", probes.value, "host waits", waits.value)
                assert (probes.value, waits.value) == schedule_psnr(sse, max_sse, qmin, qmax, depth) and waits.value == 1
            assert (want_q is None or q == want_q) and (want_sse is None or s == want_sse), (max_sse, qmin, qmax, q, s)
            if want_rc == N.TIC_E_SPACE and want_q is not None and want_q > 0:
                assert n == 0  # (what tells "out of reach" from "does not fit cap", which reports the stream's length)
            assert np.array_equal(d.download(d_out, cap + 64), untouched), (max_sse, qmin, qmax, c)
        assert n == sizes[49]  # (the last failure reports the length that did not fit)
        for max_sse, qmin, qmax, c in ((sse[49], 1, 97, cap), (sse[49], 1, 97, sizes[49]), (sse[29] - 1, 1, 97, cap), (2 ** 63, 1, 97, cap),
                                       (sse[39], 20, 60, cap), (sse[96], 97, 97, cap)):
            assert L.tic_memset_dev(handle, d_out, SENTINEL, cap + 64) == 0
            rc, n, q, s = search_dev(L, handle, d_img, h, w, max_sse, qmin, qmax, d_out, c)
            want = bisect_psnr(sse, max_sse, qmin, qmax)
            assert (rc, q, n, s) == (N.TIC_OK, want, sizes[want - 1], sse[want - 1]), (max_sse, qmin, qmax, rc, q, n, s)
            got = d.download(d_out, cap + 64)
            assert got[:n].tobytes() == oracle.compress(img, q)
            assert np.array_equal(got[n:], untouched[n:]), "bytes behind the stream were written"
            assert L.tic_last_rate_search(handle, C.byref(probes), C.byref(waits)) == 0
            print("max_sse", max_sse, "range", qmin, qmax, "-> q", q, n, "bytes; probes", probes.value, "host waits", waits.value)
            assert 1 <= waits.value <= 8 and waits.value <= probes.value + 1 and probes.value <= 99
            if qmin == qmax:
                assert (probes.value, waits.value) == (1, 2)
            elif (qmin, qmax) == (1, 97) and h * w >= 512 * 512:
                assert waits.value < probes.value
            assert (probes.value, waits.value) == schedule_psnr(sse, max_sse, qmin, qmax, depth), (max_sse, qmin, qmax)
    finally:
        d.close()


def test_search_dev_writes_nothing_it_should_not(ctx, shipped, fx, rate, oracle):
    for name in ("lenna", "bench06_crop203x317"):
        check_search_dev(N.load(), ctx.handle, oracle, fx["images"][name]["sse"], rate[name]["sizes"], fixture_image(name))
    L, handle = shipped
    check_search_dev(L, handle, oracle, fx["images"]["lenna"]["sse"], rate["lenna"]["sizes"], fixture_image("lenna"))
    # no blocks: the header at qmin, no error
    out = np.full(32, SENTINEL, np.uint8)
    n, q, s = C.c_size_t(0), C.c_int(-7), C.c_uint64(7)
    assert L.tic_compress_to_psnr(handle, None, 0, 8, 8, 0, 5, 80, out.ctypes.data, 32, C.byref(n), C.byref(q), C.byref(s)) == N.TIC_OK
    assert (n.value, q.value, s.value) == (16, 5, 0) and out[:16].tobytes() == oracle.compress(np.zeros((0, 8), np.uint8), 5) and (out[16:] == SENTINEL).all()
    assert T.compress_to_psnr(np.zeros((0, 8), np.uint8), 40.0, 5, 80, ctx=ctx) == (T.compress(np.zeros((0, 8), np.uint8), 5, ctx=ctx), 5, math.inf)


def test_roundtrip_sse_scaled_equals_the_fixture(ctx, shipped, fx):
    """The distortion column of the reference's C benchmark: three images, four settings, both sums; the reference's own PSNR from the
    wrapped one."""
    rows = 0
    for name, e in fx["scaled"].items():
        img = scaled_image(name)
        for setting in SETTINGS:
            r = e["settings"][setting]
            got = T.roundtrip_sse_scaled(img, setting, ctx=ctx)
            print(name, setting, got, T.psnr_from_sse(got[0], img.size))
            assert got == (r["sse"], r["sse_wrapped"]), (name, setting)
            assert T.psnr_from_sse(got[1], img.size) == r["psnr_ref"]
            rows += 1
    assert rows == 12
    L, handle = shipped
    img = scaled_image("bench47")
    out = (C.c_uint64 * 2)()
    assert L.tic_roundtrip_sse_scaled(handle, img.ctypes.data, 512, 512, 512, N.SCALED_LOW, out) == N.TIC_OK
    assert (out[0], out[1]) == (fx["scaled"]["bench47"]["settings"]["low"]["sse"], fx["scaled"]["bench47"]["settings"]["low"]["sse_wrapped"])
    assert L.tic_roundtrip_sse_scaled(handle, img.ctypes.data, 512, 512, 512, 4, out) == N.TIC_E_QUALITY
    assert L.tic_roundtrip_sse_scaled(handle, img.ctypes.data, 510, 512, 512, 2, out) == N.TIC_E_ARG
    assert L.tic_roundtrip_sse_scaled(handle, img.ctypes.data, 512, 512, 512, 2, None) == N.TIC_E_ARG


def test_cli_min_psnr(ctx, shipped, fx, tmp_path, capsys):
    """encode_cli --min-psnr: the bytes of compress_to_psnr, quality and PSNR as third and fourth lines; not together with --max-bytes,
    --scaled or --quality."""
    from tinyimgcodec_amd import encode_cli as cli

    img = fixture_image("lenna")
    src, dst = tmp_path / "lenna.npy", tmp_path / "out.img"
    np.save(src, img)
    assert cli.main([str(src), str(dst), "--min-psnr", "36.5", "--max-quality", "97"]) == 0
    out = capsys.readouterr().out.splitlines()
    bs, q, p = T.compress_to_psnr(img, 36.5, 1, 97, ctx=ctx)
    sse = fx["images"]["lenna"]["sse"]
    assert q == bisect_psnr(sse, T.max_sse_for_psnr(36.5, img.size), 1, 97) and p >= 36.5 > T.psnr_from_sse(sse[q - 2], img.size)
    assert dst.read_bytes() == bs
    assert out == [f"{len(bs)} bytes", f"Compression Ratio: {512 * 512 / len(bs)}:1", f"Quality: {q}", f"PSNR: {p}"]
    assert cli.main([str(src), str(dst), "--min-psnr", "20", "--min-quality", "10", "--max-quality", "30"]) == 0
    assert capsys.readouterr().out.splitlines()[2] == "Quality: 10" and dst.read_bytes() == T.compress(img, 10, ctx=ctx)
    for extra in (["--scaled", "med"], ["--quality", "50"], ["--max-bytes", "20000"]):
        with pytest.raises(SystemExit):
            cli.main([str(src), str(dst), "--min-psnr", "36.5"] + extra)
    capsys.readouterr()
    L, handle = shipped
    buf = np.empty(L.tic_compress_bound(512, 512), np.uint8)
    n, qq, s = C.c_size_t(0), C.c_int(0), C.c_uint64(0)
    assert L.tic_compress_to_psnr(handle, img.ctypes.data, 512, 512, 512, T.max_sse_for_psnr(36.5, img.size), 1, 97, buf.ctypes.data, buf.size,
                                  C.byref(n), C.byref(qq), C.byref(s)) == N.TIC_OK
    assert (qq.value, s.value, buf[: n.value].tobytes()) == (q, sse[q - 1], bs)


def test_size_search_is_unchanged_beside_the_new_calls(ctx, shipped, fx, rate, oracle):
    """compressed_sizes and compress_to_size on a fixture image equal the fixture after rd_points, compress_to_psnr and
    roundtrip_sse_scaled have used the same context (they share its workspaces and result buffers) - and the other way round."""
    img = fixture_image("bench40")
    sizes = rate["bench40"]["sizes"]
    sse = fx["images"]["bench40"]["sse"]
    want_sizes = [-1 if v is None else v for v in sizes]
    T.rd_points(img, range(1, 100), ctx=ctx)
    T.compress_to_psnr(img, 35.0, 1, 98, ctx=ctx)
    T.roundtrip_sse_scaled(img, "med", ctx=ctx)
    assert T.compressed_sizes(img, range(1, 100), ctx=ctx).tolist() == want_sizes
    for budget, qmin, qmax in ((sizes[49], 1, 99), (sizes[29] - 1, 1, 99), (sizes[39], 20, 60)):
        bs, q = T.compress_to_size(img, budget, qmin, qmax, ctx=ctx)
        assert q == bisect_size(sizes, budget, qmin, qmax) and bs == oracle.compress(img, q)
    got = T.rd_points(img, [50, 98], ctx=ctx)
    assert (got[0].tolist(), got[1].tolist()) == ([sizes[49], sizes[97]], [sse[49], sse[97]])
    L, handle = shipped
    first = rd_raw(L, handle, img, [50])
    qs = (C.c_int * 3)(20, 50, 98)
    sz = (C.c_longlong * 3)()
    assert L.tic_stream_sizes(handle, img.ctypes.data, 512, 512, 512, qs, 3, sz) == N.TIC_OK and list(sz) == [sizes[19], sizes[49], sizes[97]]
    assert rd_raw(L, handle, img, [50]) == first == ([sizes[49]], [sse[49]], [fx["images"]["bench40"]["sse_wrapped"][49]])


def test_rd_points_arguments(ctx, shipped):
    """The checks of tic_stream_sizes_dev in its order: a bad quality fails before anything is queued and leaves the results alone."""
    L = N.load()
    d = Dev(L, ctx.handle)
    try:
        d_img = d.upload(rand_frame(3, 64, 64))
        a, b = (C.c_uint64 * 3)(9, 9, 9), (C.c_uint64 * 3)(9, 9, 9)
        for bad in (0, 100, -1):
            qs = (C.c_int * 3)(40, bad, 50)
            sz = (C.c_longlong * 3)(-5, -5, -5)
            assert L.tic_rd_points_dev(ctx.handle, d_img, 64, 64, 64, qs, 3, sz, a, b) == N.TIC_E_QUALITY
            assert list(sz) == [-5] * 3 and list(a) == list(b) == [9] * 3
        qs = (C.c_int * 3)(40, 50, 60)
        sz = (C.c_longlong * 3)()
        assert L.tic_rd_points_dev(ctx.handle, None, 64, 64, 64, qs, 1, sz, a, b) == N.TIC_E_ARG
        assert L.tic_rd_points_dev(ctx.handle, d_img, 64, 64, 64, None, 1, sz, a, b) == N.TIC_E_ARG
        assert L.tic_rd_points_dev(ctx.handle, d_img, 64, 64, 64, qs, 1, None, a, b) == N.TIC_E_ARG
        assert L.tic_rd_points_dev(ctx.handle, d_img, 64, 64, 64, qs, 1, sz, None, b) == N.TIC_E_ARG
        assert L.tic_rd_points_dev(ctx.handle, d_img, 64, 64, 64, qs, 1, sz, a, None) == N.TIC_E_ARG
        assert L.tic_rd_points_dev(ctx.handle, d_img, 64, 64, 63, qs, 1, sz, a, b) == N.TIC_E_ARG
        assert L.tic_rd_points_dev(ctx.handle, d_img, 64, 64, 64, qs, -1, sz, a, b) == N.TIC_E_ARG
        assert L.tic_rd_points_dev(ctx.handle, d_img, 64, 64, 64, qs, 0, sz, a, b) == N.TIC_OK
        assert L.tic_rd_points_dev(ctx.handle, None, 0, 64, 64, qs, 3, sz, a, b) == N.TIC_OK and (list(sz), list(a), list(b)) == ([16] * 3, [0] * 3, [0] * 3)
    finally:
        d.close()
    Ls, hs = shipped
    qs = (C.c_int * 1)(100)
    sz, a, b = (C.c_longlong * 1)(), (C.c_uint64 * 1)(), (C.c_uint64 * 1)()
    img = rand_frame(3, 64, 64)
    assert Ls.tic_rd_points(hs, img.ctypes.data, 64, 64, 64, qs, 1, sz, a, b) == N.TIC_E_QUALITY
    assert Ls.tic_rd_points(hs, None, 64, 64, 64, (C.c_int * 1)(50), 1, sz, a, b) == N.TIC_E_ARG
