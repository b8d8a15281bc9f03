"""The table behind tests/test_context_state_cpu.py and tests/test_context_state_gpu.py: one record per family of calls that takes a
context - a callable, the context buffers it touches (by the names of the library's registry), a small, a ragged
and a dense case, and what each case must give.  No expected result comes from the library: they are the oracle's (oracle/) or a
fixture's of the unmodified reference (tests/golden/).  No test lives here."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

POISON_BYTES = (0x00, 0xFF, 0xA5)
# Lowered, the small streams reach the device decoders; without them they take the host route (tic_hooks.h)
DEVICE_ROUTE = {"TIC_DECODE_MIN_BLOCKS": "1", "TIC_DECODE_MIN_BITS": "0"}
HOST_ROUTE = {}

# ---- the registry's names (tic_api.hip: each written once, where its Buf field is declared) ---------------------------------------------
STATE = {
    "d_consts": "quantiser constants of qualities 1..99, written at creation; slot 0 by tic_set_custom_quality only",
    "d_huff": "the fixed Huffman table of the device entropy stage, written at creation",
    "d_total_bits": "payload bits [2] and the two error flags used in turn: the placing kernel leaves the next call's flag zero",
    "h_stat": "host-mapped {bits, error} pairs of the entropy stage and of every compress ticket: a pair is rewritten by the call that reads it",
    "d_fallback": "guard-band counters: zero at creation, cleared by the calls that report them",
    "d_size_tab": "the size kernel's table, written once",
    "d_dec_luts": "the decoder's look-up tables, written once",
    "lane.d_err": "four error flags of a compress lane used in turn: a placing kernel zeroes the flag three frames ahead",
    "bslot.d_err": "two error flags of a batch slot used in turn: zero when the slot is allocated, the chunk's last kernel clears the next one",
    "dec_ws.desc": "look-back words of tic_decompress / _dev: zero or stamped with a past epoch (a kernel spin-waits on them)",
    "dec_slot.desc": "look-back words of a decode ticket's slot: zero or stamped with a past epoch (a kernel spin-waits on them)",
    "dbat.desc": "look-back words of tic_decompress_batch: zero or stamped with a past epoch (a kernel spin-waits on them)",
}
SCRATCH = (
    "d_img", "d_coef", "d_ent_work", "d_stream_buf", "h_small", "h_zz", "d_dc32", "h_dec_tail", "d_rate", "h_rate", "h_rate_pix", "h_rate_tabs",
    "d_rate_tabs", "h_rd_tabs", "d_rd_tabs", "h_scaled_tabs", "d_scaled_tabs", "d_adapt_stats", "d_adapt_work", "d_adapt_out", "d_adec_tab",
    "d_adec_work", "adbat.d_work", "adbat.h_status", "dbat.h_in", "dbat.d_in", "dbat.d_pix", "dbat.h_pix", "dbat.work", "dbat.status",
    "dec_ws.work", "dec_ws.status", "dec_slot.work", "dec_slot.status", "lane.d_coef", "lane.d_work", "bslot.pin_in", "bslot.pin_out",
    "bslot.d_img", "bslot.d_coef", "bslot.d_work", "bslot.d_lens", "bslot.h_lens", "bslot.h_err", "bslot.d_streams", "bslot.h_frames",
    "bslot.d_frames", "bslot.h_rb_off", "bslot.h_sframes", "bslot.d_sframes", "bslot.d_adapt", "bslot.h_adapt",
)
_SINGLE = ("d_img", "d_coef")
_ENT = ("d_ent_work", "d_stream_buf", "h_small")
_ENT_STATE = ("d_consts", "d_huff", "d_total_bits", "h_stat", "d_fallback")
_BSLOT = ("bslot.pin_in", "bslot.pin_out", "bslot.d_img", "bslot.d_coef", "bslot.d_work", "bslot.d_lens", "bslot.h_lens", "bslot.h_err",
          "bslot.d_streams")
_BSLOT_V = _BSLOT + ("bslot.h_frames", "bslot.d_frames", "bslot.h_rb_off")
_BSLOT_STATE = ("d_consts", "d_huff", "bslot.d_err", "d_fallback")
_RATE = _SINGLE + ("d_rate", "h_rate")
_RATE_V = _RATE + ("h_rate_pix", "h_rate_tabs", "d_rate_tabs")
_RD_V = _RATE_V + ("h_rd_tabs", "d_rd_tabs")
_RATE_STATE = ("d_consts", "d_size_tab", "d_fallback")
_DEC = _SINGLE + ("h_zz", "d_dc32", "d_stream_buf", "h_dec_tail", "dec_ws.work", "dec_ws.status")
_DEC_STATE = ("d_consts", "d_dec_luts", "dec_ws.desc")
_DBAT = ("dbat.h_in", "dbat.d_in", "dbat.d_pix", "dbat.h_pix")


def rng_frame(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def sha(b):
    return hashlib.sha256(b).hexdigest()


def norm(x):
    """A result as nested tuples of bytes and ints: equality of two of them is byte-for-byte and integer equality."""
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, x.tobytes())
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    if isinstance(x, (tuple, list)):
        return tuple(norm(v) for v in x)
    if isinstance(x, (np.integer,)):
        return int(x)
    return x


# ---- frames ------------------------------------------------------------------------------------------------------------------------
# (image, quality) lists.  SMALL: the smallest frames at which a family's kernels can still go wrong - one flat block, 16 x 24 noise, a
# ragged 17 x 23 frame, of three qualities; the single-frame families run them one after the other, the batch families in one call.
# RAGGED: 9 x 9.  DENSE: 128 x 192 noise at quality 98, there to leave non-zero data everywhere (at 99 such noise has coefficients without a
# Huffman code: the size and rate-distortion families probe 99 too and must report -1 there).
SMALL = ((np.full((8, 8), 77, np.uint8), 50), (rng_frame(101, 16, 24), 90), (rng_frame(102, 17, 23), 20))
RAGGED = ((rng_frame(103, 9, 9), 75),)
DENSE = ((rng_frame(104, 128, 192), 98),)
UNIFORM_SMALL = tuple((rng_frame(110 + k, 16, 24), 60) for k in range(3))  # compress_batch of equal frames takes one quality
UNIFORM_RAGGED = tuple((rng_frame(113 + k, 9, 9), 60) for k in range(2))
UNIFORM_DENSE = tuple((rng_frame(115 + k, 128, 192), 98) for k in range(2))
# The device decoder of default-table streams takes nothing below 128 + 8,192 stream bits (device_decoder_takes, whatever the hooks say):
# the decoder families' device route has small frames of its own, the smallest whose streams clear that floor (1,058, 1,548, 1,292 and
# 1,560 bytes), two of them ragged.
DEV_SMALL = ((rng_frame(126, 24, 32), 98), (rng_frame(121, 25, 41), 95), (rng_frame(123, 24, 40), 98))
DEV_RAGGED = ((rng_frame(124, 17, 47), 98),)
QS_SMALL, QS_DENSE = (10, 50, 90), (99, 98, 60)
PSNR_MAX_QUALITY = 98  # compress_to_psnr raises KeyError when max_quality itself has a coefficient without a code
_cache = {}


def oracle():
    from oracle import pyoracle

    if "oracle" not in _cache:
        pyoracle.build()
        _cache["oracle"] = pyoracle
    return _cache["oracle"]


def _stream(img, q):
    """The oracle's compress(img, q), or None where it raises for a coefficient without a Huffman code; kept (the frames are this
    module's constants)."""
    key = ("stream", img.shape, img.tobytes(), q)
    if key not in _cache:
        try:
            _cache[key] = oracle().compress(img, q)
        except oracle().OracleError:
            _cache[key] = None
    return _cache[key]


def _size(img, q):
    return -1 if _stream(img, q) is None else len(_stream(img, q))


def _sums(img, q):
    import distortion_common as DC

    key = ("sums", img.shape, img.tobytes(), q)
    if key not in _cache:
        _cache[key] = DC.oracle_sums(oracle(), img, q)
    return _cache[key]


def _npz(name):
    if name not in _cache:
        _cache[name] = np.load(os.path.join(GOLDEN, name))
    return _cache[name]


def _json(name):
    if name not in _cache:
        with open(os.path.join(GOLDEN, name)) as f:
            _cache[name] = json.load(f)
    return _cache[name]


# the integer encoder's cases: (fixture key, setting) of tests/golden/scaled_encode.npz (sizes are multiples of 8 there)
SCALED_SMALL = (("flat8x8_med", "med"), ("noise16x24_best", "best"), ("highfreq8x16_high", "high"))
SCALED_RAGGED = (("noise16x24_low", "low"),)
SCALED_DENSE = (("noise64x96_best", "best"),)
# the adaptive encoder's: indices into tests/golden/adaptive_batch.json (8 x 8 flat, 13 x 21 noise, 1 x 1 / 64 x 64 checker / 64 x 64 noise)
ADAPT_SMALL, ADAPT_RAGGED, ADAPT_DENSE = (1, 3, 0), (10,), (9,)
# ... and what the adaptive DEVICE decoder takes of the small streams (it leaves flat and one-block frames, and 7 x 9 below quality 90, to the
# host): (name, quality) of tests/golden/adaptive_streams.json - 137, 227 and 186 bytes - beside frame 3 of the batch fixture (13 x 21, 264 bytes)
ADAPT_DEV_SMALL, ADAPT_DEV_RAGGED = (("small_7x9", 90), ("small_15x17", 50), 3), (("ragged_3", 15), ("ragged_4", 17))
ADAPT_DEV_DENSE = (9, ("ragged_2", 91))  # (two frames: a batch of one is the single call)
# the integer encoder's streams just above the device decoder's floor (1,187, 1,381, 1,216 and 1,197 bytes: the fixture's floor* cases)
SCALED_DEV_SMALL = (("floor24x56_best", "best"), ("floor32x64_high", "high"), ("floor40x64_med", "med"))
SCALED_DEV_RAGGED = (("floor16x112_high", "high"),)


def _scaled(key, what):
    """An array of a case of the integer encoder's fixtures: scaled_encode.npz, or scaled_floor.npz for the floor* cases."""
    return _npz("scaled_floor.npz" if key.startswith("floor") else "scaled_encode.npz")[key + "_" + what]


def scaled_image(key):
    return _scaled(key, "img")


def adaptive_frame(i):
    import adaptive_batch_common as AB

    e = _json("adaptive_batch.json")["frames"][i]
    return e, AB.make_frame(e["kind"], e["seed"], e["height"], e["width"])


def adaptive_entry(item):
    """The fixture entry (height, width, stream, decoded_sha256 ...) of a decoder case's item: an index into adaptive_batch.json, or a
    (name, quality) of adaptive_streams.json."""
    if isinstance(item, int):
        return adaptive_frame(item)[0]
    (e,) = [c for c in _json("adaptive_streams.json")["cases"] if (c["name"], c["quality"]) == tuple(item)]
    return e


# ---- device memory of the caller -------------------------------------------------------------------------------------------------------
class Dev:
    """A device buffer of the caller's (tic_dev_alloc: not one of the context's, so never poisoned)."""

    def __init__(self, ctx, nbytes, fill=None):
        from tinyimgcodec_amd import _native as N

        self.ctx, self.L, self.n = ctx, N.load(), max(int(nbytes), 1)
        self.p = C.c_void_p()
        ctx.check(self.L.tic_dev_alloc(ctx.handle, self.n, C.byref(self.p)))
        if fill is not None:
            ctx.check(self.L.tic_memset_dev(ctx.handle, self.p, fill, self.n))
            ctx.check(self.L.tic_sync(ctx.handle))

    def up(self, arr):
        a = np.ascontiguousarray(arr)
        if a.nbytes:
            self.ctx.check(self.L.tic_memcpy_h2d(self.ctx.handle, self.p, a.ctypes.data, a.nbytes))
        return self

    def down(self, nbytes):
        out = np.zeros(max(int(nbytes), 1), np.uint8)
        if nbytes:
            self.ctx.check(self.L.tic_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.p, int(nbytes)))
        return out[: int(nbytes)]

    def free(self):
        if self.p:
            self.ctx.check(self.L.tic_dev_free(self.ctx.handle, self.p))
            self.p = C.c_void_p()


# ---- the callables: (ctx, case) -> result ------------------------------------------------------------------------------------------------
def _T():
    import tinyimgcodec_amd as T

    return T


def _L():
    from tinyimgcodec_amd import _native as N

    return N.load()


def run_compress(ctx, case):
    return [_T().compress(img, q, ctx=ctx) for img, q in case]


def run_compress_dev(ctx, case):
    L, outs = _L(), []
    for img, q in case:
        h, w = img.shape
        cap = L.tic_compress_bound(h, w)
        d_img, d_out = Dev(ctx, img.nbytes).up(img), Dev(ctx, cap, 0xEE)
        n = C.c_size_t(0)
        try:
            ctx.check(L.tic_compress_dev(ctx.handle, d_img.p, h, w, w, q, d_out.p, cap, C.byref(n)))
            outs.append(d_out.down(n.value).tobytes())
        finally:
            d_img.free(), d_out.free()
    return outs


def open_compress_tickets(ctx, case):
    """-> [(ticket, d_img, d_out)] of one tic_compress_dev_async per frame, in order."""
    L, open_ = _L(), []
    for img, q in case:
        h, w = img.shape
        cap = L.tic_compress_bound(h, w)
        d_img, d_out = Dev(ctx, img.nbytes).up(img), Dev(ctx, cap, 0xEE)
        t = C.c_longlong(-1)
        ctx.check(L.tic_compress_dev_async(ctx.handle, d_img.p, h, w, w, q, d_out.p, cap, C.byref(t)))
        open_.append((t.value, d_img, d_out))
    return open_


def collect_compress_ticket(ctx, ticket):
    t, d_img, d_out = ticket
    n = C.c_size_t(0)
    try:
        ctx.check(_L().tic_async_result(ctx.handle, t, 1, C.byref(n)))
        return d_out.down(n.value).tobytes()
    finally:
        d_img.free(), d_out.free()


def run_compress_dev_async(ctx, case):
    return [collect_compress_ticket(ctx, t) for t in open_compress_tickets(ctx, case)]


def run_compress_batch_uniform(ctx, case):
    return _T().compress_batch([img for img, _ in case], case[0][1], ctx=ctx)


def run_compress_batch_mixed(ctx, case):
    return _T().compress_batch([img for img, _ in case], [q for _, q in case], ctx=ctx)


def run_compress_adaptive(ctx, case):
    return [_T().compress_adaptive(adaptive_frame(i)[1], adaptive_frame(i)[0]["quality"], ctx=ctx) for i in case]


def run_compress_batch_adaptive(ctx, case):
    return _T().compress_batch_adaptive([adaptive_frame(i)[1] for i in case], [adaptive_frame(i)[0]["quality"] for i in case], ctx=ctx)


def run_compress_scaled(ctx, case):
    return [_T().compress_scaled(scaled_image(k), s, ctx=ctx) for k, s in case]


def run_compress_batch_scaled(ctx, case):
    return _T().compress_batch_scaled([scaled_image(k) for k, _ in case], [s for _, s in case], ctx=ctx)


def run_rd_points_scaled_batch(ctx, case):
    return _T().rd_points_scaled_batch([scaled_image(k) for k, _ in case], [s for _, s in case], ctx=ctx)


def _qs(case):
    return QS_DENSE if case is DENSE else QS_SMALL


def run_compressed_sizes(ctx, case):
    return [_T().compressed_sizes(img, _qs(case), ctx=ctx) for img, _ in case]


def run_compressed_sizes_batch(ctx, case):
    return _T().compressed_sizes_batch([img for img, _ in case], _qs(case), ctx=ctx)


def budget(img, q):
    """The byte budget of the size searches: what the frame takes at the case's quality, so that the search ends there or above."""
    return _size(img, q)


def run_compress_to_size(ctx, case):
    return [_T().compress_to_size(img, budget(img, q), ctx=ctx) for img, q in case]


def run_compress_batch_to_size(ctx, case):
    return _T().compress_batch_to_size([img for img, _ in case], [budget(img, q) for img, q in case], ctx=ctx)


def run_rd_points(ctx, case):
    return [_T().rd_points(img, _qs(case), ctx=ctx) for img, _ in case]


def run_rd_points_batch(ctx, case):
    return _T().rd_points_batch([img for img, _ in case], _qs(case), ctx=ctx)


def target_psnr(img, q):
    """The target of the PSNR searches: what the frame reaches at the case's quality (inf for an exact round trip)."""
    return _T().psnr_from_sse(_sums(img, q)[0], img.size)


def run_compress_to_psnr(ctx, case):
    return [_T().compress_to_psnr(img, target_psnr(img, q), max_quality=PSNR_MAX_QUALITY, ctx=ctx) for img, q in case]


def run_compress_batch_to_psnr(ctx, case):
    return _T().compress_batch_to_psnr([img for img, _ in case], [target_psnr(img, q) for img, q in case], max_quality=PSNR_MAX_QUALITY, ctx=ctx)


def streams_of(case):
    return [_stream(img, q) for img, q in case]


def run_decompress(ctx, case):
    return [_T().decompress(s, ctx=ctx) for s in streams_of(case)]


def run_decompress_dev(ctx, case):
    L, outs = _L(), []
    for (img, _), s in zip(case, streams_of(case)):
        h, w = img.shape
        d_s, d_o = Dev(ctx, len(s) + 16).up(np.frombuffer(s, np.uint8)), Dev(ctx, h * w, 0xEE)
        hh, ww = C.c_int(-1), C.c_int(-1)
        try:
            ctx.check(L.tic_decompress_dev(ctx.handle, d_s.p, len(s), d_o.p, w, h * w, C.byref(hh), C.byref(ww)))
            assert (hh.value, ww.value) == (h, w)
            outs.append(d_o.down(h * w).reshape(h, w))
        finally:
            d_s.free(), d_o.free()
    return outs


def open_decompress_tickets(ctx, case):
    L, open_ = _L(), []
    for (img, _), s in zip(case, streams_of(case)):
        h, w = img.shape
        stride = (w + 7) // 8 * 8  # (a ticket is launched on a slot only into rows a multiple of 8 bytes apart)
        d_s, d_o = Dev(ctx, len(s) + 16).up(np.frombuffer(s, np.uint8)), Dev(ctx, h * stride, 0xEE)
        t = C.c_longlong(-1)
        ctx.check(L.tic_decompress_dev_async(ctx.handle, d_s.p, len(s), d_o.p, stride, h * stride, C.byref(t)))
        open_.append((t.value, d_s, d_o, h, w))
    return open_


def collect_decompress_ticket(ctx, ticket):
    t, d_s, d_o, h, w = ticket
    hh, ww = C.c_int(-1), C.c_int(-1)
    try:
        ctx.check(_L().tic_decompress_async_result(ctx.handle, t, 1, C.byref(hh), C.byref(ww)))
        assert (hh.value, ww.value) == (h, w)
        rows = d_o.down(h * ((w + 7) // 8 * 8)).reshape(h, -1)
        assert np.all(rows[:, w:] == 0xEE), "a decode ticket wrote between the rows of its frame"
        return np.ascontiguousarray(rows[:, :w])
    finally:
        d_s.free(), d_o.free()


def run_decompress_dev_async(ctx, case):
    out = []
    for k in range(0, len(case), 4):  # (four decode tickets may be open at once)
        out += [collect_decompress_ticket(ctx, t) for t in open_decompress_tickets(ctx, case[k:k + 4])]
    return out


def run_decompress_batch(ctx, case):
    return _T().decompress_batch(streams_of(case), ctx=ctx)


def _adaptive_streams(case):
    return [bytes.fromhex(adaptive_entry(i)["stream"]) for i in case]


def run_decompress_adaptive(ctx, case):
    return [sha(_T().decompress_adaptive(s, ctx=ctx).tobytes()) for s in _adaptive_streams(case)]


def run_decompress_batch_adaptive(ctx, case):
    return [sha(o.tobytes()) for o in _T().decompress_batch_adaptive(_adaptive_streams(case), ctx=ctx)]


def run_decompress_scaled(ctx, case):
    return [_T().decompress(_scaled(k, "bs").tobytes(), ctx=ctx) for k, _ in case]


# ---- what each case must give -----------------------------------------------------------------------------------------------------------
def exp_streams(case):
    return streams_of(case)


def exp_scaled_streams(case):
    return [_scaled(k, "bs").tobytes() for k, _ in case]


def exp_scaled_rd(case):
    import distortion_common as DC

    z, n = _npz("scaled_encode.npz"), len(case)
    sizes, sse, wrapped = np.zeros((n, n), np.int64), np.zeros((n, n), np.uint64), np.zeros((n, n), np.uint64)
    for i, (k, _) in enumerate(case):  # every image at every setting of the case: the fixture holds each image at all four
        for j, (_, s) in enumerate(case):
            kk = k.rsplit("_", 1)[0] + "_" + s
            assert np.array_equal(z[kk + "_img"], z[k + "_img"])
            sizes[i, j] = z[kk + "_bs"].size
            sse[i, j], wrapped[i, j] = DC.sums(z[kk + "_img"], z[kk + "_dec"])
    return sizes, sse, wrapped


def exp_adaptive_streams(case):
    return _adaptive_streams(case)


def exp_sizes(case):
    return [np.array([_size(img, q) for q in _qs(case)], np.int64) for img, _ in case]


def exp_sizes_batch(case):
    return np.array([[_size(img, q) for q in _qs(case)] for img, _ in case], np.int64)


def _best_fit(img, max_bytes):
    lo, hi = 1, 99  # compress_to_size's bisection, with the oracle's sizes
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if 0 <= _size(img, mid) <= max_bytes:
            lo = mid
        else:
            hi = mid - 1
    return _stream(img, lo), lo


def exp_to_size(case):
    return [_best_fit(img, budget(img, q)) for img, q in case]


def _rd(img, qs):
    s = [_sums(img, q) for q in qs]
    return np.array([_size(img, q) for q in qs], np.int64), np.array([a for a, _ in s], np.uint64), np.array([b for _, b in s], np.uint64)


def exp_rd(case):
    return [_rd(img, _qs(case)) for img, _ in case]


def exp_rd_batch(case):
    r = [_rd(img, _qs(case)) for img, _ in case]
    return tuple(np.stack([x[k] for x in r]) for k in range(3))


def _least_quality(img, min_psnr):
    T = _T()
    bound = T.max_sse_for_psnr(min_psnr, img.size)
    lo, hi = 1, PSNR_MAX_QUALITY  # compress_to_psnr's bisection, with the oracle's round trips
    while lo < hi:
        mid = (lo + hi) // 2
        if _size(img, mid) >= 0 and _sums(img, mid)[0] <= bound:
            hi = mid
        else:
            lo = mid + 1
    return _stream(img, lo), lo, T.psnr_from_sse(_sums(img, lo)[0], img.size)


def exp_to_psnr(case):
    return [_least_quality(img, target_psnr(img, q)) for img, q in case]


def exp_pixels(case):
    return [oracle().decompress(s) for s in streams_of(case)]


def exp_adaptive_pixels(case):
    return [adaptive_entry(i)["decoded_sha256"] for i in case]


def exp_scaled_pixels(case):
    return [_scaled(k, "dec") for k, _ in case]


# ---- which route a decoder family's last call took: (ctx, frames of the case) -> None, or what is wrong ------------------------------------
def path_is(want):
    def route(ctx, n):
        path = _L().tic_last_decode_path(ctx.handle)
        return None if path == want else "decode path %d, not %d" % (path, want)
    return route


def last_ticket(ctx):
    """What the hooks build says of the decode ticket collected last -> {"ticket", "slot", "launched", "held", "epoch"}, or None."""
    m = re.match(r"decode ticket (\d+): slot (\d+), launched (\d), guess held (\d), epoch (\d+)", _L().tic_last_error(ctx.handle).decode())
    return dict(zip(("ticket", "slot", "launched", "held", "epoch"), map(int, m.groups()))) if m else None


def last_epoch(ctx):
    """The epoch of the decoder run begun last (hooks build) -> (workspace name, epoch), or None."""
    m = re.match(r"decoder run on ([\w.]+): epoch (\d+)", _L().tic_last_error(ctx.handle).decode())
    return (m.group(1), int(m.group(2))) if m else None


def guess_held(ctx, n):
    """The last ticket collected was launched on its slot, on a guess of the header that held."""
    t = last_ticket(ctx)
    return None if t and t["launched"] and t["held"] else "the last ticket was not launched on a slot with a guess that held (%s)" % t


def batch_took_all(ctx, n):
    v = [C.c_int(-1) for _ in range(4)]
    assert _L().tic_last_decompress_batch(ctx.handle, *[C.byref(x) for x in v]) == 0
    return None if (v[0].value, v[1].value) == (n, 0) else "the batch kernels took %d of %d frames, %d took the single call" % (v[0].value, n, v[1].value)


def adaptive_batch_took_all(ctx, n):
    v = [C.c_int(-1) for _ in range(3)]
    assert _L().tic_last_decompress_batch_adaptive(ctx.handle, *[C.byref(x) for x in v]) == 0
    return None if (v[0].value, v[1].value) == (n, 0) else "the batch kernels took %d of %d frames, %d took the single call" % (v[0].value, n, v[1].value)


# ---- the table -------------------------------------------------------------------------------------------------------------------------
class Family:
    """name; calls: the C entry points the record stands for - the ones its callable calls and the device-buffer forms those are built on
    (tic_compress calls tic_compress_dev's stages, tic_stream_sizes is tic_stream_sizes_dev behind an upload, ...): LISTED here, which is all
    tests/test_context_state_cpu.py asks; only the first of each record is certain to be called; scratch / state: registry names of the
    context buffers they touch; run(ctx, case) and expect(case); cases: small, ragged, dense; env: hook variables the family runs under (the
    decoders' route); route(ctx, n): None when the last call went where the record says (the device decoder, a slot, the batch kernels),
    asked after every case when route_all, else after the dense one."""

    def __init__(self, name, calls, scratch, state, run, expect, small, ragged, dense, env=None, route=None, route_all=False):
        self.name, self.calls, self.scratch, self.state = name, tuple(calls), tuple(scratch), tuple(state)
        self.run, self.expect, self.env, self.route = run, expect, dict(env or {}), route
        self.route_all = route_all  # every case must take `route`, not only the dense one
        self.cases = {"small": small, "ragged": ragged, "dense": dense}

    def expected(self, which):
        """Of the case `which` ("small", "ragged", "dense": computed once), or of a case given as such."""
        if not isinstance(which, str):
            return norm(self.expect(which))
        key = ("expected", self.expect.__name__, which, id(self.cases[which]))
        if key not in _cache:
            _cache[key] = norm(self.expect(self.cases[which]))
        return _cache[key]

    def check(self, ctx, which, monkeypatch, what="", sink=None):
        """Runs the case under the family's hook variables: the result, byte for byte and integer for integer, is the expected one.
        sink: a list that takes the message of a result that differs, for a test that reports all of them at its end."""
        for k in DEVICE_ROUTE:
            monkeypatch.delenv(k, raising=False)
        for k, v in self.env.items():
            monkeypatch.setenv(k, v)
        got = norm(self.run(ctx, self.cases[which] if isinstance(which, str) else which))
        if self.route is not None and (self.route_all or which == "dense"):
            wrong = self.route(ctx, len(self.cases[which] if isinstance(which, str) else which))
            assert wrong is None, "%s %s %s: %s" % (self.name, which, what, wrong)
        msg = "%s: %s case differs from the reference %s" % (self.name, which if isinstance(which, str) else "given", what)
        if sink is not None and got != self.expected(which):
            sink.append(msg)
            return
        assert got == self.expected(which), msg

    def __repr__(self):
        return self.name


def _decoders():
    """Seven families on two routes.  Device: the hooks lower the decoders' thresholds and every case is one the device decoder takes -
    asserted after every call; the ticket family repeats one frame six times (a ticket is launched on a slot behind two equal headers, on a
    guess of the next one: behind another frame the first four are launched on a wrong guess or run synchronously and are decoded again,
    the last two are launched on a guess that holds, which is what is asserted).  Host: the defaults, under which none of these
    streams reaches a device decoder."""
    out = []
    for tag, env in (("device", DEVICE_ROUTE), ("host", HOST_ROUTE)):
        dev = tag == "device"
        dec = _DEC if dev else _SINGLE + ("h_zz", "d_dc32")
        small, ragged = (DEV_SMALL, DEV_RAGGED) if dev else (SMALL, RAGGED)
        tsmall, tragged, tdense = ((DEV_SMALL[0],) * 6, (DEV_RAGGED[0],) * 6, DENSE * 6) if dev else (SMALL, RAGGED, DENSE)
        asmall, aragged, adense = (ADAPT_DEV_SMALL, ADAPT_DEV_RAGGED, ADAPT_DEV_DENSE) if dev else (ADAPT_SMALL, ADAPT_RAGGED, ADAPT_DENSE)
        ssmall, sragged = (SCALED_DEV_SMALL, SCALED_DEV_RAGGED) if dev else (SCALED_SMALL, SCALED_RAGGED)
        path = path_is(1 if dev else 2)
        out += [
            Family("decompress[%s]" % tag, ("tic_decompress",), dec, _DEC_STATE, run_decompress, exp_pixels, small, ragged, DENSE, env, path, True),
            Family("decompress_dev[%s]" % tag, ("tic_decompress_dev",), dec, _DEC_STATE, run_decompress_dev, exp_pixels, small, ragged, DENSE, env, path, True),
            Family("decompress_dev_async[%s]" % tag, ("tic_decompress_dev_async", "tic_decompress_async_result"),
                   dec + ("dec_slot.work", "dec_slot.status"), _DEC_STATE + ("dec_slot.desc",), run_decompress_dev_async, exp_pixels, tsmall, tragged, tdense,
                   env, guess_held if dev else path, True),
            Family("decompress_batch[%s]" % tag, ("tic_decompress_batch",), dec + _DBAT + ("dbat.work", "dbat.status"), _DEC_STATE + ("dbat.desc",),
                   run_decompress_batch, exp_pixels, small, ragged, DENSE, env, batch_took_all if dev else None, True),
            Family("decompress_adaptive[%s]" % tag, ("tic_decompress_adaptive", "tic_decompress_adaptive_dev"),
                   _SINGLE + ("h_zz", "d_stream_buf", "d_adec_tab", "d_adec_work"), ("d_consts",), run_decompress_adaptive, exp_adaptive_pixels,
                   asmall, aragged, adense, env, path, True),
            Family("decompress_batch_adaptive[%s]" % tag, ("tic_decompress_batch_adaptive",),
                   _SINGLE + ("h_zz", "d_stream_buf", "d_adec_tab", "d_adec_work", "adbat.d_work", "adbat.h_status") + _DBAT, ("d_consts",),
                   run_decompress_batch_adaptive, exp_adaptive_pixels, asmall, aragged, adense, env, adaptive_batch_took_all if dev else None, True),
            Family("decompress_scaled[%s]" % tag, ("tic_decompress",), dec, _DEC_STATE, run_decompress_scaled, exp_scaled_pixels,
                   ssmall, sragged, SCALED_DENSE, env, path, True),
        ]
    return out


FAMILIES = [
    Family("compress", ("tic_compress",), _SINGLE + _ENT, _ENT_STATE, run_compress, exp_streams, SMALL, RAGGED, DENSE),
    Family("compress_dev", ("tic_compress_dev", "tic_dctq_dev", "tic_entropy_encode_dev"), ("d_coef", "d_ent_work"), _ENT_STATE, run_compress_dev,
           exp_streams, SMALL, RAGGED, DENSE),
    Family("compress_dev_async", ("tic_compress_dev_async", "tic_async_result"), ("lane.d_coef", "lane.d_work"),
           ("d_consts", "d_huff", "h_stat", "lane.d_err", "d_fallback"), run_compress_dev_async, exp_streams, SMALL, RAGGED, DENSE),
    Family("compress_batch[uniform]", ("tic_compress_batch",), _BSLOT, _BSLOT_STATE, run_compress_batch_uniform, exp_streams, UNIFORM_SMALL,
           UNIFORM_RAGGED, UNIFORM_DENSE),
    Family("compress_batch[mixed]", ("tic_compress_batch_v",), _BSLOT_V + _SINGLE + _ENT, _BSLOT_STATE + _ENT_STATE, run_compress_batch_mixed,
           exp_streams, SMALL, RAGGED, DENSE),
    Family("compress_adaptive", ("tic_compress_adaptive",), _SINGLE + ("d_adapt_stats", "d_adapt_work", "d_adapt_out"), ("d_consts", "d_fallback"),
           run_compress_adaptive, exp_adaptive_streams, ADAPT_SMALL, ADAPT_RAGGED, ADAPT_DENSE),
    Family("compress_batch_adaptive", ("tic_compress_batch_adaptive_v",),
           _BSLOT_V + ("bslot.d_adapt", "bslot.h_adapt") + _SINGLE + ("d_adapt_stats", "d_adapt_work", "d_adapt_out"), ("d_consts", "d_fallback"),
           run_compress_batch_adaptive, exp_adaptive_streams, ADAPT_SMALL, ADAPT_RAGGED, ADAPT_DENSE),
    Family("compress_scaled", ("tic_compress_scaled", "tic_compress_scaled_dev"), _SINGLE + _ENT, ("d_huff", "d_total_bits", "h_stat"),
           run_compress_scaled, exp_scaled_streams, SCALED_SMALL, SCALED_RAGGED, SCALED_DENSE),
    Family("compress_batch_scaled", ("tic_compress_batch_scaled_v",), _BSLOT_V + ("bslot.h_sframes", "bslot.d_sframes") + _SINGLE + _ENT,
           ("d_huff", "bslot.d_err", "d_total_bits", "h_stat"), run_compress_batch_scaled, exp_scaled_streams, SCALED_SMALL, SCALED_RAGGED, SCALED_DENSE),
    Family("rd_points_scaled_batch", ("tic_rd_points_scaled_v",), _RD_V + ("h_scaled_tabs", "d_scaled_tabs"), ("d_size_tab",),
           run_rd_points_scaled_batch, exp_scaled_rd, SCALED_SMALL, SCALED_RAGGED, SCALED_DENSE),
    Family("compressed_sizes", ("tic_stream_sizes", "tic_stream_sizes_dev"), _RATE, _RATE_STATE, run_compressed_sizes, exp_sizes, SMALL, RAGGED, DENSE),
    Family("compress_to_size", ("tic_compress_to_size", "tic_compress_to_size_dev"), _RATE + _ENT, _RATE_STATE + _ENT_STATE, run_compress_to_size,
           exp_to_size, SMALL, RAGGED, DENSE),
    Family("compressed_sizes_batch", ("tic_stream_sizes_v",), _RATE_V, _RATE_STATE, run_compressed_sizes_batch, exp_sizes_batch, SMALL, RAGGED, DENSE),
    Family("compress_batch_to_size", ("tic_compress_batch_to_size",), _RATE_V + _BSLOT_V + _ENT, _RATE_STATE + _BSLOT_STATE + _ENT_STATE,
           run_compress_batch_to_size, exp_to_size, SMALL, RAGGED, DENSE),
    Family("rd_points", ("tic_rd_points", "tic_rd_points_dev"), _RATE, _RATE_STATE, run_rd_points, exp_rd, SMALL, RAGGED, DENSE),
    Family("compress_to_psnr", ("tic_compress_to_psnr", "tic_compress_to_psnr_dev"), _RATE + _ENT, _RATE_STATE + _ENT_STATE, run_compress_to_psnr,
           exp_to_psnr, SMALL, RAGGED, DENSE),
    Family("rd_points_batch", ("tic_rd_points_v",), _RD_V, _RATE_STATE, run_rd_points_batch, exp_rd_batch, SMALL, RAGGED, DENSE),
    Family("compress_batch_to_psnr", ("tic_compress_batch_to_psnr",), _RD_V + _BSLOT_V + _ENT, _RATE_STATE + _BSLOT_STATE + _ENT_STATE,
           run_compress_batch_to_psnr, exp_to_psnr, SMALL, RAGGED, DENSE),
] + _decoders()
BY_NAME = {f.name: f for f in FAMILIES}

# Entry points that take a context and belong to no family, with the reason each.
EXEMPT = {
    "tic_destroy": "lifecycle: ends the context",
    # (tic_last_*: getters of the last call's figures, exempt by their prefix - test_context_state_cpu.py wants every call in exactly one of
    #  {a family, this table, the prefix}.  tic_last_strip_launch among them: host bookkeeping of the last tic_dctq_dev / tic_dctq_dev_frames
    #  launch - order, schedule kind, teams, grid, fast rectangle - that reads no context buffer and queues nothing.)
    "tic_device_arch": "getter", "tic_numa_info": "getter", "tic_pci_bus_id": "getter", "tic_get_stage_threads": "getter",
    "tic_set_custom_quality": "setter (writes slot 0 of d_consts, which no family reads)", "tic_set_numa_binding": "setter", "tic_set_auto_register": "setter",
    "tic_set_stats": "setter", "tic_set_entropy_lane_kernel": "setter (the after-an-error tests turn it on)", "tic_set_stage_threads": "setter",
    "tic_set_decode_guess": "setter",
    "tic_dev_alloc": "the caller's memory, not the context's", "tic_dev_free": "the caller's memory", "tic_host_alloc_pinned": "the caller's memory",
    "tic_host_free_pinned": "the caller's memory", "tic_host_register": "the caller's memory", "tic_host_unregister": "the caller's memory",
    "tic_memcpy_h2d": "a copy between the caller's buffers", "tic_memcpy_d2h": "a copy between the caller's buffers",
    "tic_memset_dev": "fills the caller's buffer", "tic_sync": "waits only", "tic_test_poison": "the hook itself",
    "tic_comm_create": "tic_comm_*: buffers of the communicator, not of the context", "tic_comm_create_ex": "tic_comm_*: as tic_comm_create",
    "tic_selftest_transpose": "self-test of an instruction sequence on buffers of its own, freed before it returns",
    # transform-only and measuring forms: they write the caller's buffers through d_img / d_coef alone, which the compress family covers
    "tic_dctq": "transform stage of tic_compress alone (d_img, d_coef: covered by compress)",
    "tic_encode": "transform stage of tic_compress alone, host layout",
    "tic_encode_wide": "float64 transform for wide pixels: host entropy coder behind it, no context buffer beside d_img / d_coef",
    # (tic_entropy_encode_dpcm, that host coder, takes no context and is declared in tinyimgcodec_hip_wide.h: nothing to record here;
    #  tests/test_wide_blocks_gpu.py runs tic_encode_wide between the calls of other families and on poisoned contexts)
    "tic_dctq_dev_frames": "transform stage on the caller's device buffers: no context buffer",
    "tic_dctq_batch": "transform stage of tic_compress_batch alone (batch slots: covered by compress_batch)",
    "tic_dctq_scaled": "transform stage of tic_compress_scaled alone", "tic_dctq_scaled_dev": "transform stage of tic_compress_scaled alone",
    "tic_dctq_scaled_dev_frames": "as tic_dctq_dev_frames", "tic_dctq_scaled_v_dev": "transform stage of tic_compress_batch_scaled_v alone",
    "tic_roundtrip_sse_scaled": "one probe of tic_rd_points_scaled_v",
    "tic_entropy_size_dev": "the size kernel of tic_stream_sizes_dev alone", "tic_distortion_dev": "the measuring kernel of tic_rd_points_dev alone",
    "tic_distortion_v_dev": "the measuring kernel of tic_rd_points_v alone",
    "tic_entropy_encode_adaptive": "entropy stage of tic_compress_adaptive alone",
    "tic_entropy_encode_adaptive_batch": "entropy stage of tic_compress_batch_adaptive_v alone",
    "tic_idctq": "inverse stage of tic_decompress alone (d_coef, d_img)", "tic_idctq_scaled": "inverse stage of tic_decompress alone",
    "tic_compress_batch_multi": "one tic_compress_batch per device, each on a context of its own",
    "tic_dctq_dev_timed": "timed loop: its results are times", "tic_dctq_dev_timed_warm": "timed loop", "tic_dctq_dev_frames_timed": "timed loop",
    "tic_dctq_dev_timed_rotating": "timed loop", "tic_entropy_size_dev_timed": "timed loop", "tic_distortion_dev_timed": "timed loop",
    "tic_idct_dev_timed": "timed loop", "tic_distortion_v_dev_timed": "timed loop", "tic_dctq_scaled_dev_timed_warm": "timed loop",
}


def header_context_calls():
    """Every tic_* function of include/tinyimgcodec_hip.h whose first parameter is a context."""
    with open(os.path.join(ROOT, "include", "tinyimgcodec_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return re.findall(r"\b(tic_\w+)\s*\(\s*(?:const\s+)?tic_ctx\s*\*", text)


def sharing_pairs():
    """Every ordered pair (A, B) of families whose records share a scratch buffer name (A == B included: a family after itself)."""
    return [(a, b) for a in FAMILIES for b in FAMILIES if set(a.scratch) & set(b.scratch)]
