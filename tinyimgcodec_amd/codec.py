"""Host-side mirror of the reference's Python API (tinyimgcodec/codec.py) on top of the C-ABI.

Same names, argument meaning and error behaviour as the reference so that it is a drop-in:

    compress(image, quality=50, auto_generate_huffman_table=False) -> bytes      codec.py:133-164
    decompress(data) -> np.ndarray[uint8]                                        codec.py:167-189
    encode(image, quality=50) -> {"height","width","quality","dc","ac"}          codec.py:26-43
    decode(data) -> np.ndarray[uint8]                                            codec.py:46-70

and, for the reference's per-image Huffman tables (compress(image, q, auto_generate_huffman_table=True), codec.py:133-164,
huffman.py:101-194), under names of their own because compress() keeps raising for that flag:

    compress_adaptive(image, quality=50) -> bytes   the reference's adaptive stream, byte for byte
    entropy_encode_adaptive(coeffs_zz, height, width, quality) -> bytes   the same from int16 [N, 64] zig-zag coefficients
    compress_batch_adaptive(images, quality=50) -> [bytes]   compress_adaptive() per frame, any shapes, a quality each, in one call
    entropy_encode_adaptive_batch(coeffs_list, shapes, qualities) -> [bytes]   the same from coefficients
    decompress_adaptive(data) -> np.ndarray[uint8]  reads such a stream as written
    decompress_batch_adaptive(streams) -> [np.ndarray[uint8]]   decompress_adaptive() per stream, any shapes, in one call

and, for the reference's standalone integer encoder (c/img.c, c/encode.c: 8-bit-constant AAN DCT, reciprocal quantiser with four
settings, header flag 1 << 30 - the streams decompress() reads through its scaled_dct branch):

    compress_scaled(image, quality="med") -> bytes        what `encode <width> <height> <setting>` is meant to write (img.c:157-253)
    dctq_scaled(image, quality="med") -> int16 [N, 64]    its coefficients in the device layout (zig-zag, absolute DC)
    entropy_encode_scaled(coeffs_zz, height, width, quality) -> bytes   its entropy stage alone (no GPU needed)

The transform stage (pad, level shift, DCT, quantise, zig-zag) and the entropy stage (DPCM, run lengths, Huffman codes, bit
packing; the Huffman decode and the inverse transform of decompress()) run in hand-written gfx950 kernels; the library's host
entropy coder (C++) serves encode()-style callers that hold coefficients on the host, and streams the device decoder hands back
(damaged or very short ones).  There is no Python or CPU fallback for the device path: without the HIP library and an MI355X these
functions raise tinyimgcodec_amd.NativeUnavailable.

Documented differences from the reference (all outside its working domain):
  * integer pixel values outside 0..255 are transformed as the reference does (exact float64 path on the device, `- 128` and the DC
    difference wrapping in int32) by encode() and compress(), exactly wherever every rounded quotient fits int32 - beyond that the
    reference's own result is numpy's invalid cast and nothing is promised; compress() codes the DC differences as they stand, so the
    running DC may leave int16; the batch and device-layout helpers (compress_batch, dctq) are 8-bit only;
  * encode()/decode() accept float qualities like the reference, integral or not (utils.py:50-53 computes with any number: the
    constants of a non-integral quality in [1, 99] are built per call, tic_set_custom_quality); qualities below 1 or negative (for
    which the reference computes with huge or negative divisors) raise ValueError;
  * auto_generate_huffman_table=True raises NotImplementedError (that path is broken in the reference:
    the table flag is written big-endian and read little-endian, codec.py:111/119); compress_adaptive() writes the reference's
    stream, and decompress() reads it back as the reference does (garbage pixels, flag misread);
  * decompress_adaptive() has no working counterpart in the reference and is strict, unlike decompress(): a malformed table or a
    truncated or damaged stream raises ValueError instead of decoding to garbage;
  * quality > 100 raises ValueError (the reference produces streams with negative divisors);
  * streams whose little-endian flag word has bit 31 set (an embedded Huffman table) raise ValueError in decompress() - what the
    reference raises for every such stream that does not hold a well-formed table; scaled_dct streams (the reference's C encoder) are
    decoded for exponents 0..62 (the C encoder writes 0..3).
"""
import ctypes as C
import math
import struct

import numpy as np

from . import _native as N


def _ctx(ctx):
    return ctx if ctx is not None else N.default_context()


def _check_quality(quality, packs_header):
    """Validates `quality` the way the reference would fail and returns it as an int.

    packs_header=True  (compress): the reference evaluates `5000 / quality` in encode() and then struct.pack("III", ...) in
                       make_header (codec.py:103-108): floats and negatives end in struct.error.
    packs_header=False (encode, dctq, decode): nothing is packed; the reference computes with whatever number it gets.
                       Integral floats give the same divisors as the int and are returned as the int; a non-integral quality
                       in [1, 99] is returned as the float it is (the caller installs its constants: _q_arg); negative values
                       and values below 1 raise ValueError - a documented difference."""
    if isinstance(quality, (bool, np.bool_)):
        quality = int(quality)
    if isinstance(quality, (float, np.floating)):
        if quality == 0:
            raise ZeroDivisionError("float division by zero")  # utils.py:50
        if packs_header:
            struct.pack("I", quality)  # raises struct.error: required argument is not an integer
        if quality != quality:
            raise ValueError("quality is not a number")
        if quality != int(quality):
            if not (1.0 <= quality <= 99.0):
                raise ValueError("non-integral quality %r outside 1..99 is not supported by the MI355X path" % (quality,))
            return float(quality)
        quality = int(quality)
    elif not isinstance(quality, (int, np.integer)):
        raise TypeError("quality must be a number")
    quality = int(quality)
    if quality == 0:
        raise ZeroDivisionError("division by zero")  # utils.py:50
    if quality < 0:
        if packs_header:
            struct.pack("I", quality)  # struct.error, codec.py:103-108
        raise ValueError("negative quality is not supported by the MI355X path")
    if quality == 100:
        if packs_header:
            raise KeyError((0, 0))  # factor 0 -> inf/NaN coefficients -> no Huffman code (huffman.py:62)
        raise ValueError("quality 100 makes every divisor zero (the reference returns inf/NaN garbage)")
    if quality > 100:
        raise ValueError("quality must be in 1..99")
    return quality


def _q_arg(ctx, q):
    """The quality argument of a transform / inverse entry point: the integer itself, or - for a non-integral quality, whose
    constants are installed in the context's spare slot first - TIC_QUALITY_CUSTOM.  Call with ctx.lock held."""
    if isinstance(q, float):
        ctx.check(N.load().tic_set_custom_quality(ctx.handle, q))
        return N.QUALITY_CUSTOM
    return q


def _as_image(image):
    """-> (array, height, width, wide).  uint8-representable images go to the 8-bit device path as uint8; integer images with
    values outside 0..255 (the reference transforms any integers after astype(int32), codec.py:29) as int32 (`wide`)."""
    image = np.asarray(image)
    height, width = image.shape  # ValueError for non 2-D input, as codec.py:27
    if image.dtype == np.uint8:  # the common case needs no conversion pass
        return np.ascontiguousarray(image), int(height), int(width), False
    a = image.astype(np.int32)  # codec.py:29 (truncation of floats, as the reference)
    if a.size and (a.min() < 0 or a.max() > 255):
        return np.ascontiguousarray(a), int(height), int(width), True
    return np.ascontiguousarray(a.astype(np.uint8)), int(height), int(width), False


def _as_u8_image(image):
    img, h, w, wide = _as_image(image)
    if wide:
        raise ValueError("pixel values outside 0..255: use encode()/compress() (the int16 device layout of dctq()/compress_batch() is 8-bit only)")
    return img, h, w


def _encode_wide(img, h, w, q, ctx):
    L = N.load()
    n = L.tic_num_blocks(h, w)
    dc = np.zeros(n, dtype=np.int32)
    ac = np.zeros((n, 63), dtype=np.int32)
    if n:
        with ctx.lock:
            ctx.check(L.tic_encode_wide(ctx.handle, img.ctypes.data, h, w, img.strides[0] // 4, _q_arg(ctx, q), dc.ctypes.data, ac.ctypes.data))
    return dc, ac


def dctq(image, quality=50, ctx=None):
    """Transform stage in the device layout: int16 [N, 64], zig-zag order, DC not differenced."""
    img, h, w = _as_u8_image(image)
    quality = _check_quality(quality, packs_header=False)
    ctx = _ctx(ctx)
    n = N.load().tic_num_blocks(h, w)
    zz = np.zeros((n, 64), dtype=np.int16)
    if n:
        with ctx.lock:
            ctx.check(N.load().tic_dctq(ctx.handle, img.ctypes.data, h, w, img.strides[0], _q_arg(ctx, quality), zz.ctypes.data))
    return zz


def encode(image, quality=50, ctx=None):
    img, h, w, wide = _as_image(image)
    q = _check_quality(quality, packs_header=False)
    ctx = _ctx(ctx)
    if wide:
        dc, ac = _encode_wide(img, h, w, q, ctx)
        return {"height": h, "width": w, "quality": quality, "dc": dc, "ac": ac}
    n = N.load().tic_num_blocks(h, w)
    dc = np.zeros(n, dtype=np.int32)
    ac = np.zeros((n, 63), dtype=np.int32)
    if n:
        with ctx.lock:
            ctx.check(N.load().tic_encode(ctx.handle, img.ctypes.data, h, w, img.strides[0], _q_arg(ctx, q), dc.ctypes.data, ac.ctypes.data))
    return {"height": h, "width": w, "quality": quality, "dc": dc, "ac": ac}


def compress(image, quality=50, auto_generate_huffman_table=False, ctx=None):
    img, h, w, wide = _as_image(image)
    q = _check_quality(quality, packs_header=True)
    if auto_generate_huffman_table:
        raise NotImplementedError("auto_generate_huffman_table=True is not supported by compress() (broken in the reference): "
                                  "use compress_adaptive()")
    ctx = _ctx(ctx)
    L = N.load()
    if wide:  # integer pixels outside 0..255: exact float64 transform on the device, host entropy coder
        # (the reference codes the DC differences as encode() returns them, codec.py:153-162: the running DC may leave int16)
        dc, ac = _encode_wide(img, h, w, q, ctx)
        return _entropy_encode_dpcm(dc, ac, h, w, q)
    cap = L.tic_compress_bound(h, w)
    # worst-case sized landing buffer kept on the context: a fresh 50 MB mapping per call would be faulted in page by page
    # under the device-to-host copy (20+ ms for a 4096x4096 frame whose whole C-level round trip takes 0.6 ms)
    # (the buffer belongs to the context: the context's lock is held from the call to the copy into the returned bytes)
    with ctx.lock:
        out = getattr(ctx, "_out_buf", None)
        if out is None or out.size < cap:
            out = ctx._out_buf = np.empty(cap, dtype=np.uint8)
        n = C.c_size_t(0)
        rc = L.tic_compress(ctx.handle, img.ctypes.data, h, w, img.strides[0] if img.size else max(w, 1), q, out.ctypes.data, cap, C.byref(n))
        if rc == N.TIC_E_RANGE:
            raise KeyError("coefficient magnitude has no Huffman code")  # as the reference's dict lookup
        ctx.check(rc)
        return out[: n.value].tobytes()


def compress_batch(images, quality=50, threads=0, ctx=None, devices=None):
    """Batch of frames through the stream-overlapped pipeline -> list of bytes (frame order).

    Frames of one shape at one quality (an int): threads=0: entropy stage on the GPU; threads>0: host entropy coder on that many worker threads.
    devices=[0, 1, ...]: the batch is cut into contiguous shards, one per listed device, and every shard runs its own pipeline on its
    own context and host thread inside this process (tic_compress_batch_multi; the GIL is released for the whole call) - the
    multi-GPU form of a loop over images (/root/reference/tests/benchmark.py:12-23) without a launcher.  A device may be listed
    twice (two pipelines on one GPU).

    Frames of different shapes, or `quality` a sequence with one entry per frame: one call of tic_compress_batch_v, entropy stage on the GPU -
    the reference's whole loop over image x quality, or a folder of photographs, in one call; every stream is what compress(image, q) gives.
    Such a mixed call takes neither threads > 0 nor devices= (ValueError)."""
    per_frame = not isinstance(quality, (int, float, np.integer, np.floating, bool, np.bool_, str, bytes)) and hasattr(quality, "__len__")
    if per_frame:
        frames = [_as_u8_image(im) for im in images]
        if len(quality) != len(frames):
            raise ValueError("quality has %d entries for %d frames" % (len(quality), len(frames)))
        qs = [_check_quality(qi, packs_header=True) for qi in quality]
        if not frames:
            return []
        return _compress_batch_mixed(frames, qs, threads, ctx, devices)
    q = _check_quality(quality, packs_header=True)
    frames = [_as_u8_image(im) for im in images]
    if not frames:
        return []
    if any((f[1], f[2]) != (frames[0][1], frames[0][2]) for f in frames):
        return _compress_batch_mixed(frames, [q] * len(frames), threads, ctx, devices)
    if devices is not None:
        return _compress_batch_multi(frames, q, int(threads), list(devices))
    ctx = _ctx(ctx)
    h, w = frames[0][1], frames[0][2]
    if any((f[1], f[2]) != (h, w) for f in frames):
        raise ValueError("all frames of a batch must have the same shape")
    L = N.load()
    n = len(frames)
    cap = L.tic_compress_bound(h, w)
    # one mapping, kept on the context: only the bytes actually written are ever touched, and a second batch of the same
    # geometry finds them already faulted in (first-touch page faults cost more than the whole GPU pipeline)
    with ctx.lock:
        pool = getattr(ctx, "_batch_pool", None)
        if pool is None or pool.shape[0] < n or pool.shape[1] != cap:
            pool = ctx._batch_pool = np.empty((n, cap), dtype=np.uint8)
        outs = [pool[i] for i in range(n)]
        inp = (C.c_void_p * n)(*[f[0].ctypes.data for f in frames])
        outp = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        caps = (C.c_size_t * n)(*([cap] * n))
        lens = (C.c_size_t * n)()
        rc = L.tic_compress_batch(ctx.handle, inp, n, h, w, max(w, 1), q, outp, caps, lens, int(threads))
        if rc == N.TIC_E_RANGE:
            raise KeyError("coefficient magnitude has no Huffman code")
        ctx.check(rc)
        return [outs[i][: lens[i]].tobytes() for i in range(n)]


def _compress_batch_mixed(frames, qs, threads, ctx, devices):
    """Frames of any shapes, a quality each: tic_compress_batch_v, with a pool of per-frame capacities kept on the context."""
    if int(threads) > 0:
        raise ValueError("a batch of mixed shapes or qualities is not supported with threads > 0 (device entropy stage only)")
    if devices is not None:
        raise ValueError("a batch of mixed shapes or qualities is not supported with devices= (one context only)")
    ctx = _ctx(ctx)
    L = N.load()
    n = len(frames)
    caps_l = [L.tic_compress_bound(f[1], f[2]) for f in frames]
    offs = np.concatenate(([0], np.cumsum([(c + 63) // 64 * 64 for c in caps_l]))).astype(np.int64)
    with ctx.lock:
        pool = getattr(ctx, "_mixed_pool", None)
        if pool is None or pool.size < offs[-1]:
            pool = ctx._mixed_pool = np.empty(int(offs[-1]), dtype=np.uint8)
        base = pool.ctypes.data
        inp = (C.c_void_p * n)(*[f[0].ctypes.data if f[0].size else None for f in frames])
        hs = (C.c_int * n)(*[f[1] for f in frames])
        ws = (C.c_int * n)(*[f[2] for f in frames])
        strides = (C.c_ssize_t * n)(*[max(f[2], 1) for f in frames])
        qa = (C.c_int * n)(*qs)
        outp = (C.c_void_p * n)(*[base + int(o) for o in offs[:-1]])
        caps = (C.c_size_t * n)(*caps_l)
        lens = (C.c_size_t * n)()
        rc = L.tic_compress_batch_v(ctx.handle, inp, n, hs, ws, strides, qa, outp, caps, lens)
        if rc == N.TIC_E_RANGE:
            raise KeyError("coefficient magnitude has no Huffman code")
        ctx.check(rc)
        return [pool[int(offs[i]): int(offs[i]) + lens[i]].tobytes() for i in range(n)]


def _compress_batch_multi(frames, q, threads, devices):
    if not devices:
        raise ValueError("devices must name at least one device")
    ctxs = N.device_contexts(devices)
    h, w = frames[0][1], frames[0][2]
    if any((f[1], f[2]) != (h, w) for f in frames):
        raise ValueError("all frames of a batch must have the same shape")
    L = N.load()
    n = len(frames)
    cap = L.tic_compress_bound(h, w)
    pool = np.empty((n, cap), dtype=np.uint8)
    handles = (C.c_void_p * len(ctxs))(*[c.handle for c in ctxs])
    inp = (C.c_void_p * n)(*[f[0].ctypes.data for f in frames])
    outp = (C.c_void_p * n)(*[pool[i].ctypes.data for i in range(n)])
    caps = (C.c_size_t * n)(*([cap] * n))
    lens = (C.c_size_t * n)()
    failed = C.c_int(-1)
    locked = sorted(ctxs, key=id)  # (one global order: two threads that list the same devices in different orders cannot deadlock)
    for c in locked:
        c.lock.acquire()
    try:
        rc = L.tic_compress_batch_multi(handles, len(ctxs), inp, n, h, w, max(w, 1), q, outp, caps, lens, threads, C.byref(failed))
        if rc == N.TIC_E_RANGE:
            raise KeyError("coefficient magnitude has no Huffman code")
        if rc != N.TIC_OK:
            ctxs[max(failed.value, 0)].check(rc)
    finally:
        for c in reversed(locked):
            c.lock.release()
    return [pool[i, : lens[i]].tobytes() for i in range(n)]


def entropy_encode(coeffs_zz, height, width, quality):
    """Host entropy stage alone (no GPU needed): int16 [N,64] zig-zag coefficients -> stream bytes."""
    L = N.load()
    zz = np.ascontiguousarray(coeffs_zz, dtype=np.int16)
    cap = L.tic_compress_bound(height, width)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = L.tic_entropy_encode(zz.ctypes.data, int(height), int(width), int(quality), out.ctypes.data, cap, C.byref(n))
    if rc == N.TIC_E_RANGE:
        raise KeyError("coefficient magnitude has no Huffman code")
    if rc != N.TIC_OK:
        raise N.NativeError(rc, "tic_entropy_encode failed")
    return out[: n.value].tobytes()


def _entropy_encode_dpcm(dc, ac, height, width, quality):
    """Host entropy stage on encode()'s own arrays (no GPU needed): int32 [N] DC differences and int32 [N, 63] AC values -> stream
    bytes.  KeyError where a difference or an AC value has no Huffman code, as the reference's dict lookup - never for the running DC."""
    L = N.load()
    n = L.tic_num_blocks(int(height), int(width))
    dc = np.ascontiguousarray(dc, dtype=np.int32)
    ac = np.ascontiguousarray(ac, dtype=np.int32)
    if dc.shape != (n,) or ac.shape != (n, 63):
        raise ValueError("dc of shape %r and ac of shape %r do not match %d blocks" % (dc.shape, ac.shape, n))
    cap = L.tic_compress_bound(int(height), int(width))
    out = np.empty(cap, dtype=np.uint8)
    length = C.c_size_t(0)
    rc = L.tic_entropy_encode_dpcm(dc.ctypes.data, ac.ctypes.data, int(height), int(width), int(quality), out.ctypes.data, cap, C.byref(length))
    if rc == N.TIC_E_RANGE:
        raise KeyError("coefficient magnitude has no Huffman code")
    if rc != N.TIC_OK:
        raise N.NativeError(rc, "tic_entropy_encode_dpcm failed")
    return out[: length.value].tobytes()


def entropy_size(coeffs_zz, height, width):
    """len(entropy_encode(coeffs_zz, height, width, q)) for any quality, from a walk that only sums code lengths (no GPU needed).
    KeyError where entropy_encode raises it."""
    L = N.load()
    height, width = int(height), int(width)
    zz = np.ascontiguousarray(coeffs_zz, dtype=np.int16)
    if height < 0 or width < 0:
        raise ValueError("negative image size")
    nb = L.tic_num_blocks(height, width)
    if zz.size != nb * 64:
        raise ValueError("coefficients of shape %r do not match %d blocks of 64" % (zz.shape, nb))
    n = C.c_size_t(0)
    rc = L.tic_entropy_size(zz.ctypes.data, height, width, C.byref(n))
    if rc == N.TIC_E_RANGE:
        raise KeyError("coefficient magnitude has no Huffman code")
    if rc != N.TIC_OK:
        raise N.NativeError(rc, "tic_entropy_size failed")
    return int(n.value)


def compressed_sizes(image, qualities, ctx=None):
    """len(compress(image, q)) for every q of `qualities` -> int64 array, -1 where compress() would raise KeyError for a coefficient
    without a Huffman code.  No stream is produced: per quality the transform and a size kernel that reads the coefficients once, all
    queued without a host wait in between, one read-back.  8-bit images only (ValueError otherwise, as compress_batch); an invalid
    quality raises what compress() raises for it, before any GPU work."""
    img, h, w = _as_u8_image(image)
    qs = [_check_quality(q, packs_header=True) for q in qualities]
    sizes = np.zeros(len(qs), dtype=np.int64)
    if not qs:
        return sizes
    ctx = _ctx(ctx)
    qarr = np.asarray(qs, dtype=np.intc)
    with ctx.lock:
        ctx.check(N.load().tic_stream_sizes(ctx.handle, img.ctypes.data, h, w, img.strides[0] if img.size else max(w, 1), qarr.ctypes.data, len(qs),
                                            sizes.ctypes.data))
    return sizes


def compressed_size(image, quality=50, ctx=None):
    """len(compress(image, quality)) without producing the stream; the same exceptions for the same arguments."""
    size = int(compressed_sizes(image, [quality], ctx=ctx)[0])
    if size < 0:
        raise KeyError("coefficient magnitude has no Huffman code")  # as the reference's dict lookup
    return size


def compress_to_size(image, max_bytes, min_quality=1, max_quality=99, ctx=None):
    """The best stream within a byte budget -> (bytes, quality): compress(image, quality) of the quality at which a bisection over
    min_quality..max_quality ends, with "compress() succeeds and len(...) <= max_bytes" as its test -

        lo, hi = min_quality, max_quality
        while lo < hi: mid = (lo + hi + 1) // 2;  lo = mid if fits(mid) else hi = mid - 1

    which is the largest fitting quality wherever sizes do not decrease with the quality (observed on every image tried; a quality at
    which a coefficient has no Huffman code counts as not fitting).  The probes run on the GPU without producing streams
    (compressed_sizes) and several steps ahead per submission.  ValueError naming the size at min_quality when even that exceeds the
    budget, KeyError when min_quality has a coefficient without a code; 8-bit images only."""
    img, h, w = _as_u8_image(image)
    qmin = _check_quality(min_quality, packs_header=True)
    qmax = _check_quality(max_quality, packs_header=True)
    if qmin > qmax:
        raise ValueError("min_quality %d above max_quality %d" % (qmin, qmax))
    max_bytes = int(max_bytes)
    if max_bytes < 0:
        raise ValueError("max_bytes must not be negative")
    ctx = _ctx(ctx)
    L = N.load()
    cap = L.tic_compress_bound(h, w)
    with ctx.lock:
        out = getattr(ctx, "_out_buf", None)  # compress()'s landing buffer
        if out is None or out.size < cap:
            out = ctx._out_buf = np.empty(cap, dtype=np.uint8)
        n, q = C.c_size_t(0), C.c_int(0)
        rc = L.tic_compress_to_size(ctx.handle, img.ctypes.data, h, w, img.strides[0] if img.size else max(w, 1), max_bytes, qmin, qmax,
                                    out.ctypes.data, cap, C.byref(n), C.byref(q))
        if rc == N.TIC_E_RANGE:
            raise KeyError("coefficient magnitude has no Huffman code")
        if rc == N.TIC_E_SPACE:
            raise ValueError("%d bytes at quality %d exceed max_bytes = %d" % (n.value, qmin, max_bytes))
        ctx.check(rc)
        return out[: n.value].tobytes(), int(q.value)


def _frame_arrays(frames):
    """The per-frame arguments the calls for mixed frames share: image pointers, heights, widths, row strides."""
    n = len(frames)
    inp = (C.c_void_p * n)(*[f[0].ctypes.data if f[0].size else None for f in frames])
    hs = (C.c_int * n)(*[f[1] for f in frames])
    ws = (C.c_int * n)(*[f[2] for f in frames])
    strides = (C.c_ssize_t * n)(*[max(f[2], 1) for f in frames])
    return inp, hs, ws, strides


def compressed_sizes_batch(images, qualities, ctx=None):
    """compressed_sizes(image, qualities) of every image of a list, of any shapes, in one call -> int64 array (n, nq); -1 where compress()
    would raise KeyError.  The reference's whole benchmark table (49 images x 6 qualities) is one call: per chunk of up to 64 frames one
    upload, every probe queued, one read-back (tic_stream_sizes_v).  8-bit images only; an invalid quality raises what compress() raises for
    it, before any GPU work."""
    frames = [_as_u8_image(im) for im in images]
    qs = [_check_quality(q, packs_header=True) for q in qualities]
    sizes = np.zeros((len(frames), len(qs)), dtype=np.int64)
    if not frames or not qs:
        return sizes
    ctx = _ctx(ctx)
    qarr = np.asarray(qs, dtype=np.intc)
    inp, hs, ws, strides = _frame_arrays(frames)
    with ctx.lock:
        ctx.check(N.load().tic_stream_sizes_v(ctx.handle, inp, len(frames), hs, ws, strides, qarr.ctypes.data, len(qs), sizes.ctypes.data))
    return sizes


def compress_batch_to_size(images, max_bytes, min_quality=1, max_quality=99, ctx=None):
    """compress_to_size(image, max_bytes, min_quality, max_quality) of every image of a list, of any shapes, in one call ->
    [(bytes, quality), ...].  max_bytes: one budget for all, or a sequence with one per frame.  The bisections of up to 64 frames run in
    lockstep - one submission and one wait per round for all of them - and the streams of all frames come from one mixed batch
    (tic_compress_batch_to_size).  Argument errors are compress_to_size's, raised before any GPU work; a frame that fails raises, for the
    first such frame, what compress_to_size raises for it, the message prefixed "frame i: ".  8-bit images only."""
    frames = [_as_u8_image(im) for im in images]
    qmin = _check_quality(min_quality, packs_header=True)
    qmax = _check_quality(max_quality, packs_header=True)
    if qmin > qmax:
        raise ValueError("min_quality %d above max_quality %d" % (qmin, qmax))
    n = len(frames)
    if hasattr(max_bytes, "__len__"):
        if len(max_bytes) != n:
            raise ValueError("max_bytes has %d entries for %d frames" % (len(max_bytes), n))
        budgets = [int(b) for b in max_bytes]
    else:
        budgets = [int(max_bytes)] * n
    if any(b < 0 for b in budgets):
        raise ValueError("max_bytes must not be negative")
    if not frames:
        return []
    ctx = _ctx(ctx)
    L = N.load()
    caps_l = [L.tic_compress_bound(f[1], f[2]) for f in frames]
    offs = np.concatenate(([0], np.cumsum([(c + 63) // 64 * 64 for c in caps_l]))).astype(np.int64)
    inp, hs, ws, strides = _frame_arrays(frames)
    with ctx.lock:
        pool = getattr(ctx, "_mixed_pool", None)  # compress_batch()'s landing buffer for mixed frames
        if pool is None or pool.size < offs[-1]:
            pool = ctx._mixed_pool = np.empty(int(offs[-1]), dtype=np.uint8)
        base = pool.ctypes.data
        outp = (C.c_void_p * n)(*[base + int(o) for o in offs[:-1]])
        caps = (C.c_size_t * n)(*caps_l)
        budg = (C.c_size_t * n)(*budgets)
        lens = (C.c_size_t * n)()
        qout = (C.c_int * n)()
        status = (C.c_int * n)()
        rc = L.tic_compress_batch_to_size(ctx.handle, inp, n, hs, ws, strides, budg, qmin, qmax, outp, caps, lens, qout, status)
        bad = next((i for i in range(n) if status[i] != N.TIC_OK), None)
        if bad is None:
            ctx.check(rc)  # (a failure of the call itself: no frame to name)
        elif status[bad] == N.TIC_E_RANGE:
            raise KeyError("frame %d: coefficient magnitude has no Huffman code" % bad)
        elif status[bad] == N.TIC_E_SPACE:
            raise ValueError("frame %d: %d bytes at quality %d exceed max_bytes = %d" % (bad, lens[bad], qmin, budgets[bad]))
        else:
            ctx.check(status[bad])
        return [(pool[int(offs[i]): int(offs[i]) + lens[i]].tobytes(), int(qout[i])) for i in range(n)]


def psnr_from_sse(sse, npixels, max_pixel=255):
    """PSNR in dB from a sum of squared differences over `npixels` pixels, with the operations of the reference's tests/psnr.py (its
    np.mean of the squares is the exact integer sum divided by the count): inf for a sum of 0.  The one place PSNR is defined for
    roundtrip_psnr and compress_to_psnr.  Fed the wrapped sum (rd_points' third array) it returns the very float the reference's
    psnr() returns for the two uint8 arrays - that function squares uint8 differences in uint8 arithmetic."""
    sse, npixels = int(sse), int(npixels)
    if sse < 0 or npixels < 0:
        raise ValueError("negative sum or pixel count")
    if sse == 0:
        return math.inf
    mse = sse / npixels
    return 20 * math.log10(max_pixel / mse ** 0.5)


def max_sse_for_psnr(min_psnr, npixels):
    """The largest integer sum of squared differences over `npixels` pixels whose psnr_from_sse is still >= min_psnr (0 for inf: an
    exact round trip), capped at 255^2 per pixel, which no 8-bit round trip exceeds.  Computed from the inverted formula, then corrected
    against the predicate itself, so that `psnr_from_sse(s, n) >= min_psnr` and `s <= max_sse_for_psnr(min_psnr, n)` agree for every
    reachable s."""
    min_psnr, npixels = float(min_psnr), int(npixels)
    if math.isnan(min_psnr):
        raise ValueError("min_psnr is not a number")
    top = npixels * 255 * 255
    if min_psnr == math.inf or npixels == 0:
        return 0
    if psnr_from_sse(top, npixels) >= min_psnr:
        return top
    est = min(top, max(0, int(npixels * 255.0 * 255.0 / 10.0 ** (min_psnr / 10.0)))) if min_psnr < 3000 else 0
    while est > 0 and not psnr_from_sse(est, npixels) >= min_psnr:
        est -= 1
    while est < top and psnr_from_sse(est + 1, npixels) >= min_psnr:
        est += 1
    return est


def rd_points(image, qualities, ctx=None):
    """Rate and distortion at every q of `qualities` from one submission -> (sizes int64, sse uint64, sse_wrapped uint64):
    sizes as compressed_sizes (-1 where compress() would raise KeyError); sse[i] the exact sum of squared differences between the image
    and decompress(compress(image, q)), sse_wrapped[i] the sum of those squares modulo 256, which is what the reference's tests/psnr.py
    sums - both reported for the -1 entries too.  No stream is produced and no frame decoded into memory: per quality the transform, the
    size kernel and a measuring instance of the inverse transform, one read-back.  Validation as compressed_sizes."""
    img, h, w = _as_u8_image(image)
    qs = [_check_quality(q, packs_header=True) for q in qualities]
    sizes = np.zeros(len(qs), dtype=np.int64)
    sse = np.zeros(len(qs), dtype=np.uint64)
    wrapped = np.zeros(len(qs), dtype=np.uint64)
    if not qs:
        return sizes, sse, wrapped
    ctx = _ctx(ctx)
    qarr = np.asarray(qs, dtype=np.intc)
    with ctx.lock:
        ctx.check(N.load().tic_rd_points(ctx.handle, img.ctypes.data, h, w, img.strides[0] if img.size else max(w, 1), qarr.ctypes.data, len(qs),
                                         sizes.ctypes.data, sse.ctypes.data, wrapped.ctypes.data))
    return sizes, sse, wrapped


def roundtrip_psnr(image, quality=50, reference_arithmetic=False, ctx=None):
    """PSNR of decompress(compress(image, quality)) against the image, from the exact squared error (rd_points).  With
    reference_arithmetic=True the float the reference's tests/psnr.py returns for that pair, which wraps every squared difference to
    8 bits (Lenna at quality 50: 35.8 dB that way, 35.41 dB in truth).  KeyError where compress() raises it."""
    img, h, w = _as_u8_image(image)
    sizes, sse, wrapped = rd_points(img, [quality], ctx=ctx)
    if sizes[0] < 0:
        raise KeyError("coefficient magnitude has no Huffman code")  # as the reference's dict lookup
    return psnr_from_sse(int(wrapped[0] if reference_arithmetic else sse[0]), h * w)


def compress_to_psnr(image, min_psnr, min_quality=1, max_quality=99, ctx=None):
    """The smallest stream at no less than `min_psnr` dB -> (bytes, quality, psnr): compress(image, quality) of the quality at which a
    bisection over min_quality..max_quality ends, with "compress() succeeds and the PSNR of its round trip is >= min_psnr" as its test -

        lo, hi = min_quality, max_quality
        while lo < hi: mid = (lo + hi) // 2;  hi = mid if meets(mid) else lo = mid + 1

    which is the smallest quality that meets the target wherever the error does not grow with the quality.  The PSNR is the true one
    (psnr_from_sse of the exact squared error); min_psnr = inf asks for an exact round trip.  The probes run on the GPU without streams
    or decoded frames (rd_points) and several steps ahead per submission.  ValueError naming the PSNR at max_quality when even that
    falls short; KeyError when max_quality has a coefficient without a Huffman code (on photographs 98 and 99 usually have one: pass a
    lower max_quality); 8-bit images only."""
    img, h, w = _as_u8_image(image)
    qmin = _check_quality(min_quality, packs_header=True)
    qmax = _check_quality(max_quality, packs_header=True)
    if qmin > qmax:
        raise ValueError("min_quality %d above max_quality %d" % (qmin, qmax))
    max_sse = max_sse_for_psnr(min_psnr, h * w)
    ctx = _ctx(ctx)
    L = N.load()
    cap = L.tic_compress_bound(h, w)
    with ctx.lock:
        out = getattr(ctx, "_out_buf", None)  # compress()'s landing buffer
        if out is None or out.size < cap:
            out = ctx._out_buf = np.empty(cap, dtype=np.uint8)
        n, q, sse = C.c_size_t(0), C.c_int(0), C.c_uint64(0)
        rc = L.tic_compress_to_psnr(ctx.handle, img.ctypes.data, h, w, img.strides[0] if img.size else max(w, 1), max_sse, qmin, qmax,
                                    out.ctypes.data, cap, C.byref(n), C.byref(q), C.byref(sse))
        if rc == N.TIC_E_RANGE:
            raise KeyError("coefficient magnitude has no Huffman code")
        if rc == N.TIC_E_SPACE and n.value == 0:  # (a stream that does not fit cap reports its length; cap is the bound here)
            raise ValueError("%r dB at quality %d fall short of min_psnr = %r" % (psnr_from_sse(sse.value, h * w), qmax, float(min_psnr)))
        ctx.check(rc)
        return out[: n.value].tobytes(), int(q.value), psnr_from_sse(sse.value, h * w)


def rd_points_batch(images, qualities, ctx=None):
    """rd_points(image, qualities) of every image of a list, of any shapes, in one call -> (sizes int64 (n, nq), sse uint64 (n, nq),
    sse_wrapped uint64 (n, nq)).  The reference's benchmark loop compress -> decompress -> psnr over 49 images x 6 qualities is one call:
    per chunk of up to 64 frames one upload, every probe queued, one launch of the size kernel and one of the measuring kernel per 64
    probes, one read-back (tic_rd_points_v).  Validation as compressed_sizes_batch."""
    frames = [_as_u8_image(im) for im in images]
    qs = [_check_quality(q, packs_header=True) for q in qualities]
    sizes = np.zeros((len(frames), len(qs)), dtype=np.int64)
    sse = np.zeros((len(frames), len(qs)), dtype=np.uint64)
    wrapped = np.zeros((len(frames), len(qs)), dtype=np.uint64)
    if not frames or not qs:
        return sizes, sse, wrapped
    ctx = _ctx(ctx)
    qarr = np.asarray(qs, dtype=np.intc)
    inp, hs, ws, strides = _frame_arrays(frames)
    with ctx.lock:
        ctx.check(N.load().tic_rd_points_v(ctx.handle, inp, len(frames), hs, ws, strides, qarr.ctypes.data, len(qs), sizes.ctypes.data,
                                           sse.ctypes.data, wrapped.ctypes.data))
    return sizes, sse, wrapped


def compress_batch_to_psnr(images, min_psnr, min_quality=1, max_quality=99, ctx=None):
    """compress_to_psnr(image, min_psnr, min_quality, max_quality) of every image of a list, of any shapes, in one call ->
    [(bytes, quality, psnr), ...].  min_psnr: one target for all, or a sequence with one per frame; each frame's bound is
    max_sse_for_psnr of its target over its own h * w pixels, its psnr is psnr_from_sse of its exact squared error.  The bisections of up
    to 64 frames run in lockstep - one submission and one wait per round for all of them - and the streams of all frames come from one
    mixed batch (tic_compress_batch_to_psnr).  Argument errors are compress_to_psnr's, raised before any GPU work; a frame that fails
    raises, for the first such frame, what compress_to_psnr raises for it, the message prefixed "frame i: ".  8-bit images only."""
    frames = [_as_u8_image(im) for im in images]
    qmin = _check_quality(min_quality, packs_header=True)
    qmax = _check_quality(max_quality, packs_header=True)
    if qmin > qmax:
        raise ValueError("min_quality %d above max_quality %d" % (qmin, qmax))
    n = len(frames)
    if hasattr(min_psnr, "__len__"):
        if len(min_psnr) != n:
            raise ValueError("min_psnr has %d entries for %d frames" % (len(min_psnr), n))
        targets = [float(t) for t in min_psnr]
    else:
        targets = [float(min_psnr)] * n
    bounds = [max_sse_for_psnr(t, f[1] * f[2]) for t, f in zip(targets, frames)]
    if not frames:
        return []
    ctx = _ctx(ctx)
    L = N.load()
    caps_l = [L.tic_compress_bound(f[1], f[2]) for f in frames]
    offs = np.concatenate(([0], np.cumsum([(c + 63) // 64 * 64 for c in caps_l]))).astype(np.int64)
    inp, hs, ws, strides = _frame_arrays(frames)
    with ctx.lock:
        pool = getattr(ctx, "_mixed_pool", None)  # compress_batch()'s landing buffer for mixed frames
        if pool is None or pool.size < offs[-1]:
            pool = ctx._mixed_pool = np.empty(int(offs[-1]), dtype=np.uint8)
        base = pool.ctypes.data
        outp = (C.c_void_p * n)(*[base + int(o) for o in offs[:-1]])
        caps = (C.c_size_t * n)(*caps_l)
        bnd = (C.c_uint64 * n)(*bounds)
        lens = (C.c_size_t * n)()
        qout = (C.c_int * n)()
        sse = (C.c_uint64 * n)()
        status = (C.c_int * n)()
        rc = L.tic_compress_batch_to_psnr(ctx.handle, inp, n, hs, ws, strides, bnd, qmin, qmax, outp, caps, lens, qout, sse, status)
        bad = next((i for i in range(n) if status[i] != N.TIC_OK), None)
        npix = [f[1] * f[2] for f in frames]
        if bad is None:
            ctx.check(rc)  # (a failure of the call itself: no frame to name)
        elif status[bad] == N.TIC_E_RANGE:
            raise KeyError("frame %d: coefficient magnitude has no Huffman code" % bad)
        elif status[bad] == N.TIC_E_SPACE and lens[bad] == 0:
            raise ValueError("frame %d: %r dB at quality %d fall short of min_psnr = %r"
                             % (bad, psnr_from_sse(sse[bad], npix[bad]), qmax, targets[bad]))
        else:
            ctx.check(status[bad])
        return [(pool[int(offs[i]): int(offs[i]) + lens[i]].tobytes(), int(qout[i]), psnr_from_sse(sse[i], npix[i])) for i in range(n)]


SCALED_SETTINGS = ("best", "high", "med", "low")  # encode.c:20-34; the header's quality field holds the index


def _scaled_setting(quality):
    """"best" | "high" | "med" | "low" or 0..3 -> 0..3 (ValueError for anything else; the reference program prints "Invalid quality factor")."""
    if isinstance(quality, str):
        if quality in SCALED_SETTINGS:
            return SCALED_SETTINGS.index(quality)
    elif isinstance(quality, (int, np.integer)) and not isinstance(quality, (bool, np.bool_)) and 0 <= int(quality) <= 3:
        return int(quality)
    raise ValueError("scaled-DCT quality must be one of %r or 0..3, not %r" % (SCALED_SETTINGS, quality))


def _scaled_image(image):
    img, h, w = _as_u8_image(image)  # 8-bit pixels only (ValueError otherwise), as compress_batch
    if h % 8 or w % 8:
        raise ValueError("Width and height must be multiples of 8")  # encode.c:37-39
    return img, h, w


def dctq_scaled(image, quality="med", ctx=None):
    """Transform stage of the reference's integer encoder (IMG_fdct + IMG_quantize, img.c:47-125, 194-205) on the GPU, in the device
    layout: int16 [N, 64], zig-zag order, DC not differenced."""
    img, h, w = _scaled_image(image)
    qf = _scaled_setting(quality)
    L = N.load()
    n = L.tic_num_blocks(h, w)
    zz = np.zeros((n, 64), dtype=np.int16)
    if n:
        ctx = _ctx(ctx)
        with ctx.lock:
            ctx.check(L.tic_dctq_scaled(ctx.handle, img.ctypes.data, h, w, img.strides[0], qf, zz.ctypes.data))
    return zz


def roundtrip_sse_scaled(image, quality="med", ctx=None):
    """(sse, sse_wrapped) of decompress(compress_scaled(image, quality)) against the image - the distortion column of the reference's
    tests/cbenchmark.py - as exact integers, from the integer encoder's coefficients and a measuring instance of the inverse transform:
    no stream, no decoded frame.  psnr_from_sse turns either into dB (the wrapped sum into the reference's own figure)."""
    img, h, w = _scaled_image(image)
    qf = _scaled_setting(quality)
    sums = (C.c_uint64 * 2)(0, 0)
    if N.load().tic_num_blocks(h, w):
        ctx = _ctx(ctx)
        with ctx.lock:
            ctx.check(N.load().tic_roundtrip_sse_scaled(ctx.handle, img.ctypes.data, h, w, img.strides[0], qf, sums))
    return int(sums[0]), int(sums[1])


def compress_scaled(image, quality="med", ctx=None):
    """The stream of the reference's integer encoder (c/img.c: IMG_init, IMG_encodeHeader, IMG_encodeBlock per block,
    IMG_encodeComplete), byte for byte; every stage on the GPU.  quality: "best" | "high" | "med" | "low" or 0..3 (default as
    encode.c:33).  KeyError when a coefficient has no Huffman code (|AC| > 1023, possible at "best" only: the C encoder reads past its
    table there)."""
    img, h, w = _scaled_image(image)
    qf = _scaled_setting(quality)
    ctx = _ctx(ctx)
    L = N.load()
    cap = L.tic_compress_scaled_bound(h, w)
    with ctx.lock:
        out = getattr(ctx, "_out_buf", None)  # compress()'s landing buffer
        if out is None or out.size < cap:
            out = ctx._out_buf = np.empty(cap, dtype=np.uint8)
        n = C.c_size_t(0)
        rc = L.tic_compress_scaled(ctx.handle, img.ctypes.data, h, w, img.strides[0] if img.size else max(w, 1), qf, out.ctypes.data, cap, C.byref(n))
        if rc == N.TIC_E_RANGE:
            raise KeyError("coefficient magnitude has no Huffman code")
        ctx.check(rc)
        return out[: n.value].tobytes()


def _per_frame_settings(quality, n):
    """One setting (a name or 0..3) for all n frames, or a sequence with one per frame -> list of 0..3."""
    if isinstance(quality, (str, bytes, int, np.integer, float, np.floating, bool, np.bool_)) or not hasattr(quality, "__len__"):
        return [_scaled_setting(quality)] * n
    if len(quality) != n:
        raise ValueError("quality has %d entries for %d frames" % (len(quality), n))
    return [_scaled_setting(q) for q in quality]


def compress_batch_scaled(images, quality="med", ctx=None):
    """compress_scaled(image, quality) of every image of a list, of any shapes (multiples of 8), in one call -> list of bytes in the
    caller's order.  quality: one setting for all, or a sequence with one per frame - the loop over image x setting of the reference's
    tests/cbenchmark.py is one call (tic_compress_batch_scaled_v): per chunk of up to 64 frames one upload, ONE transform launch whatever
    the frames' sizes and settings, the device entropy stage, one read-back.  ValueError for a list of the wrong length, a bad setting or a
    frame compress_scaled refuses, before any GPU work; KeyError when a coefficient of any frame has no Huffman code."""
    frames = [_scaled_image(im) for im in images]
    qs = _per_frame_settings(quality, len(frames))
    if not frames:
        return []
    ctx = _ctx(ctx)
    L = N.load()
    n = len(frames)
    caps_l = [L.tic_compress_scaled_bound(f[1], f[2]) for f in frames]
    offs = np.concatenate(([0], np.cumsum([(c + 63) // 64 * 64 for c in caps_l]))).astype(np.int64)
    with ctx.lock:
        pool = getattr(ctx, "_mixed_pool", None)  # the mixed batch's landing pool
        if pool is None or pool.size < offs[-1]:
            pool = ctx._mixed_pool = np.empty(int(offs[-1]), dtype=np.uint8)
        base = pool.ctypes.data
        inp, hs, ws, strides = _frame_arrays(frames)
        qa = (C.c_int * n)(*qs)
        outp = (C.c_void_p * n)(*[base + int(o) for o in offs[:-1]])
        caps = (C.c_size_t * n)(*caps_l)
        lens = (C.c_size_t * n)()
        rc = L.tic_compress_batch_scaled_v(ctx.handle, inp, n, hs, ws, strides, qa, outp, caps, lens)
        if rc == N.TIC_E_RANGE:
            raise KeyError("coefficient magnitude has no Huffman code")
        ctx.check(rc)
        return [pool[int(offs[i]): int(offs[i]) + lens[i]].tobytes() for i in range(n)]


def rd_points_scaled_batch(images, qualities=SCALED_SETTINGS, ctx=None):
    """The table of the reference's tests/cbenchmark.py in one call -> (sizes int64 (n, nq), sse uint64 (n, nq), sse_wrapped uint64 (n, nq)):
    sizes[i, j] is len(compress_scaled(images[i], qualities[j])) (-1 where it would raise KeyError), the two sums are
    roundtrip_sse_scaled's; psnr_from_sse turns them into dB.  Per chunk one upload, and per 64 image x setting pairs one launch each of
    the transform, the size kernel and the measuring kernel (tic_rd_points_scaled_v).  Validation as compress_batch_scaled."""
    frames = [_scaled_image(im) for im in images]
    qs = [_scaled_setting(q) for q in qualities]
    sizes = np.zeros((len(frames), len(qs)), dtype=np.int64)
    sse = np.zeros((len(frames), len(qs)), dtype=np.uint64)
    wrapped = np.zeros((len(frames), len(qs)), dtype=np.uint64)
    if not frames or not qs:
        return sizes, sse, wrapped
    ctx = _ctx(ctx)
    qarr = np.asarray(qs, dtype=np.intc)
    inp, hs, ws, strides = _frame_arrays(frames)
    with ctx.lock:
        ctx.check(N.load().tic_rd_points_scaled_v(ctx.handle, inp, len(frames), hs, ws, strides, qarr.ctypes.data, len(qs), sizes.ctypes.data,
                                                  sse.ctypes.data, wrapped.ctypes.data))
    return sizes, sse, wrapped


def entropy_encode_scaled(coeffs_zz, height, width, quality):
    """Host entropy stage of the integer encoder alone (no GPU needed): int16 [N, 64] zig-zag coefficients -> stream bytes."""
    L = N.load()
    height, width = int(height), int(width)
    qf = _scaled_setting(quality)
    if height < 0 or width < 0 or height % 8 or width % 8:
        raise ValueError("Width and height must be multiples of 8")
    zz = np.ascontiguousarray(coeffs_zz, dtype=np.int16)
    nb = L.tic_num_blocks(height, width)
    if zz.size != nb * 64:
        raise ValueError("coefficients of shape %r do not match %d blocks of 64" % (zz.shape, nb))
    cap = L.tic_compress_scaled_bound(height, width)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = L.tic_entropy_encode_scaled(zz.ctypes.data, height, width, qf, out.ctypes.data, cap, C.byref(n))
    if rc == N.TIC_E_RANGE:
        raise KeyError("coefficient magnitude has no Huffman code")
    if rc != N.TIC_OK:
        raise N.NativeError(rc, "tic_entropy_encode_scaled failed")
    return out[: n.value].tobytes()


def _adaptive_encode(ctx, fn, args, cap):
    """fn(ctx, *args, out, cap, &len) of an adaptive entry point (call with ctx.lock held); once more with the exact size when the
    first guess of the stream's size was short (the library reports it and writes nothing)."""
    for _ in range(2):
        out = getattr(ctx, "_adapt_buf", None)  # kept on the context, as compress()'s landing buffer (first-touch page faults)
        if out is None or out.size < cap:
            out = ctx._adapt_buf = np.empty(cap, dtype=np.uint8)
        n = C.c_size_t(0)
        rc = fn(ctx.handle, *args, out.ctypes.data, cap, C.byref(n))
        if rc == N.TIC_E_SPACE and n.value > cap:
            cap = n.value
            continue
        break
    if rc == N.TIC_E_RANGE:  # a category above 15 (int2ba in write_huffman_table, codec.py:73-84), or a code past 64 bits
        raise OverflowError(N.load().tic_last_error(ctx.handle).decode())
    ctx.check(rc)
    return out[: n.value].tobytes()


def compress_adaptive(image, quality=50, ctx=None):
    """compress(image, quality, auto_generate_huffman_table=True) of the reference (codec.py:133-164): the stream with the image's own
    Huffman tables (huffman.py:101-194), byte for byte.  Transform, symbol statistics and packing on the GPU, the table on the host."""
    img, h, w = _as_u8_image(image)  # 8-bit pixels only (ValueError otherwise), as compress_batch
    q = _check_quality(quality, packs_header=True)
    L = N.load()
    if L.tic_num_blocks(h, w) == 0:
        raise IndexError("index -1 is out of bounds for axis 0 with size 0")  # calc_huffman_table on an empty symbol list
    ctx = _ctx(ctx)
    with ctx.lock:
        return _adaptive_encode(ctx, L.tic_compress_adaptive, (img.ctypes.data, h, w, img.strides[0], q), L.tic_compress_bound(h, w) + 4096)


def entropy_encode_adaptive(coeffs_zz, height, width, quality, ctx=None):
    """The adaptive twin of entropy_encode(), on the GPU: int16 [N, 64] zig-zag coefficients (absolute DC) -> adaptive stream."""
    L = N.load()
    height, width = int(height), int(width)
    q = _check_quality(quality, packs_header=True)
    n = L.tic_num_blocks(height, width)
    zz = np.ascontiguousarray(coeffs_zz, dtype=np.int16)
    if zz.shape != (n, 64):
        raise ValueError("coefficients of shape %r do not match %d blocks of 64" % (zz.shape, n))
    if n == 0:
        raise IndexError("index -1 is out of bounds for axis 0 with size 0")
    ctx = _ctx(ctx)
    with ctx.lock:
        return _adaptive_encode(ctx, L.tic_entropy_encode_adaptive, (zz.ctypes.data, height, width, q),
                                L.tic_compress_bound(height, width) + 4096)


def _adaptive_batch(ctx, call, frames, caps_l):
    """call(n, index list, outp, caps, lens) -> rc of one adaptive batch entry point over the listed frames; the landing pool lives on the
    context.  After TIC_E_SPACE one second call, for exactly the frames the library left unwritten, with the sizes it reported."""
    n = len(frames)
    streams = [None] * n
    todo, caps_l = list(range(n)), list(caps_l)
    with ctx.lock:
        for attempt in range(2):
            m = len(todo)
            offs = np.concatenate(([0], np.cumsum([(caps_l[i] + 63) // 64 * 64 for i in todo]))).astype(np.int64)
            pool = getattr(ctx, "_adapt_batch_pool", None)  # (first-touch page faults, as compress_batch's pool)
            if pool is None or pool.size < offs[-1]:
                pool = ctx._adapt_batch_pool = np.empty(int(offs[-1]), dtype=np.uint8)
            base = pool.ctypes.data
            outp = (C.c_void_p * m)(*[base + int(o) for o in offs[:-1]])
            caps = (C.c_size_t * m)(*[caps_l[i] for i in todo])
            lens = (C.c_size_t * m)()
            rc = call(m, todo, outp, caps, lens)
            if rc == N.TIC_E_RANGE:  # a category above 15 (int2ba in write_huffman_table, codec.py:73-84), or a code past 64 bits
                raise OverflowError(N.load().tic_last_error(ctx.handle).decode())
            if rc != N.TIC_E_SPACE or attempt == 1:
                ctx.check(rc)
            short = []
            for k, i in enumerate(todo):
                if lens[k] > caps_l[i]:
                    caps_l[i] = int(lens[k])
                    short.append(i)
                else:
                    streams[i] = pool[int(offs[k]): int(offs[k]) + lens[k]].tobytes()
            todo = short
            if not todo:
                break
    return streams


def _per_frame_qualities(quality, n):
    per_frame = not isinstance(quality, (int, float, np.integer, np.floating, bool, np.bool_, str, bytes)) and hasattr(quality, "__len__")
    if not per_frame:
        return [quality] * n
    if len(quality) != n:
        raise ValueError("quality has %d entries for %d frames" % (len(quality), n))
    return list(quality)


def compress_batch_adaptive(images, quality=50, ctx=None):
    """compress_adaptive() for a list of frames of any shapes in ONE call -> list of bytes (frame order): every stream is what
    compress_adaptive(image, q) gives, i.e. the reference's compress(image, q, auto_generate_huffman_table=True), byte for byte.
    `quality`: an int, or a sequence with one entry per frame.  The exceptions are compress_adaptive's, raised for the first offending
    frame before any GPU work (pixel range, quality, a frame without blocks) or from the call (OverflowError names the frame)."""
    images = list(images)
    quals = _per_frame_qualities(quality, len(images))
    L = N.load()
    frames, qs = [], []
    for im, qi in zip(images, quals):
        img, h, w = _as_u8_image(im)
        qs.append(_check_quality(qi, packs_header=True))
        if L.tic_num_blocks(h, w) == 0:
            raise IndexError("index -1 is out of bounds for axis 0 with size 0")  # calc_huffman_table on an empty symbol list
        frames.append((img, h, w))
    if not frames:
        return []
    ctx = _ctx(ctx)

    def call(m, idx, outp, caps, lens):
        inp = (C.c_void_p * m)(*[frames[i][0].ctypes.data for i in idx])
        hs = (C.c_int * m)(*[frames[i][1] for i in idx])
        ws = (C.c_int * m)(*[frames[i][2] for i in idx])
        strides = (C.c_ssize_t * m)(*[frames[i][0].strides[0] for i in idx])
        qa = (C.c_int * m)(*[qs[i] for i in idx])
        return L.tic_compress_batch_adaptive_v(ctx.handle, inp, m, hs, ws, strides, qa, outp, caps, lens)

    return _adaptive_batch(ctx, call, frames, [L.tic_compress_bound(f[1], f[2]) + 4096 for f in frames])


def entropy_encode_adaptive_batch(coeffs_list, shapes, qualities, ctx=None):
    """The coefficient-domain twin of compress_batch_adaptive(): coeffs_list[i] = int16 [N_i, 64] zig-zag coefficients (absolute DC) of a
    frame of shapes[i] = (height, width) -> entropy_encode_adaptive(coeffs_list[i], height, width, qualities[i]) per frame, in one call."""
    coeffs_list, shapes = list(coeffs_list), [(int(h), int(w)) for h, w in shapes]
    if len(shapes) != len(coeffs_list):
        raise ValueError("%d shapes for %d frames" % (len(shapes), len(coeffs_list)))
    quals = _per_frame_qualities(qualities, len(coeffs_list))
    L = N.load()
    frames, qs = [], []
    for zz, (h, w), qi in zip(coeffs_list, shapes, quals):
        qs.append(_check_quality(qi, packs_header=True))
        nb = L.tic_num_blocks(h, w)
        zz = np.ascontiguousarray(zz, dtype=np.int16)
        if zz.shape != (nb, 64):
            raise ValueError("coefficients of shape %r do not match %d blocks of 64" % (zz.shape, nb))
        if nb == 0:
            raise IndexError("index -1 is out of bounds for axis 0 with size 0")
        frames.append((zz, h, w))
    if not frames:
        return []
    ctx = _ctx(ctx)

    def call(m, idx, outp, caps, lens):
        inp = (C.c_void_p * m)(*[frames[i][0].ctypes.data for i in idx])
        hs = (C.c_int * m)(*[frames[i][1] for i in idx])
        ws = (C.c_int * m)(*[frames[i][2] for i in idx])
        qa = (C.c_int * m)(*[qs[i] for i in idx])
        return L.tic_entropy_encode_adaptive_batch(ctx.handle, inp, m, hs, ws, qa, outp, caps, lens)

    return _adaptive_batch(ctx, call, frames, [L.tic_compress_bound(f[1], f[2]) + 4096 for f in frames])


def _no_blocks_adaptive(L, h, w):
    if L.tic_num_blocks(h, w) == 0:
        raise IndexError("index -1 is out of bounds for axis 0 with size 0")  # calc_huffman_table on an empty symbol list, as compress_adaptive


def entropy_size_adaptive(coeffs_zz, height, width):
    """len(entropy_encode_adaptive(coeffs_zz, height, width, q)) for any quality, from a host walk of the symbols and the table they give
    (no GPU needed): the length of an adaptive stream is a function of its symbol statistics alone.  IndexError for a frame without
    blocks, OverflowError where the encoder raises it (a DC category or AC size above 15, a code and its value bits beyond 64 bits)."""
    L = N.load()
    height, width = int(height), int(width)
    zz = np.ascontiguousarray(coeffs_zz, dtype=np.int16)
    if height < 0 or width < 0:
        raise ValueError("negative image size")
    nb = L.tic_num_blocks(height, width)
    if zz.size != nb * 64:
        raise ValueError("coefficients of shape %r do not match %d blocks of 64" % (zz.shape, nb))
    _no_blocks_adaptive(L, height, width)
    n = C.c_size_t(0)
    rc = L.tic_entropy_size_adaptive(zz.ctypes.data, height, width, C.byref(n))
    if rc == N.TIC_E_RANGE:
        raise OverflowError("a DC category or AC size above 15, or a Huffman code and its value bits beyond 64 bits")
    if rc != N.TIC_OK:
        raise N.NativeError(rc, "tic_entropy_size_adaptive failed")
    return int(n.value)


def compressed_sizes_adaptive(image, qualities, ctx=None):
    """len(compress_adaptive(image, q)) for every q of `qualities` -> int64 array, -1 where compress_adaptive() would raise
    OverflowError.  No stream is produced: per quality the transform, one statistics launch for up to 64 qualities, one read-back of the
    symbol statistics, the tables and lengths on the host.  Validation as compressed_sizes; a frame without blocks raises IndexError, as
    compress_adaptive."""
    img, h, w = _as_u8_image(image)
    qs = [_check_quality(q, packs_header=True) for q in qualities]
    L = N.load()
    _no_blocks_adaptive(L, h, w)
    sizes = np.zeros(len(qs), dtype=np.int64)
    if not qs:
        return sizes
    ctx = _ctx(ctx)
    qarr = np.asarray(qs, dtype=np.intc)
    with ctx.lock:
        ctx.check(L.tic_adaptive_sizes(ctx.handle, img.ctypes.data, h, w, img.strides[0], qarr.ctypes.data, len(qs), sizes.ctypes.data))
    return sizes


def compressed_size_adaptive(image, quality=50, ctx=None):
    """len(compress_adaptive(image, quality)) without producing the stream; the same exceptions for the same arguments."""
    size = int(compressed_sizes_adaptive(image, [quality], ctx=ctx)[0])
    if size < 0:
        raise OverflowError("a DC category or AC size above 15, or a Huffman code and its value bits beyond 64 bits")  # as compress_adaptive
    return size


def compress_adaptive_to_size(image, max_bytes, min_quality=1, max_quality=99, ctx=None):
    """compress_to_size with per-image Huffman tables -> (bytes, quality): compress_adaptive(image, quality) of the quality at which
    compress_to_size's bisection over min_quality..max_quality ends, with "compress_adaptive() succeeds and len(...) <= max_bytes" as its
    test.  The adaptive stream is the smallest at any quality, so the same budget buys a higher quality.  Probes are compressed_sizes_adaptive's,
    several steps ahead per submission.  ValueError naming the size at min_quality when even that exceeds the budget, OverflowError when
    min_quality has no adaptive stream, IndexError for a frame without blocks; 8-bit images only."""
    img, h, w = _as_u8_image(image)
    qmin = _check_quality(min_quality, packs_header=True)
    qmax = _check_quality(max_quality, packs_header=True)
    if qmin > qmax:
        raise ValueError("min_quality %d above max_quality %d" % (qmin, qmax))
    max_bytes = int(max_bytes)
    if max_bytes < 0:
        raise ValueError("max_bytes must not be negative")
    L = N.load()
    _no_blocks_adaptive(L, h, w)
    ctx = _ctx(ctx)
    cap = L.tic_compress_bound(h, w) + 4096
    with ctx.lock:
        for _ in range(2):
            out = getattr(ctx, "_adapt_buf", None)  # compress_adaptive's landing buffer
            if out is None or out.size < cap:
                out = ctx._adapt_buf = np.empty(cap, dtype=np.uint8)
            n, q = C.c_size_t(0), C.c_int(0)
            rc = L.tic_compress_adaptive_to_size(ctx.handle, img.ctypes.data, h, w, img.strides[0], max_bytes, qmin, qmax, out.ctypes.data, cap,
                                                 C.byref(n), C.byref(q))
            if rc == N.TIC_E_SPACE and n.value > cap and n.value <= max_bytes:  # the first guess of the stream's size was short
                cap = n.value
                continue
            break
        if rc == N.TIC_E_RANGE:
            raise OverflowError(L.tic_last_error(ctx.handle).decode())
        if rc == N.TIC_E_SPACE:
            raise ValueError("%d bytes at quality %d exceed max_bytes = %d" % (n.value, qmin, max_bytes))
        ctx.check(rc)
        return out[: n.value].tobytes(), int(q.value)


def compressed_sizes_adaptive_batch(images, qualities, ctx=None):
    """compressed_sizes_adaptive(image, qualities) of every image of a list, of any shapes, in one call -> int64 array (n, nq); -1 where
    compress_adaptive() would raise OverflowError.  Per chunk of up to 64 frames one upload, every probe queued, one statistics launch per
    64 probes, one read-back (tic_adaptive_sizes_v).  Validation as compressed_sizes_batch; a frame without blocks raises IndexError."""
    frames = [_as_u8_image(im) for im in images]
    qs = [_check_quality(q, packs_header=True) for q in qualities]
    L = N.load()
    for _, h, w in frames:
        _no_blocks_adaptive(L, h, w)
    sizes = np.zeros((len(frames), len(qs)), dtype=np.int64)
    if not frames or not qs:
        return sizes
    ctx = _ctx(ctx)
    qarr = np.asarray(qs, dtype=np.intc)
    inp, hs, ws, strides = _frame_arrays(frames)
    with ctx.lock:
        ctx.check(L.tic_adaptive_sizes_v(ctx.handle, inp, len(frames), hs, ws, strides, qarr.ctypes.data, len(qs), sizes.ctypes.data))
    return sizes


def decompress_adaptive(data, ctx=None):
    """Reads a stream of compress_adaptive() (or of the reference's compress(..., auto_generate_huffman_table=True)) as written:
    Huffman decode with the embedded table (on the GPU for streams of 16,384 blocks, or 1,024 blocks and 32 KB of payload, and more;
    else and for anything unusual on the host), inverse transform on the GPU.  Strict: ValueError for a malformed table, a truncated
    or damaged stream - the reference has no working counterpart, and decompress() keeps the reference's reading (garbage)."""
    ctx = _ctx(ctx)
    buf = _as_bytes_view(data)
    if buf.size < 16:
        raise ValueError("stream shorter than its 16-byte header")
    hdr = parse_header(buf)
    h, w = hdr["height"], hdr["width"]
    if h < 0 or w < 0:
        raise ValueError("negative image size in the header")
    out = np.zeros((h, w), dtype=np.uint8)
    with ctx.lock:
        rc = N.load().tic_decompress_adaptive(ctx.handle, buf.ctypes.data, buf.size, out.ctypes.data, out.size)
        if rc in (N.TIC_E_STREAM, N.TIC_E_SPACE):
            raise ValueError(N.load().tic_last_error(ctx.handle).decode())
        ctx.check(rc)
    return out


def decompress_batch_adaptive(streams, ctx=None):
    """decompress_adaptive() of many streams in one call -> list of uint8 arrays (stream order): the mirror of compress_batch_adaptive.
    Every element is what decompress_adaptive() returns for that stream; the exceptions are decompress_adaptive()'s - ValueError naming
    the frame: the first offending header's before anything is decoded, else the first stream's that fails to decode (every other frame
    has been decoded by then).  The streams and a look-up table each go up in one copy, one launch per kernel decodes a chunk of them
    whatever their sizes, the pixels come down in one copy (tic_decompress_batch_adaptive); flat and one-block frames, and anything the
    kernels give up on, take the single call behind the batch."""
    bufs = [_as_bytes_view(d) for d in streams]
    n = len(bufs)
    if n == 0:
        return []
    shapes = []
    for i, b in enumerate(bufs):
        if b.size < 16:
            raise ValueError("frame %d: stream shorter than its 16-byte header" % i)
        hd = parse_header(b)
        if hd["height"] < 0 or hd["width"] < 0:
            raise ValueError("frame %d: negative image size in the header" % i)
        shapes.append((hd["height"], hd["width"]))
    ctx = _ctx(ctx)  # (behind the checks that need no device)
    # one block for all frames, as decompress_batch: the library copies the pixels of a chunk straight into it where they are dense
    sizes = [h * w for h, w in shapes]
    block = np.zeros(sum(sizes), dtype=np.uint8)
    outs, at = [], 0
    for (h, w), sz in zip(shapes, sizes):
        outs.append(block[at:at + sz].reshape(h, w) if sz else np.zeros((h, w), np.uint8))
        at += sz
    L = N.load()
    sp = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    sl = (C.c_size_t * n)(*[b.size for b in bufs])
    op = (C.c_void_p * n)(*[o.ctypes.data if o.size else None for o in outs])
    oc = (C.c_size_t * n)(*[o.size for o in outs])
    with ctx.lock:
        rc = L.tic_decompress_batch_adaptive(ctx.handle, sp, sl, n, op, oc, None, None)
        if rc in (N.TIC_E_STREAM, N.TIC_E_SPACE):
            msg = L.tic_last_error(ctx.handle).decode()
            raise ValueError(msg if msg.startswith("frame ") else "frame 0: " + msg)  # (a batch of one is the single call: its message names no frame)
        ctx.check(rc)
    return outs


def _as_bytes_view(data):
    """uint8 view of a bytes-like object without copying it (bytes, bytearray, memoryview, uint8 arrays)."""
    if isinstance(data, np.ndarray) and data.dtype == np.uint8 and data.flags.c_contiguous:
        return data.reshape(-1)
    try:
        return np.frombuffer(data, dtype=np.uint8)
    except (TypeError, ValueError):
        return np.frombuffer(bytes(data), dtype=np.uint8)


def parse_header(data):
    L = N.load()
    buf = _as_bytes_view(data)
    h, w, q, flag = C.c_int(), C.c_int(), C.c_int(), C.c_uint32()
    rc = L.tic_parse_header(buf.ctypes.data, buf.size, C.byref(h), C.byref(w), C.byref(q), C.byref(flag))
    if rc != N.TIC_OK:
        raise struct.error("unpack requires a buffer of 16 bytes")  # codec.py:119
    return {"height": h.value, "width": w.value, "quality": q.value, "flag": flag.value}


def decompress(data, ctx=None):
    ctx = _ctx(ctx)
    buf = _as_bytes_view(data)  # one view for the header and the payload: the stream is not copied
    hdr = parse_header(buf)     # struct.error for fewer than 16 bytes, as codec.py:118-119
    if hdr["flag"] & (1 << 31):
        # codec.py:124-126 parses a Huffman table from the stream here.  The reference's own writer cannot produce such a stream
        # (it writes the flag MSB-first and reads it back little-endian: codec.py:111/119), and on anything that is not a
        # well-formed table its read_huffman_table ends in ValueError (tests/golden/decoder_edges.npz); embedded tables are out
        # of scope here, so every such stream gets that exception
        raise ValueError("stream carries an embedded Huffman table (little-endian flag bit 31): not supported")
    out = np.zeros((hdr["height"], hdr["width"]), dtype=np.uint8)
    with ctx.lock:
        ctx.check(N.load().tic_decompress(ctx.handle, buf.ctypes.data, buf.size, out.ctypes.data, out.size))
    return out


def decompress_batch(streams, ctx=None):
    """decompress() of many streams in one call -> list of uint8 arrays (stream order): the mirror of compress_batch, i.e. the loop of the
    reference's benchmark (/root/reference/tests/benchmark.py:12-23: `decompress(data)` per image) as ONE call.  Every element is what
    decompress() returns for that stream; the exceptions are decompress()'s (the first offending stream's, before anything is decoded).
    The streams go up in one copy, two kernel launches decode all of them, the pixels come down in one copy (tic_decompress_batch)."""
    ctx = _ctx(ctx)
    bufs = [_as_bytes_view(d) for d in streams]
    n = len(bufs)
    if n == 0:
        return []
    hdrs = [parse_header(b) for b in bufs]  # struct.error for fewer than 16 bytes, as codec.py:118-119
    for hd in hdrs:
        if hd["flag"] & (1 << 31):
            raise ValueError("stream carries an embedded Huffman table (little-endian flag bit 31): not supported")
    # one block for all frames: equal geometries follow each other in memory, and the library copies the pixels of a chunk straight into it
    sizes = [max(hd["height"], 0) * max(hd["width"], 0) for hd in hdrs]
    block = np.zeros(sum(sizes), dtype=np.uint8)
    outs, at = [], 0
    for hd, sz in zip(hdrs, sizes):
        outs.append(block[at:at + sz].reshape(max(hd["height"], 0), max(hd["width"], 0)) if sz else np.zeros((max(hd["height"], 0), max(hd["width"], 0)), np.uint8))
        at += sz
    L = N.load()
    sp = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    sl = (C.c_size_t * n)(*[b.size for b in bufs])
    op = (C.c_void_p * n)(*[o.ctypes.data if o.size else None for o in outs])
    oc = (C.c_size_t * n)(*[o.size for o in outs])
    with ctx.lock:
        ctx.check(L.tic_decompress_batch(ctx.handle, sp, sl, n, op, oc, None, None))
    return outs


def _info_of(zz, hdr):
    """The dictionary the reference's decompress() hands to decode() (codec.py:167-188), from zz16 rows: dc int32 DPCM differences with
    the first one raw, ac int16 [N, 63]."""
    dc = zz[:, 0].astype(np.int32)
    info = dict(hdr)
    info["dc"] = np.diff(dc, prepend=np.int32(0)).astype(np.int32) if dc.size else dc
    info["ac"] = np.ascontiguousarray(zz[:, 1:])
    return info


def _default_header(buf):
    """The header checks of decompress() that need no device, with its exceptions: struct.error below 16 bytes, ValueError for the
    little-endian bit 31 and for a negative size (np.zeros in decompress()), the library's own error for a quality it refuses."""
    hdr = parse_header(buf)
    if hdr["flag"] & (1 << 31):
        raise ValueError("stream carries an embedded Huffman table (little-endian flag bit 31): not supported")
    if hdr["height"] < 0 or hdr["width"] < 0:
        raise ValueError("negative dimensions are not allowed")
    scaled = bool(hdr["flag"] & (1 << 30))
    q = hdr["quality"]
    if scaled and not 0 <= q <= 62:
        raise N.NativeError(N.TIC_E_QUALITY, "scaled_dct exponent %d in header outside 0..62" % q)
    if not scaled and not 1 <= q <= 99:
        raise N.NativeError(N.TIC_E_QUALITY, "quality %d in header outside 1..99" % q)
    return {"height": hdr["height"], "width": hdr["width"], "quality": q, "scaled_dct": scaled}


def _adaptive_header(buf):
    """decompress_adaptive()'s header checks that need no device, with its exceptions."""
    if buf.size < 16:
        raise ValueError("stream shorter than its 16-byte header")
    hdr = parse_header(buf)
    if hdr["height"] < 0 or hdr["width"] < 0:
        raise ValueError("negative image size in the header")
    if not 1 <= hdr["quality"] <= 99:
        raise ValueError("quality %d in the header outside 1..99" % hdr["quality"])
    return {"height": hdr["height"], "width": hdr["width"], "quality": hdr["quality"], "scaled_dct": False}


def entropy_decode_zz(data, ctx=None):
    """The mirror of entropy_encode(): a default-table or scaled_dct stream -> (coefficients int16 [N, 64] in zig-zag order with the
    absolute DC - the layout entropy_encode, entropy_size and entropy_encode_adaptive take -, header dict with height, width, quality,
    scaled_dct).  The reference's reading of the stream, as decompress() reads it (long streams on the GPU).  Exceptions as
    decompress(); ValueError when the running DC leaves int16, which the layout cannot hold."""
    buf = _as_bytes_view(data)
    hdr = _default_header(buf)
    L = N.load()
    n = L.tic_num_blocks(hdr["height"], hdr["width"])
    zz = np.empty((n, 64), dtype=np.int16)
    ctx = _ctx(ctx)
    with ctx.lock:
        rc = L.tic_entropy_decode(ctx.handle, buf.ctypes.data, buf.size, zz.ctypes.data, n, None, None, None, None)
        if rc == N.TIC_E_RANGE:
            raise ValueError(L.tic_last_error(ctx.handle).decode())
        ctx.check(rc)
    return zz, hdr


def entropy_decode(data, ctx=None):
    """The first half of the reference's decompress() (codec.py:167-188): the dictionary it hands to decode() - height, width, quality,
    scaled_dct, dc (int32 DPCM differences, the first one raw), ac (int16 [N, 63]).  decode(entropy_decode(s)) is decompress(s)."""
    zz, hdr = entropy_decode_zz(data, ctx=ctx)
    return _info_of(zz, hdr)


def entropy_decode_adaptive(data, ctx=None):
    """entropy_decode() for a stream with an embedded table (compress_adaptive): the same dictionary; strict, with
    decompress_adaptive()'s exceptions."""
    buf = _as_bytes_view(data)
    hdr = _adaptive_header(buf)
    L = N.load()
    n = L.tic_num_blocks(hdr["height"], hdr["width"])
    zz = np.empty((n, 64), dtype=np.int16)
    ctx = _ctx(ctx)
    with ctx.lock:
        rc = L.tic_entropy_decode_adaptive(ctx.handle, buf.ctypes.data, buf.size, zz.ctypes.data, n, None, None, None)
        if rc in (N.TIC_E_STREAM, N.TIC_E_SPACE):
            raise ValueError(L.tic_last_error(ctx.handle).decode())
        ctx.check(rc)
    return _info_of(zz, hdr)


def _retable(ctx, fn, buf, cap, missing_code):
    """A re-tabling entry point under the context's lock: _adaptive_encode's retry and OverflowError, KeyError for a symbol without a
    default code, ValueError for a refused stream or a DC outside int16."""
    L = N.load()
    with ctx.lock:
        try:
            return _adaptive_encode(ctx, fn, (buf.ctypes.data, buf.size), cap)
        except OverflowError as e:
            if "running DC" in str(e):
                raise ValueError(str(e)) from None
            if missing_code:
                raise KeyError(str(e)) from None
            raise
        except N.NativeError as e:
            if e.code == N.TIC_E_STREAM:
                raise ValueError(L.tic_last_error(ctx.handle).decode()) from None
            raise


def _retable_adaptive_header(buf):
    """retable_adaptive()'s checks that need no device, with its exceptions (the single call and the batch call share them)"""
    hdr = parse_header(buf)
    if hdr["flag"] & (1 << 31):
        raise ValueError("stream carries an embedded Huffman table already (little-endian flag bit 31)")
    if hdr["flag"] & (1 << 30):
        raise ValueError("a scaled_dct stream cannot carry an embedded table: the flag word has room for one family")
    if hdr["height"] < 0 or hdr["width"] < 0:
        raise ValueError("negative image size in the header")
    if not 1 <= hdr["quality"] <= 99:
        raise ValueError("quality %d in the header outside 1..99" % hdr["quality"])
    if N.load().tic_num_blocks(hdr["height"], hdr["width"]) == 0:
        raise IndexError("index -1 is out of bounds for axis 0 with size 0")  # calc_huffman_table on an empty symbol list
    return hdr


def retable_adaptive(data, ctx=None):
    """A stored default-table stream rewritten with its image's own Huffman tables, losslessly: the reference's reader (codec.py:167-188)
    followed by its writer with auto_generate_huffman_table=True (codec.py:133-164) on the same coefficients.  For a stream of
    compress(image, q) the result is compress_adaptive(image, q), byte for byte.  ValueError for scaled_dct streams, refused headers and
    a running DC outside int16; IndexError for a frame without blocks; OverflowError as compress_adaptive."""
    buf = _as_bytes_view(data)
    hdr = _retable_adaptive_header(buf)
    L = N.load()
    ctx = _ctx(ctx)
    return _retable(ctx, L.tic_retable_adaptive, buf, L.tic_compress_bound(hdr["height"], hdr["width"]) + 4096, False)


def retable_default(data, ctx=None):
    """The way back: a stream with an embedded table rewritten with the default tables.  KeyError where a symbol has no default code (as
    compress() raises it); ValueError as decompress_adaptive()."""
    buf = _as_bytes_view(data)
    hdr = _adaptive_header(buf)
    L = N.load()
    ctx = _ctx(ctx)
    # (the default stream is the longer one as a rule, by a few per cent at most qualities: one retry with the reported length otherwise)
    cap = min(L.tic_compress_bound(hdr["height"], hdr["width"]), buf.size + buf.size // 2 + 4096)
    return _retable(ctx, L.tic_retable_default, buf, cap, True)


def _requant_header(buf):
    """The checks of requantize() / requantized_sizes() / requantize_to_size() that need no device, with their exceptions: struct.error
    below 16 bytes, ValueError for the header refusals."""
    hdr = parse_header(buf)
    if hdr["flag"] & (1 << 31):
        raise ValueError("stream carries an embedded Huffman table (little-endian flag bit 31): requantisation reads default-table streams")
    if hdr["flag"] & (1 << 30):
        raise ValueError("a scaled_dct stream has no quality to requantise from")
    if hdr["height"] < 0 or hdr["width"] < 0:
        raise ValueError("negative image size in the header")
    if not 1 <= hdr["quality"] <= 99:
        raise ValueError("quality %d in the header outside 1..99" % hdr["quality"])
    return hdr


def _requant_quality(quality):
    """A target quality of the requantisation calls: compress()'s exceptions (it ends in a header), integers only."""
    q = _check_quality(quality, packs_header=True)
    if isinstance(q, float):
        raise ValueError("non-integral quality %r: requantisation takes the integers 1..99" % (quality,))
    return q


def requantize_zz(coeffs_zz, from_quality, to_quality, ctx=None):
    """int16 [N, 64] zig-zag coefficients (absolute DC) of quality from_quality at quality to_quality, on the GPU: per coefficient the
    reference's block_quantize(block_quantize(c, q1, inverse=True), q2) (utils.py:48-53), its three float64 operations in its order.
    requantize_zz(c, q, q) is c.  KeyError where a result leaves int16 (the reference's writer has no code for it)."""
    q1, q2 = _requant_quality(from_quality), _requant_quality(to_quality)
    zz = np.ascontiguousarray(coeffs_zz, dtype=np.int16)
    if zz.ndim != 2 or zz.shape[1] != 64:
        raise ValueError("coefficients of shape %r are not [N, 64]" % (zz.shape,))
    out = np.empty_like(zz)
    if zz.shape[0] == 0:
        return out
    ctx = _ctx(ctx)
    with ctx.lock:
        rc = N.load().tic_requantize_zz(ctx.handle, zz.ctypes.data, zz.shape[0], q1, q2, out.ctypes.data)
        if rc == N.TIC_E_RANGE:
            raise KeyError(N.load().tic_last_error(ctx.handle).decode())
        ctx.check(rc)
    return out


def _requant_call(ctx, L, call):
    """rc of a requantisation call with its exceptions (call with ctx.lock held): KeyError for TIC_E_RANGE, ValueError for a refused stream."""
    rc = call()
    if rc == N.TIC_E_RANGE:
        raise KeyError(L.tic_last_error(ctx.handle).decode())
    if rc == N.TIC_E_STREAM:
        raise ValueError(L.tic_last_error(ctx.handle).decode())
    return rc


def requantize(stream, quality, adaptive=False, ctx=None):
    """A stored default-table stream at another quality, without pixels -> bytes: the reference's reader (codec.py:167-188), its
    block_quantize(block_quantize(c, q_of_stream, inverse=True), quality) on the coefficients, its writer (codec.py:133-164; adaptive=True:
    with the image's own Huffman tables, as compress_adaptive) with `quality` in the header.  requantize(s, q_of_s) is s for a stream our
    encoders wrote.  struct.error below 16 bytes, ValueError for scaled_dct streams, embedded tables and refused headers, KeyError where
    the reference's writer raises it (a value without a Huffman code), IndexError for adaptive output of a frame without blocks."""
    buf = _as_bytes_view(stream)
    hdr = _requant_header(buf)
    q = _requant_quality(quality)
    L = N.load()
    if adaptive and L.tic_num_blocks(hdr["height"], hdr["width"]) == 0:
        raise IndexError("index -1 is out of bounds for axis 0 with size 0")  # calc_huffman_table on an empty symbol list
    ctx = _ctx(ctx)
    cap = L.tic_compress_bound(hdr["height"], hdr["width"]) + (4096 if adaptive else 0)
    with ctx.lock:
        for _ in range(2):
            out = getattr(ctx, "_adapt_buf", None)
            if out is None or out.size < cap:
                out = ctx._adapt_buf = np.empty(cap, dtype=np.uint8)
            n = C.c_size_t(0)
            rc = _requant_call(ctx, L, lambda: L.tic_requantize(ctx.handle, buf.ctypes.data, buf.size, q, int(bool(adaptive)), out.ctypes.data, cap, C.byref(n)))
            if rc == N.TIC_E_SPACE and n.value > cap:  # (an adaptive table longer than the guess: once more with the reported length)
                cap = n.value
                continue
            break
        ctx.check(rc)
        return out[: n.value].tobytes()


def requantized_sizes(stream, qualities, ctx=None):
    """len(requantize(stream, q)) for every q of `qualities` -> int64 array, -1 where requantize() raises KeyError.  The stream is read
    once; no stream is produced."""
    buf = _as_bytes_view(stream)
    _requant_header(buf)
    qs = [_requant_quality(q) for q in qualities]
    sizes = np.zeros(len(qs), dtype=np.int64)
    if not qs:
        return sizes
    ctx = _ctx(ctx)
    L = N.load()
    qarr = np.asarray(qs, dtype=np.intc)
    with ctx.lock:
        ctx.check(_requant_call(ctx, L, lambda: L.tic_requantized_sizes(ctx.handle, buf.ctypes.data, buf.size, qarr.ctypes.data, len(qs), sizes.ctypes.data)))
    return sizes


def requantize_to_size(stream, max_bytes, min_quality=1, max_quality=None, ctx=None):
    """The best requantised stream within a byte budget -> (bytes, quality): requantize(stream, quality) of the quality at which
    compress_to_size()'s bisection over min_quality..max_quality ends, with "requantize() succeeds and len(...) <= max_bytes" as its
    test.  max_quality=None: the stream's own quality.  The stream is read once and the probes run on the resident coefficients.
    ValueError naming the size at min_quality when even that exceeds the budget, KeyError when min_quality has no stream."""
    buf = _as_bytes_view(stream)
    hdr = _requant_header(buf)
    qmin = _requant_quality(min_quality)
    qmax = hdr["quality"] if max_quality is None else _requant_quality(max_quality)
    if qmin > qmax:
        raise ValueError("min_quality %d above max_quality %d" % (qmin, qmax))
    max_bytes = int(max_bytes)
    if max_bytes < 0:
        raise ValueError("max_bytes must not be negative")
    ctx = _ctx(ctx)
    L = N.load()
    cap = L.tic_compress_bound(hdr["height"], hdr["width"])
    with ctx.lock:
        out = getattr(ctx, "_out_buf", None)  # compress()'s landing buffer
        if out is None or out.size < cap:
            out = ctx._out_buf = np.empty(cap, dtype=np.uint8)
        n, q = C.c_size_t(0), C.c_int(0)
        rc = _requant_call(ctx, L, lambda: L.tic_requantize_to_size(ctx.handle, buf.ctypes.data, buf.size, max_bytes, qmin, qmax, out.ctypes.data, cap,
                                                                     C.byref(n), C.byref(q)))
        if rc == N.TIC_E_SPACE:
            raise ValueError("%d bytes at quality %d exceed max_bytes = %d" % (n.value, qmin, max_bytes))
        ctx.check(rc)
        return out[: n.value].tobytes(), int(q.value)


def last_requantize(ctx=None):
    """What the context's last requantisation call did: {"route": 1 device reader / 2 host reader / 0 none, "measure_launches",
    "store_launches", "rounds"} (tic_last_requantize)."""
    ctx = _ctx(ctx)
    v = [C.c_int(0) for _ in range(4)]
    with ctx.lock:
        ctx.check(N.load().tic_last_requantize(ctx.handle, *[C.byref(x) for x in v]))
    return dict(zip(("route", "measure_launches", "store_launches", "rounds"), (int(x.value) for x in v)))


def _frame_exception(i, e):
    """The exception a single call raised for frame i of a batch: the same class, the message naming the frame."""
    if isinstance(e, N.NativeError):
        msg = str(e).split(": ", 1)[-1]
        return N.NativeError(e.code, "frame %d: %s" % (i, msg))
    try:
        return type(e)("frame %d: %s" % (i, e.args[0] if e.args else ""))
    except Exception:  # noqa: BLE001 - a class with another constructor: the original object
        return e


def _check_errors_arg(errors):
    if errors not in ("raise", "return"):
        raise ValueError("errors must be 'raise' or 'return', not %r" % (errors,))


def _transcode_batch(streams, ctx, errors, precheck, call, single):
    """The common part of the batch transcoders.  precheck(i, buf): the single call's checks that need no device (raises as it does), returns what
    call() needs of the frame; call(ctx, L, idx, bufs, pre) -> (results, rcs) runs the C-ABI batch call on the frames that passed; a frame
    whose code is not TIC_OK goes through single(data) once more, which raises the single call's own exception.
    (Such a frame is read up to three times - by the batch kernels, by the library's single call behind them, by single() here for the
    exception's class and wording: nothing for the odd bad stream of an archive, a real cost for an archive of damaged streams.)"""
    _check_errors_arg(errors)
    streams = list(streams)
    out = [None] * len(streams)
    bufs, pre, idx = [], [], []
    for i, s in enumerate(streams):
        try:
            b = _as_bytes_view(s)
            p = precheck(i, b)
        except Exception as e:  # noqa: BLE001 - whatever the single call raises for this frame
            out[i] = _frame_exception(i, e)
            continue
        bufs.append(b), pre.append(p), idx.append(i)
    if idx:
        L = N.load()
        ctx = _ctx(ctx)
        with ctx.lock:
            results, rcs = call(ctx, L, bufs, pre)
        for k, i in enumerate(idx):
            if rcs[k] == N.TIC_OK:
                out[i] = results[k]
                continue
            try:  # (rare: the single call words the error and picks the exception's class)
                out[i] = single(streams[i], ctx)
            except Exception as e:  # noqa: BLE001
                out[i] = _frame_exception(i, e)
    if errors == "raise":  # the lowest failing index, wherever its error was found
        for r in out:
            if isinstance(r, Exception):
                raise r from None
    return out


def _ptr_array(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def entropy_decode_zz_batch(streams, ctx=None, errors="raise"):
    """entropy_decode_zz() of many streams in one call: [(coefficients, header), ...], frame i exactly what entropy_decode_zz(streams[i]) gives.
    The streams of a chunk (up to 64) share one upload, the device reader's two launches and one download; a stream the batch kernels do
    not take goes through the single call.  errors="return": a failing frame's place holds its exception (the class the single call
    raises, the message naming the frame) instead of the first one being raised."""

    def precheck(i, buf):
        hdr = _default_header(buf)
        return hdr, N.load().tic_num_blocks(hdr["height"], hdr["width"])

    def call(ctx, L, bufs, pre):
        n = len(bufs)
        zzs = [np.empty((nb, 64), dtype=np.int16) for _, nb in pre]
        lens = (C.c_size_t * n)(*[b.size for b in bufs])
        caps = (C.c_size_t * n)(*[nb for _, nb in pre])
        rcs = (C.c_int * n)()
        L.tic_entropy_decode_batch(ctx.handle, _ptr_array(bufs), lens, n, _ptr_array(zzs), caps, None, None, None, None, rcs)
        return [(zzs[k], pre[k][0]) for k in range(n)], list(rcs)

    return _transcode_batch(streams, ctx, errors, precheck, call, lambda s, c: entropy_decode_zz(s, ctx=c))


def _retable_batch(streams, ctx, errors, precheck, fn_name, single):
    def call(ctx, L, bufs, caps0):
        n = len(bufs)
        fn = getattr(L, fn_name)
        results, rcs = [None] * n, [N.TIC_OK] * n
        todo, caps = list(range(n)), list(caps0)
        for _ in range(2):  # (once more, with the lengths the library reported, for the frames whose first guess was short)
            m = len(todo)
            outs = [np.empty(caps[k], dtype=np.uint8) for k in todo]
            lens = (C.c_size_t * m)(*[bufs[k].size for k in todo])
            ccaps = (C.c_size_t * m)(*[caps[k] for k in todo])
            olens = (C.c_size_t * m)()
            crcs = (C.c_int * m)()
            fn(ctx.handle, _ptr_array([bufs[k] for k in todo]), lens, m, _ptr_array(outs), ccaps, olens, crcs)
            again = []
            for j, k in enumerate(todo):
                rcs[k] = crcs[j]
                if crcs[j] == N.TIC_OK:
                    results[k] = outs[j][: olens[j]].tobytes()
                elif crcs[j] == N.TIC_E_SPACE and olens[j] > caps[k]:
                    caps[k] = olens[j]
                    again.append(k)
            todo = again
            if not todo:
                break
        return results, rcs

    return _transcode_batch(streams, ctx, errors, precheck, call, single)


def retable_adaptive_batch(streams, ctx=None, errors="raise"):
    """retable_adaptive() of many stored streams in one call: a list of streams, frame i byte for byte what retable_adaptive(streams[i])
    gives.  The coefficients of a chunk (up to 64 frames) stay on the GPU between the reader and the adaptive writer: one upload, the
    reader's launches and one statistics launch, one read-back, the tables on the host, the packing launches, one download.
    errors="return": a failing frame's place holds its exception instead of the first one being raised."""

    def precheck(i, buf):
        _retable_adaptive_header(buf)
        return buf.size + 4096  # (the adaptive stream is the shorter one as a rule: once more with the reported length otherwise)

    return _retable_batch(streams, ctx, errors, precheck, "tic_retable_adaptive_batch", lambda s, c: retable_adaptive(s, ctx=c))


def retable_default_batch(streams, ctx=None, errors="raise"):
    """retable_default() of many streams with embedded tables in one call, frame i byte for byte what retable_default(streams[i]) gives:
    the adaptive batch reader, then the default writer's descriptor-form launches on the resident coefficients.  errors as above."""

    def precheck(i, buf):
        hdr = _adaptive_header(buf)
        # (the default stream is the longer one, by 40 % at the lowest qualities: once more with the reported lengths otherwise)
        return min(N.load().tic_compress_bound(hdr["height"], hdr["width"]), 2 * buf.size + 4096)

    return _retable_batch(streams, ctx, errors, precheck, "tic_retable_default_batch", lambda s, c: retable_default(s, ctx=c))


def last_transcode_batch(ctx=None):
    """(batch_frames, single_frames, chunks) of the context's last batch transcoding call."""
    ctx = _ctx(ctx)
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    with ctx.lock:
        ctx.check(N.load().tic_last_transcode_batch(ctx.handle, C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def decode(data, ctx=None):
    """decode() of the reference: dict with height, width, quality, scaled_dct, dc (DPCM'd), ac."""
    ctx = _ctx(ctx)
    height, width, quality = data["height"], data["width"], data["quality"]
    scaled = bool(data["scaled_dct"])
    dc = np.cumsum(np.asarray(data["dc"], dtype=np.int64))  # codec.py:53
    ac = np.asarray(data["ac"])
    n = N.load().tic_num_blocks(int(height), int(width))
    if dc.shape[0] != n or ac.shape != (n, 63):
        raise ValueError("dc/ac shapes do not match the image geometry")
    if n and (np.abs(dc).max() > 32767 or np.abs(ac).max(initial=0) > 32767):
        raise ValueError("coefficients exceed the int16 device layout")
    zz = np.empty((n, 64), dtype=np.int16)
    zz[:, 0] = dc
    zz[:, 1:] = ac
    out = np.zeros((int(height), int(width)), dtype=np.uint8)
    if scaled:  # codec.py:59-62: the quality field is an exponent, the inverse quantiser runs at quality 50
        if int(quality) != quality or not (0 <= int(quality) <= 62):
            raise ValueError("scaled_dct exponent outside 0..62")
        if n:
            with ctx.lock:
                ctx.check(N.load().tic_idctq_scaled(ctx.handle, zz.ctypes.data, int(height), int(width), int(quality), out.ctypes.data, out.size))
        return out
    q = _check_quality(quality, packs_header=False)
    if n:
        with ctx.lock:
            ctx.check(N.load().tic_idctq(ctx.handle, zz.ctypes.data, int(height), int(width), _q_arg(ctx, q), out.ctypes.data, out.size))
    return out
