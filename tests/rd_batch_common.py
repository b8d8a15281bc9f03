"""Helpers of the batch rate-distortion tests (test_rd_batch_gpu.py): the C calls tic_rd_points_v / tic_compress_batch_to_psnr /
tic_distortion_v_dev through any bound library, the frame list the tests share, built coefficient probes with known sums, and the replay
of the lockstep search by distortion on recorded errors.  No test lives here."""
import ctypes as C

import numpy as np

from tinyimgcodec_amd import _native as N

import rate_batch_common as R
from conftest import rand_frame

SENTINEL = R.SENTINEL
# behind rate_batch_common.small_frames(): 33 blocks in a row (5 tiles: a second workgroup with one wave at work) and 27 tiles (9 block rows
# of 3 strips: a tile count that is no multiple of a workgroup's 4)
EXTRA_SHAPES = ((8, 264), (72, 136))
QUALITIES = R.SMALL_QUALITIES


def frames():
    return R.small_frames() + [rand_frame(200 + i, h, w) for i, (h, w) in enumerate(EXTRA_SHAPES)]


def bind(path):
    """A library bound beside the one this process runs (the build that ships, in the tests)."""
    L = C.CDLL(path)
    for fn, (res, args) in N.SIGNATURES.items():
        f = getattr(L, fn)
        f.restype, f.argtypes = res, args
    return L


def rd_v(L, handle, frame_list, qs, inputs=None, scaled=False):
    """tic_rd_points_v (scaled: tic_rd_points_scaled_v, `qs` its settings) -> (rc, sizes, sse, wrapped), (n, nq) each, filled with markers the
    call must overwrite."""
    keep, inp, hs, ws, strides = R.frame_arrays(frame_list, inputs)
    qarr = (C.c_int * len(qs))(*qs)
    shape = (len(frame_list), len(qs))
    sizes, sse, wrapped = np.full(shape, -7, np.int64), np.full(shape, 7, np.uint64), np.full(shape, 7, np.uint64)
    rc = (L.tic_rd_points_scaled_v if scaled else L.tic_rd_points_v)(handle, inp, len(frame_list), hs, ws, strides, qarr, len(qs), sizes.ctypes.data, sse.ctypes.data, wrapped.ctypes.data)
    return rc, sizes, sse, wrapped


def rd_single(L, handle, img, qs):
    """tic_rd_points -> (sizes, sse, wrapped) lists."""
    img = np.ascontiguousarray(img)
    h, w = img.shape
    qa = (C.c_int * len(qs))(*qs)
    sz = (C.c_longlong * len(qs))(*([-5] * len(qs)))
    a, b = (C.c_uint64 * len(qs))(), (C.c_uint64 * len(qs))()
    rc = L.tic_rd_points(handle, img.ctypes.data if img.size else None, h, w, max(w, 1), qa, len(qs), sz, a, b)
    assert rc == N.TIC_OK, (rc, L.tic_last_error(handle).decode())
    return list(sz), list(a), list(b)


def sse_launches(L, handle):
    v = C.c_int(-1)
    assert L.tic_last_rd_batch(handle, C.byref(v)) == 0
    return v.value


class PsnrCall:
    """One tic_compress_batch_to_psnr: every output a sentinel-filled buffer of caps[i] + 8 bytes.  run() -> rc; then status, lens, quals,
    sse, stream(i), tail_intact(i) (the bytes behind the stream, or the whole buffer of a failed frame)."""

    def __init__(self, L, handle, frame_list, bounds, qmin=1, qmax=99, caps=None, inputs=None):
        self.L, self.handle, self.n = L, handle, len(frame_list)
        self.keep, self.inp, self.hs, self.ws, self.strides = R.frame_arrays(frame_list, inputs)
        n = self.n
        caps = [L.tic_compress_bound(f.shape[0], f.shape[1]) for f in frame_list] if caps is None else list(caps)
        self.bufs = [np.full(c + 8, SENTINEL, np.uint8) for c in caps]
        self.outp = (C.c_void_p * n)(*[b.ctypes.data for b in self.bufs])
        self.caps = (C.c_size_t * n)(*caps)
        self.bounds = (C.c_uint64 * n)(*bounds)
        self.lens = (C.c_size_t * n)(*([77] * n))
        self.quals = (C.c_int * n)(*([-1] * n))
        self.sse = (C.c_uint64 * n)(*([7] * n))
        self.status = (C.c_int * n)(*([-99] * n))
        self.qmin, self.qmax = qmin, qmax

    def run(self):
        return self.L.tic_compress_batch_to_psnr(self.handle, self.inp, self.n, self.hs, self.ws, self.strides, self.bounds, self.qmin, self.qmax,
                                                 self.outp, self.caps, self.lens, self.quals, self.sse, self.status)

    def stream(self, i):
        return self.bufs[i][: self.lens[i]].tobytes()

    def tail_intact(self, i):
        start = self.lens[i] if self.status[i] == N.TIC_OK else 0
        return bool((self.bufs[i][start:] == SENTINEL).all())


def psnr_single(L, handle, img, max_sse, qmin, qmax, cap):
    """tic_compress_to_psnr into a sentinel-filled buffer of cap + 8 bytes -> (rc, len, quality, sse, buffer); the three side values start
    at PsnrCall's markers."""
    img = np.ascontiguousarray(img)
    h, w = img.shape
    buf = np.full(cap + 8, SENTINEL, np.uint8)
    n, q, s = C.c_size_t(77), C.c_int(-1), C.c_uint64(7)
    rc = L.tic_compress_to_psnr(handle, img.ctypes.data if img.size else None, h, w, max(w, 1), max_sse, qmin, qmax, buf.ctypes.data, cap,
                                C.byref(n), C.byref(q), C.byref(s))
    return rc, n.value, q.value, s.value, buf


def lockstep_probes(sse, max_sse, qmin, qmax, depth):
    """The lockstep search of one frame replayed on recorded errors (index q - 1; None = no code) -> (rounds, probes): in every round qmax
    (the first one) and every middle the bisection can reach within `depth` further steps, then the bisection as far as they carry."""
    known = set()

    def meets(q):
        return sse[q - 1] is not None and sse[q - 1] <= max_sse

    def cands(lo, hi, d, out):
        if lo >= hi or d == 0:
            return
        mid = (lo + hi) // 2
        if mid not in known and mid not in out:
            out.append(mid)
        cands(lo, mid, d - 1, out)
        cands(mid + 1, hi, d - 1, out)

    lo, hi, rounds, probes = qmin, qmax, 0, 0
    while True:
        out = [] if qmax in known else [qmax]
        cands(lo, hi, depth, out)
        if not out:
            return rounds, probes
        rounds, probes = rounds + 1, probes + len(out)
        known.update(out)
        if not meets(qmax):
            return rounds, probes
        while lo < hi:
            mid = (lo + hi) // 2
            if mid not in known:
                break
            if meets(mid):
                hi = mid
            else:
                lo = mid + 1


def rate_depth(chunk_blocks):
    """tic_rate_plan.h's look-ahead of a chunk."""
    for d in (3, 2):
        if (chunk_blocks * 128) << d <= 128 << 20:
            return d
    return 1


class BuiltProbes:
    """Probes for tic_distortion_v_dev whose sums are known in closed form: every block's DC is +2000 or -2000 and its AC zero, which decodes
    to all 255 or all 0 at any quality (|2000 * Q00 * factor / 8| is far beyond the clip); the image is one constant per probe.  With
    d = |decoded - constant| the sums are h * w * d * d and h * w * ((d * d) & 255).  Coefficients back to back, every image at an offset
    of its own in one device buffer (8-byte aligned, pitch a multiple of 8 - or neither, for the ragged probes)."""

    def __init__(self, specs):
        """specs: [(h, w, quality, decoded 0 or 255, image constant, aligned)]."""
        self.specs = specs
        zz, off = [], 0
        self.img_off, self.stride = [], []
        chunks = []
        for h, w, q, dec, const, aligned in specs:
            nb = ((h + 7) // 8) * ((w + 7) // 8)
            blocks = np.zeros((nb, 64), np.int16)
            blocks[:, 0] = 2000 if dec == 255 else -2000
            zz.append(blocks)
            stride = (w + 7) // 8 * 8 if aligned else w + (1 if w % 2 == 0 else 2)
            off = (off + 7) // 8 * 8 + (0 if aligned else 3)
            img = np.full((h, stride), 0x5A, np.uint8)  # (padding that would show in the sums if it were counted)
            img[:, :w] = const
            self.img_off.append(off)
            self.stride.append(stride)
            chunks.append((off, img))
            off += img.size
        self.zz = np.ascontiguousarray(np.concatenate(zz))
        self.pixels = np.full(off + 8, 0x5A, np.uint8)
        for o, img in chunks:
            self.pixels[o: o + img.size] = img.ravel()
        self.want = []
        for h, w, q, dec, const, aligned in specs:
            d = abs(dec - const)
            self.want.append((h * w * d * d, h * w * ((d * d) & 255)))

    def run(self, L, handle, dev):
        """-> (rc, [(sse, wrapped), ...], launches)."""
        n = len(self.specs)
        d_zz, d_px = dev.upload(self.zz), dev.upload(self.pixels)
        imgs = (C.c_void_p * n)(*[d_px.value + o for o in self.img_off])
        hs = (C.c_int * n)(*[s[0] for s in self.specs])
        ws = (C.c_int * n)(*[s[1] for s in self.specs])
        strides = (C.c_ssize_t * n)(*self.stride)
        qs = (C.c_int * n)(*[s[2] for s in self.specs])
        out = np.full((n, 2), 7, np.uint64)
        rc = L.tic_distortion_v_dev(handle, d_zz, imgs, n, hs, ws, strides, qs, out.ctypes.data)
        ms = C.c_float(-1.0)
        assert L.tic_distortion_v_dev_timed(handle, d_zz, imgs, n, hs, ws, strides, qs, 1, 2, C.byref(ms)) == N.TIC_OK and ms.value > 0
        return rc, [tuple(r) for r in out.tolist()], sse_launches(L, handle)
