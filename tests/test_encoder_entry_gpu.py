"""The encoder entry points' shared set-up (tic_api.hip: upload_image, set_frames, timed_launches, stream_result and friends): every
argument check answers what it answered before the entry points were folded onto these helpers (tests/golden/encoder_errors.json), a
frame whose rows are further apart than its width is uploaded right by all seven host-image entry points, the timed entries report
per-launch times only for launches that recorded them, and images without blocks leave the header-only stream the host coder writes."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

import encoder_error_rows as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def env(ctx):
    e = R.Env(N.load(), ctx.handle)
    yield e
    e.close()


def test_error_table(env):
    """Return code and tic_last_error text of every argument check, equal to the recording made from the commit before the refactor."""
    with open(os.path.join(GOLDEN, "encoder_errors.json")) as f:
        want = json.load(f)
    assert want["async_slots"] == R.ASYNC_SLOTS
    got = R.play(env)
    assert sorted(got) == sorted(want["rows"])
    bad = {k: (got[k], want["rows"][k]) for k in got if got[k] != want["rows"][k]}
    assert not bad, bad


def strided_frames():
    """(view, contiguous copy) of a 40 x 72 and a 64 x 64 frame inside wider arrays (row stride 100 and 96).  The 64 x 64 frame is a
    case of the scaled-DCT fixtures, whose coefficients and stream were recorded from the reference's C encoder."""
    rng = np.random.default_rng(20261018)
    wide = rng.integers(0, 256, (50, 100), dtype=np.uint8)
    a = wide[5:45, 7:79]
    wide2 = rng.integers(0, 256, (70, 96), dtype=np.uint8)
    wide2[3:67, 16:80] = np.load(os.path.join(GOLDEN, "scaled_encode.npz"))["twolevel64x64_best_img"]
    b = wide2[3:67, 16:80]
    return [(v, np.ascontiguousarray(v)) for v in (a, b)]


def test_strided_upload(ctx, oracle):
    """All seven host-image entry points on views whose row stride exceeds the width == the oracle on the contiguous copy."""
    L, c = N.load(), ctx.handle
    n, qout = C.c_size_t(0), C.c_int(0)
    for view, img in strided_frames():
        assert not view.flags["C_CONTIGUOUS"] and view.strides[0] > view.shape[1]
        h, w = view.shape
        s, p = view.strides[0], view.ctypes.data
        for q in (10, 75):
            want_zz, want_bs = oracle.encode_zz16(img, q), oracle.compress(img, q)
            zz = np.zeros_like(want_zz)
            ctx.check(L.tic_dctq(c, p, h, w, s, q, zz.ctypes.data))
            assert np.array_equal(zz, want_zz), ("tic_dctq", h, w, q)
            out = np.zeros(L.tic_compress_adaptive_bound(h, w) + 64, np.uint8)
            ctx.check(L.tic_compress(c, p, h, w, s, q, out.ctypes.data, out.size, C.byref(n)))
            assert out[: n.value].tobytes() == want_bs, ("tic_compress", h, w, q)
            quals, sizes = np.array([q], np.int32), np.zeros(1, np.int64)
            ctx.check(L.tic_stream_sizes(c, p, h, w, s, quals.ctypes.data, 1, sizes.ctypes.data))
            assert sizes[0] == len(want_bs), ("tic_stream_sizes", h, w, q)
            out[:] = 0
            ctx.check(L.tic_compress_to_size(c, p, h, w, s, 10 ** 9, q, q, out.ctypes.data, out.size, C.byref(n), C.byref(qout)))
            assert (n.value, qout.value) == (len(want_bs), q) and out[: n.value].tobytes() == want_bs, ("tic_compress_to_size", h, w, q)
            # per-image tables: the stream the library builds from the oracle's coefficients of the contiguous copy
            ref = np.zeros_like(out)
            m = C.c_size_t(0)
            ctx.check(L.tic_entropy_encode_adaptive(c, want_zz.ctypes.data, h, w, q, ref.ctypes.data, ref.size, C.byref(m)))
            out[:] = 0
            ctx.check(L.tic_compress_adaptive(c, p, h, w, s, q, out.ctypes.data, out.size, C.byref(n)))
            assert n.value == m.value and np.array_equal(out[: n.value], ref[: m.value]), ("tic_compress_adaptive", h, w, q)
    # the scaled forms: the 64 x 64 frame, against the reference encoder's recorded coefficients and stream
    npz = np.load(os.path.join(GOLDEN, "scaled_encode.npz"))
    zz = np.zeros((64, 64), np.int16)
    ctx.check(L.tic_dctq_scaled(c, p, 64, 64, s, 0, zz.ctypes.data))
    assert np.array_equal(zz, npz["twolevel64x64_best_zz"].reshape(64, 64))
    out = np.zeros(L.tic_compress_scaled_bound(64, 64), np.uint8)
    ctx.check(L.tic_compress_scaled(c, p, 64, 64, s, 0, out.ctypes.data, out.size, C.byref(n)))
    assert out[: n.value].tobytes() == npz["twolevel64x64_best_bs"].tobytes()


def test_timed_loop(ctx, env):
    """One context throughout.  Only signs and order of the times are asserted."""
    L, c = env.L, ctx.handle
    ms, per = C.c_float(0), (C.c_float * 6)()
    d_img, d_zz = env.alloc(64 * 72), env.alloc(L.tic_num_blocks(64, 72) * 128 + 16)
    assert L.tic_memset_dev(c, d_img, 0x55, 64 * 72) == 0 and L.tic_sync(c) == 0

    def warm(h, w, variant):
        for k in range(6):
            per[k] = -1.0
        ms.value = -1.0
        return L.tic_dctq_dev_timed_warm(c, d_img, h, w, w, 50, d_zz, variant, 1, 3, C.byref(ms), per)

    for h, w in ((64, 64), (64, 72)):  # the strip kernel alone / the strip kernel and the exact kernel for the remaining column
        ctx.check(warm(h, w, N.KERNEL_HYBRID))
        print(h, w, "ms_total", ms.value, "per launch", list(per))
        assert ms.value > 0
        assert all(per[2 * i] > 0 for i in range(3))
        assert 0 < per[1] <= per[3] <= per[5]
    # The exact kernel binds no events.  Before the per-launch events lived for one call only, this call found the recordings of
    # the call above in the context's events and returned TIC_OK with that call's numbers; now it is the documented error.
    assert warm(64, 64, N.KERNEL_EXACT) == N.TIC_E_ARG
    assert L.tic_last_error(c).decode() == "per-launch times need a frame that takes the strip kernel in one launch"
    ctx.check(warm(64, 64, N.KERNEL_HYBRID))  # ... and the next call is unaffected
    assert all(per[2 * i] > 0 for i in range(3))
    ms.value = -1.0
    ctx.check(L.tic_dctq_scaled_dev_timed_warm(c, d_img, 64, 64, 64, 2, d_zz, 1, 3, C.byref(ms), per))
    assert ms.value > 0 and all(per[2 * i] > 0 for i in range(3)) and 0 < per[1] <= per[3] <= per[5]
    ms.value = -1.0
    ctx.check(L.tic_entropy_size_dev_timed(c, d_zz, 64, 64, 1, 3, C.byref(ms)))
    assert ms.value > 0


@pytest.mark.parametrize("h,w", [(0, 16), (16, 0)])
def test_empty_images(ctx, env, h, w):
    """Images without blocks through the device forms: the header-only stream of the host coder, 16 bytes (17 for a scaled-DCT stream)."""
    L, c = env.L, ctx.handle
    want, want_s, n = np.zeros(32, np.uint8), np.zeros(32, np.uint8), C.c_size_t(0)
    assert L.tic_entropy_encode(None, h, w, 50, want.ctypes.data, 32, C.byref(n)) == 0 and n.value == 16
    assert L.tic_entropy_encode_scaled(None, h, w, 2, want_s.ctypes.data, 32, C.byref(n)) == 0 and n.value == 17

    def fetch(nbytes):
        got = np.zeros(nbytes, np.uint8)
        assert L.tic_memcpy_d2h(c, got.ctypes.data, env.d_out, nbytes) == 0
        assert L.tic_memset_dev(c, env.d_out, 0xA5, 32) == 0 and L.tic_sync(c) == 0
        return got

    fetch(32)
    ctx.check(L.tic_compress_dev(c, None, h, w, w, 50, env.d_out, env.cap, C.byref(n)))
    assert n.value == 16 and np.array_equal(fetch(16), want[:16])
    tk = C.c_longlong(-1)
    ctx.check(L.tic_compress_dev_async(c, None, h, w, w, 50, env.d_out, env.cap, C.byref(tk)))
    ctx.check(L.tic_async_result(c, tk.value, 1, C.byref(n)))
    assert n.value == 16 and np.array_equal(fetch(16), want[:16])
    q = C.c_int(0)
    ctx.check(L.tic_compress_to_size_dev(c, None, h, w, w, 16, 50, 50, env.d_out, env.cap, C.byref(n), C.byref(q)))
    assert (n.value, q.value) == (16, 50) and np.array_equal(fetch(16), want[:16])
    ctx.check(L.tic_compress_scaled_dev(c, None, h, w, w, 2, env.d_out, env.cap, C.byref(n)))
    assert n.value == 17 and np.array_equal(fetch(17), want_s[:17])
