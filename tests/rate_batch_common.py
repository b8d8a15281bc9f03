"""Helpers of the batch rate-control tests (test_rate_batch_gpu.py): the C calls tic_stream_sizes_v / tic_compress_batch_to_size through any
bound library, the frame lists the tests share, and the replay of the 66-frame search list on the recorded sizes."""
import ctypes as C

import numpy as np

from tinyimgcodec_amd import _native as N

from conftest import rand_frame
from test_rate_control_cpu import IMAGES, fixture_image

SENTINEL = 0xA5
SMALL_SHAPES = ((1, 1), (8, 8), (7, 9), (15, 17), (24, 8), (72, 8), (128, 8), (136, 8), (40, 52), (203, 317), (0, 8), (8, 0))
SMALL_QUALITIES = (5, 50, 90)


def small_frames():
    """The smallest shapes at which the descriptor form can go wrong: one block, ragged edges, 3 blocks, 9 blocks (a second, partial chunk
    of 8), 16 and 17 blocks, several block rows, the fixture's ragged crop, and two frames without blocks."""
    return [rand_frame(100 + i, h, w) for i, (h, w) in enumerate(SMALL_SHAPES)]


def frame_arrays(frames, inputs=None):
    """`inputs`: (pointers, strides) of frames that lie elsewhere than in `frames` (batch_inputs_common.Arena.inputs(); a pointer of 0 is
    passed as null), which then only give the shapes."""
    n = len(frames)
    frames = [np.ascontiguousarray(f) for f in frames]
    inp = (C.c_void_p * n)(*([f.ctypes.data if f.size else None for f in frames] if inputs is None else [p or None for p in inputs[0]]))
    hs = (C.c_int * n)(*[f.shape[0] for f in frames])
    ws = (C.c_int * n)(*[f.shape[1] for f in frames])
    strides = (C.c_ssize_t * n)(*([max(f.shape[1], 1) for f in frames] if inputs is None else inputs[1]))
    return frames, inp, hs, ws, strides


def sizes_v(L, handle, frames, qs, inputs=None):
    """tic_stream_sizes_v -> (rc, int64 array (n, nq))."""
    keep, inp, hs, ws, strides = frame_arrays(frames, inputs)
    qarr = (C.c_int * len(qs))(*qs)
    out = np.full((len(frames), len(qs)), -7, np.int64)
    rc = L.tic_stream_sizes_v(handle, inp, len(frames), hs, ws, strides, qarr, len(qs), out.ctypes.data)
    return rc, out


def figures(L, handle):
    """tic_last_rate_batch -> (batch_frames, single_frames, chunks, probes, search_waits, size_launches)."""
    v = [C.c_int(-1) for _ in range(6)]
    assert L.tic_last_rate_batch(handle, *[C.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


class SearchCall:
    """One tic_compress_batch_to_size: every output a sentinel-filled buffer of caps[i] + 8 bytes.  run() -> rc; then status, lens, quals,
    stream(i), tail_intact(i) (the bytes behind the stream, or the whole buffer of a failed frame)."""

    def __init__(self, L, handle, frames, budgets, qmin=1, qmax=99, caps=None, inputs=None):
        self.L, self.handle, self.n = L, handle, len(frames)
        self.keep, self.inp, self.hs, self.ws, self.strides = frame_arrays(frames, inputs)
        n = self.n
        caps = [L.tic_compress_bound(f.shape[0], f.shape[1]) for f in frames] if caps is None else list(caps)
        self.bufs = [np.full(c + 8, SENTINEL, np.uint8) for c in caps]
        self.outp = (C.c_void_p * n)(*[b.ctypes.data for b in self.bufs])
        self.caps = (C.c_size_t * n)(*caps)
        self.budgets = (C.c_size_t * n)(*budgets)
        self.lens = (C.c_size_t * n)(*([0] * n))
        self.quals = (C.c_int * n)(*([-1] * n))
        self.status = (C.c_int * n)(*([-99] * n))
        self.qmin, self.qmax = qmin, qmax

    def run(self):
        return self.L.tic_compress_batch_to_size(self.handle, self.inp, self.n, self.hs, self.ws, self.strides, self.budgets, self.qmin, self.qmax,
                                                 self.outp, self.caps, self.lens, self.quals, self.status)

    def stream(self, i):
        return self.bufs[i][: self.lens[i]].tobytes()

    def tail_intact(self, i):
        start = self.lens[i] if self.status[i] == N.TIC_OK else 0
        return bool((self.bufs[i][start:] == SENTINEL).all())


def search_list(fx):
    """The 66 frames of the search test: per fixture image the budgets size(q) for q in (1, 7, 20, 33, 50, 64, 90, last encodable),
    size(20) - 1, size(50) - 1 and 10^9 -> [(name, budget), ...]."""
    out = []
    for name in IMAGES:
        s = fx[name]["sizes"]
        last = max(q for q in range(1, 100) if s[q - 1] is not None)
        for b in [s[q - 1] for q in (1, 7, 20, 33, 50, 64, 90, last)] + [s[19] - 1, s[49] - 1, 10 ** 9]:
            out.append((name, b))
    return out


class Streams:
    """oracle.compress(fixture image, q), computed once per (name, q)."""

    def __init__(self, oracle):
        self.oracle, self.cache, self.images = oracle, {}, {}

    def image(self, name):
        if name not in self.images:
            self.images[name] = fixture_image(name)
        return self.images[name]

    def get(self, name, q):
        if (name, q) not in self.cache:
            self.cache[(name, q)] = self.oracle.compress(self.image(name), q)
        return self.cache[(name, q)]
