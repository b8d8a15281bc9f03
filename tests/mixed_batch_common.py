"""What the tests of the mixed batch (tic_compress_batch_v, compress_batch with shapes or qualities that differ) share: the small frame set of
the issue, a C-ABI caller that keeps every array alive and shows what the call wrote, and the call's figures."""
import ctypes as C
import os

import numpy as np

from tinyimgcodec_amd import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (h, w, content, quality).  One block; a partition tail of the 8-lane form (blocks % 8 != 0: 7 x 9, 15 x 17, 40 x 52, 200 x 264); a partition tail
# of the lane form (blocks % 64 != 0: all but 64 x 64 and 512 x 512); more than one group (128 x 136: 272 blocks = 34 partitions of 8; 512 x 512: 32
# groups of 8-lane partitions, 16 of lane partitions); more than one place (200 x 264, 512 x 512); ragged edges for the exact kernel (7 x 9, 15 x 17,
# 40 x 52, 200 x 264).  Qualities from {5, 10, 50, 90, 99} so that neighbours differ.  The last two frames are there for the transform's runs: 24 x 52
# joins 40 x 52 and the second 64 x 64 the first (equal width and quality, heights that are multiples of 8 but differ: two runs that merge).
SMALL = [(1, 1, "noise", 50), (8, 8, "noise", 5), (7, 9, "noise", 90), (15, 17, "fixture", 10), (40, 52, "noise", 99), (64, 64, "flat", 50),
         (72, 40, "noise", 5), (128, 136, "noise", 90), (200, 264, "noise", 10), (512, 512, "noise", 50), (24, 52, "noise", 99), (64, 64, "flat", 50)]
MERGED_RUNS = 2  # of SMALL in one chunk: 12 frames, 10 transform launches


def small_frames():
    """-> (frames, qualities) of SMALL.  Noise at q = 99 is kept within 64..191 so that every coefficient has a Huffman code."""
    fixture = np.load(os.path.join(GOLDEN, "transform_small.npz"))["rand_15x17_q50_img"]
    frames, qs = [], []
    for k, (h, w, kind, q) in enumerate(SMALL):
        if kind == "fixture":
            img = np.ascontiguousarray(fixture)
            assert img.shape == (h, w)
        elif kind == "flat":
            img = np.full((h, w), 128, np.uint8)
        else:
            lo, hi = (64, 192) if q == 99 else (0, 256)
            img = np.random.default_rng(4200 + k).integers(lo, hi, (h, w), dtype=np.uint8)
        frames.append(img)
        qs.append(q)
    return frames, qs


class VCall:
    """One tic_compress_batch_v call.  outs[i] is a buffer of caps[i] bytes filled with 0xAB in front of the call (so that a test sees what
    the call wrote); `null_images`: frames whose pixel pointer is null while their sizes stay; `caps`, `strides` override what the frames give;
    `null_arrays`: arguments passed as null pointers; `n`: the count passed, if not len(frames); `inputs`: (pointers, strides) of frames that lie
    elsewhere than in `frames` (batch_inputs_common.Arena.inputs(); a pointer of 0 is passed as null), which then only give the shapes."""

    def __init__(self, ctx, frames, quals, caps=None, strides=None, null_arrays=(), null_images=(), n=None, inputs=None):
        L = self.L = N.load()
        count, n = n, len(frames)
        self.n = n
        self.keep = [np.ascontiguousarray(f) for f in frames]
        shapes = [f.shape for f in self.keep]
        self.bounds = [L.tic_compress_bound(h, w) for h, w in shapes]
        self.caps = list(self.bounds if caps is None else caps)
        self.outs = [np.full(max(c, 1), 0xAB, np.uint8) for c in self.caps]
        arr = {
            "images": (C.c_void_p * n)(*[None if i in null_images or f.size == 0 else f.ctypes.data for i, f in enumerate(self.keep)])
            if inputs is None else (C.c_void_p * n)(*[p or None for p in inputs[0]]),
            "hs": (C.c_int * n)(*[s[0] for s in shapes]),
            "ws": (C.c_int * n)(*[s[1] for s in shapes]),
            "strides": (C.c_ssize_t * n)(*(strides if strides is not None else inputs[1] if inputs is not None else [max(s[1], 1) for s in shapes])),
            "quals": (C.c_int * n)(*quals),
            "outs": (C.c_void_p * n)(*[o.ctypes.data for o in self.outs]),
            "caps": (C.c_size_t * n)(*self.caps),
            "lens": (C.c_size_t * n)(),
        }
        self.lens = arr["lens"]
        a = {k: (None if k in null_arrays else v) for k, v in arr.items()}
        self.rc = L.tic_compress_batch_v(ctx.handle, a["images"], n if count is None else count, a["hs"], a["ws"], a["strides"], a["quals"], a["outs"], a["caps"], a["lens"])
        self.error = L.tic_last_error(ctx.handle).decode()

    def streams(self):
        assert self.rc == 0, (self.rc, self.error)
        return [self.outs[i][: self.lens[i]].tobytes() for i in range(self.n)]

    def untouched(self):
        return all(bool((o == 0xAB).all()) for o in self.outs)


def figures(ctx):
    """-> (batch_frames, single_frames, chunks, transform_launches) of the context's last tic_compress_batch_v."""
    v = [C.c_int(-1) for _ in range(4)]
    assert N.load().tic_last_compress_batch_v(ctx.handle, *[C.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)
