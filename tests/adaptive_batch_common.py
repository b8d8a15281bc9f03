"""What the tests of the adaptive batch encoder (tic_compress_batch_adaptive_v, compress_batch_adaptive) share: the fixture's frames rebuilt by
the recipes of tests/golden/gen/make_goldens_adaptive_batch.py, a C-ABI caller that keeps every array alive and shows what the call wrote, and
the call's figures."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

from tinyimgcodec_amd import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sha(b):
    return hashlib.sha256(b).hexdigest()


def make_frame(kind, seed, h, w):
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    if kind.startswith("flat"):
        return np.full((h, w), int(kind[4:]), np.uint8)
    if kind == "checker":  # 8x8 blocks alternating between 0 and 255 (raster order)
        by, bx = np.indices(((h + 7) // 8, (w + 7) // 8))
        return np.kron(np.where((by + bx) % 2 == 0, 0, 255).astype(np.uint8), np.ones((8, 8), np.uint8))[:h, :w]
    raise KeyError(kind)


def load_fixture():
    """-> (entries, frames, qualities) of tests/golden/adaptive_batch.json."""
    with open(os.path.join(GOLDEN, "adaptive_batch.json")) as f:
        entries = json.load(f)["frames"]
    frames = [make_frame(e["kind"], e["seed"], e["height"], e["width"]) for e in entries]
    return entries, frames, [e["quality"] for e in entries]


def check_stream(out, e):
    assert len(out) == e["bytes"], (len(out), e["bytes"])
    if "stream" in e:
        assert out.hex() == e["stream"]
    assert sha(out) == e["sha256"]


class ACall:
    """One tic_compress_batch_adaptive_v call (or, with coeffs=True, tic_entropy_encode_adaptive_batch: `frames` are then int16 [N, 64] arrays and
    `shapes` their (h, w)).  outs[i] is a buffer of caps[i] + 64 bytes filled with 0xAB in front of the call, so that a test sees what the call
    wrote, behind the capacity it gave away too.  `inputs`: (pointers, strides) of frames that lie elsewhere than in `frames`
    (batch_inputs_common.Arena.inputs()), which then only give the shapes."""

    def __init__(self, ctx, frames, quals, caps, coeffs=False, shapes=None, inputs=None):
        L = N.load()
        n = self.n = len(frames)
        self.keep = [np.ascontiguousarray(f) for f in frames]
        shapes = [f.shape for f in self.keep] if shapes is None else shapes
        self.caps = list(caps)
        self.outs = [np.full(c + 64, 0xAB, np.uint8) for c in self.caps]
        inp = (C.c_void_p * n)(*([f.ctypes.data for f in self.keep] if inputs is None else [p or None for p in inputs[0]]))
        hs = (C.c_int * n)(*[s[0] for s in shapes])
        ws = (C.c_int * n)(*[s[1] for s in shapes])
        qa = (C.c_int * n)(*quals)
        outp = (C.c_void_p * n)(*[o.ctypes.data for o in self.outs])
        capa = (C.c_size_t * n)(*self.caps)
        self.lens = (C.c_size_t * n)()
        if coeffs:
            self.rc = L.tic_entropy_encode_adaptive_batch(ctx.handle, inp, n, hs, ws, qa, outp, capa, self.lens)
        else:
            strides = (C.c_ssize_t * n)(*([max(s[1], 1) for s in shapes] if inputs is None else inputs[1]))
            self.rc = L.tic_compress_batch_adaptive_v(ctx.handle, inp, n, hs, ws, strides, qa, outp, capa, self.lens)
        self.error = L.tic_last_error(ctx.handle).decode()


def figures(ctx):
    """-> (batch_frames, single_frames, chunks) of the context's last adaptive batch call."""
    v = [C.c_int(-1) for _ in range(3)]
    assert N.load().tic_last_compress_batch_adaptive(ctx.handle, *[C.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)
