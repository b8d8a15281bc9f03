"""Shared by tests/test_inverse_edges_cpu.py, tests/test_inverse_transform_gpu.py and tests/golden/gen/make_goldens_inverse.py: the
fixture tests/golden/inverse_edges.npz / .json (built coefficients for the two inverse transforms and what the unmodified reference
decodes them to) and the plain numpy restatements the tests compare with.  No test lives here.

A frame of the fixture: int32 DC differences `dc` [N] and `ac` [N, 63] in zig-zag order (the dictionary of the reference's decode(),
codec.py:46-70), height, width, the header's quality field (an exponent when flag = 1 << 30; a float for the one frame that only decode()
can carry) and the flag; of the reference's pixels their sha256 and three 64 x 64 crops.
"""
import hashlib
import json
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCALED = 1 << 30
CROP = 64


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def px_sha(px):
    return sha(np.ascontiguousarray(px, dtype=np.uint8).tobytes())


def crop_origins(h, w):
    """Top left, middle, bottom right (clamped to the frame)."""
    ch, cw = min(CROP, h), min(CROP, w)
    return [(0, 0), ((h - ch) // 2, (w - cw) // 2), (h - ch, w - cw)], ch, cw


def crops_of(px):
    org, ch, cw = crop_origins(*px.shape)
    return np.stack([px[y:y + ch, x:x + cw] for y, x in org])


class Fixture:
    def __init__(self, golden_dir=GOLDEN):
        self.npz = np.load(os.path.join(golden_dir, "inverse_edges.npz"))
        with open(os.path.join(golden_dir, "inverse_edges.json")) as f:
            self.meta = json.load(f)
        self.frames = self.meta["frames"]  # name -> {family, height, width, quality, flag, ...}
        self.zigzag = self.npz["zigzag"]
        self.annscales = self.npz["annscales"]
        self.qtable = self.npz["qtable"]

    def names(self, family=None, streams_only=False):
        return [n for n, e in self.frames.items() if (family is None or e["family"] == family) and not (streams_only and e["stream_sha256"] is None)]

    def coeffs(self, name):
        return self.npz["dc_" + name], self.npz["ac_" + name]

    def crops(self, name):
        return self.npz["crop_" + name]

    def matches_reference(self, name, px):
        """px is what the reference decoded this frame to: digest and crops."""
        e = self.frames[name]
        return px.shape == (e["height"], e["width"]) and px.dtype == np.uint8 and px_sha(px) == e["pixels_sha256"] and np.array_equal(crops_of(px), self.crops(name))


def stream_of(O, dc, ac, h, w, quality, flag):
    """The default-table stream of these coefficients: the oracle's entropy coder, then the header's quality and flag fields as asked
    (codec.py:102-114 writes the flag word 0; the C encoder's streams carry 1 << 30 and an exponent, codec.py:127-128)."""
    s = bytearray(O.entropy_encode(np.asarray(dc, np.int32), np.asarray(ac, np.int32), h, w, 50))
    s[:16] = struct.pack("<IIII", h, w, int(quality), flag)
    return bytes(s)


def zz_absolute(dc, ac):
    """[N, 64] int64 zig-zag coefficients with the DC integrated (np.cumsum, codec.py:53; int32 there: equal while it fits)."""
    zz = np.empty((len(dc), 64), np.int64)
    zz[:, 0] = np.cumsum(np.asarray(dc, np.int64))
    zz[:, 1:] = ac
    return zz


def dequantised(fx, O, zz, quality, flag):
    """[N, 8, 8] float64: natural order, codec.py:55-65 (the scaled_dct branch's three roundings in its order), utils.py:50-52."""
    nat = np.zeros(zz.shape, np.float64)
    nat[:, fx.zigzag] = zz
    x = nat.reshape(-1, 8, 8)
    if flag & SCALED:
        x = x / fx.annscales
        x *= 2 ** int(quality)
        quality = 50
    if float(quality) == int(quality):
        div = O.divisors(int(quality))
    else:
        factor = 5000 / quality if quality < 50 else 200 - 2 * quality
        div = fx.qtable * factor / 100
    return x * div


def assemble(blocks, h, w):
    """[N, 8, 8] float64 pixel-domain blocks -> uint8 [h, w]: + 128, clip, truncating cast, crop (codec.py:67-70)."""
    bh, bw = (h + 7) // 8, (w + 7) // 8
    img = blocks.reshape(bh, bw, 8, 8).swapaxes(1, 2).reshape(bh * 8, bw * 8)
    return np.clip(img + 128, 0, 255)[:h, :w].astype(np.uint8)


def pixels_block_idct(fx, O, zz, h, w, quality, flag):
    """The oracle's block_idct route: its divisors and its inverse transform (scipy's operation order), block by block."""
    x = dequantised(fx, O, zz, quality, flag)
    return assemble(np.stack([O.block_idct(b) for b in x]), h, w)


_k = np.arange(8)
CM = np.cos((2 * _k[:, None] + 1) * _k[None, :] * np.pi / 16) * np.where(_k == 0, np.sqrt(1 / 8), np.sqrt(2 / 8))[None, :]  # [x, u]


def idct_matrix(x):
    """[N, 8, 8] -> [N, 8, 8]: the orthonormal inverse DCT as two float64 matrix products - the same function, another operation order."""
    return np.einsum("xu,nuv,yv->nxy", CM, x, CM)


def pixels_matrix(fx, O, zz, h, w, quality, flag):
    return assemble(idct_matrix(dequantised(fx, O, zz, quality, flag)), h, w)


def worst_magnitude(fx, O, zz, quality, flag):
    """max |16 r + 2048| over the pixels r of these blocks: what the fused kernel converts to int without a clamp on its non-scaled branch."""
    return float(np.abs(16.0 * idct_matrix(dequantised(fx, O, zz, quality, flag)) + 2048.0).max())


def clamp_running_dc(dc):
    """The DC differences of the same frame with the running DC saturated to int16 - what a saturating decoder transforms."""
    sat = np.clip(np.cumsum(np.asarray(dc, np.int64)), -32768, 32767)
    return np.diff(sat, prepend=0).astype(np.int64)
