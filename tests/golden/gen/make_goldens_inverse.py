#!/usr/bin/env python3
"""Golden fixtures for the two inverse transforms (idct_kernel; phase 2 of the fused decode kernel): BUILT coefficients - no encoder
made them - decoded by RUNNING THE UNMODIFIED REFERENCE in the build container (same import recipe as make_goldens_r4b.py: stand-ins
on the path, the reference imported, only inputs and the reference's outputs stored).

    python tests/golden/gen/make_goldens_inverse.py     ->  tests/golden/inverse_edges.npz, inverse_edges.json

Per frame: int32 DC differences and AC coefficients (the dictionary of decode(), codec.py:46-70); the stream is the oracle's
entropy_encode of them with the header's quality and flag fields rewritten where needed (tests/inverse_edges.py stream_of) and is not
stored, only its sha256; of the reference's pixels - decompress() of the stream, which must equal decode() of the dictionary - the sha256
and three 64 x 64 crops.  Every frame with a stream has 1,024 .. 4,096 blocks and at least 8,192 payload bits: the device decoder takes it.

Families (ISSUE: adversarial coefficient tests for both inverse transforms):
  sparse    a small DC plus one AC coefficient in -8..8 at each of the 64 scan positions, 64 x 64 blocks, q = 1, 10, 50, 75, 99: pixels
            that sit so close to an integer that the reference's operation order decides the truncating cast; and the q = 50 coefficients
            at quality 37.5 (decode() only: a float cannot be packed into a header)
  ragged    the same construction in a 259 x 517 frame (33 x 65 blocks): partial rows and columns of blocks
  extremes  every |AC| = 1023 with the signs of the basis function of pixel (0,0), (7,7), (3,4), a checkerboard and alternating rows, both
            ways, under a DC that walks between +32767 and -32768 in legal steps; q = 1 and 99 - the largest magnitudes the tables allow
  clip      DC-only and DC + one AC blocks whose pixels land within +-1 of 0 and of 255, q = 10, 50, 90
  dense     63 non-zero AC per block (over 256 stream bits per block: the fused kernel's large window; sparse is the small one)
  scaled    flag 1 << 30, exponents 0, 1, 2, 3, 5, 13, 30, 31, 32, 62: sparse coefficients of both signs, for e <= 3 also |AC| up to 1023
  wide      a running DC that leaves int16: a triangle walk in steps of +-2047 beyond +-60,000, every AC about 300 against the DC's sign;
            the reference integrates in int32 and transforms what it holds.  Four frames with 63 equal AC per block, two ("varied") in which
            every AC has a magnitude of its own in 200 .. 420
The generator asserts and records: pixels of the sparse family that differ from a float64 matrix-form IDCT (>= 1,000), the largest
|16 r + 2048| of the extremes (>= 4.0e8, < 2**31), and per wide frame the pixels that differ when the running DC is saturated (>= 100).
"""
import io
import json
import os
import sys
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLD))
sys.path.insert(0, os.path.join(HERE, "standins"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import tinyimgcodec as ref  # noqa: E402  (the unmodified reference)
from tinyimgcodec.constants import ANNSCALES, LUMINANCE_QUANTIZATION_TABLE, ZIGZAG_ORDER  # noqa: E402

import inverse_edges as IE  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

SCALED = IE.SCALED


class Consts:  # what tests/inverse_edges.py's Fixture gives the restatements
    zigzag = np.asarray(ZIGZAG_ORDER, np.int64)
    annscales = np.asarray(ANNSCALES, np.float64)
    qtable = np.asarray(LUMINANCE_QUANTIZATION_TABLE, np.int64)


def diffs(absolute_dc):
    return np.diff(np.asarray(absolute_dc, np.int64), prepend=0).astype(np.int32)


def sparse_coeffs(rng, n, q):
    """exp: block k has its one AC coefficient at scan position k % 64 (position 0: the DC itself, a small one)."""
    zz = np.zeros((n, 64), np.int64)
    lim = min(int(800 / O.divisors(q)[0, 0]) + 1, 1000)
    zz[:, 0] = rng.integers(-lim, lim + 1, n)
    pos = np.arange(n) % 64
    zz[np.arange(n), pos] = rng.integers(-8, 9, n)
    zz[pos == 0, 0] = rng.integers(-3, 4, int((pos == 0).sum()))
    return zz


def sign_patterns():
    """Eight natural-order sign matrices: the basis function of pixel (0,0), (7,7), (3,4) and its negation handled by the caller, a
    checkerboard, alternating rows, alternating columns, all plus, and the basis function of pixel (4,3)."""
    pats = []
    for (x, y) in ((0, 0), (7, 7), (3, 4), (4, 3)):
        s = np.sign(np.outer(IE.CM[x], IE.CM[y]))
        s[s == 0] = 1
        pats.append(s)
    u, v = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    pats += [np.where((u + v) % 2 == 0, 1.0, -1.0), np.where(u % 2 == 0, 1.0, -1.0), np.where(v % 2 == 0, 1.0, -1.0), np.ones((8, 8))]
    return [p.astype(np.int64) for p in pats]


def dc_walk(n, step, top, bottom, hold):
    """0 -> top in steps of at most `step`, `hold` blocks there, down to bottom, `hold` blocks, up again ..."""
    out, v, target = [], 0, top
    held = 0
    while len(out) < n:
        out.append(v)
        if v == target:
            held += 1
            if held >= hold:
                held, target = 0, (bottom if target == top else top)
        else:
            v = min(v + step, target) if target > v else max(v - step, target)
    return np.asarray(out, np.int64)


def extremes_coeffs(n, amp=1023):
    pats = sign_patterns()
    dcs = dc_walk(n, 2047, 32767, -32768, 40)
    zz = np.zeros((n, 64), np.int64)
    for b in range(n):
        s = 1 if (b // 8) % 2 == 0 else -1
        nat = (s * amp * pats[b % 8]).reshape(64)
        zz[b] = nat[Consts.zigzag]
        zz[b, 0] = dcs[b]
    return zz


def clip_coeffs(rng, n, q):
    d00 = O.divisors(q)[0, 0]
    lo, hi = -128.0 * 8 / d00, 127.0 * 8 / d00  # the DC at which a DC-only block sits on 0 / on 255
    zz = np.zeros((n, 64), np.int64)
    edge = np.where(rng.random(n) < 0.5, lo, hi)
    zz[:, 0] = np.round(edge).astype(np.int64) + rng.integers(-1, 2, n)
    with_ac = rng.random(n) < 0.75
    pos = rng.integers(1, 64, n)
    zz[np.arange(n)[with_ac], pos[with_ac]] = rng.integers(-3, 4, int(with_ac.sum()))
    return zz


def wide_coeffs(n, mag, steps=30, rng=None):
    """rng: every AC gets a magnitude of its own in mag - 100 .. mag + 120 (still against the DC's sign).  63 equal coefficients per block are
    a periodic bit pattern in which the device decoder's speculative walks stay out of step, and it hands such a stream to the host decoder
    for THAT reason; with magnitudes of their own the stream is walked to the end and the running DC is all that is unusual about it."""
    run = np.cumsum(np.resize(np.concatenate([np.full(steps, 2047), np.full(2 * steps, -2047), np.full(steps, 2047)]), n))
    zz = np.zeros((n, 64), np.int64)
    zz[:, 0] = run
    mags = np.full((n, 63), mag) if rng is None else rng.integers(mag - 100, mag + 121, (n, 63))
    zz[:, 1:] = np.where(run > 0, -1, 1)[:, None] * mags
    return zz


def main():
    rng = np.random.default_rng(20251017)
    frames = {}  # name -> (family, h, w, quality, flag, zz absolute)

    def add(name, family, h, w, q, flag, zz):
        assert zz.shape == (O.nblocks(h, w), 64), (name, zz.shape)
        frames[name] = (family, h, w, q, flag, zz)

    # sparse + ragged
    for q in (1, 10, 50, 75, 99):
        add("sparse_q%d" % q, "sparse", 512, 512, q, 0, sparse_coeffs(rng, 4096, q))
    add("sparse_q37_5", "sparse", 512, 512, 37.5, 0, frames["sparse_q50"][5])
    for q in (50, 99):
        add("ragged_q%d" % q, "ragged", 259, 517, q, 0, sparse_coeffs(rng, 33 * 65, q))
    # extremes
    for q in (1, 99):
        add("extremes_q%d" % q, "extremes", 256, 256, q, 0, extremes_coeffs(1024))
    # clip edges
    for q in (10, 50, 90):
        add("clip_q%d" % q, "clip", 256, 512, q, 0, clip_coeffs(rng, 2048, q))
    # dense
    zz = rng.integers(-40, 41, (1024, 64))
    zz[zz == 0] = 1
    zz[:, 0] = np.cumsum(rng.integers(-300, 301, 1024))
    add("dense_q50", "dense", 256, 256, 50, 0, zz)
    # scaled
    for e in (0, 1, 2, 3, 5, 13, 30, 31, 32, 62):
        n = 2048
        zz = np.zeros((n, 64), np.int64)
        zz[:, 0] = rng.integers(-3, 4, n)
        pos = rng.integers(1, 64, n)
        if e <= 3:
            zz[np.arange(n), pos] = rng.integers(-1023, 1024, n)
            zz[:, 1:] = np.where(rng.random((n, 63)) < 0.1, rng.integers(-40, 41, (n, 63)), zz[:, 1:])
            zz[:, 0] = np.cumsum(rng.integers(-40, 41, n))
        else:
            zz[np.arange(n), pos] = rng.integers(-2, 3, n)
        add("scaled_e%d" % e, "scaled", 256, 512, e, SCALED, zz)
    add("scaled_dense_e1", "scaled", 256, 256, 1, SCALED, extremes_coeffs(1024, amp=1023))
    # wide DC
    for q in (10, 50, 99):
        add("wide_q%d" % q, "wide", 256, 256, q, 0, wide_coeffs(1024, 300))
    add("wide_scaled_e0", "wide", 256, 256, 0, SCALED, wide_coeffs(1024, 300))
    add("wide_varied_q50", "wide", 256, 256, 50, 0, wide_coeffs(1024, 300, rng=rng))
    add("wide_varied_scaled_e0", "wide", 256, 256, 0, SCALED, wide_coeffs(1024, 300, rng=rng))

    arrays = {"zigzag": Consts.zigzag, "annscales": Consts.annscales, "qtable": Consts.qtable}
    meta = {"frames": {}}
    order_sensitive = 0
    worst = 0.0
    for name, (family, h, w, q, flag, zz) in frames.items():
        dc, ac = diffs(zz[:, 0]), zz[:, 1:].astype(np.int32)
        assert np.abs(dc).max() <= 2047 and np.abs(ac).max() <= 1023, name
        as_dict = {"height": h, "width": w, "quality": q, "scaled_dct": bool(flag & SCALED), "dc": dc, "ac": ac}
        want = ref.decode(as_dict)
        stream = None
        if float(q) == int(q):
            stream = IE.stream_of(O, dc, ac, h, w, q, flag)
            n = O.nblocks(h, w)
            assert 1024 <= n <= 4096 and (len(stream) - 16) * 8 >= 8192, (name, n, len(stream))
            got = ref.decompress(stream)
            assert np.array_equal(got, want), name  # decompress() of the stream is decode() of the dictionary
            assert np.array_equal(O.decompress(stream), want), name
        assert np.array_equal(IE.pixels_block_idct(Consts, O, zz, h, w, q, flag), want), name
        e = {"family": family, "height": h, "width": w, "quality": q, "flag": flag, "blocks": int(zz.shape[0]),
             "stream_bytes": len(stream) if stream else None, "stream_sha256": IE.sha(stream) if stream else None,
             "pixels_sha256": IE.px_sha(want), "unclipped_pixels": int(((want > 0) & (want < 255)).sum())}
        if family in ("sparse", "ragged"):
            e["order_sensitive_pixels"] = int((want != IE.pixels_matrix(Consts, O, zz, h, w, q, flag)).sum())
            if family == "sparse":
                order_sensitive += e["order_sensitive_pixels"]
        if family == "extremes":
            e["worst_magnitude"] = IE.worst_magnitude(Consts, O, zz, q, flag)
            worst = max(worst, e["worst_magnitude"])
        if family == "clip":
            r = IE.idct_matrix(IE.dequantised(Consts, O, zz, q, flag)) + 128.0
            e["pixels_within_1_of_0"], e["pixels_within_1_of_255"] = int((np.abs(r) <= 1.0).sum()), int((np.abs(r - 255.0) <= 1.0).sum())
            assert min(e["pixels_within_1_of_0"], e["pixels_within_1_of_255"]) >= 200, (name, e)  # (coarse divisors at q = 10: steps of 10 grey levels)
        if family == "wide":
            run = zz[:, 0]
            assert run.max() > 60000 and run.min() < -60000 and (np.diff(np.sign(run)) != 0).any(), name
            sat = zz.copy()
            sat[:, 0] = np.clip(run, -32768, 32767)
            alt = ref.decode(dict(as_dict, dc=diffs(sat[:, 0])))
            e["pixels_a_saturating_decoder_gets_wrong"] = int((alt != want).sum())
            assert e["pixels_a_saturating_decoder_gets_wrong"] >= 100, (name, e)
        meta["frames"][name] = e
        arrays["dc_" + name] = dc
        arrays["ac_" + name] = ac
        arrays["crop_" + name] = IE.crops_of(want)
        print(name, {k: v for k, v in e.items() if k not in ("stream_sha256", "pixels_sha256")})
    assert order_sensitive >= 1000, order_sensitive
    assert 4.0e8 <= worst < 2.0 ** 31, worst
    meta["sparse_order_sensitive_pixels"] = order_sensitive
    meta["extremes_worst_magnitude"] = worst
    print("sparse family: %d pixels differ from the float64 matrix-form IDCT; extremes: largest |16 r + 2048| = %.6g (2**31 = %.6g)"
          % (order_sensitive, worst, 2.0 ** 31))

    # a zip written by hand: np.savez stamps every member with the current time, and the fixture must come out byte for byte
    with zipfile.ZipFile(os.path.join(GOLD, "inverse_edges.npz"), "w") as z:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, b.getvalue(), compresslevel=9)
    with open(os.path.join(GOLD, "inverse_edges.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote inverse_edges.npz (%d bytes), inverse_edges.json" % os.path.getsize(os.path.join(GOLD, "inverse_edges.npz")))


if __name__ == "__main__":
    main()
