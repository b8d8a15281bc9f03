"""Shared by tests/test_requantize_cpu.py, tests/test_requantize_gpu.py and tests/golden/gen/make_goldens_requantize.py: the BUILT coefficient
corpus of requantisation, the pairs of qualities it is run at, the small images whose streams are requantised, a plain numpy model of the
stage with two mutants, and the fixture tests/golden/requantize.json with what the unmodified reference computes.  No test lives here.

The stage is block_quantize(block_quantize(c, q1, inverse=True), q2) of the reference (utils.py:48-53): in float64 and in this order
x = c * ((T * f1) / 100), t = x / ((T * f2) / 100), np.round(t).  T cancels in exact arithmetic, not in float64: `rational` is the mutant that
lets it cancel, `away` the one that rounds halves away from zero.

Corpus (int16 [n, 64], zig-zag order, absolute DC in column 0 - the device layout): 2,047 Latin-square blocks - block b holds
((b + 31 p) mod 2047) - 1023 at position p, so every value -1023..1023 stands at every one of the 64 positions exactly once - and 4 blocks
with the int16 extremes: DC 32767, -32767 and -32768 (int16 has no +32768), and one with +32767 and -32768 among its AC values.  The Latin
part alone (2,047 blocks: not a multiple of the 8 blocks a wave takes at a time) is what the overflow counts of the issue speak about; the
extremes overflow at every pair that scales up.
"""
import hashlib
import json
import os

import numpy as np

import wide_blocks as WB

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "requantize.json")
N_LATIN, N_CORPUS = 2047, 2051
Q_FROM = (1, 3, 25, 50, 99)
STREAM_Q_FROM = (10, 50, 90)
STREAM_Q_TO = (5, 25, 50, 75, 95)
SIZE_TABLES = (("bench0_64x64", 90), ("bench2_40x72", 50))  # (image, source quality): len(requantize(s, q)) for q = 1..99
ZIGZAG = WB.ZIGZAG


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def digest(values):
    """sha256 of the values as little-endian int32 (a result outside int16 has a digest too)."""
    return sha(np.ascontiguousarray(values, dtype="<i4").tobytes())


def pairs():
    """(q1, q2): every q2 = 1..99 from each q1 of Q_FROM, and (q, q) for every q."""
    out = [(q1, q2) for q1 in Q_FROM for q2 in range(1, 100)]
    return out + [(q, q) for q in range(1, 100) if q not in Q_FROM]


def corpus():
    b = np.arange(N_LATIN, dtype=np.int64)[:, None]
    p = np.arange(64, dtype=np.int64)[None, :]
    zz = np.zeros((N_CORPUS, 64), np.int16)
    zz[:N_LATIN] = ((b + 31 * p) % N_LATIN) - 1023
    zz[N_LATIN, 0], zz[N_LATIN + 1, 0], zz[N_LATIN + 2, 0] = 32767, -32767, -32768
    zz[N_LATIN + 3, 1], zz[N_LATIN + 3, 63], zz[N_LATIN + 3, 0] = 32767, -32768, 5
    return zz


def check_corpus(zz):
    lat = zz[:N_LATIN].astype(np.int64)
    for p in range(64):
        assert np.array_equal(np.sort(lat[:, p]), np.arange(-1023, 1024)), p
    assert zz.min() == -32768 and zz.max() == 32767 and zz.shape == (N_CORPUS, 64)


def zz_divisors(q):
    """float64 [64] in zig-zag order: the reference's quantization_table * factor / 100."""
    return WB.divisors(q).reshape(64)[ZIGZAG]


def model(zz, q1, q2, rounding="even"):
    """The stage in plain numpy -> int64 [n, 64].  rounding="away": the mutant that rounds halves away from zero."""
    x = np.asarray(zz).astype(np.float64) * zz_divisors(q1)
    t = x / zz_divisors(q2)
    if rounding == "even":
        return np.round(t).astype(np.int64)
    assert rounding == "away"
    return (np.sign(t) * np.floor(np.abs(t) + 0.5)).astype(np.int64)


def _ratio(q1, q2):
    """f1 / f2 as a pair of integers (a, b), b > 0: factor = 5000 / q below 50, 200 - 2 q from 50; the table value has cancelled."""
    from fractions import Fraction

    f = [Fraction(5000, q) if q < 50 else Fraction(200 - 2 * q) for q in (q1, q2)]
    r = f[0] / f[1]
    return r.numerator, r.denominator


def model_rational(zz, q1, q2):
    """The mutant that computes c * f1 / f2 exactly and rounds half to even -> (int64 [n, 64], bool [n, 64] exact ties)."""
    a, b = _ratio(q1, q2)
    num = np.asarray(zz).astype(np.int64) * a
    fl, rem = np.divmod(num, b)
    tie = 2 * rem == b
    up = (2 * rem > b) | (tie & (fl % 2 != 0))
    return fl + up, tie


def outside_int16(r):
    return int(np.count_nonzero((r < -32768) | (r > 32767)))


def images():
    """name -> uint8 image: four crops of the benchmark set, the smallest frame and a ragged one."""
    px = np.load(os.path.join(GOLDEN, "benchmark_set.npz"))["pixels"]
    rng = np.random.default_rng(20261021)
    return {
        "bench0_64x64": np.ascontiguousarray(px[0, 200:264, 200:264]),
        "bench1_64x64": np.ascontiguousarray(px[1, 100:164, 300:364]),
        "bench2_40x72": np.ascontiguousarray(px[2, 250:290, 100:172]),
        "bench3_72x40": np.ascontiguousarray(px[3, 50:122, 400:440]),
        "one_1x1": np.full((1, 1), 201, np.uint8),
        "noise_15x17": rng.integers(0, 256, (15, 17), dtype=np.uint8),
    }


def requantized_info(zz, hdr, q2):
    """The dictionary the reference's writer gets: the reader's coefficients (zz16 rows) through `model`, DPCM'd again."""
    r = model(zz, hdr["quality"], q2)
    dc = r[:, 0].copy()
    dc[1:] = np.diff(r[:, 0])
    return {"height": hdr["height"], "width": hdr["width"], "quality": q2, "dc": dc, "ac": r[:, 1:]}


def bisect(sizes, budget, qmin, qmax):
    """compress_to_size()'s bisection over a table sizes[q] (-1: no stream) -> the quality it ends at, or None when qmin does not fit."""
    fits = lambda q: 0 <= sizes[q] <= budget  # noqa: E731
    if not fits(qmin):
        return None
    lo, hi = qmin, qmax
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if fits(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


_fixture = None


def load_fixture():
    global _fixture
    if _fixture is None:
        with open(FIXTURE) as f:
            _fixture = json.load(f)
    return _fixture
