"""Shared by tests/test_wide_blocks_cpu.py, tests/test_wide_blocks_gpu.py and tests/golden/gen/make_goldens_wide_blocks.py: the corpus of
integer frames with values outside 0..255 that pins encode() / compress() of such images (dctq_exact_wide_kernel, tic_encode_wide, the
routing of tinyimgcodec_amd/codec.py) on the unmodified reference; the loader of tests/golden/wide_blocks.npz / .json; a plain numpy
model of the transform whose switches are the mutants the corpus has to tell from the reference; and the helper that words a first
difference.  No test lives here, and nothing here needs the reference: the generator alone runs it.

build_frames() is deterministic: every random draw comes from np.random.default_rng([SEED, tag...]), no global state.  The fixture holds
the sha256 of every frame's pixels, not the pixels: the builder rebuilds them.

Families.  A tile of the kernel is eight blocks of one block row (one wave), a workgroup four tiles:
  geometry   int16-range noise at the shapes where the tile walk can go wrong (GEOMETRY_SHAPES says what each reaches), at 10, 50, 90;
  reflect    every (h, w) with h, w in 1..7, and (9, 15), (15, 9), (17, 23); every pixel a distinct value of magnitude above 1,000, so a
             wrong source index is a wrong coefficient (np.pad(..., "reflect") bounces several times on an axis shorter than 5);
  magnitude  40 x 72 noise of amplitude 2^k, k = 9, 12, 16, 20, 24, 28, 31: over [-2^k, 2^k), over [0, 2^k) and over [-2^k, 0), at
             quality 10, where every rounded quotient fits int32;
  extremes   flat, two-level and checkerboard blocks of INT32_MIN, INT32_MIN + 127 (the last pixel whose `- 128` wraps in int32),
             INT32_MIN + 128 (the first that does not) and INT32_MAX at quality 10; INT32_MAX beside INT32_MIN + 128 at quality 75,
             where the DC difference wraps;
  ties       four frames of 512 blocks (64 x 512) whose quotient at (0,0), (0,4), (4,0), (4,4) is exactly k + 1/2 at quality 50: flat
             blocks of 128 + odd for the DC, two-level blocks with one pixel adjusted, in exact integer arithmetic, for the others.  The
             reference's rounding there is decided by the last-ulp error of its FFT, not by half-even of the exact quotient;
  floatq     one geometry frame and one magnitude frame at the qualities 1.5, 33.3, 71.9, 98.5;
  streams    frames whose coefficients compress() can code, or just cannot: 12-bit noise with its deviations divided by 4, a ramp of flat
             block rows whose running DC reaches 46,000 in differences of 2,000, the ramp up and down again, a DC difference of exactly
             +-2,047 and of +-2,048, an AC value of exactly +-1,023 and of +-1,024 (2,048 and 1,024 have no Huffman code);
  routing    what encode() of the package has to tell apart before it picks a kernel: 13 x 21 noise that an int8 array can hold and noise
             that a uint16 array can hold, and an 11 x 19 frame of 0..255 whose LAST pixel alone is 256, -1 (wide) or 255, 0 (8-bit).
"""
import collections
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 20261021
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
FAMILIES = ("geometry", "reflect", "magnitude", "extremes", "ties", "floatq", "streams", "routing")

QTABLE = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
                  np.int64).reshape(8, 8)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# (h, w): what the shape reaches in the kernel's tile walk
GEOMETRY_SHAPES = collections.OrderedDict([
    ((1, 1), "the smallest frame"), ((2, 3), "one ragged block"), ((7, 9), "two blocks, both ragged"), ((8, 8), "one whole block"),
    ((3, 70), "9 blocks, tiles_x = 2, a last tile of one block"),
    ((9, 65), "two block rows of 9 blocks"),
    ((8, 264), "33 blocks in one row: five tiles, a second workgroup"),
    ((264, 8), "33 tiles of one block: nine workgroups, the last with one wave at work"),
    ((72, 136), "tiles_x = 3, 27 tiles: the last workgroup has a wave without a tile, which still takes part in both LDS transposes"),
    ((40, 200), "tiles_x = 4, a last tile of one block in every row, 5 workgroups"),
])
GEOMETRY_QUALITIES = (10, 50, 90)
REFLECT_SHAPES = [(h, w) for h in range(1, 8) for w in range(1, 8)] + [(9, 15), (15, 9), (17, 23)]
MAGNITUDE_K = (9, 12, 16, 20, 24, 28, 31)
MAGNITUDE_RANGES = ("sym", "pos", "neg")
EXTREME_VALUES = collections.OrderedDict([("min", I32_MIN), ("min127", I32_MIN + 127), ("min128", I32_MIN + 128), ("max", I32_MAX)])
TIE_POSITIONS = ((0, 0), (0, 4), (4, 0), (4, 4))
TIE_SHAPE = (64, 512)
FLOAT_QUALITIES = (1.5, 33.3, 71.9, 98.5)
PAIR_FRAME = "ext_pair_max_min128_q75"

Frame = collections.namedtuple("Frame", "name family img quality")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _rng(*tag):
    return np.random.default_rng([SEED] + [int(t) for t in tag])


def qtag(q):
    return ("q%g" % q).replace(".", "p")


# ---- the builder --------------------------------------------------------------------------------------------------------------------

def geometry_image(h, w):
    return _rng(1, h, w).integers(-32768, 32768, (h, w)).astype(np.int32)


def reflect_image(h, w):
    """Distinct magnitudes 1,001 + 97 j in a seeded order, seeded signs."""
    r = _rng(2, h, w)
    mags = 1001 + 97 * r.permutation(h * w)
    return (mags * r.choice((-1, 1), h * w)).reshape(h, w).astype(np.int32)


def magnitude_image(k, kind):
    lo, hi = {"sym": (-2 ** k, 2 ** k), "pos": (0, 2 ** k), "neg": (-2 ** k, 0)}[kind]
    return _rng(3, k, MAGNITUDE_RANGES.index(kind)).integers(lo, hi, (40, 72)).astype(np.int32)


def _two_blocks(a, b):
    """8 x 16: a | b split left / right in the first block, top / bottom in the second."""
    img = np.empty((8, 16), np.int64)
    img[:, :4], img[:, 4:8] = a, b
    img[:4, 8:], img[4:, 8:] = a, b
    return img.astype(np.int32)


def _checker(a, b):
    r, c = np.indices((8, 16))
    return np.where((r + c) & 1, a, b).astype(np.int32)


def extremes_frames():
    out = []
    V = EXTREME_VALUES
    for n, v in V.items():
        out.append(Frame("ext_flat_%s_q10" % n, "extremes", np.full((8, 16), v, np.int32), 10))
    for a, b in (("min", "min127"), ("min127", "min128"), ("min", "max"), ("min128", "max")):
        out.append(Frame("ext_two_%s_%s_q10" % (a, b), "extremes", _two_blocks(V[a], V[b]), 10))
    for a, b in (("max", "min128"), ("max", "min"), ("min127", "min128")):
        out.append(Frame("ext_checker_%s_%s_q10" % (a, b), "extremes", _checker(V[a], V[b]), 10))
    pair = np.empty((8, 16), np.int32)
    pair[:, :8], pair[:, 8:] = I32_MAX, I32_MIN + 128
    out.append(Frame(PAIR_FRAME, "extremes", pair, 75))
    return out


def tie_odds():
    """The 512 odd numbers of the DC tie frame: pixel = 128 + odd, exact DC quotient at quality 50 = 8 odd / 8 / 16 = odd / 2."""
    return 2 * _rng(5, 0, 0).integers(-500_000_000, 500_000_000, 512) + 1


def tie_image(u, v):
    """64 x 512, block b = 64 by + bx.  (0, 0): flat 128 + odd.  The others: X(u, v) = N / 8 with N = sum(x W), W the +-1 pattern of the
    basis function; a two-level block (a where W > 0, b elsewhere: N = 32 (a - b)), then one pixel moved so that N = 4 div (2 k + 1)."""
    nb = 512
    if (u, v) == (0, 0):
        blocks = np.repeat((128 + tie_odds())[:, None], 64, 1).reshape(nb, 8, 8)
    else:
        s4 = np.array([1, -1, -1, 1, 1, -1, -1, 1])
        W = np.outer(np.ones(8, np.int64) if u == 0 else s4, np.ones(8, np.int64) if v == 0 else s4)
        div = int(QTABLE[u, v])  # quality 50: the divisor is the table entry
        r = _rng(5, u, v)
        blocks = np.empty((nb, 8, 8), np.int64)
        for i in range(nb):
            a, b = (int(x) for x in r.integers(-250_000_000, 250_000_000, 2))
            blk = np.where(W > 0, a, b).astype(np.int64)
            need = (4 * div - int((blk * W).sum())) % (8 * div)
            y, x = (int(t) for t in r.integers(0, 8, 2))
            blk[y, x] += need * W[y, x]
            assert int((blk * W).sum()) % (8 * div) == 4 * div
            blocks[i] = blk + 128
    bh, bw = TIE_SHAPE[0] // 8, TIE_SHAPE[1] // 8
    return blocks.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(TIE_SHAPE).astype(np.int32)


def tie_exact_twice(u, v, img):
    """int64 [512]: twice the exact quotient at (u, v) at quality 50 (an odd number for every block: the tie)."""
    s4 = np.array([1, -1, -1, 1, 1, -1, -1, 1])
    W = np.outer(np.ones(8, np.int64) if u == 0 else s4, np.ones(8, np.int64) if v == 0 else s4)
    n = (to_blocks(img.astype(np.int64) - 128) * W).sum((1, 2))
    div = int(QTABLE[u, v])
    assert (n % (4 * div) == 0).all()
    return n // (4 * div)


def _flat_rows(levels):
    """len(levels) * 8 x 8: one flat block per level, stacked."""
    return np.repeat(np.asarray(levels, np.int64), 8)[:, None].repeat(8, 1).astype(np.int32)


def _flat_cols(levels):
    return np.ascontiguousarray(_flat_rows(levels).T)


def _ac04(amp):
    """8 x 16: a pure (0, 4) pattern of +-amp about 128 and its negative: X(0, 4) = 8 amp, at quality 50 (divisor 24) amp / 3."""
    s4 = np.array([1, -1, -1, 1, 1, -1, -1, 1])
    row = np.concatenate([128 + amp * s4, 128 - amp * s4])
    return np.repeat(row[None], 8, 0).astype(np.int32)


def streams_frames():
    n = _rng(7, 12).integers(0, 4096, (24, 40))
    ramp = [128 + 4000 * k for k in range(24)]
    updown = [128 + 4000 * k for k in list(range(12)) + list(range(11, -1, -1))]
    return [
        Frame("str_12bit_q50", "streams", (2048 + (n - 2048) // 4).astype(np.int32), 50),
        Frame("str_ramp_q50", "streams", _flat_rows(ramp), 50),              # DC 2,000 k: differences of 2,000, running DC 46,000
        Frame("str_ramp_updown_q50", "streams", _flat_rows(updown), 50),
        Frame("str_dc2047_q50", "streams", _flat_cols([128, 128 + 4094, 128]), 50),  # DC = (v - 128) / 2: differences 0, +2,047, -2,047
        Frame("str_dc2048_q50", "streams", _flat_cols([128, 128 + 4096, 128]), 50),  # +-2,048: no code
        Frame("str_ac1023_q50", "streams", _ac04(3069), 50),                 # (0, 4) = +-1,023
        Frame("str_ac1024_q50", "streams", _ac04(3072), 50),                 # +-1,024: no code
    ]


def routing_frames():
    base = _rng(8, 0).integers(0, 256, (11, 19))
    out = [Frame("rt_int8_q50", "routing", _rng(8, 1).integers(-128, 128, (13, 21)).astype(np.int32), 50),
           Frame("rt_uint16_q50", "routing", _rng(8, 2).integers(0, 65536, (13, 21)).astype(np.int32), 50)]
    for tag, last in (("256", 256), ("m1", -1), ("255", 255), ("0", 0)):
        img = base.copy()
        img[-1, -1] = last
        out.append(Frame("rt_last_%s_q50" % tag, "routing", img.astype(np.int32), 50))
    return out


FLOATQ_SOURCES = (("geo_9x65", lambda: geometry_image(9, 65)), ("mag_k16_sym", lambda: magnitude_image(16, "sym")))
# The generator stores the reference's decode() of its own dictionary for these two: the magnitude frames whose coefficients still fit the
# int16 layout decode() of the package works in (from k = 20 on it raises its ValueError).
DECODE_FRAMES = ("mag_k12_sym_q10", "mag_k16_pos_q10")


def build_frames():
    """-> [Frame(name, family, int32 [h, w], quality)], in a fixed order."""
    out = []
    for (h, w) in GEOMETRY_SHAPES:
        img = geometry_image(h, w)
        out += [Frame("geo_%dx%d_q%d" % (h, w, q), "geometry", img, q) for q in GEOMETRY_QUALITIES]
    out += [Frame("ref_%dx%d_q50" % (h, w), "reflect", reflect_image(h, w), 50) for (h, w) in REFLECT_SHAPES]
    out += [Frame("mag_k%d_%s_q10" % (k, kind), "magnitude", magnitude_image(k, kind), 10) for k in MAGNITUDE_K for kind in MAGNITUDE_RANGES]
    out += extremes_frames()
    out += [Frame("tie_%d%d_q50" % (u, v), "ties", tie_image(u, v), 50) for (u, v) in TIE_POSITIONS]
    for tag, make in FLOATQ_SOURCES:
        img = make()
        out += [Frame("fq_%s_%s" % (tag, qtag(q)), "floatq", img, q) for q in FLOAT_QUALITIES]
    out += streams_frames()
    out += routing_frames()
    assert len({f.name for f in out}) == len(out)
    return out


_frames = None


def frames():
    """build_frames(), built once per process; name -> Frame in the builder's order.  The arrays are shared: do not write to them."""
    global _frames
    if _frames is None:
        _frames = collections.OrderedDict((f.name, f) for f in build_frames())
        for f in _frames.values():
            f.img.setflags(write=False)
    return _frames


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------

class Fixture:
    """wide_blocks.npz / .json.  meta["frames"]: name -> {family, h, w, quality, sha256, and for the streams family "stream": "bytes" or the
    exception's name}; arrays <name>_dc int32 [N], <name>_ac int32 [N, 63], <name>_bs / <name>_dec (streams), <name>_pix (DECODE_FRAMES)."""

    def __init__(self, golden_dir=GOLDEN):
        self.npz = np.load(os.path.join(golden_dir, "wide_blocks.npz"))
        with open(os.path.join(golden_dir, "wide_blocks.json")) as f:
            self.meta = json.load(f)
        self.entries = self.meta["frames"]
        self.census = self.meta["census"]

    def names(self, family=None):
        return [n for n, e in self.entries.items() if family is None or e["family"] == family]

    def quality(self, name):
        return self.entries[name]["quality"]

    def dc(self, name):
        return self.npz[name + "_dc"]

    def ac(self, name):
        return np.ascontiguousarray(self.npz[name + "_ac"])

    def stream(self, name):
        """bytes, or the name of the exception the reference's compress() raised."""
        e = self.entries[name]["stream"]
        return self.npz[name + "_bs"].tobytes() if e == "bytes" else e

    def decompressed(self, name):
        return self.npz[name + "_dec"]

    def decoded(self, name):
        return self.npz[name + "_pix"]


# ---- words for a difference ---------------------------------------------------------------------------------------------------------

def differing_blocks(got_dc, got_ac, want_dc, want_ac):
    """Indices of the blocks in which the DC difference or any AC value differs."""
    got_dc, got_ac, want_dc, want_ac = (np.asarray(a).astype(np.int64) for a in (got_dc, got_ac, want_dc, want_ac))
    if got_dc.shape != want_dc.shape or got_ac.shape != want_ac.shape:
        return np.arange(max(len(got_dc), len(want_dc)))
    return np.flatnonzero((got_dc != want_dc) | (got_ac != want_ac).any(1))


def first_difference(got_dc, got_ac, want_dc, want_ac):
    """None where both pairs are equal, else "block b, scan position k: got x, want y" for the first place (k = 0: the DC difference),
    and how many blocks differ."""
    got_dc, got_ac, want_dc, want_ac = (np.asarray(a) for a in (got_dc, got_ac, want_dc, want_ac))
    if got_dc.shape != want_dc.shape or got_ac.shape != want_ac.shape:
        return "shapes differ: got dc %r ac %r, want dc %r ac %r" % (got_dc.shape, got_ac.shape, want_dc.shape, want_ac.shape)
    bad = differing_blocks(got_dc, got_ac, want_dc, want_ac)
    if bad.size == 0:
        return None
    b = int(bad[0])
    got = np.concatenate([got_dc[b: b + 1], got_ac[b]]).astype(np.int64)
    want = np.concatenate([want_dc[b: b + 1], want_ac[b]]).astype(np.int64)
    k = int(np.flatnonzero(got != want)[0])
    return "block %d, scan position %d: got %d, want %d (%d of %d blocks differ)" % (b, k, got[k], want[k], bad.size, len(want_dc))


# ---- the model and its mutants -----------------------------------------------------------------------------------------------------

def to_blocks(x):
    """[8 bh, 8 bw] -> [bh * bw, 8, 8] in raster order."""
    h, w = x.shape
    return x.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)


def reflect_map(n, padded, single=False):
    """Source index of every position 0..padded-1 of an axis of n samples: np.pad(..., "reflect"), which bounces as often as it takes;
    single (a mutant): one reflection about the last sample, and sample 0 for whatever that leaves in front of the axis."""
    i = np.arange(padded)
    if single:
        return np.where(i < n, i, np.maximum(2 * (n - 1) - i, 0))
    if n == 1:
        return np.zeros(padded, np.int64)
    j = i % (2 * (n - 1))
    return np.where(j < n, j, 2 * (n - 1) - j)


def divisors(quality):
    """float64 [8, 8]: table * factor / 100 evaluated left to right, factor = 5000 / q below 50, 200 - 2 q from 50."""
    factor = 5000 / quality if quality < 50 else 200 - 2 * quality
    return QTABLE * factor / 100


# The 8-point DCT-II as the JPEG standard writes it: X(k) = 1/2 C(k) sum x(n) cos((2 n + 1) k pi / 16), C(0) = 1 / sqrt 2, C(k) = 1.
# (How such a product rounds an exact tie hangs on the last bit of its constants and on the order of its sums: with this spelling it
# differs from the reference on 443 of the 512 flat tie blocks; with np.sqrt(0.125) for row 0 - one ulp more - on 62, and summed by
# np.einsum on none.  That is the point of the ties family: only the reference's own operation order reproduces it everywhere.)
DCT_MATRIX = np.array([[0.5 * (1 / np.sqrt(2) if k == 0 else 1.0) * np.cos((2 * n + 1) * k * np.pi / 16) for n in range(8)] for k in range(8)])


def model(img, quality, dct8, float_sub=False, single_bounce=False, matrix_dct=False, wide_diff=False, tiles_x_one=False):
    """-> (dc int64 [N], ac int64 [N, 63]): encode() of an integer image in plain numpy, with dct8 (a float64 vector of 8 -> its 8-point
    transform in the reference's operation order: pyoracle.dct8) down the columns, then along the rows.  The switches are the mutants:
      float_sub      `- 128` in float64 instead of wrapping int32;
      single_bounce  one reflection at the frame's edge;
      matrix_dct     D @ X @ D.T instead of dct8 (np.round after it, as always);
      wide_diff      the DC difference without the int32 wrap;
      tiles_x_one    the kernel's tile walk with tiles_x taken as 1: tile t is block row t, blocks 0..7; every block it does not reach keeps
                     the zeros the output held (rows beyond the frame, which such a kernel would also touch, are left out)."""
    img = np.asarray(img)
    h, w = img.shape
    ph, pw = -(-h // 8) * 8, -(-w // 8) * 8
    src = img.astype(np.int32)[np.ix_(reflect_map(h, ph, single_bounce), reflect_map(w, pw, single_bounce))]
    if float_sub:
        x = src.astype(np.float64) - 128.0
    else:
        x = ((src.astype(np.int64) - 128 + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.float64)
    blocks = to_blocks(x)
    if matrix_dct:
        X = DCT_MATRIX @ blocks @ DCT_MATRIX.T
    else:
        X = np.empty_like(blocks)
        for b, blk in enumerate(blocks):
            cols = np.stack([dct8(blk[:, c]) for c in range(8)], axis=1)   # axis -2
            X[b] = np.stack([dct8(cols[r]) for r in range(8)], axis=0)      # axis -1
    q = np.round(X / divisors(quality)).astype(np.int64).reshape(-1, 64)[:, ZIGZAG]
    if tiles_x_one:
        bh, bw = ph // 8, pw // 8
        reached = np.zeros((bh, bw), bool)
        reached[:, :8] = True
        q = np.where(reached.reshape(-1, 1), q, 0)
    dc = q[:, 0].copy()
    d = np.diff(dc)
    dc[1:] = d if wide_diff else (d + 2 ** 31) % 2 ** 32 - 2 ** 31
    return dc, q[:, 1:]
