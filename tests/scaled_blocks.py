"""Shared by tests/test_scaled_blocks_cpu.py, tests/test_scaled_blocks_gpu.py and tests/golden/gen/make_goldens_scaled_blocks.py: the
fixture tests/golden/scaled_blocks.npz / .json (built 8 x 8 pixel blocks at the edges of the integer encoder's arithmetic, and what the
unmodified reference makes of them), a plain numpy restatement of tinyimgcodec_amd/csrc/tic_scaled_math.h, the mutants of that restatement
the corpus has to tell from the reference, and the deterministic search that builds the corpus.  No test lives here, and nothing here needs
the reference: the generator alone runs it.

The model works on int64 arrays and wraps to int16 where the C code stores an int16; it is licensed by the fixture (model == reference for
every reference-pinned block and setting), never the other way round.

Families (every block is 8 x 8 uint8):
  peak     per (u, v) and polarity the block that maximises |d(u, v)| in front of the quantiser: the basis function's sign pattern, then
           single-pixel flips while one of them gains;
  line1023 (1, 1) at `best` exactly +1023, -1023, +1024, -1024 (1023 is the last coefficient with a Huffman code), and the blocks that
           reach the `best` maxima of (0, 1), (0, 2), (1, 0), (1, 2) in both signs;
  word     per word of the quantiser table (4 settings x 64 positions) and single-word mutant (reciprocal +-1, half-divisor +-1) a block
           whose d at that position is a value at which the mutant quantises differently; signs alternate;
  dcswing  flat 0 and flat 255 side by side: the largest DC difference 8-bit pixels can give.
Frames are 72 pixels wide (9 blocks: every second strip of 8 holds one block), 8 block rows at most; the last frame of a family holds the
remainder, filled up to whole block rows with flat 128.
"""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETTINGS = ("best", "high", "med", "low")
FRAME_W = 72
FRAME_ROWS = 8  # block rows of a full frame
FILL = 128      # the filler blocks' pixel value

QTABLE = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
                  np.int64).reshape(8, 8)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
# the multipliers of one 8-point pass (181 stands twice: z1 of the even part, z3 of the odd part) and its four arithmetic shifts
CONSTS = {"z1_181": 181, "z3_181": 181, "z5_98": 98, "z2_139": 139, "z4_334": 334}
SHIFTS = ("z1", "z2", "z4", "z3")
WORD_KINDS = ("recip+1", "recip-1", "half+1", "half-1")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the model ----------------------------------------------------------------------------------------------------------------------

def i16(x):
    """What storing x in an int16 keeps."""
    return ((np.asarray(x, np.int64) + 32768) & 0xFFFF) - 32768


def _shr8(x, trunc):
    return np.where(x < 0, -((-x) >> 8), x >> 8) if trunc else x >> 8


def fdct8(s, consts=None, trunc=()):
    """One 8-point pass along the last axis (fdct8_scaled).  consts: changed multipliers by CONSTS' names; trunc: names of SHIFTS whose
    >> 8 becomes a division that truncates toward zero (mutants only)."""
    k = dict(CONSTS, **(consts or {}))
    s = np.asarray(s, np.int64)
    s0, s1, s2, s3, s4, s5, s6, s7 = (s[..., j] for j in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = s0 + s7, s0 - s7, s1 + s6, s1 - s6, s2 + s5, s2 - s5, s3 + s4, s3 - s4
    e10, e13, e11, e12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    z1 = _shr8((e12 + e13) * k["z1_181"], "z1" in trunc)
    o10, o11, o12 = t4 + t5, t5 + t6, t6 + t7
    z5 = (o10 - o12) * k["z5_98"]
    z2 = _shr8(z5 + o10 * k["z2_139"], "z2" in trunc)
    z4 = _shr8(z5 + o12 * k["z4_334"], "z4" in trunc)
    z3 = _shr8(o11 * k["z3_181"], "z3" in trunc)
    z11, z13 = t7 + z3, t7 - z3
    return np.stack([e10 + e11, z11 + z4, e13 + z1, z13 - z2, e10 - e11, z13 + z2, e13 - z1, z11 - z4], axis=-1)


def row_pass(blocks, row=None):
    """uint8 [N, 64] -> the int16 the row pass leaves, [N, r, v]."""
    px = np.asarray(blocks, np.uint8).reshape(-1, 8, 8).astype(np.int64) - 128  # (pixel ^ 0x80) read as int8
    return i16(fdct8(px, **(row or {})))


def predct(blocks, row=None, col=None):
    """uint8 [N, 64] (row-major blocks) -> d [N, u, v]: both passes with their int16 truncations, in front of the quantiser."""
    r = row_pass(blocks, row)
    return i16(fdct8(r.transpose(0, 2, 1), **(col or {}))).transpose(0, 2, 1)


def d_at(blocks, u, v):
    """predct(blocks)[:, u, v] without the seven other columns."""
    return i16(fdct8(row_pass(blocks)[:, :, v]))[:, u]


def table(qf):
    """(reciprocals, half-divisors) of a setting, [u, v] each: what the words of scaled_tab hold."""
    return 65536 // (QTABLE << qf), QTABLE >> 1


def quantise(d, recip, half, floor=False):
    """quant_scaled on every element; floor (a mutant): one shift of the signed sum, which rounds toward minus infinity."""
    d = np.asarray(d, np.int64)
    if floor:
        return i16(((half + d) * recip) >> 16)
    q = ((half + np.abs(d)) * recip) >> 16
    return i16(np.where(d < 0, -q, q))


def to_zz(q):
    """[N, u, v] -> [N, 64] in scan order."""
    return np.asarray(q).reshape(-1, 64)[:, ZIGZAG]


def model(blocks, qf, row=None, col=None):
    """fdctq_scaled_block_host on every block: uint8 [N, 64] -> zz [N, 64] (absolute DC)."""
    recip, half = table(qf)
    return to_zz(quantise(predct(blocks, row, col), recip, half))


def frame_blocks(img):
    h, w = img.shape
    return img.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)


def blocks_frame(blocks, w=FRAME_W):
    bw = w // 8
    n = len(blocks)
    assert n % bw == 0
    return np.asarray(blocks, np.uint8).reshape(n // bw, bw, 8, 8).transpose(0, 2, 1, 3).reshape(n // bw * 8, w)


# ---- mutants ------------------------------------------------------------------------------------------------------------------------

def transform_mutants():
    """[(name, row kwargs, col kwargs)]: every multiplier +-1 and every >> 8 as a truncating division, in one pass only."""
    out = []
    for which in ("row", "col"):
        for name, val in CONSTS.items():
            for step in (1, -1):
                kw = {"consts": {name: val + step}}
                out.append(("%s:%s%+d" % (which, name, step), kw if which == "row" else None, kw if which == "col" else None))
        for site in SHIFTS:
            kw = {"trunc": (site,)}
            out.append(("%s:%s>>8 as /256" % (which, site), kw if which == "row" else None, kw if which == "col" else None))
    return out


def table_mutants(qf):
    """[(name, reciprocals, half-divisors, floor)]: the whole-table mistakes."""
    recip, half = table(qf)
    div = QTABLE << qf
    return [("(Q+1)>>1", recip, (QTABLE + 1) >> 1, False), ("rounded reciprocals", (65536 + div // 2) // div, half, False),
            ("floor quantiser", recip, half, True)]


def word_mutant(qf, u, v, kind):
    """(reciprocals, half-divisors) with the one word (qf, u, v) changed."""
    recip, half = (t.copy() for t in table(qf))
    (recip if kind.startswith("recip") else half)[u, v] += 1 if kind.endswith("+1") else -1
    return recip, half


def separating_values(qf, u, v, kind, top):
    """bool [top + 1]: the |d| in 0..top at which the single-word mutant quantises differently (the quantiser is sign-symmetric, so are
    these mutants)."""
    a = np.arange(top + 1, dtype=np.int64)
    recip, half = table(qf)
    mr, mh = word_mutant(qf, u, v, kind)
    return (((half[u, v] + a) * recip[u, v]) >> 16) != (((mh[u, v] + a) * mr[u, v]) >> 16)


# ---- the search ---------------------------------------------------------------------------------------------------------------------

def sign_pattern(u, v):
    """+1 / -1 [8, 8]: the sign of basis function (u, v) (no sample of it is zero)."""
    y = (2 * np.arange(8) + 1) * np.pi / 16
    return np.where(np.outer(np.cos(y * u), np.cos(y * v)) >= 0, 1, -1)


def peak_block(u, v, pol):
    """-> (block [64], d): extreme pixels in the sign pattern, then the single-pixel flip that gains most, until none gains."""
    blk = np.where(sign_pattern(u, v) * pol > 0, 255, 0).astype(np.uint8).reshape(64)
    cur = int(d_at(blk[None], u, v)[0]) * pol
    while True:
        cand = np.repeat(blk[None], 64, 0)
        cand[np.arange(64), np.arange(64)] ^= 255
        got = d_at(cand, u, v) * pol
        j = int(np.argmax(got))
        if got[j] <= cur:
            return blk, cur * pol
        blk, cur = cand[j], int(got[j])


def reach(u, v, target, start=None):
    """-> block [64] with d(u, v) == target, or None.  The amplitude of the sign pattern about 128 that comes closest from below (or
    `start`, a block at or beyond the target), then single-pixel +-1 steps, each the one that lands closest to the target without passing
    it; where every step stands still or passes it, one step drawn from a generator seeded with (u, v, target), and on from there."""
    pol = 1 if target >= 0 else -1
    if start is None:
        amps = np.arange(129)[:, None]
        cand = np.clip(128 + amps * (sign_pattern(u, v) * pol).reshape(1, 64), 0, 255).astype(np.uint8)
        got = d_at(cand, u, v) * pol
        ok = np.flatnonzero(got <= target * pol)
        if ok.size == 0:
            return None
        j = ok[np.argmax(got[ok])]
        blk, cur = cand[j], int(got[j]) * pol
    else:
        blk, cur = np.array(start, np.uint8).reshape(64), int(d_at(np.asarray(start, np.uint8).reshape(1, 64), u, v)[0])
    rng = None
    for _ in range(4096):
        if cur == target:
            return blk
        cand = np.repeat(blk[None].astype(np.int64), 128, 0)
        cand[np.arange(64), np.arange(64)] += 1
        cand[64 + np.arange(64), np.arange(64)] -= 1
        valid = (cand.min(1) >= 0) & (cand.max(1) <= 255)
        got = d_at(np.clip(cand, 0, 255).astype(np.uint8), u, v)
        lo, hi = min(cur, target), max(cur, target)
        inside = valid & (got >= lo) & (got <= hi) & (got != cur)
        if not inside.any():  # every step stands still or passes the target: one seeded step anywhere, then on from there
            if rng is None:
                rng = np.random.default_rng([u, v, abs(target), int(target < 0)])
            j = int(rng.choice(np.flatnonzero(valid)))
            blk, cur = cand[j].astype(np.uint8), int(got[j])
            continue
        valid = inside
        dist = np.where(valid, np.abs(got - target), 1 << 40)
        j = int(np.argmin(dist))
        blk, cur = cand[j].astype(np.uint8), int(got[j])
    return None


def row_maxima():
    """max |row-pass output k| over the 256 rows of extreme pixels, k = 0..7."""
    rows = (((np.arange(256)[:, None] >> np.arange(8)) & 1) * 255).astype(np.int64) - 128
    return [int(x) for x in np.abs(i16(fdct8(rows))).max(0)]


def build_peaks():
    """-> (blocks [128, 64] in (u, v, +, -) order, peak+ [8, 8], peak- [8, 8])."""
    blocks, pos, neg = [], np.zeros((8, 8), np.int64), np.zeros((8, 8), np.int64)
    for u in range(8):
        for v in range(8):
            for pol, tab in ((1, pos), (-1, neg)):
                blk, d = peak_block(u, v, pol)
                blocks.append(blk)
                tab[u, v] = d
    return np.stack(blocks), pos, neg


def build_corpus(log=None):
    """-> (families: name -> uint8 [n, 64], notes: name -> list of per-block dicts, info dict).  Deterministic: the only random
    steps are reach()'s, drawn from generators seeded with the position and the target."""
    peaks, pos, neg = build_peaks()
    top = np.maximum(pos, -neg)
    peak_notes = [{"u": u, "v": v, "d": int((pos if pol > 0 else neg)[u, v])} for u in range(8) for v in range(8) for pol in (1, -1)]

    def peak_of(u, v, pol):
        return peaks[(u * 8 + v) * 2 + (0 if pol > 0 else 1)]

    # line1023: the d range of (1, 1) at best that quantises to 1023 / 1024, its middle as the target
    recip, half = table(0)
    a = np.arange(int(top[1, 1]) + 1)
    q11 = ((half[1, 1] + a) * recip[1, 1]) >> 16
    line, line_notes = [], []
    for want in (1023, 1024):
        vals = np.flatnonzero(q11 == want)
        for pol in (1, -1):
            t = int(vals[len(vals) // 2]) * pol
            blk = reach(1, 1, t)
            assert blk is not None, (want, pol)
            line.append(blk)
            line_notes.append({"u": 1, "v": 1, "d": t, "q_best": want * pol})
    for (u, v) in ((0, 1), (0, 2), (1, 0), (1, 2)):
        for pol in (1, -1):
            d = int((pos if pol > 0 else neg)[u, v])
            line.append(peak_of(u, v, pol))
            line_notes.append({"u": u, "v": v, "d": d, "q_best": int(quantise(d, recip[u, v], half[u, v]))})

    # word: per position the values that separate the mutants of its four words, as few as a greedy cover finds, smallest first
    word, word_notes, cache, exceptions, flip = [], [], {}, [], 1
    for u in range(8):
        for v in range(8):
            chosen = {}  # |d| -> ["setting:kind"]
            for qf in range(4):
                sets = {kind: separating_values(qf, u, v, kind, int(top[u, v])) for kind in WORD_KINDS}
                left = [k for k in WORD_KINDS if sets[k].any()]
                exceptions += ["%s:%d,%d:%s" % (SETTINGS[qf], u, v, k) for k in WORD_KINDS if not sets[k].any()]
                for val in sorted(chosen):  # values already built for this position
                    hit = [k for k in left if sets[k][val]]
                    chosen[val] += ["%s:%s" % (SETTINGS[qf], k) for k in hit]
                    left = [k for k in left if k not in hit]
                while left:
                    cover = np.sum([sets[k] for k in left], axis=0)
                    val = int(np.argmax(cover))  # (the smallest of the best)
                    hit = [k for k in left if sets[k][val]]
                    chosen.setdefault(val, []).extend("%s:%s" % (SETTINGS[qf], k) for k in hit)
                    left = [k for k in left if k not in hit]
            for val in sorted(chosen):
                blk = None
                for pol in (flip, -flip):
                    lim = int((pos if pol > 0 else -neg)[u, v])
                    if val > lim:
                        continue
                    blk = reach(u, v, val * pol)
                    if blk is None:  # from above: down from the peak block
                        blk = reach(u, v, val * pol, start=peak_of(u, v, pol))
                    if blk is not None:
                        break
                assert blk is not None, ("no block found", u, v, val)
                word.append(blk)
                word_notes.append({"u": u, "v": v, "d": val * pol, "kills": chosen[val]})
                flip = -flip
            if log:
                log("word (%d, %d): %d blocks so far" % (u, v, len(word)))

    flat0, flat255 = np.zeros(64, np.uint8), np.full(64, 255, np.uint8)
    dc = [flat0, flat255, flat0, flat255, flat0, flat255, flat0, peak_of(0, 0, 1), peak_of(0, 0, -1)]
    dc_notes = [{"u": 0, "v": 0, "d": int(d_at(b[None], 0, 0)[0])} for b in dc]
    info = {"peak_pos": pos.tolist(), "peak_neg": neg.tolist(), "peak_max": int(top.max()), "row_maxima": row_maxima(),
            "unseparable_words": exceptions}
    return ({"peak": peaks, "line1023": np.stack(line), "word": np.stack(word), "dcswing": np.stack(dc)},
            {"peak": peak_notes, "line1023": line_notes, "word": word_notes, "dcswing": dc_notes}, info)


def arrange(families, notes):
    """-> [(frame name, family, uint8 [h, 72], notes of its blocks)]: frames of FRAME_ROWS x 9 blocks per family, the remainder in a last
    frame filled to whole block rows with flat FILL.  Blocks whose coefficients leave the code table at `best` (|AC| > 1023) go to a
    frame of their own, `nocode_0`."""
    per_row, per_frame = FRAME_W // 8, FRAME_W // 8 * FRAME_ROWS
    recip, half = table(0)
    out, nocode, nocode_notes = [], [], []
    for fam in ("peak", "line1023", "word", "dcswing"):
        blocks, nts = families[fam], [dict(n, i=i) for i, n in enumerate(notes[fam])]  # i: the block's place in its family
        q = np.abs(quantise(predct(blocks), recip, half)).reshape(-1, 64)[:, 1:].max(1)
        keep = np.flatnonzero(q <= 1023)
        for i in np.flatnonzero(q > 1023):
            nocode.append(blocks[i])
            nocode_notes.append(dict(nts[i], family=fam))
        for k in range(0, len(keep), per_frame):
            idx = keep[k: k + per_frame]
            out.append(("%s_%d" % (fam, k // per_frame), fam, _padded(blocks[idx], per_row), [nts[i] for i in idx]))
    out.append(("nocode_0", "nocode", _padded(np.stack(nocode), per_row), nocode_notes))
    return out


def _padded(blocks, per_row):
    pad = (-len(blocks)) % per_row
    return blocks_frame(np.concatenate([blocks, np.full((pad, 64), FILL, np.uint8)]) if pad else blocks)


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------

class Fixture:
    """scaled_blocks.npz / .json.  frames: name -> {family, h, w, blocks (the built ones, fillers behind them), notes, settings: {setting:
    {pinned_by, payload_bits, bytes, sha256, zz_sha256, dec_sha256, max_abs_ac}}}; a model-pinned entry has no stream."""

    def __init__(self, golden_dir=GOLDEN):
        self.npz = np.load(os.path.join(golden_dir, "scaled_blocks.npz"))
        with open(os.path.join(golden_dir, "scaled_blocks.json")) as f:
            self.meta = json.load(f)
        self.frames = self.meta["frames"]
        self.info = self.meta["info"]

    def names(self, family=None):
        return [n for n, e in self.frames.items() if family is None or e["family"] == family]

    def pixels(self, name):
        return self.npz[name + "_img"]

    def zz(self, name, setting):
        return self.npz["%s_%s_zz" % (name, setting)]

    def stream(self, name, setting):
        """bytes, or None where the reference has no defined stream."""
        key = "%s_%s_bs" % (name, setting)
        return self.npz[key].tobytes() if key in self.npz.files else None

    def entry(self, name, setting):
        return self.frames[name]["settings"][setting]

    def cases(self):
        """[(frame, setting)] frame by frame, the settings inside."""
        return [(n, s) for n in self.frames for s in SETTINGS]

    def family_blocks(self, family):
        """(uint8 [n, 64], notes) of the built blocks of a family in the order they were built, wherever `arrange` put them (the no-code
        frame included)."""
        blocks, notes = [], []
        for n, e in self.frames.items():
            b = frame_blocks(self.pixels(n))[: e["blocks"]]
            for blk, note in zip(b, e["notes"]):
                if e["family"] == family or note.get("family") == family:
                    blocks.append(blk)
                    notes.append(note)
        order = sorted(range(len(notes)), key=lambda k: notes[k]["i"])
        return np.stack([blocks[k] for k in order]), [notes[k] for k in order]

    def all_blocks(self):
        """uint8 [n, 64]: every block of every frame, fillers included."""
        return np.concatenate([frame_blocks(self.pixels(n)) for n in self.frames])
