"""Shared by tests/test_entropy_blocks_cpu.py, tests/test_entropy_blocks_gpu.py and tests/golden/gen/make_goldens_entropy_blocks.py: BUILT
coefficient frames for the entropy encoder (no transform made them), and the fixture tests/golden/entropy_blocks.json with what the
unmodified reference's compress() wrote for each.  No test lives here.

A frame is int16 [n, 64] in zig-zag order with the ABSOLUTE DC in column 0 (the device layout); the fixture stores per frame its name,
h, w, the header's quality, the sha256 of the little-endian coefficients, the reference's default-table stream (length and sha256, or the
exception it raised), the same for the stream with the image's own tables, and the frame's CENSUS: figures that show the frame reaches
the edge it was built for.  The census comes from bit lengths of the oracle's table dump (oracle/tic_oracle.c tico_dump_tables), never
from the library under test.

Families (DESIGN.md 5.4 names the kernels' limits they aim at):
  runs        one block per pair of AC positions and per single position: every (end position, run length) pair, every run carried into
              every group of 8 scan positions; in construction order and under a seeded permutation; strips of the permuted frame;
              9 blocks whose last groups of 8 positions are as long as the format allows (245 bits)
  symbols     every (run, size) symbol at its four extreme values, every DC category at its extreme differences, a DC that walks
              between +32767 and -32768 in legal steps; strips
  dense_max   63 AC of size 10 and a DC difference of category 11 in every block: 1,662 bits per block, the format's maximum
  lane_limit  sparse frames with blocks of exactly 511, 512 and 513 bits (the lane-per-block packer holds 512)
  dc_edges    DC differences of +-2047 exactly where the packers take the previous DC from another wave, partition or workgroup
  alignment   48-bit partitions and small symbols: every residue mod 32 of the partition ends under 8- and 64-block partitioning; payloads
              of whole words, whole bytes and neither; all-zero frames at every strip count
  long_short  8-block partitions beyond 2,048 bits (the placing kernel reads those from memory) next to 48-bit ones (through LDS)
  nocode      a symbols frame with ONE coefficient or DC difference that has no code in the default tables
"""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "entropy_blocks.json")
BASE_H, BASE_W = 264, 520  # 33 x 65 = 2,145 blocks: 268 partitions of 8 and one of 1; 33 partitions of 64 and one of 33
BASE_N = 2145
STRIPS = (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)
DENSE_STRIPS = (1, 8, 9, 64, 65)
DC_EDGES = (8, 64, 128, 256, 512, 2144)  # the difference of block b against block b - 1
LANE_BITS = 512                          # what a block may take in the lane-per-block packer
MAX_BLOCK_BITS = 1662                    # DC 9 + 11, 63 x (16 + 10), EOB 4
MAX_LANE_BITS = 245                      # 8 scan positions: 3 ZRL x 11, 8 x (16 + 10), EOB 4
AC_OFFENDERS = (1024, -1024, 2047, 2048, 32767, -32768)
DC_OFFENDERS = (2048, -2048, 4096, -4096, 32768, -32768, 65535, -65535)
MIDDLE = 1088                            # 17 x 64: first block of a partition of either packer
FAMILIES = ("runs", "symbols", "dense_max", "lane_limit", "dc_edges", "alignment", "long_short", "nocode")

_BL = np.array([i.bit_length() for i in range(65537)], np.int64)


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def coeff_sha(zz):
    return sha(np.ascontiguousarray(zz, dtype="<i2").tobytes())


def size_of(v):
    """Size category: the bit length of |v| (utils.py bits_required)."""
    return _BL[np.abs(np.asarray(v, np.int64))]


def dc_ac(zz):
    """The reference's dictionary entries: int32 DC differences (first block raw) and int32 AC [n, 63]."""
    dc = zz[:, 0].astype(np.int32)
    dc[1:] = np.diff(zz[:, 0].astype(np.int32))
    return dc, np.ascontiguousarray(zz[:, 1:], dtype=np.int32)


class Lengths:
    """Code lengths of the default tables, parsed from the oracle's table dump ('D,0,size,code' / 'A,run,size,code' lines)."""

    def __init__(self, dump):
        self.dc = np.zeros(17, np.int64)        # code + value bits per DC category, 0: no code
        self.ac = np.zeros((16, 17), np.int64)  # code + value bits per (run, size); (0, 0) EOB, (15, 0) ZRL
        for line in dump.split():
            kind, run, size, code = line.split(",")
            run, size = int(run), int(size)
            if kind == "D":
                self.dc[size] = len(code) + size
            else:
                self.ac[run, size] = len(code) + size
        self.eob, self.zrl = int(self.ac[0, 0]), int(self.ac[15, 0])


def walk(zz):
    """Per non-zero AC coefficient of the frame: (block, position, run of zeros in front of it, size)."""
    ac = np.asarray(zz, np.int64)[:, 1:]
    blk, col = np.nonzero(ac)
    pos = col + 1
    prev = np.zeros_like(pos)
    same = np.zeros(len(pos), bool)
    same[1:] = blk[1:] == blk[:-1]
    prev[1:] = np.where(same[1:], pos[:-1], 0)
    return blk, pos, pos - 1 - prev, size_of(ac[blk, col])


def block_bits(zz, L):
    """int64 [n]: bits of every block in a default-table stream, -1 for a block that holds a symbol without a code."""
    zz = np.asarray(zz, np.int64)
    n = zz.shape[0]
    cat = size_of(np.diff(zz[:, 0], prepend=0))
    bits = L.dc[cat] + L.eob
    bad = L.dc[cat] == 0
    blk, pos, run, size = walk(zz)
    sym = L.ac[run & 15, size]
    np.add.at(bits, blk, sym + (run >> 4) * L.zrl)
    bad_blocks = np.zeros(n, bool)
    bad_blocks[blk[sym == 0]] = True
    bits[bad | bad_blocks] = -1
    return bits


def zrls_per_block(zz):
    blk, pos, run, size = walk(zz)
    out = np.zeros(np.asarray(zz).shape[0], np.int64)
    np.add.at(out, blk, run >> 4)
    return out


def lane_bits(zz, L):
    """int64 [n, 8]: bits of the symbols that start in each group of 8 scan positions of every block (the strings the 8-lane packer
    builds: the DC in group 0, the EOB in group 7, a symbol's ZRLs with the symbol).  Frames without no-code symbols only."""
    zz = np.asarray(zz, np.int64)
    out = np.zeros((zz.shape[0], 8), np.int64)
    out[:, 0] += L.dc[size_of(np.diff(zz[:, 0], prepend=0))]
    out[:, 7] += L.eob
    blk, pos, run, size = walk(zz)
    np.add.at(out, (blk, pos >> 3), L.ac[run & 15, size] + (run >> 4) * L.zrl)
    return out


def partition_ends(bits, per):
    """Stream bit offsets at which the partitions of `per` blocks end."""
    c = np.cumsum(bits)
    idx = np.minimum(np.arange(per, len(bits) + per, per), len(bits)) - 1
    return c[idx]


def strip_shape(n):
    return 8, 8 * n


# ---------------------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------------------
def value_of_size(rng, s):
    """A seeded value of exactly s bits, either sign."""
    lo = 1 << (s - 1)
    v = int(rng.integers(lo, 2 * lo))
    return v if rng.random() < 0.5 else -v


def runs_blocks():
    rng = np.random.default_rng(101)
    zz = np.zeros((BASE_N, 64), np.int64)
    k = 0
    for b in range(1, 64):
        zz[k, b] = value_of_size(rng, int(rng.integers(1, 11)))
        k += 1
    for a in range(1, 64):
        for b in range(a + 1, 64):
            zz[k, a] = value_of_size(rng, int(rng.integers(1, 11)))
            zz[k, b] = value_of_size(rng, int(rng.integers(1, 11)))
            k += 1
    assert k == 2016
    for j in range(k, BASE_N):  # all-zero blocks and blocks with only position 63
        if (j - k) % 2:
            zz[j, 63] = value_of_size(rng, int(rng.integers(1, 11)))
    zz[:, 0] = np.cumsum(rng.integers(-40, 41, BASE_N))
    return zz


def lane_full_blocks():
    """9 blocks: for k = 1 .. 7 zeros up to position 8k - 1 and a size-10 coefficient at every position behind (k = 7: the last group
    of 8 positions emits 3 ZRL, eight 26-bit symbols and the EOB, 245 bits - the most the 8-lane packer's lane string has to hold), one
    block of 63 size-10 coefficients, one of zeros."""
    rng = np.random.default_rng(808)
    zz = np.zeros((9, 64), np.int64)
    for k in range(1, 8):
        for p in range(8 * k, 64):
            zz[k - 1, p] = value_of_size(rng, 10)
    for p in range(1, 64):
        zz[7, p] = value_of_size(rng, 10)
    zz[:, 0] = np.cumsum(rng.integers(-1000, 1001, 9))
    return zz


def dc_walk(n, step, top, bottom, hold):
    """0 -> top in steps of at most `step`, `hold` blocks there, down to bottom, `hold` blocks, up again ..."""
    out, v, target, held = [], 0, top, 0
    while len(out) < n:
        out.append(v)
        if v == target:
            held += 1
            if held >= hold:
                held, target = 0, (bottom if target == top else top)
        else:
            v = min(v + step, target) if target > v else max(v - step, target)
    return np.asarray(out, np.int64)


def symbol_values(s):
    return sorted({1 << (s - 1), -(1 << (s - 1)), (1 << s) - 1, -((1 << s) - 1)})


def dc_extreme_diffs():
    return [0] + [d for c in range(1, 12) for d in symbol_values(c)]


def symbols_blocks(n=BASE_N):
    rng = np.random.default_rng(202)
    required = [(r, v) for r in range(16) for s in range(1, 11) for v in symbol_values(s)]
    order = rng.permutation(len(required))
    zz = np.zeros((n, 64), np.int64)
    b, p = 0, 1
    for i in order:  # the required symbols first, packed block after block
        r, v = required[i]
        if p + r > 63:
            b, p = b + 1, 1
        zz[b, p + r] = v
        p += r + 1
    for b in range(b + 1, n):  # then seeded draws from the same set, blocks of every density
        p, fill = 1, int(rng.integers(0, 64))
        while True:
            r, v = required[int(rng.integers(0, len(required)))]
            if p + r > fill:
                break
            zz[b, p + r] = v
            p += r + 1
    # DC: every category's extreme differences as +d, -d pairs from 0, then the triangle walk
    diffs = []
    for d in dc_extreme_diffs():
        diffs += [d, -d]
    head = np.cumsum(diffs)
    zz[:len(head), 0] = head
    zz[len(head):, 0] = dc_walk(n - len(head), 2047, 32767, -32768, 3)
    return zz


def dense_blocks(n):
    rng = np.random.default_rng(303 + n)
    zz = rng.integers(512, 1024, (n, 64)) * np.where(rng.random((n, 64)) < 0.5, -1, 1)
    zz[:, 0] = np.where(np.arange(n) % 2 == 0, 2047, 0)  # raw 2047, then -2047, +2047, ...
    return zz


def exact_block(rng, L, target, prefix):
    """One block of exactly `target` bits with a DC difference of 0: `prefix` seeded symbols, then the fewest run-0 symbols that make up
    the rest (a coin-change over the lengths of the (0, size) symbols)."""
    row = np.zeros(64, np.int64)
    p, left = 1, target - int(L.dc[0]) - L.eob
    for _ in range(prefix):
        r, s = int(rng.integers(0, 4)), int(rng.integers(1, 11))
        row[p + r] = value_of_size(rng, s)
        p += r + 1
        left -= int(L.ac[r, s])
    coins = [(int(L.ac[0, s]), s) for s in range(1, 11)]
    best = [None] * (left + 1)
    best[0] = []
    for t in range(1, left + 1):
        for c, s in coins:
            if t >= c and best[t - c] is not None and (best[t] is None or len(best[t - c]) + 1 < len(best[t])):
                best[t] = best[t - c] + [s]
    sizes = best[left]
    assert sizes is not None and p + len(sizes) <= 64, (target, prefix)
    for s in (sizes[i] for i in rng.permutation(len(sizes))):
        row[p] = value_of_size(rng, s)
        p += 1
    return row


def lane_limit_blocks(L, over_at):
    """A sparse frame with 24 blocks of 511 and 24 of 512 bits at seeded places and one of 513 at block `over_at` (None: none).  Every
    block keeps the DC of its predecessor where a built block sits, so that the count is the block's own."""
    rng = np.random.default_rng(404)
    zz = np.zeros((BASE_N, 64), np.int64)
    sprinkle = rng.random(BASE_N) < 0.2
    zz[sprinkle, 1] = rng.integers(1, 4, int(sprinkle.sum()))
    dcs = np.cumsum(rng.integers(-3, 4, BASE_N))
    places = [int(x) for x in rng.choice(np.arange(1, BASE_N - 1), 48, replace=False)]
    for i, b in enumerate(places):
        zz[b] = exact_block(rng, L, 511 + (i % 2), i % 5)
        dcs[b:] += dcs[b - 1] - dcs[b]
    if over_at is not None:
        zz[over_at] = exact_block(rng, L, 513, 2)
        if over_at:
            dcs[over_at:] += dcs[over_at - 1] - dcs[over_at]
        else:
            dcs -= dcs[0]
    zz[:, 0] = dcs
    return zz


def dc_edges_blocks(sign, ac63):
    """Differences of +-2047 at block 0 and at DC_EDGES, in turn; every other difference is seeded inside +-5 and keeps the running DC
    next to a level: between two edges 0 or +-2047 as the edges leave it, and from block 512 on a ramp from 0 to -+2047, so that the
    last edge brings the DC home.  (A decoder's pixels show a DC only near 0 - a block at +-2047 is clipped under every header - and a
    wrong DC difference moves every block behind it: with blocks near 0 behind every block, the last one included, any such error
    shows; tests/test_decoder_streams_cpu.py test_dc_visibility.)"""
    rng = np.random.default_rng(505)
    edges = (0,) + DC_EDGES
    last, ramp_from = DC_EDGES[-1], DC_EDGES[-2]
    d = np.zeros(BASE_N, np.int64)
    s, dc, level = -sign, 0, 0
    for b in range(BASE_N):
        if b in edges:
            s = -s
            d[b] = s * 2047
            level += s * 2047
        else:
            if b > ramp_from:  # (the level in front of the last edge: the far side of it)
                level = s * 2047 * (b - ramp_from) // (last - 1 - ramp_from)
            d[b] = int(np.clip(level - dc + int(rng.integers(-3, 4)), -5, 5))
        dc += int(d[b])
    zz = np.zeros((BASE_N, 64), np.int64)
    zz[:, 0] = np.cumsum(d)
    if ac63:
        zz[:, 63] = 1
    return zz


def alignment_blocks(L, total_mod):
    """All-zero blocks (6 bits) with small symbols sprinkled so that every partition of 64 blocks is 1 bit longer than a whole number
    of words: the partition ends walk through every residue mod 32.  The last partition is then topped up with 3-bit symbols until the
    payload is `total_mod` mod 32."""
    rng = np.random.default_rng(606)
    extras = [(1, 1, int(L.ac[0, 1])), (1, 2, int(L.ac[0, 2])), (2, 1, int(L.ac[1, 1]))]  # (position, value, bits)
    three = int(L.ac[0, 1])
    assert three % 2 == 1
    zz = np.zeros((BASE_N, 64), np.int64)
    zero = int(L.dc[0]) + L.eob
    for first in range(0, BASE_N, 64):
        nb = min(64, BASE_N - first)
        last = first + 64 >= BASE_N
        want = (total_mod - (first // 64)) % 32 if last else 1  # bits mod 32 this partition adds
        have = nb * zero
        blocks = [int(x) for x in rng.permutation(nb)]
        for _ in range(int(rng.integers(0, 3 if last else 8))):  # (the last partition has 33 blocks: 2 + at most 31 below)
            pos, val, bits = extras[int(rng.integers(0, 3))]
            zz[first + blocks.pop(), pos] = val if rng.random() < 0.5 else -val
            have += bits
        while have % 32 != want:
            zz[first + blocks.pop(), 1] = 1 if rng.random() < 0.5 else -1
            have += three
    return zz


def long_short_blocks(confined):
    """8-block partitions of 8 dense blocks (20 AC of sizes 6..10 each: beyond 2,048 bits) and all-zero ones (48 bits) in turn;
    confined: only in the placing workgroup of partitions 96..127 (blocks 768..1023), all-zero everywhere else."""
    rng = np.random.default_rng(707)
    zz = np.zeros((BASE_N, 64), np.int64)
    dcs = np.zeros(BASE_N, np.int64)
    for part in range(0, (BASE_N + 7) // 8, 2):
        if confined and not 96 <= part < 128:
            continue
        for b in range(part * 8, min(part * 8 + 8, BASE_N)):
            for p in rng.choice(np.arange(1, 64), 20, replace=False):
                zz[b, p] = value_of_size(rng, int(rng.integers(6, 11)))
            dcs[b] = int(rng.integers(-200, 201))
    zz[:, 0] = np.cumsum(dcs)
    return zz


def with_dc_offender(base, b, d):
    """`base` with a DC difference of d at block b and nowhere else a difference beyond +-2047: the blocks in front of b ramp to a level
    from which b can jump by d inside int16, the blocks behind ramp back to the base's own DC."""
    zz = base.copy()
    n = zz.shape[0]
    if b == 0:
        zz[0, 0] = d
        hi = min(n, 1 + 40)
        back = zz[hi - 1, 0] if hi - 1 >= 1 and hi < n else None
        ramp(zz, 0, hi, back)
        return zz
    before = int(np.clip(-(d // 2), -32768, 32767 - max(d, 0)))
    if before + d < -32768:
        before = -32768 - d
    first = max(b - 40, 1)
    zz[b - 1, 0] = before
    ramp_to(zz, first - 1, b - 1)
    zz[b, 0] = before + d
    hi = min(n, b + 41)
    ramp(zz, b, hi, zz[hi - 1, 0] if hi < n else None)
    return zz


def ramp_to(zz, a, b):
    """DC of blocks a + 1 .. b - 1: from zz[a] towards zz[b] in equal steps."""
    if b - a > 1:
        zz[a + 1:b, 0] = np.round(np.linspace(zz[a, 0], zz[b, 0], b - a + 1)[1:-1]).astype(np.int64)


def ramp(zz, a, hi, back):
    """DC of blocks a + 1 .. hi - 1: from zz[a] back to `back` (the base's DC at hi - 1), or level when the frame ends first."""
    if back is None:
        zz[a + 1:hi, 0] = zz[a, 0]
    else:
        ramp_to(zz, a, hi - 1)


def nocode_frames(base):
    """name -> (h, w, zz, kind, block, value): one offender per frame."""
    out = {}
    n = base.shape[0]
    one = base[:1].copy()
    one[0, 0] = 5
    places = (("first", 0), ("middle", MIDDLE), ("last", n - 1), ("only", 0))
    for vi, v in enumerate(AC_OFFENDERS):
        for pi, (pname, b) in enumerate(places):
            pos = (1, 8, 63)[(vi + pi) % 3]
            zz = (one if pname == "only" else base).copy()
            zz[b, pos] = v
            out["nocode_ac_%s_p%d_%s" % (str(v).replace("-", "m"), pos, pname)] = (zz, "ac", b, v)
    for d in DC_OFFENDERS:
        for pname, b in places:
            v = d
            if b == 0:  # the first block's difference is its DC: what an int16 holds
                v = int(np.clip(d, -32768, 32767))
                if v != d and d != 32768:
                    continue  # (+-65535 needs a neighbour; +32768 becomes the largest raw DC, 32767)
            zz = with_dc_offender(one if pname == "only" else base, b, v)
            out["nocode_dc_%s_%s" % (str(d).replace("-", "m"), pname)] = (zz, "dc", b, v)
    return out


def build_frames(L):
    """name -> {"family", "h", "w", "quality", "zz" int16 [n, 64]} for every frame of the fixture, in a fixed order."""
    frames = {}

    def add(name, family, zz, q=50, shape=None):
        n = zz.shape[0]
        h, w = shape or ((BASE_H, BASE_W) if n == BASE_N else strip_shape(n))
        assert ((h + 7) // 8) * ((w + 7) // 8) == n and name not in frames, name
        assert zz.min() >= -32768 and zz.max() <= 32767, name
        frames[name] = {"family": family, "h": h, "w": w, "quality": q, "zz": np.ascontiguousarray(zz, dtype=np.int16)}

    runs = runs_blocks()
    add("runs_ordered", "runs", runs, 50)
    perm = np.random.default_rng(111).permutation(BASE_N)
    permuted = runs[perm]
    permuted[:, 0] = runs[:, 0]  # (the DC walk stays a walk)
    add("runs_permuted", "runs", permuted, 37)
    for n in STRIPS:
        add("runs_strip_%d" % n, "runs", permuted[:n], 37)
    add("runs_lane_full", "runs", lane_full_blocks(), 50)
    sym = symbols_blocks()
    add("symbols", "symbols", sym, 50)
    for n in STRIPS:
        add("symbols_strip_%d" % n, "symbols", sym[:n], 90)
    add("dense_max", "dense_max", dense_blocks(BASE_N), 99)
    for n in DENSE_STRIPS:
        add("dense_max_strip_%d" % n, "dense_max", dense_blocks(n), 99)
    add("lane_limit_none", "lane_limit", lane_limit_blocks(L, None), 50)
    add("lane_limit_last", "lane_limit", lane_limit_blocks(L, BASE_N - 1), 50)
    add("lane_limit_first", "lane_limit", lane_limit_blocks(L, 0), 50)
    for sign, sname in ((1, "pos"), (-1, "neg")):
        for ac63 in (False, True):
            add("dc_edges_%s%s" % (sname, "_ac63" if ac63 else ""), "dc_edges", dc_edges_blocks(sign, ac63), 50)
    for name, mod in (("alignment_words", 0), ("alignment_bytes", 8), ("alignment_bits", 5)):
        add(name, "alignment", alignment_blocks(L, mod), 50)
    add("zeros", "alignment", np.zeros((BASE_N, 64), np.int64), 1)
    for n in STRIPS:
        add("zeros_strip_%d" % n, "alignment", np.zeros((n, 64), np.int64), 1)
    add("long_short_alternating", "long_short", long_short_blocks(False), 50)
    add("long_short_confined", "long_short", long_short_blocks(True), 50)
    for name, (zz, kind, b, v) in nocode_frames(sym).items():
        add(name, "nocode", zz, 50, shape=(8, 8) if zz.shape[0] == 1 else None)
        frames[name]["offender"] = (kind, b, v)
    return frames


# ---------------------------------------------------------------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------------------------------------------------------------
def census(name, fr, L):
    """The figures that show frame `name` reaches its edge (ints and short lists only: they go into the JSON as they are); asserts
    what the family promises."""
    zz = fr["zz"].astype(np.int64)
    n = zz.shape[0]
    fam = fr["family"]
    bits = block_bits(zz, L)
    valid = bool((bits >= 0).all())
    c = {"blocks": n, "max_block_bits": int(bits.max()), "payload_bits": int(bits.sum()) if valid else None}
    blk, pos, run, size = walk(zz)
    diffs = np.diff(zz[:, 0], prepend=0)
    if fam == "runs":
        z = zrls_per_block(zz)
        c["end_run_pairs"] = len(set(zip(pos.tolist(), run.tolist())))
        c["blocks_with_zrls"] = [int((z == k).sum()) for k in (1, 2, 3)]
        carried = set()  # (lane k, run carried into it) for every first non-zero coefficient of a lane that has one
        for p, r in zip(pos.tolist(), run.tolist()):
            k = p >> 3
            if k >= 1 and p - r <= 8 * k:  # the run started in front of the lane
                carried.add((k, 8 * k - (p - r)))
        c["carried_runs"] = len(carried)
        need = z > 0
        parts = [need[i:i + 8] for i in range(0, n, 8)]
        # the 8-lane packer compiles the ZRL tests in per wave: partitions (waves) without a ZRL, and with blocks of both kinds
        c["partitions_without_zrl"] = sum(1 for p in parts if not p.any())
        c["partitions_mixing_zrl_and_none"] = sum(1 for p in parts if p.any() and not p.all())
        c["max_lane_bits"] = int(lane_bits(zz, L).max())
        if name == "runs_lane_full":
            assert c["max_lane_bits"] == MAX_LANE_BITS and lane_bits(zz, L)[6, 7] == MAX_LANE_BITS and c["blocks_with_zrls"] == [2, 2, 1], (name, c)
        if n == BASE_N:
            assert c["end_run_pairs"] == 2016 and c["carried_runs"] == 8 * 28 and min(c["blocks_with_zrls"]) > 0, (name, c)
            assert carried == {(k, r) for k in range(1, 8) for r in range(8 * k)}, name
            if name == "runs_permuted":  # (blocks with a ZRL are 84 % of the frame: under the permutation every wave has one)
                assert c["partitions_mixing_zrl_and_none"] > 200, (name, c)
            else:
                assert c["partitions_without_zrl"] > 20 and c["partitions_mixing_zrl_and_none"] > 0, (name, c)
    elif fam in ("symbols", "nocode"):
        vals = zz[blk, pos]
        c["ac_symbols"] = len({(r, s) for r, s in zip(run.tolist(), size.tolist()) if r < 16 and s <= 10})
        c["ac_symbol_values"] = len({(r, v) for r, v, s in zip(run.tolist(), vals.tolist(), size.tolist())
                                     if r < 16 and s <= 10 and v in symbol_values(s)})
        c["dc_extreme_diffs"] = len(set(diffs.tolist()) & set(dc_extreme_diffs()))
        c["dc_min"], c["dc_max"] = int(zz[:, 0].min()), int(zz[:, 0].max())
        if fam == "symbols" and n == BASE_N:
            assert c["ac_symbols"] == 160 and c["ac_symbol_values"] == 16 * 38 and c["dc_extreme_diffs"] == 43, (name, c)
            assert (c["dc_min"], c["dc_max"]) == (-32768, 32767) and np.abs(diffs).max() == 2047 and valid, (name, c)
        if fam == "nocode":
            kind, b, v = fr["offender"]
            bad = np.nonzero(bits < 0)[0].tolist()
            c["offender"] = [kind, int(b), int(v)]
            assert bad == [b], (name, bad)  # one offending block, and it is the one
            assert (zz[b, 1:].tolist().count(v) >= 1 and size_of(v) > 10) if kind == "ac" else (diffs[b] == v and size_of(v) > 11), name
            assert (np.abs(np.delete(diffs, b)) <= 2047).all() and (size_of(np.delete(zz[:, 1:], b, 0)) <= 10).all(), name
    elif fam == "dense_max":
        assert (bits == MAX_BLOCK_BITS).all() and (size_of(zz[:, 1:]) == 10).all() and (np.abs(diffs) == 2047).all(), name
    elif fam == "lane_limit":
        c["blocks_of_511_512_513"] = [int((bits == t).sum()) for t in (511, 512, 513)]
        over = np.nonzero(bits > LANE_BITS)[0].tolist()
        c["blocks_over_512"] = over
        want = {"lane_limit_none": [], "lane_limit_last": [BASE_N - 1], "lane_limit_first": [0]}[name]
        assert over == want and c["blocks_of_511_512_513"] == [24, 24, len(want)] and c["max_block_bits"] == 512 + len(want), (name, c)
    elif fam == "dc_edges":
        c["edge_diffs"] = [int(diffs[b]) for b in (0,) + DC_EDGES]
        assert all(abs(d) == 2047 for d in c["edge_diffs"]) and np.abs(np.delete(diffs, (0,) + DC_EDGES)).max() <= 5, (name, c)
        assert (zz[:, 1:63] == 0).all() and len(set(zz[:, 63].tolist())) == 1, name
    elif fam == "alignment":
        c["end_residues_8"] = len(set((partition_ends(bits, 8) % 32).tolist()))
        c["end_residues_64"] = len(set((partition_ends(bits, 64) % 32).tolist()))
        if name.startswith("zeros"):
            assert (bits == 6).all() and not zz.any(), name
        else:
            assert c["end_residues_8"] == 32 and c["end_residues_64"] == 32, (name, c)
            mod = {"alignment_words": 0, "alignment_bytes": 8, "alignment_bits": 5}[name]
            assert c["payload_bits"] % 32 == mod, (name, c)
    elif fam == "long_short":
        pb = np.add.reduceat(bits, np.arange(0, n, 8))
        long_groups = sorted({int(i) // 32 for i in np.nonzero(pb > 2048)[0]})
        c["partitions_over_2048"] = int((pb > 2048).sum())
        c["partitions_of_48"] = int((pb == 48).sum())
        c["placing_workgroups_with_long"] = long_groups
        c["max_partition_bits"] = int(pb.max())
        both = [g for g in long_groups if (pb[g * 32:(g + 1) * 32] == 48).any()]
        assert both == long_groups and (long_groups == [3] if "confined" in name else long_groups == list(range(9))), (name, c)
        assert c["partitions_over_2048"] == (16 if "confined" in name else 134), (name, c)  # (partition 268 has one block)
    if valid:
        assert c["payload_bits"] == int(bits.sum())
    return c


def expected_len(c):
    """Stream bytes from the census (16 + the payload rounded up to a byte), None for a frame that has no default-table stream."""
    return None if c["payload_bits"] is None else 16 + (c["payload_bits"] + 7) // 8


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def first_difference(got, want, zz, L):
    """For a failure message: the first differing byte of two streams and the block whose bits it holds."""
    m = min(len(got), len(want))
    i = next((k for k in range(m) if got[k] != want[k]), m)
    bits = block_bits(zz, L)
    ends = np.cumsum(np.where(bits < 0, 0, bits))
    blk = int(np.searchsorted(ends, (i - 16) * 8, side="right")) if i >= 16 else -1
    return "lengths %d / %d, first difference at byte %d (block %d of %d)" % (len(got), len(want), i, blk, len(bits))
