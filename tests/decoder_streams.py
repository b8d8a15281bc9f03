"""Shared by tests/test_decoder_streams_cpu.py, tests/test_decoder_streams_gpu.py, tests/test_entropy_blocks_gpu.py and
tests/golden/gen/make_goldens_decoder_streams.py: BUILT coefficient frames for the device decoder's Huffman walk (the measure walk's chain
tables, the stitch, the fused kernel's pair table and long-codeword table - tinyimgcodec_amd/csrc/tic_entropy_dec_gpu.hip) and the
fixture tests/golden/decoder_streams.json with what the unmodified reference wrote for each and read back.  No test lives here.

A frame is int16 [n, 64] in zig-zag order with the ABSOLUTE DC in column 0 (the two dc_bounds twins, whose running DC leaves int16 for
one block, are int32), 264 x 520 pixels (2,145 blocks); its default-table payload is longer than 1,040 bytes, so tic_decompress gives
every one to the device decoder.  A frame carries a list of HEADER VARIANTS (flag, quality field): plain qualities, and one with the
1 << 30 flag and an exponent - the payload is the same under all of them.  The fixture stores per frame and variant the length and
sha256 of the reference's stream and the sha256 of the pixels the reference decoded it to; no stream bytes (the oracle writes them
again, tests/test_decoder_streams_cpu.py ties them to the digests).

Everything the census says comes from the code LENGTHS of the oracle's table dump (EB.Lengths), never from the library: which pairs of
AC symbols the pair table fuses is derived by the rule of dec_pair_luts_fill's comment (tic_entropy.cpp) - the first symbol's codeword
plus its size plus the second symbol's codeword is at most 11 bits, and the first is not EOB.  With the default tables a ZRL (11 bits)
can be neither half of a fused pair; the pairs frame holds it in front of and behind every kind of symbol all the same, unfused.

Families:
  reused      symbols, runs_ordered, runs_permuted, dense_max, lane_limit_none, dc_edges_*, alignment_*, zeros, long_short_* of
              EB.build_frames, as they are
  pairs       every fused (first, second) pair at the 4 x 4 extreme values of both, as the FIRST look-up behind the DC and behind other
              fused pairs; for every first symbol the successors that miss the 11-bit window by one bit; ZRLs in front of and behind
              short symbols.  Bit positions are censused per pair LENGTH (6 .. 18 bits), not per pair: the pairs of every length start
              at all 32 residues of the bit position mod 32 and meet a word boundary at every one of their inner bit offsets; a single
              pair has some 50 instances and does not reach all of that
  long_codes  every AC symbol with a codeword of 12..16 bits behind the DC, a fused pair, an unfused short symbol, another long
              codeword and a ZRL, followed by the EOB, a short symbol and a long one
  values      one to three AC symbols per block at seeded positions and extreme values, every (run, size) symbol
  spikes      6- and 8-bit blocks with single blocks of 600, 1,100 and 1,662 bits: two frames below 7 stream bits per block (range
              rule: 1,056 bits per lane), one between 7 and 72 (288: a 1,662-bit block passes over five whole ranges)
  cap         6- and 8-bit blocks under a seed behind 336 blocks of 6 bits: the first range of every length holds as many block starts
              as the format allows (zeros is the exactly periodic twin)
  dc_bounds   a running DC of exactly +32767 / -32768 for 3 blocks, reached in legal steps; twins that reach +32768 / -32769 for one
              block.  (tests/inverse_edges.py has no frame at exactly these values: its wide family walks beyond +-60,000.)

pairs, long_codes and values are VALUE-BEARING: the fused kernel gives out pixels only, so these frames keep to a visibility rule - the
sizes inside one block span at most 5, the DC lies within +-20, the
variants are the qualities 5 .. 99 below and one scaled one - and visibility() measures that a wrong coefficient would change a pixel.
The span rule has exceptions, counted in the census (blocks_spanning_more_than_5_sizes) and held to the same bars: in pairs the blocks of
the one fused pair that itself spans 6 sizes, (0, 1) with (0, 7); in long_codes the 114 blocks with a long codeword of size 9 or 10
behind a fused pair - there the span is the builder's choice, not the codeword's: nearest() takes the pair closest in size, and no
fused pair holds a size above 3 in one half and 5 in the other.
"""
import ctypes as C
import json
import os
import struct

import numpy as np

import entropy_blocks as EB
import inverse_edges as IE

FIXTURE = os.path.join(EB.GOLDEN, "decoder_streams.json")
SCALED = IE.SCALED
N = EB.BASE_N
H, W = EB.BASE_H, EB.BASE_W
EOB, ZRL = (0, 0), (15, 0)
REUSED = ("symbols", "runs_ordered", "runs_permuted", "dense_max", "lane_limit_none", "dc_edges_pos", "dc_edges_pos_ac63", "dc_edges_neg",
          "dc_edges_neg_ac63", "alignment_words", "alignment_bytes", "alignment_bits", "zeros", "long_short_alternating", "long_short_confined")
VALUE_FRAMES = ("pairs", "long_codes", "values")
VALUE_QUALITIES = (5, 10, 25, 50, 75, 90, 97, 99)
VALUE_VARIANTS = tuple((0, q) for q in VALUE_QUALITIES) + ((SCALED, 0),)
NEW_FAMILIES = ("pairs", "long_codes", "values", "spikes", "cap", "dc_bounds")
DC_ONLY = ("cap", "dc_edges_pos", "dc_edges_neg")       # frames without AC: the DC visibility check
SPIKE_BITS = (600, 1100, 1662)
RANGES = (288, 1056, 2016)
MIN_PAYLOAD_BYTES = 1040
SAMPLE = 20000
CLASSES = ("sign", "half", "top_bit", "position", "one")


# ---------------------------------------------------------------------------------------------------------------------------------
# restated from tinyimgcodec_amd/csrc/tic_entropy_dec_gpu.h (two lines of arithmetic each)
# ---------------------------------------------------------------------------------------------------------------------------------
def range_rule(stream_bytes, nblocks):
    """dec_range_rule: the stream bits per lane a frame asks for."""
    floor_words = 33 if stream_bytes * 8 < 7 * nblocks else 9
    k = ((2 * stream_bytes * 8) // nblocks + 31) // 32 | 1
    return min(max(k, floor_words), 63) * 32


def cap_of(range_bits):
    """dec_cap_of: the block starts a range's trace holds."""
    return range_bits // 6 + 2


# ---------------------------------------------------------------------------------------------------------------------------------
# symbols and code lengths
# ---------------------------------------------------------------------------------------------------------------------------------
def code_len(L, sym):
    return int(L.ac[sym]) - sym[1]


def ac_symbols(L):
    return [(r, s) for r in range(16) for s in range(1, 11) if L.ac[r, s]]


def long_symbols(L):
    return [y for y in ac_symbols(L) if code_len(L, y) >= 12]


def fuses(L, a, b):
    """dec_pair_luts_fill's rule: a's codeword and value bits and b's codeword lie inside one 11-bit window; a is not EOB."""
    return a != EOB and int(L.ac[a]) + code_len(L, b) <= 11


def fused_pairs(L):
    firsts = ac_symbols(L) + [ZRL]
    return [(a, b) for a in firsts for b in ac_symbols(L) + [ZRL, EOB] if fuses(L, a, b)]


def near_misses(L):
    """For every first symbol of a fused pair: the successors whose codeword ends one bit behind the window."""
    firsts = sorted({a for a, b in fused_pairs(L)})
    return [(a, b) for a in firsts for b in ac_symbols(L) + [ZRL, EOB] if int(L.ac[a]) + code_len(L, b) == 12]


def block_symbols(row):
    """The AC symbols of one block as the encoder writes them: [(run, size, value)], ZRLs expanded, the EOB last."""
    out, prev = [], 0
    for p in np.nonzero(row[1:])[0] + 1:
        run = int(p) - 1 - prev
        out += [(15, 0, 0)] * (run >> 4)
        v = int(row[p])
        out.append((run & 15, abs(v).bit_length(), v))
        prev = int(p)
    return out + [(0, 0, 0)]


def lookups(L, syms):
    """The fused kernel's walk over one block's AC symbols: [(index of the first symbol, fused)] per look-up."""
    out, i = [], 0
    while i < len(syms):
        a = syms[i][:2]
        f = i + 1 < len(syms) and fuses(L, a, syms[i + 1][:2])
        out.append((i, f))
        i += 2 if f else 1
    return out


def place(row, syms):
    """Write symbols [(run, size, value)] (ZRL: (15, 0, 0)) into a block's row from position 1 on; True when they fit."""
    p = 1
    for r, s, v in syms:
        if (r, s) == ZRL:
            p += 16
            continue
        if p + r > 63:
            return False
        row[p + r] = v
        p += r + 1
    return True


def positions_of(syms):
    return sum(16 if (r, s) == ZRL else r + 1 for r, s, v in syms)


def small_dc(rng, n, bound=20):
    """A seeded DC walk inside +-bound with differences of -3 .. 3."""
    out, v = np.zeros(n, np.int64), 0
    for i in range(n):
        v = int(np.clip(v + int(rng.integers(-3, 4)), -bound, bound))
        out[i] = v
    return out


def extreme(rng, s):
    vals = EB.symbol_values(s)
    return vals[int(rng.integers(0, len(vals)))]


# ---------------------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------------------
def pairs_blocks(L):
    rng = np.random.default_rng(1101)
    fused, body, tail = fused_pairs(L), [], []  # body: units another unit may follow; tail: units that end their block
    for a, b in fused:
        for va in EB.symbol_values(a[1]):
            if b == EOB:
                tail.append([a + (va,)])
            else:
                body += [[a + (va,), b + (vb,)] for vb in EB.symbol_values(b[1])]
    for a, b in near_misses(L):  # (the look-up behind a stands on b alone: what b fuses with is the block's end)
        tail += [[a + (va,)] + ([] if b == EOB else [b + (extreme(rng, b[1]),)]) for va in EB.symbol_values(a[1]) if b != ZRL]
    shorts = [y for y in ac_symbols(L) if code_len(L, y) <= 11 and y[0] <= 7]
    for y in shorts:  # a ZRL as the first look-up, a ZRL behind a short symbol
        c = shorts[int(rng.integers(0, len(shorts)))]
        tail.append([(15, 0, 0), y + (extreme(rng, y[1]),)])
        tail.append([y + (extreme(rng, y[1]),), (15, 0, 0), c + (extreme(rng, c[1]),)])
    body = [body[i] for i in rng.permutation(len(body))]
    tail = [tail[i] for i in rng.permutation(len(tail))]
    blocks = []
    while body or tail:
        syms = []
        for _ in range(int(rng.integers(0, 4)) if tail else 3):
            if not body:
                break
            u = body[-1]
            sizes = [s for r, s, v in syms + u]
            if positions_of(syms + u) > 40 or (syms and max(sizes) - min(sizes) > 5):
                break
            syms += body.pop()
        if tail and (not syms or rng.random() < 0.7 or not body):
            sizes = [s for r, s, v in syms + tail[-1] if s]
            if not syms or (max(sizes) - min(sizes) <= 5 and positions_of(syms + tail[-1]) <= 63):
                syms += tail.pop()
        assert syms
        blocks.append(syms)
    assert len(blocks) <= N, len(blocks)
    # seeded repeats, two or three fused pairs a block; the longest pairs (16 bits and more: few pairs, many offsets to meet a word
    # boundary at) and the shortest (6 and 7 bits: few pairs) more often than the others
    def weight(p):
        t = int(L.ac[p[0]]) + int(L.ac[p[1]])
        return 24 if t >= 18 else 8 if t >= 16 or t <= 7 else 1
    draw = [p for p in fused if p[1] != EOB for _ in range(weight(p))]
    while len(blocks) < N:
        syms = []
        for _ in range(int(rng.integers(2, 4))):
            a, b = draw[int(rng.integers(0, len(draw)))]
            u = [a + (extreme(rng, a[1]),), b + (extreme(rng, b[1]),)]
            sizes = [s for r, s, v in syms + u]
            if not syms or max(sizes) - min(sizes) <= 5:
                syms += u
        blocks.append(syms or [(0, 1, 1)])
    zz = np.zeros((N, 64), np.int64)
    for i in rng.permutation(N):
        assert place(zz[i], blocks.pop()), i
    zz[:, 0] = small_dc(rng, N)
    return zz


def nearest(rng, cands, s, width=4):
    """A seeded choice among the candidates [(.., size ..)] whose sizes are nearest to s (within `width` where any is)."""
    def dist(c):
        sizes = [y[1] for y in c] if isinstance(c[0], tuple) else [c[1]]
        return max(abs(t - s) for t in sizes)
    best = min(dist(c) for c in cands)
    pool = [c for c in cands if dist(c) <= max(best, width // 2)]
    return pool[int(rng.integers(0, len(pool)))]


def long_codes_blocks(L):
    rng = np.random.default_rng(1202)
    longs = long_symbols(L)
    shorts = [y for y in ac_symbols(L) if code_len(L, y) <= 11]
    fused = [(a, b) for a, b in fused_pairs(L) if b != EOB]
    blocks = []

    def val(y):
        return y + (extreme(rng, y[1]),)

    def one(t, pred, succ):
        s, syms = t[1], []
        if pred == "fused":
            a, b = nearest(rng, fused, s)
            syms += [val(a), val(b)]
        elif pred == "short":
            syms.append(val(nearest(rng, shorts, s)))
        elif pred == "long":
            syms.append(val(nearest(rng, longs, s)))
        elif pred == "zrl":
            syms.append((15, 0, 0))
        syms.append(val(t))
        if succ == "short":
            syms.append(val(nearest(rng, shorts, s)))
        elif succ == "long":
            syms.append(val(nearest(rng, longs, s)))
        least = min(y[1] for y in syms if y[1])
        # (where a context forces sizes more than 5 apart - the largest fused pair has sizes 3 and 5 - the large values are the smallest
        #  of their size: fewer clipped pixels for the small ones to hide behind)
        return [(r, z, v if z - least <= 5 else (1 << (z - 1)) * (1 if v > 0 else -1)) for r, z, v in syms]

    for t in longs:
        for pred in LONG_PREDS:
            for succ in LONG_SUCCS:
                blocks.append(one(t, pred, succ))
    assert len(blocks) <= N, len(blocks)
    while len(blocks) < N:
        blocks.append(one(longs[int(rng.integers(0, len(longs)))], LONG_PREDS[int(rng.integers(0, 5))], LONG_SUCCS[int(rng.integers(0, 3))]))
    zz = np.zeros((N, 64), np.int64)
    for i in rng.permutation(N):
        assert place(zz[i], blocks.pop()), i
    zz[:, 0] = small_dc(rng, N)
    return zz


LONG_PREDS = ("dc", "fused", "short", "long", "zrl")
LONG_SUCCS = ("eob", "short", "long")


def values_blocks(L):
    rng = np.random.default_rng(1303)
    syms = ac_symbols(L)
    order = [syms[i] for i in rng.permutation(len(syms))]
    zz = np.zeros((N, 64), np.int64)
    for b in range(N):
        first = order[b] if b < len(order) else syms[int(rng.integers(0, len(syms)))]
        lo = int(rng.integers(max(1, first[1] - 4), min(first[1], 6) + 1))  # the block's sizes: lo .. lo + 4, first[1] among them
        row, p = zz[b], 1
        for k in range(int(rng.integers(1, 4))):
            r, s = first if k == 0 else (int(rng.integers(0, 16)), int(rng.integers(lo, min(lo + 4, 10) + 1)))
            if p + r > 63:
                break
            row[p + r] = extreme(rng, s)
            p += r + 1
    zz[:, 0] = small_dc(rng, N)
    return zz


def flat_dc(rng, n, share, bound=20):
    """DC differences of 0 (a 6-bit block) and, with probability `share`, +-1 (8 bits), the running DC inside +-bound."""
    d, v = np.zeros(n, np.int64), 0
    for i in range(n):
        if rng.random() < share:
            step = 1 if rng.random() < 0.5 else -1
            if abs(v + step) > bound:
                step = -step
            d[i], v = step, v + step
    return d


def spike_block(rng, L, bits):
    """(row with a zero DC, DC difference) of a block of exactly `bits` bits."""
    if bits == EB.MAX_BLOCK_BITS:
        row = rng.integers(512, 1024, 64) * np.where(rng.random(64) < 0.5, -1, 1)
        row[0] = 0
        return row, 2047
    return EB.exact_block(rng, L, bits, 2), 0


def spikes_blocks(L, places, share, seed):
    """6- and 8-bit blocks with spikes: places = {block: bits}.  A 1,662-bit spike needs a DC difference of +-2047: up at one spike,
    down again at the next of its size."""
    rng = np.random.default_rng(seed)
    zz = np.zeros((N, 64), np.int64)
    d = flat_dc(rng, N, share)
    up = False
    for b in sorted(places):
        row, step = spike_block(rng, L, places[b])
        zz[b] = row
        d[b] = 0
        if step:
            d[b] = -step if up else step
            up = not up
    zz[:, 0] = np.cumsum(d)
    assert np.abs(zz[:, 0]).max() <= 2047 + 20
    return zz


def spike_places(rng):
    """Block 0, the last block, the first and last block of every fused-kernel workgroup and their neighbours (multiples of 256, +-1),
    two pairs of spikes back to back, a dozen seeded places; sizes in turn, a 1,662-bit spike wherever the DC can take it."""
    fixed = [0, N - 1] + [m + k for m in range(256, N, 256) for k in (-1, 0, 1)]
    free = []
    for x in rng.permutation(np.arange(4, N - 4)).tolist():
        if all(abs(x - y) > 4 for y in fixed + free):
            free.append(x)
        if len(free) == 14:
            break
    where = sorted(fixed + free + [free[0] + 1, free[1] + 1])
    big = where[2::3]
    return {b: SPIKE_BITS[2] if b in big else SPIKE_BITS[i % 2] for i, b in enumerate(where)}


def cap_blocks():
    rng = np.random.default_rng(1505)
    zz = np.zeros((N, 64), np.int64)
    d = np.zeros(N, np.int64)  # 336 blocks of 6 bits from payload bit 0 on: 2,016 bits, the first range of every length
    d[RANGES[-1] // 6:] = flat_dc(rng, N - RANGES[-1] // 6, 0.3, 5)  # (+-5: at quality 5 a DC step is 20 grey levels, and a clipped block hides its DC)
    zz[:, 0] = np.cumsum(d)
    return zz


def dc_bounds_blocks(top, over):
    """A flat walk; in front of block 1024 a ramp in steps of at most 2047 to `top` (+32767 or -32768), held for blocks 1023, 1024 and
    1025; over: block 1024 alone one step beyond it.  Then the ramp back."""
    rng = np.random.default_rng(1606)
    sign = 1 if top > 0 else -1
    dcs = np.cumsum(flat_dc(rng, N, 0.4))
    ramp = [sign * 2027 * k for k in range(1, 17)]  # (2027: the step from and to the flat walk, +-20, stays legal)
    dcs[1007:1023] = ramp
    dcs[1023:1026] = top
    if over:
        dcs[1024] = top + sign
    dcs[1026:1042] = ramp[::-1]
    zz = np.zeros((N, 64), np.int64)
    zz[:, 0] = dcs
    zz[::7, 5] = 1  # (a few AC symbols: the frame is not DC alone)
    return zz


def variants_of(name, quality):
    if name in VALUE_FRAMES:
        return [list(v) for v in VALUE_VARIANTS]
    other = quality if quality != 5 else 50
    return [[0, 5], [0, other], [SCALED, 3]]


def build_frames(L):
    """name -> {"family", "h", "w", "variants" [[flag, quality field]], "zz" [2145, 64]} in a fixed order."""
    eb = EB.build_frames(L)
    frames = {}

    def add(name, family, zz, quality=50):
        wide = zz[:, 0].min() < -32768 or zz[:, 0].max() > 32767
        assert zz.shape == (N, 64) and name not in frames and np.abs(zz[:, 1:]).max() <= 1023, name
        frames[name] = {"family": family, "h": H, "w": W, "variants": variants_of(name, quality),
                        "zz": np.ascontiguousarray(zz, dtype=np.int32 if wide else np.int16)}

    for name in REUSED:
        add(name, eb[name]["family"], eb[name]["zz"], eb[name]["quality"])
    add("pairs", "pairs", pairs_blocks(L))
    add("long_codes", "long_codes", long_codes_blocks(L))
    add("values", "values", values_blocks(L))
    add("spikes_flat_one", "spikes", spikes_blocks(L, {512: 1662}, 0.05, 1401))
    add("spikes_flat_two", "spikes", spikes_blocks(L, {255: 600, 256: 1100}, 0.05, 1402))
    add("spikes_sparse", "spikes", spikes_blocks(L, spike_places(np.random.default_rng(1403)), 0.5, 1404))
    add("cap", "cap", cap_blocks())
    add("dc_bounds_pos", "dc_bounds", dc_bounds_blocks(32767, False))
    add("dc_bounds_neg", "dc_bounds", dc_bounds_blocks(-32768, False))
    add("dc_bounds_pos_over", "dc_bounds", dc_bounds_blocks(32767, True))
    add("dc_bounds_neg_over", "dc_bounds", dc_bounds_blocks(-32768, True))
    return frames


def is_twin(name):
    return name.endswith("_over")


def dc_ac(zz):
    """int32 DC differences (first block raw) and AC [n, 63] - EB.dc_ac for a DC of any width."""
    dc = np.diff(zz[:, 0].astype(np.int64), prepend=0).astype(np.int32)
    return dc, np.ascontiguousarray(zz[:, 1:], dtype=np.int32)


def payload_stream(O, fr):
    """The default-table stream of a frame under its first variant (the oracle's entropy coder)."""
    dc, ac = dc_ac(fr["zz"])
    return O.entropy_encode(dc, ac, fr["h"], fr["w"], fr["variants"][0][1])


def with_header(stream, fr, variant):
    flag, q = variant
    return struct.pack("<IIII", fr["h"], fr["w"], int(q), flag) + bytes(stream[16:])


def key(variant):
    return ("s%d" if variant[0] else "q%d") % variant[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------------------------------------------------------------
def census(name, fr, L):
    """Figures that show the frame reaches its edge (ints, short lists and small dicts of them); asserts what its family promises."""
    zz = fr["zz"].astype(np.int64)
    fam = fr["family"]
    bits = EB.block_bits(zz, L)
    assert (bits >= 0).all(), name
    payload = int(bits.sum())
    nbytes = 16 + (payload + 7) // 8
    ends = np.cumsum(bits)
    starts = ends - bits
    c = {"payload_bits": payload, "stream_bytes": nbytes, "max_block_bits": int(bits.max()), "range_rule": range_rule(nbytes, N),
         "bits_per_block": nbytes * 8 // N, "dc_min": int(zz[:, 0].min()), "dc_max": int(zz[:, 0].max()),
         "periodic": bool((zz == zz[0]).all() and not zz[0].any())}
    assert nbytes - 16 >= MIN_PAYLOAD_BYTES, (name, nbytes)
    assert np.abs(np.diff(zz[:, 0], prepend=0)).max() <= 2047, name
    if fam in NEW_FAMILIES and fam != "dc_bounds":
        assert max(abs(c["dc_min"]), abs(c["dc_max"])) <= 2047 + 20, (name, c)
    if fam in ("pairs", "long_codes", "values"):
        assert max(abs(c["dc_min"]), abs(c["dc_max"])) <= 20, (name, c)
        sizes = EB.size_of(zz[:, 1:])
        span = np.where(sizes > 0, sizes, 99).min(1)
        span = np.where(span == 99, 0, sizes.max(1) - span)
        c["blocks_spanning_more_than_5_sizes"] = int((span > 5).sum())
    if fam == "pairs":
        want = fused_pairs(L)
        seen, residues, cross, instances = {}, {}, {}, 0
        lone_zrl_first = zrl_behind_short = misses = 0
        for b in range(N):
            syms = block_symbols(zz[b])
            off = [int(starts[b] + L.dc[EB.size_of(zz[b, 0] - (zz[b - 1, 0] if b else 0))])]
            for y in syms:
                off.append(off[-1] + int(L.ac[y[:2]]))
            lk = lookups(L, syms)
            for j, (i, f) in enumerate(lk):
                a = syms[i]
                if f:
                    bsym = syms[i + 1]
                    seen.setdefault((a[:2], bsym[:2]), set()).add((a[2], bsym[2]))
                    instances += 1
                    p, t = off[i], off[i + 2] - off[i]
                    residues.setdefault(t, set()).add(p % 32)
                    cross.setdefault(t, set()).update(k for k in range(1, t) if (p + k) % 32 == 0)
                else:
                    nxt = syms[i + 1][:2] if i + 1 < len(syms) else None
                    if a[:2] == ZRL:
                        lone_zrl_first += j == 0
                        zrl_behind_short += j > 0
                    if nxt is not None and a[:2] != EOB and int(L.ac[a[:2]]) + code_len(L, nxt) == 12:
                        misses += 1
        full = [p for p in want if len(seen.get(p, ())) == len(EB.symbol_values(p[0][1])) * (len(EB.symbol_values(p[1][1])) if p[1] != EOB else 1)]
        longest = max(int(L.ac[a]) + int(L.ac[b]) for a, b in want)
        c.update({"fused_pairs_by_the_lengths": len(want), "fused_pairs_seen": len(seen), "fused_pairs_at_all_extreme_values": len(full),
                  "fused_pairs_with_eob_second": sum(1 for a, b in seen if b == EOB), "fused_pairs_with_zrl": sum(1 for a, b in want if ZRL in (a, b)),
                  "fused_instances": instances, "longest_pair_bits": longest,
                  # per pair LENGTH (code and value bits of both symbols): [start residues mod 32, offsets inside the pair at which a
                  # 32-bit word boundary falls, of length - 1] over all instances of the pairs of that length
                  "residues_and_boundary_offsets_by_pair_bits": {str(t): [len(residues[t]), len(cross[t]), t - 1] for t in sorted(cross)}, "near_misses_by_the_lengths": len(near_misses(L)), "near_miss_instances": int(misses),
                  "zrl_as_first_lookup": int(lone_zrl_first), "zrl_behind_a_symbol": int(zrl_behind_short)})
        assert set(seen) == set(want) and len(full) == len(want), (name, c)
        assert max(cross) == longest and all(len(residues[t]) == 32 and cross[t] == set(range(1, t)) for t in cross), (name, c)
        assert set(cross) == {int(L.ac[a]) + int(L.ac[b]) for a, b in want}, (name, c)
        assert c["fused_pairs_with_eob_second"] > 0 and lone_zrl_first > 0 and zrl_behind_short > 0, (name, c)
        near_seen = set()
        for b in range(N):
            syms = block_symbols(zz[b])
            near_seen |= {(syms[i][:2], syms[i + 1][:2]) for i, f in lookups(L, syms) if not f and i + 1 < len(syms)}
        assert {p for p in near_misses(L) if p[1] != ZRL} <= near_seen, name
    elif fam == "long_codes":
        longs = set(long_symbols(L))
        got = set()
        for b in range(N):
            syms = block_symbols(zz[b])
            lk = lookups(L, syms)
            for j, (i, f) in enumerate(lk):
                t = syms[i][:2]
                if t not in longs:
                    continue
                assert not f
                if j == 0:
                    pred = "dc"
                else:
                    pi, pf = lk[j - 1]
                    p = syms[pi][:2]
                    pred = "fused" if pf else "zrl" if p == ZRL else "long" if p in longs else "short"
                nxt = syms[i + 1][:2]
                succ = "eob" if nxt == EOB else "long" if nxt in longs else "short" if nxt != ZRL else "zrl"
                got.add((t, pred, succ))
        need = {(t, p, s) for t in longs for p in LONG_PREDS for s in LONG_SUCCS}
        c.update({"long_symbols": len(longs), "long_codeword_lengths": sorted({code_len(L, t) for t in longs}), "contexts_needed": len(need),
                  "contexts_seen": len(got & need)})
        assert need <= got and c["long_codeword_lengths"][0] == 12 and c["long_codeword_lengths"][-1] == 16, (name, c)
    elif fam == "values":
        blk, pos, run, size = EB.walk(zz)
        per = np.bincount(blk, minlength=N)
        c.update({"ac_symbols": len({(r, s) for r, s in zip(run.tolist(), size.tolist()) if r < 16}), "ac_per_block": [int(per.min()), int(per.max())]})
        vals = zz[blk, pos]
        assert c["ac_symbols"] == len(ac_symbols(L)) == 160 and c["ac_per_block"] == [1, 3], (name, c)
        assert all(int(v) in EB.symbol_values(int(s)) for v, s in zip(vals, size)), name
    elif fam == "spikes":
        R = c["range_rule"]
        covered = {str(r): int(np.maximum(ends // r - (starts + r - 1) // r, 0).max()) for r in RANGES}
        where = np.nonzero(bits > 8)[0]
        c.update({"spikes": [[int(b), int(bits[b])] for b in where], "whole_ranges_one_block_covers": covered,
                  "small_blocks": sorted(set(bits[bits <= 8].tolist()))})
        assert set(bits[where].tolist()) <= set(SPIKE_BITS) and c["small_blocks"] == [6, 8], (name, c)
        if name == "spikes_sparse":
            assert R == 288 and 7 <= c["bits_per_block"] < 72 and covered["288"] == 5 and set(bits[where].tolist()) == set(SPIKE_BITS), (name, c)
            w = set(where.tolist())
            assert {0, N - 1} <= w and all({m - 1, m, m + 1} <= w for m in range(256, N, 256)), (name, c)
            assert sum(1 for b in w if b + 1 in w and b - 1 not in w and b + 2 not in w and b % 256 not in (255, 0)) >= 2, (name, c)
        else:
            assert R == 1056 and nbytes * 8 < 7 * N and covered["1056"] >= (1 if name == "spikes_flat_one" else 0), (name, c)
    elif fam == "cap" or name == "zeros":
        most = {str(r): [int(np.bincount(starts // r).max()), cap_of(r)] for r in RANGES}
        c["block_starts_in_one_range"] = most
        assert all(most[str(r)][0] == r // 6 <= cap_of(r) for r in RANGES), (name, c)
        assert set(bits.tolist()) == ({6, 8} if fam == "cap" else {6}) and not zz[:, 1:].any(), (name, c)
        if fam == "cap":
            assert not c["periodic"] and (bits[336:] == 8).sum() > 300, (name, c)
    elif fam == "dc_bounds":
        top = 32767 if "pos" in name else -32768
        run = zz[:, 0]
        c["blocks_at_the_bound"] = int((run == top).sum())
        c["blocks_beyond_int16"] = int(((run > 32767) | (run < -32768)).sum())
        if is_twin(name):
            assert c["blocks_beyond_int16"] == 1 and run[1024] == top + (1 if top > 0 else -1) and c["blocks_at_the_bound"] == 2, (name, c)
        else:
            assert c["blocks_beyond_int16"] == 0 and c["blocks_at_the_bound"] == 3 and (run[1023:1026] == top).all(), (name, c)
        assert np.abs(np.delete(run, np.arange(1007, 1043))).max() <= 2047, (name, c)
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# visibility: would a wrong coefficient change a pixel of the oracle's?
# ---------------------------------------------------------------------------------------------------------------------------------
def block_pixels(fx, O, rows, variant):
    """uint8 [m, 64]: the oracle's pixels of single blocks (its divisors and block_idct, codec.py:55-70) from int64 rows [m, 64]."""
    flag, q = variant
    x = np.ascontiguousarray(IE.dequantised(fx, O, rows, q, flag), dtype=np.float64)
    out = np.empty_like(x)
    f, P = O.lib().tico_block_idct, C.POINTER(C.c_double)
    a, b = x.ctypes.data, out.ctypes.data
    for i in range(x.shape[0]):
        f(C.cast(a + 512 * i, P), C.cast(b + 512 * i, P))
    return np.clip(out.reshape(-1, 64) + 128, 0, 255).astype(np.uint8)


def sensitive_first(variants):
    return sorted(variants, key=lambda v: (v[0] != 0, -v[1]))


def visibility(fx, O, fr, seed=9):
    """Per class of mutation [seen, of] over the frame's non-zero AC coefficients (a seeded sample of 20,000 beyond that); the class
    `one` split at size 4.  A mutation is seen when the block's pixels change under at least one of the frame's variants."""
    zz = fr["zz"].astype(np.int64)
    blk, col = np.nonzero(zz[:, 1:])
    pos = col + 1
    if len(blk) > SAMPLE:
        pick = np.sort(np.random.default_rng(seed).choice(len(blk), SAMPLE, replace=False))
        blk, pos = blk[pick], pos[pick]
    v = zz[blk, pos]
    mag, sgn, size = np.abs(v), np.sign(v), EB.size_of(v)
    k = np.arange(len(blk))
    out = {}
    order = sensitive_first(fr["variants"])
    base = {key(va): block_pixels(fx, O, zz, va) for va in order}
    movable = (pos < 63) & (zz[blk, np.minimum(pos + 1, 63)] == 0)
    for cls in CLASSES:
        rows = zz[blk].copy()
        use = np.ones(len(blk), bool)
        if cls == "sign":
            rows[k, pos] = -v
        elif cls == "half":
            rows[k, pos] = sgn * (mag >> 1)
        elif cls == "top_bit":
            rows[k, pos] = sgn * (mag - (1 << (size - 1)))
        elif cls == "one":
            rows[k, pos] = sgn * (mag - 1)
        else:
            use = movable
            rows[k[use], pos[use] + 1] = v[use]
            rows[k[use], pos[use]] = 0
        seen = np.zeros(len(blk), bool)
        for va in order:
            todo = np.nonzero(use & ~seen)[0]
            if not len(todo):
                break
            px = block_pixels(fx, O, rows[todo], va)
            seen[todo] = (px != base[key(va)][blk[todo]]).any(1)
        if cls == "one":
            small = size <= 4
            out["one_sizes_1_4"] = [int(seen[small].sum()), int(small.sum())]
            out["one_sizes_5_10"] = [int(seen[~small].sum()), int((~small).sum())]
        else:
            out[cls] = [int(seen[use].sum()), int(use.sum())]
    return out


def dc_visibility(fx, O, fr, variant=(0, 5)):
    """[seen, of] over both signs and all blocks: a DC difference changed by +-1 at block b moves the DC of every block from b on; it is
    seen when a pixel of any of them changes under `variant`."""
    zz = fr["zz"].astype(np.int64)
    assert [int(x) for x in variant] in [list(v) for v in fr["variants"]]
    base = block_pixels(fx, O, zz, variant)
    seen = 0
    for step in (1, -1):
        rows = zz.copy()
        rows[:, 0] += step
        changed = (block_pixels(fx, O, rows, variant) != base).any(1)
        seen += int(np.logical_or.accumulate(changed[::-1])[::-1].sum())  # any block from b on
    return [seen, 2 * len(zz)]


# ---------------------------------------------------------------------------------------------------------------------------------
def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def first_difference(got, want, w=W):
    """For a failure message: how many pixels differ, the first one and its block."""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    if not len(bad):
        return "no pixel differs"
    y, x = (int(t) for t in bad[0])
    return "%d pixels differ, first at (%d, %d): got %d, want %d, block %d" % (len(bad), y, x, got[y, x], want[y, x], (y // 8) * ((w + 7) // 8) + x // 8)


BARRED = ("sign", "half", "top_bit", "position", "one_sizes_1_4")  # `one_sizes_5_10` and every class on the other frames: figures only


def check_bars(name, v):
    """The value-bearing frames' bars: every mutation of these classes changes a pixel of the oracle's under some variant."""
    for cls in BARRED:
        assert v[cls][1] > 0 and v[cls][0] == v[cls][1], (name, cls, v[cls])
