"""Shared by tests/test_adaptive_tables_cpu.py, tests/test_adaptive_tables_gpu.py and tests/golden/gen/make_goldens_adaptive_tables.py:
streams with HAND-BUILT embedded Huffman tables for the device decoder of per-image table streams (tinyimgcodec_amd/csrc/
tic_adaptive_dec_gpu.hip: lookup, value_of, walk_block, the stitch rounds, the descriptor form), plain Python models of what that decoder
computes, and the fixture tests/golden/adaptive_tables.json with what the unmodified reference wrote for each stream.  No test lives here.

A table is {"DC": [(category, code01), ...], "AC": [((run, size), code01), ...]} in stream order; a frame is int16 [n, 64] in zig-zag
order with the ABSOLUTE DC in column 0.

  write_stream    make_header + write_huffman_table + encode_huffman (codec.py:73-84, 102-114, huffman.py:41-63) for a given table
  decode_model    the plain reference of the operation: bit-serial, a dict look-up of growing prefixes up to 64 bits, read_int,
                  decode_run_length, np.cumsum.  (The reference's own read_huffman_code stops at 17 bits and its decompress() misreads
                  the flag - tests/golden/gen/make_goldens_adaptive.py - so this model is pinned by the fixture: the reference WROTE every
                  stream, and for tables of at most 16-bit codes its own reader read it back.)
  lut_model, lookup_model   the rule of adaptive_dec_tab_build's comment (tic_adaptive.h) and of lookup(): an 11-bit primary table, 0 where
                  the window starts a longer code or none, the longer codes left-aligned in 64 bits in ascending order, the last one not
                  above the window, its prefix confirmed
  stitch_model    the rounds of the stitch, written from the header comment of tic_adaptive_dec_gpu.hip: a lane per range of
                  range_rule() bits, re-walks inside a workgroup of 256 ranges until no exit of it moves, the workgroup's first lane takes
                  its entry from the round before, two exit buffers swapped by round parity; the incidents (a window without a code:
                  next = p + 1; more than 63 AC entries: next = the bit behind the entry; past the end: exit = total bits).  It returns
                  (range_bits, nranges, changed[]): changed[0] is 1 by the kernel's convention, changed[r] the exits round r left
                  different from the round before, and the list ends with the first 0.

Families (build_cases): boundary, all_long, order, incomplete, widest_eob / widest_zrl, max_table, max_distinct_table, too_wide, damaged_chain and rounds_*;
the docstrings of the builders say what each reaches, census() counts it from the tables and coefficients alone.
DAMAGED tables and payloads - one seeded corpus through every decoder route, pinned on the reference's own reader - are
tests/damaged_adaptive.py's (it takes its bases `incomplete` and `all_long` and its stream writer from here); damaged_chain is the one case of that kind kept here.

max_table: kAdaptMaxTableBytes (2,610) is 32 + 16 x 23 + 256 x 80 bits, an AC entry of 16 + 64 bits 256 times.  The parser asks for a prefix
code and for code + value bits of at most 64; it does not ask for distinct symbols.  So a table reaches that length with entries of size
0 under 64-bit codes - the sixteen (run, 0) bytes, each many times - and max_table is such a table: 252 of them, four symbols with a
value, a 14-bit DC code, 20,874 bits in 2,610 bytes, the payload starting inside a byte.  The reference holds a table as a dict of
bidicts, one code per symbol, so its make_header cannot be given this one: write_stream alone writes it (a symbol is coded with the LAST
of its entries) and the reference's encode_huffman confirms the payload bits.  No table with DISTINCT symbols is longer than 32 + 368 +
20,480 - 16 x 120 = 18,960 bits = 2,370 bytes (the entry of a symbol of size s has at most 16 + 64 - s bits, every size sixteen times);
max_distinct_table holds that table less one bit, every one of the 256 symbols exactly 64 bits wide, written by the reference.

The value-bearing families (VALUE_CASES) keep to the visibility rule of tests/decoder_streams.py - the sizes inside a block span at most 5,
the DC lies within +-20, the header qualities are its VALUE_QUALITIES - and visibility() measures, with the oracle's divisors and
block_idct, that a wrong sign, top bit, lowest bit or position of a coefficient changes a pixel under at least one of those qualities.
"""
import bisect
import hashlib
import json
import os
import struct

import numpy as np

import decoder_streams as DS
import entropy_blocks as EB

GOLDEN = EB.GOLDEN
FIXTURE = os.path.join(GOLDEN, "adaptive_tables.json")
K = 11                    # kAdaptDecK
LANES = 256               # lanes of a workgroup of the range grid
MAX_ROUNDS = 512          # kAdaptDecMaxRounds
BATCH_ROUNDS = 19         # kAdaptBatchRounds
MAX_SYMBOL_BITS = 64      # kAdaptMaxSymbolBits
MAX_TABLE_BYTES = (32 + 16 * 23 + 256 * 80 + 7) // 8  # kAdaptMaxTableBytes
MAX_DISTINCT_TABLE_BITS = 32 + 16 * 23 + 256 * 80 - 16 * sum(range(16))
M64 = (1 << 64) - 1
EOB, ZRL = (0, 0), (15, 0)
QUALITIES = DS.VALUE_QUALITIES
VALUE_CASES = ("boundary", "all_long", "order", "incomplete", "widest_eob", "widest_zrl")
ROUNDS = {"rounds_early": (26, None), "rounds_few": (25, None), "rounds_mid": (27, 7160), "rounds_late": (29, None)}  # name -> (k, blocks kept)


SETTLES = {"rounds_early": (1, 2), "rounds_few": (3, 6), "rounds_mid": (10, 18), "rounds_late": (19, 63)}  # the round of the first 0 of changed[]


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def check_settles(name, changed):
    lo, hi = SETTLES[name]
    assert changed[0] == 1 and changed[-1] == 0 and 0 not in changed[:-1] and lo <= len(changed) - 1 <= hi, (name, changed)


def parts_of(name):
    return ("small", "large") if name.startswith("widest") else ("all",)


class NoCode(ValueError):
    pass


# ---------------------------------------------------------------------------------------------------------------------------------
# the stream writer and the bit-serial reader
# ---------------------------------------------------------------------------------------------------------------------------------
def value_bits(v, size):
    """BitBuffer.write of encode_huffman's value bits: the magnitude, inverted (one's complement) for a negative value."""
    if size == 0:
        return ""
    return format(v if v > 0 else (-v) ^ ((1 << size) - 1), "0%db" % size)


def table_bits(table):
    out = [format(len(table["DC"]), "016b")]
    for cat, code in table["DC"]:
        out.append(format(cat, "04b") + format(len(code), "04b") + code)
    out.append(format(len(table["AC"]), "016b"))
    for (r, s), code in table["AC"]:
        out.append(format(r, "04b") + format(s, "04b") + format(len(code), "08b") + code)
    return "".join(out)


def write_stream(table, zz, h, w, q):
    """(Where a table holds a symbol more than once, the symbol is coded with the last of its entries.)"""
    dcc, acc = dict(table["DC"]), dict(table["AC"])
    out, prev = [table_bits(table)], 0
    for row in np.asarray(zz, np.int64):
        d, prev = int(row[0]) - prev, int(row[0])
        c = abs(d).bit_length()
        out += [dcc[c], value_bits(d, c)]
        for r, s, v in DS.block_symbols(row):
            out += [acc[(r, s)], value_bits(v, s)]
    bits = "".join(out)
    bits += "0" * (-len(bits) % 8)
    return struct.pack("<III", h, w, q) + struct.pack(">I", 1 << 31) + int(bits, 2).to_bytes(len(bits) // 8, "big")


def with_quality(stream, q):
    return stream[:8] + struct.pack("<I", q) + stream[12:]


def bit_string(stream):
    return bin(int.from_bytes(stream, "big") | (1 << (8 * len(stream))))[3:]


def parse(stream):
    """-> (h, w, q, table, payload_bit) as read_huffman_table reads the stream."""
    h, w, q = struct.unpack("<III", stream[:12])
    assert struct.unpack(">I", stream[12:16])[0] == 1 << 31
    bits = bit_string(stream[: 16 + MAX_TABLE_BYTES + 8])
    p = 128
    table = {"DC": [], "AC": []}
    ndc = int(bits[p : p + 16], 2)
    p += 16
    for _ in range(ndc):
        cat, n = int(bits[p : p + 4], 2), int(bits[p + 4 : p + 8], 2)
        table["DC"].append((cat, bits[p + 8 : p + 8 + n]))
        p += 8 + n
    nac = int(bits[p : p + 16], 2)
    p += 16
    for _ in range(nac):
        r, s, n = int(bits[p : p + 4], 2), int(bits[p + 4 : p + 8], 2), int(bits[p + 8 : p + 16], 2)
        table["AC"].append(((r, s), bits[p + 16 : p + 16 + n]))
        p += 16 + n
    return h, w, q, table, p


def blocks_of(h, w):
    return (h + 7) // 8 * ((w + 7) // 8)


def read_code(bits, p, inverse):
    """read_huffman_code without its 17-bit stop: the symbol of the first prefix that is a code, and the bit behind it."""
    for n in range(1, MAX_SYMBOL_BITS + 1):
        if p + n > len(bits):
            raise ValueError("stream truncated")
        sym = inverse.get(bits[p : p + n])
        if sym is not None:
            return sym, p + n
    raise NoCode("a window without a code at bit %d" % p)


def read_int(bits, p, size):
    """BitBuffer.read_int (bitbuffer.py:56-66)."""
    if size == 0:
        return 0, p
    if p + size > len(bits):
        raise ValueError("stream truncated")
    v = int(bits[p : p + size], 2)
    return (v if bits[p] == "1" else -(v ^ ((1 << size) - 1))), p + size


def decode_model(stream):
    h, w, q, table, p = parse(stream)
    bits = bit_string(stream)
    dci = {code: cat for cat, code in table["DC"]}
    aci = {code: sym for sym, code in table["AC"]}
    n = blocks_of(h, w)
    dc, zz = np.zeros(n, np.int64), np.zeros((n, 64), np.int64)
    for b in range(n):
        cat, p = read_code(bits, p, dci)
        dc[b], p = read_int(bits, p, cat)
        pos = 1
        while True:
            (run, size), p = read_code(bits, p, aci)
            v, p = read_int(bits, p, size)
            if (run, size) == EOB:
                break
            pos += run
            if pos > 63:
                raise ValueError("block of more than 63 AC coefficients")
            zz[b, pos] = v
            pos += 1
    zz[:, 0] = np.cumsum(dc)
    if zz[:, 0].min() < -32768 or zz[:, 0].max() > 32767:
        raise ValueError("DC outside int16")
    return zz.astype(np.int16)


# ---------------------------------------------------------------------------------------------------------------------------------
# the look-up tables of the device decoder
# ---------------------------------------------------------------------------------------------------------------------------------
def lut_model(table):
    """-> {"DC" / "AC": {"prim": 2,048 entries (length, symbol byte) or None, "codes": ascending left-aligned long codes, "ls": their
    (length, symbol byte)}}."""
    out = {}
    for key in ("DC", "AC"):
        prim, longs = [None] * (1 << K), []
        for sym, code in table[key]:
            s, n, c = (sym if key == "DC" else (sym[0] << 4) | sym[1]), len(code), int(code, 2)
            if n <= K:
                first = c << (K - n)
                for j in range(1 << (K - n)):
                    prim[first + j] = (n, s)
            else:
                longs.append((c << (64 - n), n, s))
        longs.sort()
        out[key] = {"prim": prim, "codes": [x[0] for x in longs], "ls": [(x[1], x[2]) for x in longs]}
    return out


def lookup_model(lut, win):
    """(length, symbol byte) of the code the 64-bit window starts with, or None."""
    e = lut["prim"][win >> (64 - K)]
    if e:
        return e
    i = bisect.bisect_right(lut["codes"], win)
    if i == 0:
        return None
    n, s = lut["ls"][i - 1]
    return (n, s) if (lut["codes"][i - 1] ^ win) >> (64 - n) == 0 else None


def range_rule(stream_bytes, payload_bit, nblocks):
    """adaptive_dec_range_rule: two average blocks, 256 bits at least, 4,096 at most."""
    return min(max(2 * (stream_bytes * 8 - payload_bit) // max(nblocks, 1), 256), 4096)


# ---------------------------------------------------------------------------------------------------------------------------------
# the stitch
# ---------------------------------------------------------------------------------------------------------------------------------
OK, INCIDENT, END = 0, 1, 2


class Walker:
    """walk_block and walk_range over one stream: windows of 64 bits with zeros behind the stream's end."""

    def __init__(self, stream, table):
        self.data = bytes(stream) + bytes(24)
        self.total = len(stream) * 8
        lut = lut_model(table)
        self.dc, self.ac = lut["DC"], lut["AC"]
        self.memo = {}
        self.nocode = set()  # block starts whose walk met a window without a code

    def window(self, p):
        b = p >> 3
        return (int.from_bytes(self.data[b : b + 9], "big") >> (8 - (p & 7))) & M64

    def block(self, p):
        """-> (OK / INCIDENT / END, the bit the walk goes on from)."""
        r = self.memo.get(p)
        if r is None:
            r = self.memo[p] = self.block_(p)
        return r

    def block_(self, p0):
        p = p0
        e = lookup_model(self.dc, self.window(p))
        if e is None:
            self.nocode.add(p0)
            return (END if p + 1 > self.total else INCIDENT), p + 1
        if p + e[0] + e[1] > self.total:
            return END, p
        p += e[0] + e[1]
        pos = 1
        while True:
            e = lookup_model(self.ac, self.window(p))
            if e is None:
                self.nocode.add(p0)
                return (END if p + 1 > self.total else INCIDENT), p + 1
            n, sym = e
            if p + n + (sym & 15) > self.total:
                return END, p
            p += n + (sym & 15)
            if sym == 0:
                return OK, p
            pos += sym >> 4
            if pos > 63:
                return INCIDENT, p
            pos += 1

    def range(self, entry, limit):
        """-> (exit, blocks counted, blocks whole before the first incident or None)."""
        p, cnt, bad = entry, 0, None
        while p < limit:
            r, nxt = self.block(p)
            if r == END:
                if bad is None:
                    bad = cnt
                p = self.total
                break
            if r == INCIDENT:
                if bad is None:
                    bad = cnt
            else:
                cnt += 1
            p = nxt
        return p, cnt, bad


def stitch_model(stream, census=None, max_rounds=MAX_ROUNDS):
    """-> (range_bits, nranges, changed[]).  census (a dict): receives "nocode_out_of_step_round0", the first walks of round 0 that do
    not start on the true chain and meet a window without a code, and "chain_incident", whether the true chain meets an incident or the
    stream's end before block N."""
    h, w, q, table, base = parse(stream)
    n = blocks_of(h, w)
    W = Walker(stream, table)
    rb = range_rule(len(stream), base, n)
    nr = (W.total - base + rb - 1) // rb
    limit = [W.total if t + 1 == nr else base + (t + 1) * rb for t in range(nr)]
    buf = [[0] * nr, [0] * nr]
    frm = [None] * nr
    changed = []
    if census is not None:
        chain, p, bad = set(), base, False
        while len(chain) < n and p < W.total:
            chain.add(p)
            r, p = W.block(p)
            if r != OK:
                bad = True
                break
        census["chain_incident"] = bad or len(chain) < n
        hits = 0
        for t in range(nr):
            e = base + t * rb
            if e in chain:
                continue
            p = e
            while p < limit[t]:
                r, nxt = W.block(p)
                if p in W.nocode:
                    hits += 1
                    break
                if r == END:
                    break
                p = nxt
        census["nocode_out_of_step_round0"] = hits
    for rnd in range(max_rounds):
        src, dst = buf[(rnd & 1) ^ 1], buf[rnd & 1]
        moved = 0
        for g0 in range(0, nr, LANES):
            g1 = min(g0 + LANES, nr)
            if rnd == 0:
                entry = [base + t * rb for t in range(g0, g1)]
                x = [0] * (g1 - g0)
            else:
                entry = [base + g0 * rb if g0 == 0 else src[g0 - 1]] + src[g0 : g1 - 1]
                x = src[g0:g1]
            x0 = list(x)
            walked = [False] * (g1 - g0)
            active = [i for i in range(g1 - g0) if entry[i] != frm[g0 + i]]
            for it in range(LANES + 1):
                m = False
                for i in active:
                    nx = W.range(entry[i], limit[g0 + i])[0]
                    m |= True if (rnd == 0 and not walked[i]) else nx != x[i]
                    frm[g0 + i], x[i], walked[i] = entry[i], nx, True
                nxt = []
                for i in active:  # every lane but the first takes the exit in front of it: only these can have changed
                    if i + 1 < g1 - g0:
                        entry[i + 1] = x[i]
                        if entry[i + 1] != frm[g0 + i + 1]:
                            nxt.append(i + 1)
                if not m:
                    break
                active = nxt
            dst[g0:g1] = x
            if rnd:
                moved += sum(1 for a, b in zip(x, x0) if a != b)
        changed.append(1 if rnd == 0 else moved)
        if changed[-1] == 0:
            break
    return rb, nr, changed


# ---------------------------------------------------------------------------------------------------------------------------------
# codes
# ---------------------------------------------------------------------------------------------------------------------------------
def canonical(symbols_lengths, prefix=""):
    """A prefix code under `prefix`: codes in ascending order of length, each the next free value (tree order)."""
    out, code, last = {}, 0, None
    for sym, n in sorted(symbols_lengths, key=lambda x: x[1]):
        m = n - len(prefix)
        assert m >= 1
        if last is not None:
            code = (code + 1) << (m - last)
        assert code < (1 << m), (sym, n)
        out[sym] = prefix + format(code, "0%db" % m)
        last = m
    return out


def tagged(rng, symbols_lengths, tag_bits, prefix=""):
    """A prefix code under `prefix`: a distinct tag of `tag_bits` bits per symbol (in a seeded order), then seeded bits up to its
    length - prefix-free by the tags, spread over the whole code space, with no order between length and value."""
    tags = rng.permutation(1 << tag_bits)[: len(symbols_lengths)]
    assert len(tags) == len(symbols_lengths)
    out = {}
    for (sym, n), t in zip(symbols_lengths, tags):
        m = n - len(prefix) - tag_bits
        assert m >= 0, (sym, n)
        tail = "".join("01"[int(b)] for b in rng.integers(0, 2, m))
        out[sym] = prefix + format(int(t), "0%db" % tag_bits) + tail
    return out


def is_prefix_free(codes):
    s = sorted(codes)
    return all(not b.startswith(a) for a, b in zip(s, s[1:])) and len(set(s)) == len(s)


def kraft(codes):
    return sum(2.0 ** -len(c) for c in codes)


def entries(code, order=None):
    keys = list(code) if order is None else order
    return [(k, code[k]) for k in keys]


def extreme(rng, s):
    vals = EB.symbol_values(s)
    return vals[int(rng.integers(0, len(vals)))]


def frame_of(blocks, dcs):
    """int16 [n, 64] from lists of (run, size, value) symbols (a ZRL is (15, 0, 0)) and the absolute DCs."""
    zz = np.zeros((len(blocks), 64), np.int64)
    for row, syms in zip(zz, blocks):
        assert DS.place(row, syms), syms
    zz[:, 0] = dcs
    assert np.abs(zz).max() <= 32767
    return zz.astype(np.int16)


def sides(n):
    r = next(r for r in (8, 4, 2, 1) if n % r == 0)
    return 8 * r, 8 * (n // r)


SMALL_DC = {0: "0", 1: "10", 2: "110", 3: "111"}  # the DC differences of DS.small_dc are -6 .. 6 at the clamp: categories 0 .. 3


# ---------------------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------------------
BOUNDARY_SYMS = {10: [(0, 3), (1, 2), (2, 1)], 11: [(0, 4), (1, 3), (2, 2)], 12: [(0, 5), (1, 4), (2, 3)], 13: [(3, 1), (3, 2), (1, 5)]}


def boundary_case():
    """AC codes of 10, 11, 12 and 13 bits around the 11-bit primary table, numerically next to each other (tree order under "11"): every
    11- and 12-bit code is the first look-up behind the DC and stands behind every other one, and starts at all 32 residues of the bit
    position mod 32."""
    rng = np.random.default_rng(3101)
    ac = {EOB: "00", (0, 1): "010", (0, 2): "011", (1, 1): "100", (2, 4): "1010"}
    ac.update(canonical([(y, n) for n, ys in BOUNDARY_SYMS.items() for y in ys], "11"))
    table = {"DC": entries(SMALL_DC), "AC": entries(ac)}
    mid = BOUNDARY_SYMS[11] + BOUNDARY_SYMS[12]
    fillers = [(0, 1), (0, 2), (1, 1), (2, 4)]
    outer = BOUNDARY_SYMS[10] + BOUNDARY_SYMS[13]

    def val(y):
        return y + (extreme(rng, y[1]),)

    blocks = [[val(a), val(b)] for a in mid for b in mid]
    blocks += [[val(o), val(a), val(p)] for a in mid for o, p in zip(outer, outer[::-1])]
    for _ in range(760 - len(blocks)):
        syms = [val(fillers[int(rng.integers(0, 4))]) for _ in range(int(rng.integers(0, 4)))]
        for _ in range(int(rng.integers(1, 4))):
            syms.append(val(mid[int(rng.integers(0, 6))]))
            if rng.random() < 0.3:
                syms.append(val(fillers[int(rng.integers(0, 4))]))
        blocks.append(syms)
    blocks = [blocks[i] for i in rng.permutation(len(blocks))]
    return table, frame_of(blocks, DS.small_dc(rng, len(blocks)))


def all_symbols():
    return [(r, s) for r in range(16) for s in range(16)]


def standard_symbols():
    return [(r, s) for r in range(16) for s in range(1, 11)] + [EOB, ZRL]


FULL_DC = {c: "1" * c + "0" for c in range(15)}
FULL_DC[15] = "1" * 15  # a complete code: lengths 1 .. 15, the categories 14 and 15 at 15 bits


def all_long_case():
    """256 AC entries - every (run, size) byte value - of 12 .. 16 bits: the long list is full and the primary AC table all escapes; 16 DC
    entries of 1 .. 15 bits; the entries in a shuffled stream order.  The payload holds every standard symbol."""
    rng = np.random.default_rng(3202)
    syms = all_symbols()
    ac = tagged(rng, [(y, 12 + i % 5) for i, y in enumerate(syms)], 8)
    table = {"DC": entries(FULL_DC, [int(i) for i in rng.permutation(16)]), "AC": entries(ac, [syms[i] for i in rng.permutation(256)])}
    std = [y for y in standard_symbols() if y not in (EOB, ZRL)]
    order = [std[i] for i in rng.permutation(len(std))]
    blocks = []
    for b in range(420):
        first = order[b] if b < len(order) else std[int(rng.integers(0, len(std)))]
        lo = int(rng.integers(max(1, first[1] - 4), min(first[1], 6) + 1))
        syms_b, p = [], 1
        for k in range(int(rng.integers(1, 5))):
            r, s = first if k == 0 else (int(rng.integers(0, 16)), int(rng.integers(lo, min(lo + 4, 10) + 1)))
            if k and rng.random() < 0.25 and p + 16 + r <= 63:
                syms_b.append((15, 0, 0))
                p += 16
            if p + r > 63:
                break
            syms_b.append((r, s, extreme(rng, s)))
            p += r + 1
        blocks.append(syms_b)
    return table, frame_of(blocks, DS.small_dc(rng, len(blocks)))


def order_case():
    """Long codes numerically below ("0000..."), between ("0111...") and above ("1111...") the short ones ("010", "0110", "10", "110",
    "1110"): the lengths are not monotone in the code value, and the long list's order is not the table's."""
    rng = np.random.default_rng(3303)
    ac = {EOB: "10", (0, 1): "110", (0, 2): "1110", (1, 1): "010", (0, 3): "0110"}
    ac.update(tagged(rng, [((0, 4), 13), ((1, 2), 16), ((2, 1), 14), ((3, 3), 15)], 2, "0000"))
    ac.update(tagged(rng, [((0, 5), 14), ((1, 3), 12), ((2, 2), 13)], 2, "0111"))
    ac.update(tagged(rng, [((1, 4), 20), ((4, 1), 12), ((2, 5), 16)], 2, "1111"))
    keys = list(ac)
    table = {"DC": entries(SMALL_DC), "AC": entries(ac, [keys[i] for i in rng.permutation(len(keys))])}
    body = [y for y in keys if y != EOB]
    blocks = [[y + (v,)] for y in body for v in EB.symbol_values(y[1])]
    blocks += [[a + (extreme(rng, a[1]),), b + (extreme(rng, b[1]),)] for a in body for b in body]
    for _ in range(400 - len(blocks)):
        blocks.append([y + (extreme(rng, y[1]),) for y in (body[int(rng.integers(0, len(body)))] for _ in range(int(rng.integers(1, 6))))])
    blocks = [blocks[i] for i in rng.permutation(len(blocks))]
    return table, frame_of(blocks, DS.small_dc(rng, len(blocks)))


INCOMPLETE_DC = {0: "00", 1: "010", 2: "0110", 3: "01110"}
INCOMPLETE_AC = {EOB: "000", (0, 1): "0010", (0, 2): "0011", (1, 1): "0100", (0, 3): "01010", (1, 2): "010110", (2, 1): "011000001101",
                 (0, 4): "0110100010011", (0, 5): "01101100100101"}


def incomplete_case():
    """Kraft sums of 0.47 (DC) and 0.36 (AC): no code starts with a 1, nor with many a pattern behind "011".  The chain is valid; the
    walks of round 0 that start out of step meet windows without a code."""
    rng = np.random.default_rng(3404)
    table = {"DC": entries(INCOMPLETE_DC), "AC": entries(INCOMPLETE_AC)}
    body = [y for y in INCOMPLETE_AC if y != EOB]
    blocks = [[y + (v,)] for y in body for v in EB.symbol_values(y[1])]
    for _ in range(400 - len(blocks)):
        blocks.append([y + (extreme(rng, y[1]),) for y in (body[int(rng.integers(0, len(body)))] for _ in range(int(rng.integers(1, 7))))])
    blocks = [blocks[i] for i in rng.permutation(len(blocks))]
    return table, frame_of(blocks, DS.small_dc(rng, len(blocks)))


WIDE_SMALL, WIDE_LARGE = (1, 2, 3, 4, 5), (11, 12, 13, 14, 15)
WIDEST_DC = {0: "00", 1: "010", 2: "011", 3: "100", 15: "110101010101011"}
WIDEST_FILL = {(1, 1): "0001", (1, 2): "0010", (1, 3): "0011"}
MAX_BLOCKS_AT = (40, 255, 384, 512)  # where the blocks of the maximal length stand, singly


def widest_case(which, too_wide=False):
    """AC symbols (0, s) for s = 1 .. 5 and 11 .. 15 whose code + value is exactly 64 bits (codes of 63 .. 59 and 53 .. 49 bits), and one
    symbol of size 0 with a 64-bit code: the EOB (which = "eob"; the other blocks are then 66 bits and more, a maximal block 30 + 63 x 64
    + 64 = 4,126 bits, longer than the 4,096-bit cap of a range) or the ZRL (which = "zrl"; the EOB is 4 bits, the blocks between the
    maximal ones 6 bits).  A DC entry of category 15 with a 15-bit code.  Blocks hold wide symbols of one group only: sizes 1 .. 5 with a
    DC within +-20, or sizes 11 .. 15.  The four maximal blocks stand alone behind a 30-bit DC, so all their pixels saturate: a wrong
    symbol LENGTH in them shows (it breaks the chain behind the block), a wrong value does not - the values of the 64-bit symbols of
    sizes 1 .. 5 are checked in the short blocks only (census: wide_symbols_of_sizes_1_5_in_value_checked_blocks).  too_wide: the code of (0, 5) one bit longer - 65 bits with its value."""
    rng = np.random.default_rng(3505)
    wide = [((0, s), 64 - s) for s in WIDE_SMALL + WIDE_LARGE]
    zero = EOB if which == "eob" else ZRL
    ac = {(ZRL if which == "eob" else EOB): "0000"}
    ac.update(WIDEST_FILL)
    ac.update(tagged(rng, wide + [(zero, 64)], 5, "1"))
    if too_wide:
        ac[(0, 5)] += "0"
    table = {"DC": entries(WIDEST_DC), "AC": entries(ac)}

    def val(s):
        return (0, s, extreme(rng, s))

    fill = list(WIDEST_FILL)
    blocks, big = [], []
    n = 640 if which == "eob" else 900
    for b in range(n):
        if b in MAX_BLOCKS_AT:
            blocks.append([val(int(s)) for s in rng.choice(WIDE_LARGE if len(big) % 2 == 0 else WIDE_SMALL, 63)])
            big.append(b)
            continue
        kind = rng.random()
        if kind < (0.55 if which == "zrl" else 0.2):
            blocks.append([])  # DC and EOB alone: 6 bits (66 with the wide EOB) at a DC difference of 0
            continue
        group = WIDE_SMALL if kind < 0.7 else WIDE_LARGE
        syms = []
        for _ in range(int(rng.integers(0, 3))):
            y = fill[int(rng.integers(0, 3))]
            syms.append(y + (extreme(rng, y[1]),))
        if group is WIDE_LARGE:
            # one symbol, of the least magnitudes of its size: its sign and top bit show in the pixels (a larger magnitude saturates every
            # pixel of the block with and without its top bit, at every quality)
            s = int(group[int(rng.integers(0, 5))])
            v = (1 << (s - 1)) + int(rng.integers(0, 2))
            syms = ([(15, 0, 0)] if rng.random() < 0.3 else []) + [(0, s, v if rng.random() < 0.5 else -v)]
        else:
            for _ in range(int(rng.integers(1, 4))):
                if rng.random() < 0.3:
                    syms.append((15, 0, 0))
                syms.append(val(int(group[int(rng.integers(0, 5))])))
        blocks.append(syms)
    dcs = DS.small_dc(rng, n)
    for b in [b for b in range(n) if not blocks[b]][::3]:
        dcs[b] = dcs[b - 1] if b else 0  # (a DC difference of 0: a 2-bit code)
    for k, b in enumerate(big):  # a DC difference of category 15 into the maximal block and one out of it
        dcs[b] = (1 if k % 2 == 0 else -1) * (17000 + 1000 * k + 7)
    return table, frame_of(blocks, dcs)


MAX_TABLE_VALUED = [(0, 1), (1, 1), (2, 1), (0, 2)]


def max_table_case():
    """A table of exactly kAdaptMaxTableBytes: 16 DC entries of 15 bits (one of 14) and 256 AC entries of 16 + 64 - size bits - 252 of
    size 0, the sixteen (run, 0) bytes under fifteen or sixteen distinct 64-bit codes each (a prefix code whose symbols repeat), and
    (0, 1), (1, 1), (2, 1), (0, 2) under 63- and 62-bit codes: 20,880 - 1 - 5 = 20,874 table bits, 2,610 bytes, and the payload starts
    inside a byte.  Every AC symbol is 64 bits with its value; the payload codes each symbol with the last of its entries."""
    rng = np.random.default_rng(3707)
    syms = MAX_TABLE_VALUED + [(i % 16, 0) for i in range(252)]
    syms = [syms[i] for i in rng.permutation(256)]
    dc = tagged(rng, [(c, 14 if c == 9 else 15) for c in range(16)], 4)
    ac = tagged(rng, [((i, y), 64 - y[1]) for i, y in enumerate(syms)], 8)
    table = {"DC": entries(dc), "AC": [(y, code) for (_, y), code in ac.items()]}
    blocks = []
    for b in range(200):
        syms_b, p = [], 1
        for _ in range(int(rng.integers(0, 5))):
            r, s = MAX_TABLE_VALUED[int(rng.integers(0, 4))]
            if rng.random() < 0.25 and p + 16 + r <= 63:
                syms_b.append((15, 0, 0))
                p += 16
            syms_b.append((r, s, extreme(rng, s)))
            p += r + 1
        blocks.append(syms_b)
    return table, frame_of(blocks, DS.small_dc(rng, len(blocks)))


def max_distinct_table_case():
    """16 DC entries of 15 bits (one of 14) and 256 AC entries of 64 - size bits, every (run, size) byte once: 18,959 table bits, the most
    a table with distinct symbols can have less one, in 2,370 bytes; the payload starts inside a byte.  Every AC symbol is 64 bits with
    its value."""
    rng = np.random.default_rng(3606)
    syms = all_symbols()
    dc = tagged(rng, [(c, 14 if c == 9 else 15) for c in range(16)], 4)
    ac = tagged(rng, [(y, 64 - y[1]) for y in syms], 8)
    table = {"DC": entries(dc), "AC": entries(ac, [syms[i] for i in rng.permutation(256)])}
    std = [y for y in standard_symbols() if y not in (EOB, ZRL) and y[1] <= 5]
    blocks = []
    for b in range(200):
        syms_b, p = [], 1
        for _ in range(int(rng.integers(0, 4))):
            r, s = std[int(rng.integers(0, len(std)))]
            if p + r > 63:
                break
            syms_b.append((r, s, extreme(rng, s)))
            p += r + 1
        blocks.append(syms_b)
    return table, frame_of(blocks, DS.small_dc(rng, len(blocks)))


def longcode_coeffs(k=33):
    """longcode_coeffs() of tests/golden/gen/make_goldens_adaptive.py restricted to its last k symbol kinds (k = 33: the long-code fixture
    itself): AC symbol j of them occurs F(j + 1) times (Fibonacci), blocks are filled in order.  The one copy the tests share
    (adaptive_decode_batch_common, test_adaptive_gpu, test_adaptive_decode_gpu), checked by the fixture's coeffs_sha256."""
    syms = ([(2, s) for s in (15, 14, 13)] + [(1, s) for s in range(15, 0, -1)] + [(0, s) for s in range(15, 0, -1)])[-k:]
    fib = [1, 1]
    while len(fib) < len(syms):
        fib.append(fib[-1] + fib[-2])
    bidx, spos, vals = [], [], []
    block, pos = 0, 1
    for (run, size), cnt in zip(syms, fib):
        width = run + 1
        here = (63 - run - pos) // width + 1 if pos + run <= 63 else 0
        per = (62 - run) // width + 1
        i = np.arange(cnt)
        later = np.maximum(i - here, 0)
        b = np.where(i < here, block, block + 1 + later // per)
        p = np.where(i < here, pos + i * width, 1 + (later % per) * width)
        v = (1 << (size - 1)) + (size > 1)
        bidx.append(b)
        spos.append(p + run)
        vals.append(np.where(i % 2 == 0, v, -v))
        block, pos = int(b[-1]), int(p[-1]) + width
    zz = np.zeros((block + 1, 64), np.int16)
    zz[np.concatenate(bidx), np.concatenate(spos)] = np.concatenate(vals)
    zz[:, 0] = (np.arange(zz.shape[0]) % 5) - 2
    return zz


def rounds_coeffs(name):
    k, keep = ROUNDS[name]
    zz = longcode_coeffs(k)
    return zz if keep is None else np.ascontiguousarray(zz[:keep])


def damage(stream):
    """The stream with the first payload bit flipped (from a quarter of the payload on) that makes the true chain meet a window without a
    code before block N -> (stream, bit)."""
    base = parse(stream)[4]
    for bit in range(base + (len(stream) * 8 - base) // 4, len(stream) * 8):
        b = bytearray(stream)
        b[bit >> 3] ^= 0x80 >> (bit & 7)
        try:
            decode_model(bytes(b))
        except NoCode:
            return bytes(b), bit
        except ValueError:
            pass
    raise AssertionError("no such bit")


def build_cases(fixture_tables=None):
    """name -> {"table", "zz", "h", "w", "qualities", "well_formed"} in a fixed order.  fixture_tables: name -> table for the rounds_*
    cases, whose tables are the reference's calc_huffman_table of their coefficients (the generator passes them; the tests take them from
    the fixture)."""
    cases = {}

    def add(name, table, zz, qualities=(50,), well_formed=True):
        h, w = sides(len(zz))
        cases[name] = {"table": table, "zz": zz, "h": h, "w": w, "qualities": list(qualities), "well_formed": well_formed}

    add("boundary", *boundary_case(), QUALITIES)
    add("all_long", *all_long_case(), QUALITIES)
    add("order", *order_case(), QUALITIES)
    add("incomplete", *incomplete_case(), QUALITIES)
    add("widest_eob", *widest_case("eob"), QUALITIES)
    add("widest_zrl", *widest_case("zrl"), QUALITIES)
    add("max_table", *max_table_case())
    add("max_distinct_table", *max_distinct_table_case())
    add("too_wide", *widest_case("zrl", too_wide=True), well_formed=False)
    add("damaged_chain", *incomplete_case(), well_formed=False)
    for name in ROUNDS:
        if fixture_tables is not None and name in fixture_tables:
            add(name, fixture_tables[name], rounds_coeffs(name))
    return cases


def stream_of(name, case, q=None):
    s = write_stream(case["table"], case["zz"], case["h"], case["w"], case["qualities"][0] if q is None else q)
    return damage(s)[0] if name == "damaged_chain" else s


def table_to_json(table):
    return {"DC": [[int(c), code] for c, code in table["DC"]], "AC": [[int(r), int(s), code] for (r, s), code in table["AC"]]}


def table_from_json(j):
    return {"DC": [(c, code) for c, code in j["DC"]], "AC": [((r, s), code) for r, s, code in j["AC"]]}


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def fixture_tables(fx):
    return {name: table_from_json(e["table"]) for name, e in fx["cases"].items() if "table" in e}


# ---------------------------------------------------------------------------------------------------------------------------------
# census: from the tables and coefficients alone
# ---------------------------------------------------------------------------------------------------------------------------------
def symbol_starts(table, zz):
    """[(block, "DC" or (run, size), first bit counted from the payload's first bit, code bits, value bits)] of every symbol."""
    dcc, acc = dict(table["DC"]), dict(table["AC"])
    out, p, prev = [], 0, 0
    for b, row in enumerate(np.asarray(zz, np.int64)):
        d, prev = int(row[0]) - prev, int(row[0])
        c = abs(d).bit_length()
        out.append((b, "DC", p, len(dcc[c]), c))
        p += len(dcc[c]) + c
        for r, s, v in DS.block_symbols(row):
            out.append((b, (r, s), p, len(acc[(r, s)]), s))
            p += len(acc[(r, s)]) + s
    return out, p


def census(name, case, stream=None):
    """Figures that show the case reaches its edge; asserts what its family promises.  `stream`: for the figures stitch_model gives."""
    table, zz = case["table"], case["zz"]
    dcodes, acodes = [c for _, c in table["DC"]], [c for _, c in table["AC"]]
    tbits = len(table_bits(table))
    starts, payload = symbol_starts(table, zz)
    base = 128 + tbits
    lut = lut_model(table)
    bits_of_block = np.diff([p for b, y, p, n, s in starts if y == "DC"] + [payload])
    c = {"blocks": int(len(zz)), "table_bits": tbits, "table_bytes": (tbits + 7) // 8, "payload_bit": base, "payload_bits": int(payload),
         "dc_entries": len(dcodes), "ac_entries": len(acodes), "nlong": [len(lut["DC"]["codes"]), len(lut["AC"]["codes"])],
         "kraft": [round(kraft(dcodes), 6), round(kraft(acodes), 6)], "max_code_bits": [max(map(len, dcodes)), max(map(len, acodes))],
         "max_symbol_bits": max(max(len(code) + cat for cat, code in table["DC"]), max(len(code) + y[1] for y, code in table["AC"])),
         "max_block_bits": int(bits_of_block.max()), "min_block_bits": int(bits_of_block.min()),
         "dc_min": int(zz[:, 0].min()), "dc_max": int(zz[:, 0].max())}
    assert is_prefix_free(dcodes) and is_prefix_free(acodes), name
    assert (c["max_symbol_bits"] <= MAX_SYMBOL_BITS) == (name != "too_wide"), (name, c)
    used = {y for b, y, p, n, s in starts if y != "DC"}
    if not name.startswith("rounds_"):  # (the hand-built payloads hold standard symbols and the wide ones only)
        assert used <= set(standard_symbols()) | {(0, s) for s in WIDE_LARGE}, name
    if name in VALUE_CASES:
        sizes = EB.size_of(zz[:, 1:].astype(np.int64))
        low = np.where(sizes > 0, sizes, 99).min(1)
        span = np.where(low == 99, 0, sizes.max(1) - low)
        c["blocks_spanning_more_than_5_sizes"] = int((span > 5).sum())
        assert c["blocks_spanning_more_than_5_sizes"] == 0, (name, c)
        if not name.startswith("widest"):
            assert max(abs(c["dc_min"]), abs(c["dc_max"])) <= 20, (name, c)
        else:
            assert np.abs(np.delete(zz[:, 0], MAX_BLOCKS_AT)).max() <= 20, (name, c)

    def residues(select):
        res = {}
        for b, y, p, n, s in starts:
            if y != "DC" and select(y, n, s):
                res.setdefault("%d,%d" % y, set()).add((base + p) % 32)
        return {k: len(v) for k, v in sorted(res.items())}

    if name == "boundary":
        first, behind = set(), set()
        for i, (b, y, p, n, s) in enumerate(starts):
            if y != "DC" and n in (11, 12):
                pb, py = starts[i - 1][0], starts[i - 1][1]
                if py == "DC":
                    first.add(y)
                elif pb == b and starts[i - 1][3] in (11, 12):
                    behind.add((py, y))
        mid = BOUNDARY_SYMS[11] + BOUNDARY_SYMS[12]
        c.update({"ac_code_lengths": sorted({len(x) for x in acodes}), "mid_codes_first_behind_the_dc": len(first), "mid_pairs": len(behind),
                  "residues_of_11_and_12_bit_codes": residues(lambda y, n, s: n in (11, 12))})
        assert {10, 11, 12, 13} <= set(c["ac_code_lengths"]) and first == set(mid) and behind == {(a, b) for a in mid for b in mid}, (name, c)
        assert len(c["residues_of_11_and_12_bit_codes"]) == 6 and set(c["residues_of_11_and_12_bit_codes"].values()) == {32}, (name, c)
        assert c["nlong"] == [0, 6], (name, c)
    elif name == "all_long":
        c.update({"ac_code_lengths": sorted({len(x) for x in acodes}), "primary_ac_entries": sum(e is not None for e in lut["AC"]["prim"]),
                  "standard_symbols_used": len(used), "dc_code_lengths": sorted(len(x) for x in dcodes)})
        assert c["nlong"] == [5, 256] and c["ac_entries"] == 256 and c["primary_ac_entries"] == 0 and c["ac_code_lengths"] == [12, 13, 14, 15, 16], (name, c)
        assert c["dc_entries"] == 16 and c["dc_code_lengths"][-2:] == [15, 15] and used >= set(standard_symbols()), (name, c)
        assert [y for y, _ in table["AC"]] != sorted(y for y, _ in table["AC"]) and {y for y, _ in table["AC"]} == set(all_symbols()), name
    elif name == "order":
        aligned = sorted((int(code, 2) << (64 - len(code)), len(code)) for code in acodes)
        lens = [n for _, n in aligned]
        short = [v for v, n in aligned if n <= K]
        longs = [v for v, n in aligned if n > K]
        c.update({"code_lengths_in_value_order": lens, "long_below_between_above": [sum(v < short[0] for v in longs),
                  sum(short[0] < v < short[-1] for v in longs), sum(v > short[-1] for v in longs)], "symbols_used": len(used)})
        assert min(c["long_below_between_above"]) >= 3 and lens != sorted(lens) and lens != sorted(lens, reverse=True), (name, c)
        assert used == {y for y, _ in table["AC"]}, (name, c)
    elif name in ("incomplete", "damaged_chain"):
        assert c["kraft"][0] < 0.5 and c["kraft"][1] < 0.5 and used == set(INCOMPLETE_AC), (name, c)
    elif name.startswith("widest") or name == "too_wide":
        wide = {y for y, code in table["AC"] if len(code) + y[1] >= 64}
        total = {"%d,%d" % y: len(code) + y[1] for y, code in table["AC"] if y in wide}
        seen = {g: {(base + p) % 32 for b, y, p, n, s in starts if y != "DC" and n + s >= 64 and (s >= 11) == (g == "sizes_11_15")} for g in ("sizes_0_5", "sizes_11_15")}
        c.update({"wide_symbol_bits": total, "residues_of_64_bit_symbols": {g: len(v) for g, v in seen.items()},
                  "residues_by_symbol": residues(lambda y, n, s: n + s >= 64),
                  "wide_symbols_of_sizes_11_15": sum(1 for b, y, p, n, s in starts if y != "DC" and s >= 11),
                  "wide_symbols_of_sizes_0_5": sum(1 for b, y, p, n, s in starts if y != "DC" and n + s >= 64 and s <= 5),
                  # the maximal blocks carry a DC of +-17,000 and more: every pixel of them saturates, so a wrong VALUE inside them cannot show
                  # (a wrong length does: it breaks the chain behind the block) - the values of the 64-bit symbols are checked in these:
                  "wide_symbols_of_sizes_1_5_in_value_checked_blocks": sum(1 for b, y, p, n, s in starts if y != "DC" and n + s >= 64 and 1 <= s <= 5 and b not in MAX_BLOCKS_AT),
                  "dc_category_15": sum(1 for b, y, p, n, s in starts if y == "DC" and s == 15), "blocks_of_63_wide_symbols": list(MAX_BLOCKS_AT)})
        assert len(wide) == 11 and c["dc_category_15"] >= 4 and dict(table["DC"])[15] == WIDEST_DC[15] and len(WIDEST_DC[15]) == 15, (name, c)
        if name != "too_wide":
            assert set(total.values()) == {64} and used >= wide, (name, c)
            assert {s for b, y, p, n, s in starts if y != "DC" and n + s >= 64 and b not in MAX_BLOCKS_AT} >= set(WIDE_SMALL), (name, c)
            assert set(c["residues_of_64_bit_symbols"].values()) == {32} and len(c["residues_by_symbol"]) == 11, (name, c)
            eob = len(dict(table["AC"])[EOB])
            assert c["max_block_bits"] == 30 + 63 * 64 + eob and (eob == 64) == (name == "widest_eob"), (name, c)
            assert c["min_block_bits"] == (66 if name == "widest_eob" else 6), (name, c)
            for b in MAX_BLOCKS_AT:
                assert bits_of_block[b] == c["max_block_bits"] and bits_of_block[b - 1] < 400 and bits_of_block[b + 1] < 400, (name, b)
        else:
            assert sorted(total.values())[-1] == 65 and sorted(total.values())[-2] == 64, (name, c)
    elif name == "max_table":
        c["distinct_ac_symbols"] = len({y for y, _ in table["AC"]})
        assert 8 * MAX_TABLE_BYTES - 8 < tbits < 8 * MAX_TABLE_BYTES and c["table_bytes"] == MAX_TABLE_BYTES > (MAX_DISTINCT_TABLE_BITS + 7) // 8, (name, c)
        assert base % 8 != 0 and (c["dc_entries"], c["ac_entries"]) == (16, 256) and c["nlong"] == [16, 256] and c["distinct_ac_symbols"] == 20, (name, c)
        assert all(len(code) + y[1] == 64 for y, code in table["AC"]) and used == set(MAX_TABLE_VALUED) | {EOB, ZRL}, name
    elif name == "max_distinct_table":
        assert tbits == MAX_DISTINCT_TABLE_BITS - 1 and c["table_bytes"] == (MAX_DISTINCT_TABLE_BITS + 7) // 8 < MAX_TABLE_BYTES, (name, c)
        assert base % 8 != 0 and (c["dc_entries"], c["ac_entries"]) == (16, 256) and c["nlong"] == [16, 256], (name, c)
        assert all(len(code) + y[1] == 64 for y, code in table["AC"]) and len({y for y, _ in table["AC"]}) == 256, name
    if stream is not None:
        st = {}
        rb, nr, changed = stitch_model(stream, st)
        c.update({"range_bits": rb, "nranges": nr, "changed": changed, "nocode_out_of_step_round0": st["nocode_out_of_step_round0"]})
        assert st["chain_incident"] == (name == "damaged_chain"), (name, c)
        if name in ("incomplete", "damaged_chain"):
            assert c["nocode_out_of_step_round0"] >= 1, (name, c)
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# visibility
# ---------------------------------------------------------------------------------------------------------------------------------
def visibility(ie, O, case, part="all"):
    """DS.visibility (the oracle's divisors and block_idct) over the blocks of the case - all of them, those whose AC sizes are all at
    most 5 and whose DC is within +-20 (part = "small"), or those with a size from 11 on and such a DC ("large": the blocks of the
    maximal length, whose DC saturates every pixel, are left out) - under the case's header qualities."""
    zz = case["zz"].astype(np.int64)
    sizes = EB.size_of(zz[:, 1:])
    pick = {"all": np.ones(len(zz), bool), "small": (sizes.max(1) <= 5) & (np.abs(zz[:, 0]) <= 20), "large": (sizes.max(1) >= 11) & (np.abs(zz[:, 0]) <= 20)}[part]
    return DS.visibility(ie, O, {"zz": zz[pick], "variants": [[0, q] for q in case["qualities"]]})


def check_bars(name, v, part="all"):
    for cls in (DS.BARRED if part != "large" else ("sign", "top_bit")):
        assert v[cls][1] > 0 and v[cls][0] == v[cls][1], (name, part, cls, v[cls])
