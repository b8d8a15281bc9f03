"""Shared by tests/test_damaged_adaptive_cpu.py, tests/test_damaged_adaptive_gpu.py and tests/golden/gen/make_goldens_damaged_adaptive.py:
ONE seeded corpus of damaged per-image-table ("adaptive") streams for every decoder route, a plain statement of the decoder's documented
contract (decode_strict), and the fixture tests/golden/damaged_adaptive.json.  No test lives here.  The twin of tests/damaged_streams.py
for the only decoder of this library that builds look-up tables for the GPU from untrusted bytes.

What decides the right answer (the generator's docstring has the details): the reference's decompress() misreads the flag of such a stream,
but it decodes the FLAG-SWAPPED TWIN (the flag word written little-endian) with its own table reader, and its reader functions can be run
step by step behind the 16 header bytes.  Both hold for tables IN REACH of that reader - every code 1..16 bits long, distinct symbols,
distinct codes - and the fixture says for every entry whether it is, what the reader did, and where the pixels come from.

decode_strict(stream) -> int16 [n, 64] zig-zag coefficients with the absolute DC, or StrictError (a ValueError) whose .cls is one of CLASSES,
written from the contract of tic_decompress_adaptive (include/tinyimgcodec_hip.h) and the reference's reader (codec.py:87-99,
huffman.py:66-98), in this order: `header` (shorter than 16 bytes, or bit 31 of the flag word as written most significant bit first is
clear); then the table front to back - `dc_count` / `ac_count` (outside 1..16 / 1..256), `table_truncated` (a count, an entry's fields or
its code behind the stream's end), `too_wide` (code + value bits above 64) - then `not_prefix` (DC, then AC: a code that is another's
prefix or equal; a code of length zero beside others); then the payload block by block - `no_code` (64 bits that start with no code),
`truncated` (a code or a value behind the stream's end), `over_63` (an entry past scan position 63), `dc_range` (the running DC outside
int16, checked as it runs: the header's "a running DC").  The one table a flat frame gives, a single code of length zero, is read as the
reference reads it: its symbol takes no bits.  adaptive_tables.decode_model is the same walk without the table checks and with the DC
range looked at behind the last block; the generator holds both against each other wherever both decode.

corpus(oracle, fixture) -> [(name, base, kind, params, stream bytes)], name = base/kind/tag, in a fixed order; every position comes from
a numpy generator seeded by base, kind and ordinal (damaged_streams._rng).

Bases (a base is adaptive_tables.write_stream(table, oracle.encode_zz16(frame, q), h, w, q) with the table the reference's
calc_huffman_table gave - stored in the fixture, codes only, beside the sha256 of the stream the reference's compress(...,
auto_generate_huffman_table=True) wrote; the frames are damaged_streams.base_frame's):
  lenna64         the 64 x 64 crop, q = 50: a table region of 590 bits, 12 ranges
  noise64         64 x 64 noise, q = 50: a 12-bit code, behind the 11-bit primary table
  ragged17x33     17 x 33 noise, q = 20: 15 blocks
  noise256        256 x 256 noise, q = 75: 1,024 blocks, 512 ranges = two workgroups; the shipped single call's device route takes it
  twolevel256     two grey levels, q = 75: 513 ranges = a third workgroup with one range
  twolevel256q90  the same frame, q = 90: a 17-bit code - outside the reference reader's reach on purpose
  incomplete, all_long   adaptive_tables.build_cases() at q = 50: Kraft sums below 1; every AC code behind the primary table

Kinds.  table_flip is exhaustive on lenna64 (every bit of the table region) and a seeded sample of 48 on every other base, stratified
over the nine fields of the table (FIELDS).  These 926 entries and the cap of 1,100 leave 174 for the other twelve kinds on eight bases,
so every base has every kind, and the VARIANTS of a kind rotate over the bases (plan() is the whole allotment, a table, not a sample):
  table_swap   sym_equal_size / sym_unequal_size (the symbols of two AC entries exchanged), dc_categories, codes_equal_length,
               repeat_last (the last AC entry once more under a free code, where the Kraft sum leaves one), reversed (both entry lists
               back to front).  params["keeps_lengths"]: every symbol keeps its code length and value bits, so the chain of block starts is
               the clean stream's and a device decoder has to finish the frame itself.  All five or six on lenna64, noise64, noise256
               and twolevel256
  value_flip   ac (the lowest value bit of one AC coefficient of size >= 2), dc (the sign bit of one DC difference in the first quarter
               of the frame, of the largest category found there or one less), found by walk() over the base's own table
  flip1/flip3  payload bits: seeded, first_payload_bit, last64, range (a multiple of range_rule() behind the payload's first bit), and on
               the 256 x 256 bases seam255 / seam256 / seam (inside ranges 255 and 256, the first workgroup's last and the second's first)
  cut          at16, at17, at18, in_dc, in_ac, payload_first, seeded, one_short; res0 .. res3 on noise256 (four
               consecutive payload lengths: every residue mod 4 - the resident route reads 32-bit words up to 3 bytes behind `len`)
  garbage, ones_tail, zeros_tail, delete, insert   as in damaged_streams.py, at a payload position or (tag "table") inside the table
               region; garbage/table overwrites four bytes there
  geometry     h+8, h-8, w+8, w-8, swapped, 8x8, h-1, w-3;   quality   q1, q99, q-1, q+1
  flag         zero, scaled (1 << 30), le (1 << 31 little-endian) - `header` refusals - and c0000000 (taken: only bit 31 is read)
  dc_run       (not damage a channel does, and not in the list this corpus was specified with: none of the 1,097 entries above reaches
               a running DC outside int16 - every walk that has left the chain ends in a window without a code or a block past
               position 63 first, and no frame of these sizes holds such a sum.)  _dc_runs(): blocks of the table's largest DC category
               with extreme value bits, put in front of a block start, so that the chain stays whole and the DC sum overflows inside
               them: on all_long (category 15), twolevel256 (in the first workgroup) and noise256 (in front of block 300: the overflow
               lies in a later workgroup's part of the DC sum, downwards)
"""
import json
import os
import struct

import numpy as np

import adaptive_tables as AT
import damaged_streams as D

GOLDEN = D.GOLDEN
FIXTURE = os.path.join(GOLDEN, "damaged_adaptive.json")
MAX_ENTRIES = 1100
MAX_FIXTURE_BYTES = 256 * 1024
MAX_BASE_BYTES = 64 * 1024
OUT_OF_REACH_MAX_PERCENT = 41   # of the decoded entries of the bases not in OUT_OF_REACH_BASES: measured 83 of 205 (71 of them flips of lenna64 that repeat a symbol)
CLASSES = ("header", "dc_count", "ac_count", "table_truncated", "too_wide", "not_prefix", "no_code", "truncated", "over_63", "dc_range")
TABLE_CLASSES = CLASSES[:6]     # what the table parser alone decides
STRICTER = ("not_prefix", "too_wide", "dc_count", "ac_count", "dc_range")  # where the product refuses what the reference's reader reads
KINDS = ("table_flip", "table_swap", "value_flip", "flip1", "flip3", "cut", "garbage", "ones_tail", "zeros_tail", "delete", "insert",
         "geometry", "quality", "flag", "dc_run")
DC_RUN_BASES = {"all_long": (0, 1), "noise256": (300, -1), "twolevel256": (0, 1)}  # base -> (the block the run stands in front of, sign)
FIELDS = ("dc_count", "dc_category", "dc_length", "dc_code", "ac_count", "run", "size", "ac_length", "ac_code")
SAMPLE = 48
# name -> (h, w, quality, frame of damaged_streams.base_frame or case of adaptive_tables.build_cases)
BASES = {
    "lenna64": (64, 64, 50, "lenna64"),
    "noise64": (64, 64, 50, "noise64"),
    "ragged17x33": (17, 33, 20, "ragged17x33"),
    "noise256": (256, 256, 75, "noise256"),
    "twolevel256": (256, 256, 75, "twolevel256"),
    "twolevel256q90": (256, 256, 90, "twolevel256"),
    "incomplete": (64, 400, 50, None),
    "all_long": (32, 840, 50, None),
}
BIG = ("noise256", "twolevel256", "twolevel256q90")
OUT_OF_REACH_BASES = ("twolevel256q90", "incomplete", "all_long")  # left out of the out-of-reach share
FULL_SWAPS = ("lenna64", "noise64", "noise256", "twolevel256")
RESIDUE_BASES = ("noise256",)
SWAPS = ("sym_equal_size", "sym_unequal_size", "dc_categories", "codes_equal_length", "repeat_last", "reversed")
ONE_SWAP = {"ragged17x33": "sym_equal_size", "twolevel256q90": "reversed", "incomplete": "repeat_last", "all_long": "codes_equal_length"}
FLIP1 = ("seeded", "first_payload_bit", "last64", "range")
FLIP3 = ("seeded", "last64", "range")
CUTS = ("at16", "at17", "at18", "in_dc", "in_ac", "payload_first", "seeded", "one_short")
BYTE_KINDS = ("garbage", "ones_tail", "zeros_tail", "delete", "insert")
GEOMETRY = ("h+8", "h-8", "w+8", "w-8", "swapped", "8x8", "h-1", "w-3")
QUALITY = ("q1", "q99", "q-1", "q+1")
FLAGS = ("zero", "scaled", "le", "c0000000")
FLAG_BYTES = {"zero": bytes(4), "scaled": struct.pack(">I", 1 << 30), "le": struct.pack("<I", 1 << 31), "c0000000": struct.pack(">I", 0xC0000000)}

sha, px_sha, flip, header, with_header, _rng = D.sha, D.px_sha, D.flip, D.header, D.with_header, D._rng


class StrictError(ValueError):
    def __init__(self, cls, what=""):
        assert cls in CLASSES
        ValueError.__init__(self, "%s: %s" % (cls, what) if what else cls)
        self.cls = cls


# ---------------------------------------------------------------------------------------------------------------------------------
# the contract
# ---------------------------------------------------------------------------------------------------------------------------------
class Bits:
    """Bit positions of a stream, most significant bit first; zeros behind its end."""

    def __init__(self, s):
        self.data = bytes(s) + bytes(16)
        self.total = len(s) * 8

    def peek(self, p, k):
        """k <= 64 bits from bit p on, as a number."""
        b = p >> 3
        return (int.from_bytes(self.data[b:b + 9], "big") >> (72 - (p & 7) - k)) & ((1 << k) - 1)


def read_table(s, strict=True):
    """-> (table as adaptive_tables writes one, first payload bit).  strict: the checks of the contract, StrictError; else the table as
    the reference's read_huffman_table reads it whatever its counts and widths, None where that reads behind the stream's end."""
    bits = Bits(s)
    if len(s) < 16 or not s[12] & 0x80:
        if strict:
            raise StrictError("header")
        return None
    p = 128
    table = {"DC": [], "AC": []}
    for key, sym_bits, len_bits, most in (("DC", 4, 4, 16), ("AC", 8, 8, 256)):
        if p + 16 > bits.total:
            if strict:
                raise StrictError("table_truncated", "%s count" % key)
            return None
        count = bits.peek(p, 16)
        p += 16
        if strict and not 1 <= count <= most:
            raise StrictError("dc_count" if key == "DC" else "ac_count", str(count))
        for i in range(count):
            if p + sym_bits + len_bits > bits.total:
                if strict:
                    raise StrictError("table_truncated", "%s entry %d" % (key, i))
                return None
            sym, n = bits.peek(p, sym_bits), bits.peek(p + sym_bits, len_bits)
            p += sym_bits + len_bits
            if strict and n + (sym & 15) > 64:
                raise StrictError("too_wide", "%s entry %d: %d + %d bits" % (key, i, n, sym & 15))
            if p + n > bits.total:
                if strict:
                    raise StrictError("table_truncated", "%s code %d" % (key, i))
                return None
            code = "".join(format(bits.peek(p + at, min(64, n - at)), "0%db" % min(64, n - at)) for at in range(0, n, 64))
            p += n
            table[key].append((sym if key == "DC" else (sym >> 4, sym & 15), code))
    if strict:
        for key in ("DC", "AC"):
            if not AT.is_prefix_free([code for _, code in table[key]]):
                raise StrictError("not_prefix", key)
    return table, p


def _lookup(entries):
    """-> (distinct code lengths ascending, {(length, code value): symbol})."""
    found = {(len(code), int(code, 2) if code else 0): sym for sym, code in entries}
    return sorted({n for n, _ in found}), found


def walk(s, table, p, nblocks, zz=None, partial=False):
    """The payload's blocks from bit p on -> [{"start", "symbols": [(scan position, first value bit, size)]}], the bit behind the last
    block.  zz (int64 [n, 64]) receives the coefficients.  StrictError for what the contract refuses; partial: the walk ends there."""
    bits = Bits(s)
    total = bits.total
    (dlens, dfound), (alens, afound) = _lookup(table["DC"]), _lookup(table["AC"])
    blocks, running = [], 0

    def code(lens, found):
        nonlocal p
        w = bits.peek(p, 64)
        for n in lens:
            sym = found.get((n, w >> (64 - n)))
            if sym is not None:
                if p + n > total:
                    raise StrictError("truncated", "a code at bit %d" % p)
                p += n
                return sym
        raise StrictError("truncated" if p + 64 > total else "no_code", "bit %d" % p)

    def value(size):
        nonlocal p
        if size == 0:
            return 0
        if p + size > total:
            raise StrictError("truncated", "a value at bit %d" % p)
        v = bits.peek(p, size)
        p += size
        return v if v >> (size - 1) else v - ((1 << size) - 1)

    try:
        for b in range(nblocks):
            syms = []
            blocks.append({"start": p, "symbols": syms})
            cat = code(dlens, dfound)
            if cat:
                syms.append((0, p, cat))
            running += value(cat)
            if not -32768 <= running <= 32767:
                raise StrictError("dc_range", "block %d" % b)
            if zz is not None:
                zz[b, 0] = running
            k = 1
            while True:
                run, size = code(alens, afound)
                at = p
                v = value(size)
                if (run, size) == AT.EOB:
                    break
                k += run
                if k > 63:
                    raise StrictError("over_63", "block %d" % b)
                if size:
                    syms.append((k, at, size))
                if zz is not None:
                    zz[b, k] = v
                k += 1
    except StrictError:
        if not partial:
            raise
    return blocks, p


def decode_strict(s):
    table, p = read_table(s)
    h, w = header(s)[:2]
    zz = np.zeros((AT.blocks_of(h, w), 64), np.int64)
    walk(s, table, p, len(zz), zz)
    return zz.astype(np.int16)


def outcome_class(s):
    """-> (None, coefficients) or (class, None)."""
    try:
        return None, decode_strict(s)
    except StrictError as e:
        return e.cls, None


def reach(s):
    """Whether the reference's reader can be asked about this stream's table -> "in", or "out:" and why."""
    if len(s) < 16 or not s[12] & 0x80:
        return "out:header"
    t = read_table(s, strict=False)
    if t is None:
        return "out:table_truncated"
    table = t[0]
    lens = [len(code) for _, code in table["DC"] + table["AC"]]
    if lens and min(lens) == 0:
        return "out:zero_length"
    if lens and max(lens) > 16:
        return "out:long_code"
    for key in ("DC", "AC"):
        if len({sym for sym, _ in table[key]}) != len(table[key]):
            return "out:repeated_symbol"
        if len({code for _, code in table[key]}) != len(table[key]):
            return "out:repeated_code"
    return "in"


def twin(s):
    """The stream with its flag word as the reference's parse_header reads one (codec.py:119): 1 << 31 little-endian."""
    return bytes(s[:12]) + struct.pack("<I", 1 << 31) + bytes(s[16:])


# ---------------------------------------------------------------------------------------------------------------------------------
# bases
# ---------------------------------------------------------------------------------------------------------------------------------
def base_frame(base):
    return D.base_frame(BASES[base][3])


def base_streams(oracle, fx, tables=None):
    """base -> the clean stream.  tables: base -> table for the image bases (the generator's); else the fixture's."""
    cases = AT.build_cases()
    out = {}
    for base, (h, w, q, frame) in BASES.items():
        if frame is None:
            assert (cases[base]["h"], cases[base]["w"]) == (h, w)
            out[base] = AT.stream_of(base, cases[base], q)
        else:
            table = tables[base] if tables else AT.table_from_json(fx["bases"][base]["table"])
            out[base] = AT.write_stream(table, oracle.encode_zz16(base_frame(base), q), h, w, q)
        assert len(out[base]) <= MAX_BASE_BYTES, base
    return out


def table_fields(s):
    """[(field of FIELDS, bit)] for every bit of the table region of a well-formed stream, in stream order."""
    h, w, q, table, end = AT.parse(s)
    out, p = [], 128

    def take(field, n):
        nonlocal p
        out.extend((field, p + i) for i in range(n))
        p += n

    take("dc_count", 16)
    for cat, code in table["DC"]:
        take("dc_category", 4), take("dc_length", 4), take("dc_code", len(code))
    take("ac_count", 16)
    for sym, code in table["AC"]:
        take("run", 4), take("size", 4), take("ac_length", 8), take("ac_code", len(code))
    assert p == end
    return out


def rebuild(s, table):
    """The stream with another table in front of the same payload bits and their padding, zero-padded to a byte again where the table's
    length changed (bits behind the last block: no decoder reads them)."""
    bits = AT.bit_string(s)
    new = bits[:128] + AT.table_bits(table) + bits[AT.parse(s)[4]:]
    new += "0" * (-len(new) % 8)
    return int(new, 2).to_bytes(len(new) // 8, "big")


# ---------------------------------------------------------------------------------------------------------------------------------
# the damage
# ---------------------------------------------------------------------------------------------------------------------------------
def plan(base):
    """kind -> the variants this base gets (table_flip apart): the whole allotment."""
    i = list(BASES).index(base)
    p = {"table_swap": list(SWAPS) if base in FULL_SWAPS else [ONE_SWAP[base]],
         "value_flip": ["ac", "dc"],
         "flip1": [FLIP1[(2 * i) % 4], FLIP1[(2 * i + 1) % 4]] + (["seam255", "seam256"] if base in BIG else []),
         "flip3": [FLIP3[i % 3]] + (["seam"] if base == "noise256" else []),
         "cut": [CUTS[(3 * i + j) % 8] for j in range(3)] + (["res0", "res1", "res2", "res3"] if base in RESIDUE_BASES else [])}
    for k, kind in enumerate(BYTE_KINDS):
        p[kind] = ["table" if (i + k) % 2 == 0 else "payload"]
    p["geometry"] = [GEOMETRY[(2 * i) % 8], GEOMETRY[(2 * i + 1) % 8]]
    p["quality"] = [QUALITY[i % 4]]
    p["flag"] = [FLAGS[i % 4]]
    return p


def _table_flips(base, s):
    fields = table_fields(s)
    if base == "lenna64":
        return [("table_flip", "bit%d" % p, {"bits": [p], "field": f}, flip(s, [p])) for f, p in fields]
    by = {f: [p for g, p in fields if g == f] for f in FIELDS}
    quota = {f: SAMPLE // len(FIELDS) for f in FIELDS}
    for f in ("ac_code", "ac_length", "dc_code"):  # 48 = 9 x 5 + 3
        quota[f] += 1
    for f in FIELDS:  # (a field with fewer bits than its share gives the rest to the AC codes)
        if len(by[f]) < quota[f]:
            quota["ac_code"] += quota[f] - len(by[f])
            quota[f] = len(by[f])
    out = []
    for f in FIELDS:
        for p in sorted(int(x) for x in _rng(base, "table_flip_" + f, 0).choice(by[f], quota[f], replace=False)):
            out.append(("table_flip", "bit%d" % p, {"bits": [p], "field": f}, flip(s, [p])))
    assert len(out) == SAMPLE, (base, len(out))
    return out


def free_code(codes, longest=16):
    """The shortest (then smallest) bit string that is no code's prefix and has no code as a prefix, or None."""
    for n in range(1, longest + 1):
        for v in range(1 << n):
            c = format(v, "0%db" % n)
            if not any(c.startswith(x) or x.startswith(c) for x in codes):
                return c
        if n >= 8:
            break
    return None


def _table_swaps(base, s, variants):
    table = AT.parse(s)[3]
    out = []

    def pick(tag, pairs):
        assert pairs, (base, tag)
        return pairs[int(_rng(base, "table_swap_" + tag, 0).integers(0, len(pairs)))]

    for tag in variants:
        dc, ac = list(table["DC"]), list(table["AC"])
        params = {"keeps_lengths": tag in ("sym_equal_size", "repeat_last", "reversed")}
        if tag in ("sym_equal_size", "sym_unequal_size"):
            i, j = pick(tag, [(i, j) for i in range(len(ac)) for j in range(i + 1, len(ac)) if (ac[i][0][1] == ac[j][0][1]) == (tag == "sym_equal_size")])
            ac[i], ac[j] = (ac[j][0], ac[i][1]), (ac[i][0], ac[j][1])
            params["entries"] = [i, j]
        elif tag == "dc_categories":
            i, j = pick(tag, [(i, j) for i in range(len(dc)) for j in range(i + 1, len(dc))])
            dc[i], dc[j] = (dc[j][0], dc[i][1]), (dc[i][0], dc[j][1])
            params["entries"] = [i, j]
        elif tag == "codes_equal_length":
            i, j = pick(tag, [(i, j) for i in range(len(ac)) for j in range(i + 1, len(ac)) if len(ac[i][1]) == len(ac[j][1])])
            ac[i], ac[j] = (ac[i][0], ac[j][1]), (ac[j][0], ac[i][1])
            params["entries"] = [i, j]
        elif tag == "repeat_last":
            code = free_code([c for _, c in ac])
            if code is None:
                continue  # (a complete code: the Kraft sum leaves none)
            ac.append((ac[-1][0], code))
            params["code"] = code
        else:
            dc, ac = dc[::-1], ac[::-1]
        out.append(("table_swap", tag, params, rebuild(s, {"DC": dc, "AC": ac})))
    return out


def _value_flips(base, s, blocks):
    ac = [(b, k, p, size) for b, blk in enumerate(blocks) for k, p, size in blk["symbols"] if k >= 1 and size >= 2]
    b, k, p, size = ac[int(_rng(base, "value_flip_ac", 0).integers(0, len(ac)))]
    out = [("value_flip", "ac", {"bits": [p + size - 1], "block": b, "scan": k})]
    dc = [(b, p, size) for b, blk in enumerate(blocks[:max(1, len(blocks) // 4)]) for k, p, size in blk["symbols"] if k == 0]
    top = max(size for b, p, size in dc)
    dc = [d for d in dc if d[2] >= top - 1]
    b, p, size = dc[int(_rng(base, "value_flip_dc", 0).integers(0, len(dc)))]
    out.append(("value_flip", "dc", {"bits": [p], "block": b, "scan": 0}))
    return [(kind, tag, params, flip(s, params["bits"])) for kind, tag, params in out]


def _payload_flips(base, s, first, rb, variants1, variants3):
    nbits = len(s) * 8
    out = []

    def seam(r):
        return first + r * rb, min(first + (r + 1) * rb, nbits)

    for tag in variants1:
        if tag == "seeded":
            p = int(_rng(base, "flip1", 0).integers(first, nbits))
        elif tag == "first_payload_bit":
            p = first
        elif tag == "last64":
            p = int(_rng(base, "flip1_last64", 0).integers(nbits - 64, nbits))
        elif tag == "range":
            p = first + rb * int(_rng(base, "flip1_range", 0).integers(1, (nbits - 1 - first) // rb + 1))
        else:
            p = int(_rng(base, "flip1_" + tag, 0).integers(*seam(int(tag[4:]))))
        out.append(("flip1", tag, {"bits": [p]}))
    for tag in variants3:
        if tag == "seeded":
            ps = _rng(base, "flip3", 0).choice(np.arange(first, nbits), 3, replace=False)
        elif tag == "last64":
            ps = _rng(base, "flip3_last64", 0).choice(np.arange(nbits - 64, nbits), 3, replace=False)
        elif tag == "range":
            count = (nbits - 1 - first) // rb
            ps = [first + rb * int(m) + d for m, d in zip(_rng(base, "flip3_range", 0).integers(1, count + 1, 3), (0, 1, 2))]
        else:  # inside range 255, the first bit of range 256, inside range 256
            ps = [int(_rng(base, "flip3_seam", 0).integers(*seam(255))), seam(256)[0], int(_rng(base, "flip3_seam", 1).integers(seam(256)[0] + 1, seam(256)[1]))]
        out.append(("flip3", tag, {"bits": sorted(int(p) for p in ps)}))
    return [(kind, tag, params, flip(s, params["bits"])) for kind, tag, params in out]


def _cuts(base, s, first, variants):
    n, fields = len(s), table_fields(s)
    dc_bits = [p for f, p in fields if f.startswith("dc_") and f != "dc_count"]
    ac_bits = [p for f, p in fields if f in ("run", "size", "ac_length", "ac_code")]
    payload_first = first // 8 + 1  # the first byte that holds payload bits only
    out = []
    for tag in variants:
        if tag.startswith("at"):
            at = int(tag[2:])
        elif tag == "in_dc":
            at = int(_rng(base, "cut_in_dc", 0).integers(dc_bits[0] // 8 + 1, dc_bits[-1] // 8 + 1))
        elif tag == "in_ac":
            at = int(_rng(base, "cut_in_ac", 0).integers(ac_bits[0] // 8 + 1, ac_bits[-1] // 8 + 1))
        elif tag == "payload_first":
            at = payload_first
        elif tag == "seeded":
            at = int(_rng(base, "cut", 0).integers(payload_first + 1, n - 1))
        elif tag == "one_short":
            at = n - 1
        else:
            lo = int(_rng(base, "cut_res", 0).integers(payload_first + 1, n - 5))
            at = next(x for x in range(lo, lo + 4) if x % 4 == int(tag[3:]))
        out.append(("cut", tag, {"length": at}, s[:at]))
    return out


def _byte_damage(base, s, first, where):
    """where: kind -> "table" or "payload"."""
    n, table_end = len(s), first // 8  # bytes 16 .. table_end - 1 hold table bits only
    out = []

    def at_for(kind, room=0):
        if where[kind] == "table":
            return int(_rng(base, kind, 0).integers(16, table_end - room))
        return int(_rng(base, kind, 0).integers(table_end + 1, n - room))

    if where["garbage"] == "table":
        at = at_for("garbage", 4)
        extra = _rng(base, "garbage_bytes", 0).integers(0, 256, 4, dtype=np.uint8).tobytes()
        out.append(("garbage", "table", {"at": at, "overwritten": 4, "sha256": sha(extra)}, s[:at] + extra + s[at + 4:]))
    else:
        count = (1, 7, 300)[list(BASES).index(base) % 3]
        extra = _rng(base, "garbage_bytes", 0).integers(0, 256, count, dtype=np.uint8).tobytes()
        out.append(("garbage", "payload", {"appended": count, "sha256": sha(extra)}, s + extra))
    for kind, byte in (("ones_tail", 0xFF), ("zeros_tail", 0)):
        at = at_for(kind)
        out.append((kind, where[kind], {"from": at}, s[:at] + bytes([byte]) * (n - at)))
    count = 1 + list(BASES).index(base) % 4
    at = at_for("delete", count)
    out.append(("delete", where["delete"], {"at": at, "count": count}, s[:at] + s[at + count:]))
    at = at_for("insert")
    extra = _rng(base, "insert_bytes", 0).integers(0, 256, count, dtype=np.uint8).tobytes()
    out.append(("insert", where["insert"], {"at": at, "count": count, "sha256": sha(extra)}, s[:at] + extra + s[at:]))
    return out


def _header_entries(base, s, geometry, quality, flags):
    h, w, q, _ = header(s)
    out = []
    for tag in geometry:
        hw = {"h+8": (h + 8, w), "h-8": (h - 8, w), "w+8": (h, w + 8), "w-8": (h, w - 8), "swapped": (w, h), "8x8": (8, 8), "h-1": (h - 1, w), "w-3": (h, w - 3)}[tag]
        assert min(hw) >= 1 and hw != (h, w), (base, tag)
        out.append(("geometry", tag, {"h": hw[0], "w": hw[1]}, with_header(s, h=hw[0], w=hw[1])))
    for tag in quality:
        nq = {"q1": 1, "q99": 99, "q-1": q - 1, "q+1": q + 1}[tag]
        assert 1 <= nq <= 99 and nq != q
        out.append(("quality", tag, {"quality": nq}, with_header(s, q=nq)))
    for tag in flags:
        out.append(("flag", tag, {"flag_bytes": FLAG_BYTES[tag].hex()}, bytes(s[:12]) + FLAG_BYTES[tag] + bytes(s[16:])))
    return out


def _dc_runs(base, s, table, blocks):
    """Blocks of the largest DC category of the base's own table, every value bit 1 (or 0: the most negative difference), each closed by
    the EOB, put in front of a block of the clean stream: the chain of block starts stays whole - every walker arrives at the old
    blocks behind them, the frame's last ones fall off its end - and the running DC leaves int16 inside the run."""
    if base not in DC_RUN_BASES:
        return []
    at_block, sign = DC_RUN_BASES[base]
    cat, code = max(table["DC"])
    count = 32768 // ((1 << cat) - 1) + 2
    assert at_block + count < len(blocks), (base, cat, count)
    bits, at = AT.bit_string(s), blocks[at_block]["start"]
    new = bits[:at] + (code + ("1" if sign > 0 else "0") * cat + dict(table["AC"])[AT.EOB]) * count + bits[at:]
    new += "0" * (-len(new) % 8)
    return [("dc_run", "block%d" % at_block, {"at_bit": at, "blocks": count, "category": cat, "sign": sign}, int(new, 2).to_bytes(len(new) // 8, "big"))]


def corpus(oracle, fx=None, bases=None):
    """[(name, base, kind, params, stream bytes)] and nothing else: deterministic, in a fixed order."""
    if bases is None:
        bases = base_streams(oracle, fx if fx is not None else load_fixture())
    out = []
    for base in BASES:
        s = bases[base]
        h, w, q, table, first = AT.parse(s)
        n = AT.blocks_of(h, w)
        blocks, _ = walk(s, table, first, n)
        rb = AT.range_rule(len(s), first, n)
        p = plan(base)
        made = (_table_flips(base, s) + _table_swaps(base, s, p["table_swap"]) + _value_flips(base, s, blocks)
                + _payload_flips(base, s, first, rb, p["flip1"], p["flip3"]) + _cuts(base, s, first, p["cut"])
                + _byte_damage(base, s, first, {k: p[k][0] for k in BYTE_KINDS}) + _header_entries(base, s, p["geometry"], p["quality"], p["flag"])
                + _dc_runs(base, s, table, blocks))
        for kind, tag, params, data in made:
            out.append(("%s/%s/%s" % (base, kind, tag), base, kind, params, bytes(data)))
    assert len({e[0] for e in out}) == len(out) <= MAX_ENTRIES, len(out)
    return out


def check_population(entries):
    """Every kind on every base; every variant of a kind somewhere."""
    have = {(base, kind) for name, base, kind, params, s in entries}
    missing = [(b, k) for b in BASES for k in KINDS if (b, k) not in have and (k != "dc_run" or b in DC_RUN_BASES)]
    assert not missing, missing
    tags = {(kind, name.split("/")[2]) for name, base, kind, params, s in entries}
    for kind, variants in (("table_swap", SWAPS), ("flip1", FLIP1 + ("seam255", "seam256")), ("flip3", FLIP3 + ("seam",)), ("cut", CUTS + ("res0", "res1", "res2", "res3")),
                           ("geometry", GEOMETRY), ("quality", QUALITY), ("flag", FLAGS)) + tuple((k, ("table", "payload")) for k in BYTE_KINDS):
        assert all((kind, v) in tags for v in variants), (kind, sorted(t for t in tags if t[0] == kind))


# ---------------------------------------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------------------------------------
def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def records(fx):
    """name -> {"bytes", "sha256" (None for the exhaustive family: fx["lenna64_table_flips_sha256"] covers it), "outcome": a class of
    CLASSES or (h, w, pixels sha256), "source": where the pixels come from, "reach", "reader"}, in the corpus' order."""
    out, bit = {}, 128
    for name, nbytes, digest, outcome, rch, reader in fx["entries"]:
        if name == 0:
            name, bit = "lenna64/table_flip/bit%d" % bit, bit + 1
        rec = {"bytes": nbytes, "sha256": digest or None, "reach": rch, "reader": reader}
        if isinstance(outcome, str):
            rec["outcome"], rec["source"] = outcome, None
        else:
            rec["outcome"], rec["source"] = (outcome[0], outcome[1], outcome[2]), outcome[3]
        out[name] = rec
    return out


def family_sha(digests):
    return sha("".join(digests).encode())


def consistency(entries, rec, clean_pixels):
    """The rules the generator asserts, from the stored fields alone -> the figures the fixture records.
    entries: [(name, base, kind)]; clean_pixels: base -> digest of the clean stream's pixels."""
    inr = [(n, b, k) for n, b, k in entries if rec[n]["reach"] == "in"]
    stricter = {}
    for n, b, k in inr:
        r = rec[n]
        decodes = not isinstance(r["outcome"], str)
        assert r["reader"] != "not_run", n
        if decodes:
            assert r["reader"] == "clean" and r["source"] == "twin", (n, r)
        elif r["reader"] == "clean":
            assert r["outcome"] in STRICTER, (n, r)
            stricter[r["outcome"]] = stricter.get(r["outcome"], 0) + 1
    for n, b, k in entries:
        r = rec[n]
        if r["reach"] != "in":
            assert r["reader"] == "not_run" and r["source"] in (None, "model"), (n, r)
    nstrict = sum(stricter.values())
    assert nstrict * 100 <= 3 * len(inr), (stricter, len(inr))
    counted = [(n, b, k) for n, b, k in entries if b not in OUT_OF_REACH_BASES and not isinstance(rec[n]["outcome"], str)]
    out_decoded = sum(rec[n]["reach"] != "in" for n, b, k in counted)
    assert out_decoded * 100 <= OUT_OF_REACH_MAX_PERCENT * len(counted), (out_decoded, len(counted))
    census = {}
    for n, b, k in entries:
        o = rec[n]["outcome"]
        cls = o if isinstance(o, str) else ("pixels_of_the_base" if o[2] == clean_pixels[b] and (o[0], o[1]) == BASES[b][:2] else "other_pixels")
        census.setdefault(k, {}).setdefault(cls, 0)
        census[k][cls] += 1
    per_class = {c: sum(v.get(c, 0) for v in census.values()) for c in CLASSES + ("pixels_of_the_base", "other_pixels")}
    assert all(per_class[c] >= 3 for c in CLASSES), per_class
    assert per_class["other_pixels"] >= 150, per_class
    return {"in_reach": len(inr), "stricter_in_reach": stricter, "decoded_counted": len(counted), "decoded_counted_out_of_reach": out_decoded,
            "census": census, "per_class": per_class}
