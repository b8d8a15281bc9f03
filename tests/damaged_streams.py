"""Shared by tests/test_damaged_streams_cpu.py, tests/test_damaged_streams_gpu.py and tests/golden/gen/make_goldens_damaged.py: ONE seeded
corpus of damaged default-table streams for every decoder route, and the fixture tests/golden/damaged_streams.json with what the
unmodified reference's decompress() made of each (codec.py:178-186 swallows the exception of a block, huffman.py:66-98 reads on behind
the end of the data: a damaged stream has exactly one right answer, pixels or an exception class).  No test lives here.

corpus(oracle) -> [(name, base, kind, params, stream bytes)], in a fixed order.  Nothing in it is random at run time: every position
comes from a numpy generator seeded by the entry's base, kind and ordinal.

Bases (oracle.compress of a regenerated frame; nothing larger than 256 x 256 - range, workgroup and stream-end boundaries all exist here):
  noise64      64 x 64 noise, q = 50: 64 blocks, above the device decoder's bit floor (128 + 8,192 stream bits) once TIC_DECODE_MIN_BLOCKS=1
               lowers the block floor
  noise40x72   40 x 72 noise, q = 90
  ragged17x33  17 x 33 noise, q = 20: ragged, below the bit floor - the host decoder on every route
  lenna64      a 64 x 64 crop of Lenna, q = 50: sparse, short blocks among long ones
  noise256     256 x 256 noise, q = 50: 1,024 blocks, the smallest frame the shipped library's device decoder takes; its decode
               workgroups carry a DC sum from one to the next
  twolevel256  256 x 256 pixels of two grey levels, q = 90

Kinds (every kind on every base unless it says otherwise; `params` names the positions):
  flip1, flip3   one / three bits of the payload: seeded positions, the first payload bit, the last 2,048 bits (the tail the device
                 decoder leaves to the host), a bit at a multiple of 288 and of 2,016 behind bit 128 (the ranges of the device walk)
  value_flip     the lowest value bit of one AC coefficient; the top (sign) value bit of one DC difference in the first quarter of the
                 frame.  Found by walk() below, a plain walker of the default tables; every code LENGTH stays what it was, so the chain
                 of block starts is the clean stream's and a device decoder has to finish the stream itself - with the changed
                 coefficient and, for the DC, the changed prefix sum in every later block
  cut            at 16, 17, 18 bytes, at seeded bytes, inside the last 256 bytes, one byte short, and inside the value bits of a DC
                 difference that begin with a 0 (the reference makes a number of the bits that are left, and the block keeps it)
  garbage        1, 7, 300 seeded bytes appended; 300 zero bytes; 300 bytes 0xFF
  ones_tail, zeros_tail   from a seeded byte to the end
  delete, insert 1 .. 8 bytes removed / inserted (seeded bytes) at a seeded payload position; 2 and 3 bytes 0xFF inserted (a prefix that is
                 no codeword in the middle of valid data: the reference reads 17 bits, drops the block and goes on from there)
  geometry       the header's h or w +-8 and +-16 (not below 1), h and w swapped (where they differ), 8 x 8 on the whole payload, h - 1 and w - 3 (ragged
                 crops of the same block grid), and 512 x 512 on the payload of the 64 x 64 bases
  quality        the header's quality replaced by 1, 99, q - 1, q + 1
  flag_scaled    1 << 30 set on the 64 x 64 bases (their quality, 50, is a legal exponent): the reference's scaled branch of the payload

Not in the corpus, on purpose: qualities outside 1..99 and the flag 1 << 31, where the product differs from the reference by design
(tests/test_gpu_parity.py::test_error_paths, tests/test_oracle_golden.py::test_decoder_edges_round3).
"""
import hashlib
import json
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "damaged_streams.json")
MIN_ENTRIES = 400
DEVICE_MIN_BITS = 128 + 8192   # tic_api.hip device_decoder_takes with the block floor at 1: len * 8 >= 128 + 8192
TAIL_BITS = 2048               # the stream's last bits, whose blocks the device decoder leaves to the host
RANGES = (288, 2016)           # the shortest and the longest range of the device walk (tic_entropy_dec_gpu.h dec_range_rule)
KINDS = ("flip1", "flip3", "value_flip", "cut", "garbage", "ones_tail", "zeros_tail", "delete", "insert", "geometry", "quality", "flag_scaled")
SCALED = 1 << 30
# name -> (h, w, quality, content)
BASES = {
    "noise64": (64, 64, 50, "noise"),
    "noise40x72": (40, 72, 90, "noise"),
    "ragged17x33": (17, 33, 20, "noise"),
    "lenna64": (64, 64, 50, "lenna"),
    "noise256": (256, 256, 50, "noise"),
    "twolevel256": (256, 256, 90, "twolevel"),
}
BASE_SEEDS = {"noise64": 6401, "noise40x72": 4072, "ragged17x33": 1733, "lenna64": 0, "noise256": 25601, "twolevel256": 25602}
LENNA_CROP = (224, 264)        # top-left corner of the 64 x 64 crop: the hat's brim, flat blocks beside textured ones


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def px_sha(px):
    return sha(np.ascontiguousarray(px, dtype=np.uint8).tobytes())


def applies(kind, base):
    return kind != "flag_scaled" or BASES[base][:2] == (64, 64)


def base_frame(base):
    h, w, q, content = BASES[base]
    if content == "lenna":
        y, x = LENNA_CROP
        return np.ascontiguousarray(np.load(os.path.join(GOLDEN, "lenna.npz"))["img"][y:y + h, x:x + w])
    rng = np.random.default_rng(BASE_SEEDS[base])
    if content == "twolevel":
        return np.where(rng.integers(0, 2, (h, w)) == 1, 208, 48).astype(np.uint8)
    return rng.integers(0, 256, (h, w), dtype=np.uint8)   # (conftest.rand_frame)


def base_streams(oracle):
    """base -> the clean stream, oracle.compress of the regenerated frame."""
    return {b: oracle.compress(base_frame(b), BASES[b][2]) for b in BASES}


def nblocks(h, w):
    return ((h + 7) // 8) * ((w + 7) // 8)


def header(s):
    return struct.unpack("<IIII", bytes(s[:16]))


def with_header(s, h=None, w=None, q=None, flag=None):
    h0, w0, q0, f0 = header(s)
    return struct.pack("<IIII", h0 if h is None else h, w0 if w is None else w, q0 if q is None else q, f0 if flag is None else flag) + bytes(s[16:])


def device_eligible(s):
    return len(s) * 8 >= DEVICE_MIN_BITS


# ---------------------------------------------------------------------------------------------------------------------------------
# a plain walker of the default tables
# ---------------------------------------------------------------------------------------------------------------------------------
class Tables:
    """oracle.dump_tables() as two dictionaries: bit string -> DC category, bit string -> (run, size)."""

    def __init__(self, dump):
        self.dc, self.ac = {}, {}
        for line in dump.split("\n"):
            if line:
                kind, run, size, bits = line.split(",")
                if kind == "D":
                    self.dc[bits] = int(size)
                else:
                    self.ac[bits] = (int(run), int(size))


class NotWellFormed(Exception):
    pass


def walk(tables, s, n=None, partial=False):
    """A strict walk over the n blocks of a stream (the header's count by default): per block its first bit, the running DC in front of
    it, and its value-bearing symbols as (scan position 0..63, first value bit, size) -> (blocks, end position).  NotWellFormed for
    anything an encoder does not write: a prefix that is no codeword, a block past scan position 63, a read behind the stream's end.
    partial: no exception - the walk ends there, and the block it ended in is the last of the list (its start is still a block start:
    every decoder arrives there)."""
    text = bin(int.from_bytes(bytes(s), "big"))[2:].zfill(len(s) * 8)
    if n is None:
        h, w = header(s)[:2]
        n = nblocks(h, w)
    pos, blocks, running = 128, [], 0

    def code(table):
        nonlocal pos
        for l in range(1, 17):
            if pos + l > len(text):
                raise NotWellFormed("the stream ends inside a codeword")
            if text[pos:pos + l] in table:
                sym = table[text[pos:pos + l]]
                pos += l
                return sym
        raise NotWellFormed("no codeword at bit %d" % pos)

    def value(size):
        nonlocal pos
        if size == 0:
            return 0
        if pos + size > len(text):
            raise NotWellFormed("the stream ends inside a value")
        v = int(text[pos:pos + size], 2)
        pos += size
        return v if v >> (size - 1) else v - ((1 << size) - 1)

    try:
        for b in range(n):
            syms = []
            blocks.append({"start": pos, "dc_before": running, "symbols": syms})
            size = code(tables.dc)
            if size:
                syms.append((0, pos, size))
            running += value(size)
            k = 1
            while True:
                run, size = code(tables.ac)
                if (run, size) == (0, 0):
                    break
                if (run, size) == (15, 0):
                    k += 16
                    continue
                k += run
                if k > 63:
                    raise NotWellFormed("block %d runs past scan position 63" % b)
                syms.append((k, pos, size))
                value(size)
                k += 1
    except NotWellFormed:
        if not partial:
            raise
    return blocks, pos


def starts(blocks):
    return [b["start"] for b in blocks]


# ---------------------------------------------------------------------------------------------------------------------------------
# the damage
# ---------------------------------------------------------------------------------------------------------------------------------
def _rng(base, kind, k):
    return np.random.default_rng([zlib.crc32(("%s/%s" % (base, kind)).encode()), k])


def flip(s, bit_positions):
    a = bytearray(s)
    for p in bit_positions:
        a[p >> 3] ^= 0x80 >> (p & 7)
    return bytes(a)


def _flip_entries(base, s):
    nbits = len(s) * 8
    first, last = 128, nbits - 1
    tail_from = max(first, nbits - TAIL_BITS)
    out = []
    for k in range(6):
        p = int(_rng(base, "flip1", k).integers(first, nbits))
        out.append(("flip1", "seeded%d" % k, {"bits": [p]}))
    out.append(("flip1", "first_payload_bit", {"bits": [first]}))
    out.append(("flip1", "last_bit", {"bits": [last]}))
    for k in range(3):
        p = int(_rng(base, "flip1_tail", k).integers(tail_from, nbits))
        out.append(("flip1", "tail%d" % k, {"bits": [p]}))
    for r in RANGES:
        count = (nbits - 1 - first) // r
        if count >= 1:
            p = first + r * int(_rng(base, "flip1_range%d" % r, 0).integers(1, count + 1))
            out.append(("flip1", "range%d" % r, {"bits": [p]}))
    for k in range(5):
        ps = sorted(int(p) for p in _rng(base, "flip3", k).choice(np.arange(first, nbits), 3, replace=False))
        out.append(("flip3", "seeded%d" % k, {"bits": ps}))
    ps = sorted(int(p) for p in _rng(base, "flip3_tail", 0).choice(np.arange(tail_from, nbits), 3, replace=False))
    out.append(("flip3", "tail", {"bits": ps}))
    return [(kind, tag, params, flip(s, params["bits"])) for kind, tag, params in out]


def _value_flip_entries(base, s, blocks):
    """AC: the last value bit of seeded coefficients of size >= 2 (the magnitude moves by one, the sign stays).  DC: the first value bit
    of two differences in the first quarter of the frame, of the largest size found there or one less (the running DC of every later
    block moves by 2 ** size - 1 quantiser steps or more: no block keeps its pixels)."""
    out = []
    ac = [(b, k, p, size) for b, blk in enumerate(blocks) for k, p, size in blk["symbols"] if k >= 1 and size >= 2]
    for i in range(3):
        b, k, p, size = ac[int(_rng(base, "value_flip_ac", i).integers(0, len(ac)))]
        out.append(("value_flip", "ac%d" % i, {"bits": [p + size - 1], "block": b, "scan": k}))
    quarter = max(1, len(blocks) // 4)
    dc = [(b, p, size) for b, blk in enumerate(blocks[:quarter]) for k, p, size in blk["symbols"] if k == 0]
    top = max(size for b, p, size in dc)
    dc = [d for d in dc if d[2] >= top - 1]
    assert len(dc) >= 2, (base, top, len(dc))
    for i, j in enumerate(_rng(base, "value_flip_dc", 0).choice(len(dc), 2, replace=False)):
        b, p, size = dc[int(j)]
        out.append(("value_flip", "dc%d" % i, {"bits": [p], "block": b, "scan": 0}))
    return [(kind, tag, params, flip(s, params["bits"])) for kind, tag, params in out]


def _length_entries(base, s):
    n = len(s)
    out = [("cut", "at%d" % at, {"length": at}, s[:at]) for at in (16, 17, 18)]
    for k in range(3):
        at = int(_rng(base, "cut", k).integers(19, n - 1))
        out.append(("cut", "seeded%d" % k, {"length": at}, s[:at]))
    for k in range(2):
        at = int(_rng(base, "cut_tail", k).integers(max(19, n - 256), n - 1))
        out.append(("cut", "tail%d" % k, {"length": at}, s[:at]))
    out.append(("cut", "one_short", {"length": n - 1}, s[:n - 1]))
    for count in (1, 7, 300):
        extra = _rng(base, "garbage", count).integers(0, 256, count, dtype=np.uint8).tobytes()
        out.append(("garbage", "seeded%d" % count, {"appended": count, "sha256": sha(extra)}, s + extra))
    out.append(("garbage", "zeros300", {"appended": 300, "byte": 0}, s + bytes(300)))
    out.append(("garbage", "ones300", {"appended": 300, "byte": 255}, s + b"\xff" * 300))
    for kind, byte in (("ones_tail", 0xFF), ("zeros_tail", 0)):
        for k in range(3):
            at = int(_rng(base, kind, k).integers(16, n))
            out.append((kind, "seeded%d" % k, {"from": at}, s[:at] + bytes([byte]) * (n - at)))
    for count in range(1, 9):
        at = int(_rng(base, "delete", count).integers(16, n - count))
        out.append(("delete", "bytes%d" % count, {"at": at, "count": count}, s[:at] + s[at + count:]))
        at = int(_rng(base, "insert", count).integers(16, n))
        extra = _rng(base, "insert_bytes", count).integers(0, 256, count, dtype=np.uint8).tobytes()
        out.append(("insert", "bytes%d" % count, {"at": at, "count": count, "sha256": sha(extra)}, s[:at] + extra + s[at:]))
    for count in (2, 3):  # a run of ones in the middle of valid data: a prefix that is no codeword (huffman.py:66-74 reads 17 bits, then raises)
        at = int(_rng(base, "insert_ones", count).integers(16, n))
        out.append(("insert", "ones%d" % count, {"at": at, "count": count, "byte": 255}, s[:at] + b"\xff" * count + s[at:]))
    return out


def _cut_in_dc_value(base, s, blocks):
    """The stream ends inside the value bits of a DC difference whose first value bit is 0: read_int (bitbuffer.py:55-65) makes a number
    of the bits that are left, and the block keeps that DC (codec.py:180 assigns it before the AC symbols raise).  The last such
    difference of the stream whose value bits cross a byte boundary, where there is one."""
    text = bin(int.from_bytes(bytes(s), "big"))[2:].zfill(len(s) * 8)
    for b in range(len(blocks) - 1, -1, -1):
        for k, p, size in blocks[b]["symbols"]:
            if k == 0 and text[p] == "0" and (p + size - 1) // 8 > p // 8:
                at = (p + size - 1) // 8  # the byte that holds the value's last bit is the first one missing
                return [("cut", "in_dc_value", {"length": at, "block": b}, s[:at])]
    return []  # (ragged17x33: 15 blocks, no such difference)


def _header_entries(base, s):
    h, w, q, _ = header(s)
    out = []
    for d in (-16, -8, 8, 16):
        if h + d >= 1:
            out.append(("geometry", "h%+d" % d, {"h": h + d, "w": w}))
        if w + d >= 1:
            out.append(("geometry", "w%+d" % d, {"h": h, "w": w + d}))
    if h != w:
        out.append(("geometry", "swapped", {"h": w, "w": h}))
    out.append(("geometry", "8x8", {"h": 8, "w": 8}))
    out.append(("geometry", "h-1", {"h": h - 1, "w": w}))
    out.append(("geometry", "w-3", {"h": h, "w": w - 3}))
    if (h, w) == (64, 64):
        out.append(("geometry", "512x512", {"h": 512, "w": 512}))
    res = [(kind, tag, params, with_header(s, h=params["h"], w=params["w"])) for kind, tag, params in out]
    for tag, nq in (("q1", 1), ("q99", 99), ("q-1", q - 1), ("q+1", q + 1)):
        assert 1 <= nq <= 99 and nq != q
        res.append(("quality", tag, {"quality": nq}, with_header(s, q=nq)))
    if applies("flag_scaled", base):
        assert q <= 62
        res.append(("flag_scaled", "exp%d" % q, {"flag": SCALED}, with_header(s, flag=SCALED)))
    return res


def corpus(oracle, bases=None):
    """[(name, base, kind, params, stream bytes)] - name = base/kind/tag - and nothing else: deterministic, in a fixed order."""
    tables = Tables(oracle.dump_tables())
    if bases is None:
        bases = base_streams(oracle)
    out = []
    for base in BASES:
        s = bases[base]
        blocks, _ = walk(tables, s)
        for kind, tag, params, data in _flip_entries(base, s) + _value_flip_entries(base, s, blocks) + _length_entries(base, s) + _cut_in_dc_value(base, s, blocks) + _header_entries(base, s):
            out.append(("%s/%s/%s" % (base, kind, tag), base, kind, params, data))
    assert len({e[0] for e in out}) == len(out)
    return out


def census(entries):
    """What the issue's conditions are checked on: entries in all, per (base, kind), and how many the device decoder is offered."""
    per = {}
    for name, base, kind, params, s in entries:
        per[base, kind] = per.get((base, kind), 0) + 1
    return {"entries": len(entries), "per_base_kind": per, "device_eligible": sum(device_eligible(e[4]) for e in entries)}


def check_census(c):
    assert c["entries"] >= MIN_ENTRIES, c["entries"]
    missing = [(b, k) for b in BASES for k in KINDS if applies(k, b) and not c["per_base_kind"].get((b, k))]
    assert not missing, missing
    assert 2 * c["device_eligible"] >= c["entries"], (c["device_eligible"], c["entries"])


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)
