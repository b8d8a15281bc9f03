"""What tests/test_adaptive_rate_cpu.py and tests/test_adaptive_rate_gpu.py share: the fixtures of the unmodified reference, a plain numpy
model of the symbol statistics of per-image Huffman tables (huffman.py:12-33: counts and first-occurrence keys), built coefficient
blocks for the statistics kernels, the bisection of compress_adaptive_to_size replayed in Python, and the table of the qualities it must
end at.  No test lives here."""
import json
import os

import numpy as np

from conftest import rand_frame

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IMAGES = ("lenna", "bench01", "bench17", "bench40", "bench06_crop203x317", "noise256_seed7")
SOME_QUALITIES = (1, 2, 5, 10, 37, 50, 80, 90, 98, 99)
ALL_QUALITIES_IMAGES = ("noise256_seed7", "bench06_crop203x317")
BENCH_QUALITIES = (90, 80, 50, 20, 10, 5)  # the reference's tests/benchmark.py
DC_BIN, BINS = 256, 272
NEVER = (1 << 64) - 1  # the first key of a symbol that does not occur
_cache = {}


def adaptive_rate():
    if "rate" not in _cache:
        with open(os.path.join(GOLDEN, "adaptive_rate.json")) as f:
            _cache["rate"] = json.load(f)
    return _cache["rate"]


def adaptive_streams():
    if "streams" not in _cache:
        with open(os.path.join(GOLDEN, "adaptive_streams.json")) as f:
            _cache["streams"] = json.load(f)
    return _cache["streams"]


def fixture_image(name):
    """The pixels of an entry of adaptive_rate.json (its "pixels" field says the same in words)."""
    if name == "lenna":
        return np.load(os.path.join(GOLDEN, "lenna.npz"))["img"]
    if name == "noise256_seed7":
        return rand_frame(7, 256, 256)
    px = bench_pixels()
    if name == "bench06_crop203x317":
        return np.ascontiguousarray(px[5][:203, :317])
    return px[int(name[5:]) - 1]


def bench_pixels():
    if "bench" not in _cache:
        _cache["bench"] = np.load(os.path.join(GOLDEN, "benchmark_set.npz"))["pixels"]
    return _cache["bench"]


def hard_frame(h, w):
    by, bx = np.indices(((h + 7) // 8, (w + 7) // 8))
    blocks = np.where((by + bx) % 2 == 0, 0, 255).astype(np.uint8)
    return np.kron(blocks, np.ones((8, 8), np.uint8))[:h, :w]


def case_image(name, h, w):
    """The pixels of an entry of adaptive_streams.json's "cases" (image_jobs() of tests/golden/gen/make_goldens_adaptive.py)."""
    if name.startswith("small_"):
        return rand_frame(7 * h + w, h, w)
    if name.startswith("ragged_"):
        return rand_frame(100 + int(name[7:]), h, w)
    if name == "flat":
        return np.full((32, 32), 128, np.uint8)
    if name == "noise":
        return rand_frame(42, 64, 96)
    if name.startswith("hard_"):
        return hard_frame(h, w)
    if name == "frame_1080p":
        return rand_frame(1234, 1080, 1920)
    raise KeyError(name)


def cases_with_blocks(max_pixels=None):
    """(name, image, quality, bytes) of every case of adaptive_streams.json that has blocks (all of them have)."""
    out = []
    for c in adaptive_streams()["cases"]:
        h, w = c["height"], c["width"]
        if h == 0 or w == 0 or (max_pixels and h * w > max_pixels):
            continue
        out.append((c["name"], case_image(c["name"], h, w), c["quality"], c["bytes"]))
    return out


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def bit_length(a):
    """int.bit_length of |a|, elementwise (utils.py:9-10); exact: the exponent of a float64."""
    return np.frexp(np.abs(np.asarray(a, np.int64)).astype(np.float64))[1].astype(np.int64)


def model_stats(zz):
    """(count uint64 [272], first uint64 [272], err) of coefficients int16 [N, 64] (zig-zag, absolute DC), from the definition: the DC
    difference's category per block (key: the block), and per block the run-length list of huffman.py:12-33 - trailing zeros dropped,
    (15, 0) per 16 zeros in front of an entry, (run, value) per entry, (0, 0) at the end - whose symbols are (run, size of value) with
    key block * 64 + index in the list.  A category or size above 15 sets err and counts in bin size & 15 (what write_huffman_table's 4
    bits would hold)."""
    zz = np.asarray(zz, np.int64).reshape(-1, 64)
    n = zz.shape[0]
    count = np.zeros(BINS, np.uint64)
    first = np.full(BINS, NEVER, np.uint64)
    blocks = np.arange(n, dtype=np.int64)

    def add(bins, keys, weights=None):
        np.add.at(count, bins, np.uint64(1) if weights is None else weights.astype(np.uint64))
        np.minimum.at(first, bins, keys.astype(np.uint64))

    diff = zz[:, 0] - np.concatenate(([0], zz[:-1, 0]))
    dcat = bit_length(diff)
    err = bool((dcat > 15).any())
    add(DC_BIN + (dcat & 15), blocks)
    b, k = np.nonzero(zz[:, 1:])  # sorted by block, then position
    k = k + 1
    prev = np.where(np.concatenate(([True], b[1:] != b[:-1])), 0, np.concatenate(([0], k[:-1])))  # the entry before, or the DC's place
    run = k - prev - 1
    size = bit_length(zz[b, k])
    err = err or bool((size > 15).any())
    zrl = run >> 4
    emitted = zrl + 1
    total = np.cumsum(emitted)
    per_block = np.bincount(b, weights=emitted, minlength=n).astype(np.int64)  # symbols in front of the EOB
    block_start = np.concatenate(([0], np.cumsum(per_block)[:-1]))
    ordinal = total - emitted - block_start[b]  # of the entry's first symbol
    has = zrl > 0
    add(np.full(int(has.sum()), 0xF0), b[has] * 64 + ordinal[has], zrl[has])
    add(((run & 15) << 4) | (size & 15), b * 64 + ordinal + zrl)
    add(np.zeros(n, np.int64), blocks * 64 + per_block)
    return count, first, err


def model_stats_slow(zz):
    """The same, block by block from the list itself: the check of the vectorised model."""
    zz = np.asarray(zz, np.int64).reshape(-1, 64)
    count, first, err, prev = [0] * BINS, [NEVER] * BINS, False, 0
    for bi, c in enumerate(zz.tolist()):
        cat = abs(c[0] - prev).bit_length()
        prev = c[0]
        lst, run = [], 0
        ac = c[1:]
        while ac and ac[-1] == 0:
            ac.pop()
        for v in ac:
            if v == 0:
                run += 1
                continue
            while run > 15:
                lst.append((15, 0))
                run -= 16
            lst.append((run, v))
            run = 0
        lst.append((0, 0))
        err = err or cat > 15
        syms = [(DC_BIN + (cat & 15), bi)]
        for i, (r, v) in enumerate(lst):
            err = err or abs(v).bit_length() > 15
            syms.append(((r << 4) | (abs(v).bit_length() & 15), bi * 64 + i))
        for s, key in syms:
            count[s] += 1
            first[s] = min(first[s], key)
    return np.array(count, np.uint64), np.array(first, np.uint64), err


def stats_size(L, count, first):
    """tic_adaptive_stream_size of model statistics -> (rc, bytes)."""
    import ctypes as C

    count, first = np.ascontiguousarray(count, np.uint64), np.ascontiguousarray(first, np.uint64)
    n = C.c_size_t(0)
    rc = L.tic_adaptive_stream_size(count[DC_BIN:].ctypes.data, first[DC_BIN:].ctypes.data, count[:DC_BIN].ctypes.data, first[:DC_BIN].ctypes.data,
                                    C.byref(n))
    return rc, int(n.value)


# ---- built coefficients for the statistics kernels ------------------------------------------------------------------------------------
def block(dc=0, entries=()):
    """One block: its DC and {index: value} AC entries."""
    b = np.zeros(64, np.int16)
    b[0] = dc
    for i, v in dict(entries).items():
        assert 1 <= i <= 63
        b[i] = v
    return b


def noise_blocks(seed, n, density=0.3, amp=40):
    """n blocks of seeded coefficients: DCs that wander, AC entries non-zero with probability `density` that thins towards the end."""
    rng = np.random.default_rng(seed)
    zz = rng.integers(-amp, amp + 1, (n, 64))
    keep = rng.random((n, 64)) < density * np.linspace(1.5, 0.2, 64)
    zz = np.where(keep, zz, 0)
    zz[:, 0] = np.clip(np.cumsum(rng.integers(-30, 31, n)), -1000, 1000)
    return zz.astype(np.int16)


RUNS = (7, 8, 15, 16, 17, 31, 32, 47, 48, 55, 62)  # zero runs that end at, just before and just behind lane boundaries (8 entries a lane)


def edge_blocks():
    """name -> int16 [n, 64]: the blocks of the issue's list, a few blocks each so that neighbours differ."""
    out = {}
    out["all_zero"] = np.zeros((3, 64), np.int16)
    out["entry_63_only"] = np.stack([block(0, {63: 1}), block(5, {63: -2}), block(5, {})])
    for r in RUNS:  # the run starts behind the DC, and behind an entry
        rows = [block(1, {1 + r: 3}), block(2, {})]
        if r + 2 <= 63:
            rows.insert(1, block(-1, {1: -1, 2 + r: 7}))
        for start in (5, 9):  # ... and inside the block, so that it crosses lanes at other places
            if start + r + 1 <= 63:
                rows.append(block(0, {start: 2, start + r + 1: -2}))
        out["run_%d" % r] = np.stack(rows)
    out["three_zrls"] = np.stack([block(0, {1 + 48: 1}), block(0, {1 + 50: -9, 63: 1}), block(0, {2: 1, 3 + 49: 5})])
    out["sizes_1_to_15"] = np.stack([block(s, {s: 1 << (s - 1), 63 - s: -((1 << s) - 1), 30: (1 << s) - 1}) for s in range(1, 16)])
    out["ac_minus_32768"] = np.stack([block(3, {1: 4, 9: -32768, 12: 1}), block(3, {40: -32768}), block(4, {2: 32767})])
    out["dc_step_65535"] = np.stack([block(-32768, {1: 1}), block(32767, {17: 2}), block(-32768, {}), block(0, {3: 1})])
    # first-occurrence ties
    # bin (0 << 4) | 2 first in lane 7 of block 0 (entry 57 behind entry 56) and in lane 1 of block 1: block 0's must win although its ordinal is larger
    out["tie_lane7_lane1"] = np.stack([block(0, {1: 1, 2: 1, 3: 1, 56: 1, 57: 2}), block(0, {8: 1, 9: 3, 10: 2})])
    # bin (15, 0) first occurs as an entry's ZRLs whose SECOND one would already beat the next block's first; (1, 1) behind two ZRLs
    out["tie_second_zrl"] = np.stack([block(0, {1: 1, 35: 1}), block(0, {17: 1, 19: 1}), block(0, {34: 1})])
    # EOB ordinals 0 (an empty block first) and 63 (a full block first): the first block's key is the first key
    full = np.arange(64) % 5 + 1
    out["eob_ordinal_0"] = np.stack([block(0, {}), np.asarray(full, np.int16)])
    out["eob_ordinal_63"] = np.stack([np.asarray(full, np.int16), block(0, {})])
    return out


PROBE_BLOCKS = (1, 7, 8, 9, 127, 128, 129, 257)


# ---- the search ---------------------------------------------------------------------------------------------------------------------------
RANGES = ((1, 99), (10, 60), (37, 37))
BUDGET_KINDS = ("qmin-1", "qmin", "q50-1", "q50", "q99", "2^31")


def budgets(sizes, qmin):
    """The budgets of the search tests for a fixture entry's sizes (index q - 1), by kind."""
    return {"qmin-1": sizes[qmin - 1] - 1, "qmin": sizes[qmin - 1], "q50-1": sizes[49] - 1, "q50": sizes[49], "q99": sizes[98], "2^31": 1 << 31}


def replay(sizes, budget, qmin, qmax):
    """compress_to_size's contract on recorded sizes (index q - 1; None: no stream): (quality, bisection steps), or the exception the
    Python mirror raises."""
    def fits(q):
        return sizes[q - 1] is not None and sizes[q - 1] <= budget

    if not fits(qmin):
        return OverflowError if sizes[qmin - 1] is None else ValueError
    lo, hi, steps = qmin, qmax, 0
    while lo < hi:
        mid = (lo + hi + 1) // 2
        steps += 1
        if fits(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo, steps


# EXPECTED[image][(qmin, qmax)] = the quality per budget kind, in BUDGET_KINDS' order; "V": ValueError (min_quality exceeds the budget).
# Written down from adaptive_rate.json once; test_adaptive_rate_cpu.py replays the bisection against it.
# The sizes of all six images grow with the quality, so the rows are the same for every image: one below the size at min_quality fits
# nothing, the size at q itself ends at q (or at the range's end), one byte less at the quality below.
_ROWS = {(1, 99): ["V", 1, 49, 50, 99, 99], (10, 60): ["V", 10, 49, 50, 60, 60], (37, 37): ["V", 37, 37, 37, 37, 37]}
EXPECTED = {name: _ROWS for name in IMAGES}
