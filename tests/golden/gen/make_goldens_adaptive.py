#!/usr/bin/env python3
"""Fixtures of the adaptive (per-image) Huffman tables: compress(image, q, auto_generate_huffman_table=True) of the UNMODIFIED
reference (codec.py:133-164, huffman.py:101-194), run with the same import recipe as make_goldens_r5.py (stand-ins for the two
absent pure-container packages; every line of codec logic is the reference's own).

    python tests/golden/gen/make_goldens_adaptive.py [--procs 6]

Writes tests/golden/adaptive_streams.json (data only):
  * "cases": small, ragged, flat, noise and hard 0/255-block frames: the stream (hex) or, for long ones, its length and sha256;
    "decoded_sha256" = pixels of the reference's decode(encode(img, q)) (what the stream holds; the reference cannot read it back),
    "garbage_sha256" = pixels of the reference's decompress() of the adaptive stream (it misreads the flag, codec.py:111/119);
  * "benchmark": the 49 x 6 pairs of /root/reference/tests/benchmark.py (pixels in benchmark_set.npz): length, sha256, garbage_sha256;
  * "tables": calc_huffman_table() (huffman.py:101-108) of crafted symbol sequences: per symbol its count and first position, the
    codewords in the table's order and write_huffman_table()'s bits (codec.py:73-84);
  * "longcode": a synthetic coefficient array (longcode_coeffs() below; the tests build the same array) whose AC symbol counts
    follow the Fibonacci sequence, so that codes exceed 27 bits and code plus value bits exceed 32, entropy coded by the reference's
    calc_huffman_table / make_header / encode_huffman exactly as compress() strings them together (codec.py:136-164).
"""
import argparse
import hashlib
import json
import os
import sys
import time
from multiprocessing import Pool

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "standins"))
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

QUALITIES = (90, 80, 50, 20, 10, 5)  # benchmark.py:13
INLINE_MAX = 4096                    # streams up to this many bytes are stored whole


def sha(b):
    return hashlib.sha256(b).hexdigest()


def rand_frame(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def hard_frame(h, w):
    """8x8 blocks alternating between 0 and 255 (raster order): DC differences of category 12-13 at q >= 97."""
    by, bx = np.indices(((h + 7) // 8, (w + 7) // 8))
    blocks = np.where((by + bx) % 2 == 0, 0, 255).astype(np.uint8)
    return np.kron(blocks, np.ones((8, 8), np.uint8))[:h, :w]


def longcode_coeffs():
    """int16 [N, 64] zig-zag, absolute DC.  AC symbol k (k = 0..32: runs 2, 1, 0, sizes 15 down to 1) occurs F(k+1) times
    (Fibonacci): the rarest carry the largest values, the most frequent take one scan position each; blocks are filled in order."""
    syms = [(2, s) for s in (15, 14, 13)] + [(1, s) for s in range(15, 0, -1)] + [(0, s) for s in range(15, 0, -1)]
    fib = [1, 1]
    while len(fib) < len(syms):
        fib.append(fib[-1] + fib[-2])
    # greedy fill, one symbol kind at a time: a symbol that does not fit the current block (pos + run > 63) opens the next one
    bidx, spos, vals = [], [], []
    block, pos = 0, 1
    for (run, size), cnt in zip(syms, fib):
        width = run + 1
        here = (63 - run - pos) // width + 1 if pos + run <= 63 else 0  # still fit into the current block
        per = (62 - run) // width + 1                                    # fit into a fresh block
        i = np.arange(cnt)
        later = np.maximum(i - here, 0)
        b = np.where(i < here, block, block + 1 + later // per)
        p = np.where(i < here, pos + i * width, 1 + (later % per) * width)
        v = (1 << (size - 1)) + (size > 1)  # a value of exactly `size` bits
        bidx.append(b)
        spos.append(p + run)
        vals.append(np.where(i % 2 == 0, v, -v))
        block, pos = int(b[-1]), int(p[-1]) + width
    zz = np.zeros((block + 1, 64), np.int16)
    zz[np.concatenate(bidx), np.concatenate(spos)] = np.concatenate(vals)
    zz[:, 0] = (np.arange(zz.shape[0]) % 5) - 2
    return zz


def ref_stream_from_zz(zz, h, w, q):
    """compress()'s entropy part (codec.py:136-164) on given coefficients, with the reference's own functions."""
    from tinyimgcodec.bitbuffer import BitBuffer
    from tinyimgcodec.codec import make_header
    from tinyimgcodec.constants import AC, DC
    from tinyimgcodec.huffman import calc_huffman_table, encode_huffman, encode_run_length

    zz = zz.astype(np.int32)
    dc = zz[:, 0].copy()
    dc[1:] = np.diff(dc)
    ac = zz[:, 1:]
    ac_rle, idx = [], [0]
    for i in range(ac.shape[0]):
        ac_rle.extend(encode_run_length(ac[i]))
        idx.append(len(ac_rle))
    table = calc_huffman_table(dc, ac_rle)
    buf = BitBuffer()
    make_header(buf, {"height": h, "width": w, "quality": q}, table)
    for i in range(ac.shape[0]):
        encode_huffman(buf, dc[i : i + 1], dc_ac=DC, category_codeword=table)
        encode_huffman(buf, ac_rle[idx[i] : idx[i + 1]], dc_ac=AC, category_codeword=table)
    return buf.to_bytes(), table


def image_case(job):
    import tinyimgcodec as ref

    name, img, q = job
    out = ref.compress(img, quality=q, auto_generate_huffman_table=True)
    info = ref.encode(img, q)
    info["scaled_dct"] = False
    dec = ref.decode(info)  # what the stream holds
    garbage = ref.decompress(out)  # the reference's own reading of it
    e = {"name": name, "height": int(img.shape[0]), "width": int(img.shape[1]), "quality": q, "bytes": len(out), "sha256": sha(out),
         "decoded_sha256": sha(np.ascontiguousarray(dec).tobytes()), "garbage_sha256": sha(np.ascontiguousarray(garbage).tobytes())}
    if len(out) <= INLINE_MAX:
        e["stream"] = out.hex()
    return e


def bench_case(job):
    import tinyimgcodec as ref

    i, q = job
    img = np.load(os.path.join(GOLD, "benchmark_set.npz"))["pixels"][i - 1]
    out = ref.compress(img, quality=q, auto_generate_huffman_table=True)
    garbage = ref.decompress(out)
    return {"image": i, "quality": q, "bytes": len(out), "sha256": sha(out), "garbage_sha256": sha(np.ascontiguousarray(garbage).tobytes())}


def image_jobs():
    jobs = []
    for h, w in ((1, 1), (7, 9), (8, 8), (15, 17)):
        for q in (5, 50, 90):
            jobs.append(("small_%dx%d" % (h, w), rand_frame(7 * h + w, h, w), q))
    rng = np.random.default_rng(2024)
    for k in range(6):
        h, w = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        jobs.append(("ragged_%d" % k, rand_frame(100 + k, h, w), int(rng.integers(1, 100))))
    jobs.append(("flat", np.full((32, 32), 128, np.uint8), 50))
    for q in (5, 50, 90, 99):
        jobs.append(("noise", rand_frame(42, 64, 96), q))
    for q in (97, 98, 99):
        jobs.append(("hard_8x32", hard_frame(8, 32), q))
        jobs.append(("hard_40x72", hard_frame(40, 72), q))
    jobs.append(("frame_1080p", rand_frame(1234, 1080, 1920), 50))
    return jobs


def crafted_tables():
    """Symbol sequences for calc_huffman_table(dc, ac): DC values, AC (run, value) pairs; first occurrence = list order."""
    from tinyimgcodec.bitbuffer import BitBuffer
    from tinyimgcodec.codec import write_huffman_table
    from tinyimgcodec.constants import AC, DC
    from tinyimgcodec.huffman import calc_huffman_table

    def val(size):
        return 0 if size == 0 else (1 << (size - 1))

    def seq(counts, order_seed):
        """counts: list of (symbol, count) -> the symbols in a shuffled order that keeps first occurrences in list order."""
        rng = np.random.default_rng(order_seed)
        out = [s for s, c in counts if c > 0]  # first occurrences, in list order
        rest = [s for s, c in counts for _ in range(c - 1)]
        rng.shuffle(rest)
        return out + rest

    cases = {}
    ac_syms = [(r, s) for r in range(16) for s in range(1, 11)] + [(0, 0), (15, 0)]
    dc_syms = list(range(12))
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    cases["equal"] = ([(c, 7) for c in dc_syms], [(s, 5) for s in ac_syms[:100]])
    cases["fibonacci"] = ([(c, fib[k]) for k, c in enumerate(reversed(dc_syms))], [(s, fib[k]) for k, s in enumerate(ac_syms[:26])])
    cases["one_symbol"] = ([(3, 9)], [((0, 0), 4)])
    cases["two_symbols"] = ([(0, 5), (11, 2)], [((0, 0), 3), ((2, 7), 3)])
    rng = np.random.default_rng(5)
    cases["many_ones"] = ([(c, 1) for c in dc_syms] + [], [(s, int(rng.integers(1, 4)) if k % 9 == 0 else 1) for k, s in enumerate(ac_syms)])
    cases["ties"] = ([(c, 2 + (k % 3)) for k, c in enumerate([5, 1, 9, 0, 7, 2])], [(s, 1 + (k % 4)) for k, s in enumerate(reversed(ac_syms))])
    out = []
    for name, (dc_counts, ac_counts) in cases.items():
        dcs = seq(dc_counts, 1)
        acs = seq(ac_counts, 2)
        dc = np.array([val(c) for c in dcs], dtype=np.int32)
        ac = [(r, val(s)) for r, s in acs]
        table = calc_huffman_table(dc, ac)
        buf = BitBuffer()
        write_huffman_table(buf, table)
        nbits = buf.tell()
        first_dc, first_ac = {}, {}
        for k, c in enumerate(dcs):
            first_dc.setdefault(c, k)
        for k, s in enumerate(acs):
            first_ac.setdefault((s[0] << 4) | s[1], k)
        out.append({"name": name,
                    "dc": [[c, n, first_dc[c]] for c, n in dc_counts],
                    "ac": [[(s[0] << 4) | s[1], n, first_ac[(s[0] << 4) | s[1]]] for s, n in ac_counts],
                    "dc_codes": [[int(k), v] for k, v in table[DC].items()],
                    "ac_codes": [[(int(k[0]) << 4) | int(k[1]), v] for k, v in table[AC].items()],
                    "table_bits": nbits, "table": buf.to_bytes().hex()})
    return out


def longcode():
    import tinyimgcodec as ref  # noqa: F401  (package import first: the submodules' relative imports)

    zz = longcode_coeffs()
    n = zz.shape[0]
    h, w = 8, 8 * n
    t0 = time.perf_counter()
    out, table = ref_stream_from_zz(zz, h, w, 50)
    lens = [len(v) for v in table["AC"].values()]
    most = max(len(v) + int(k[1]) for k, v in table["AC"].items())
    assert max(lens) > 27 and most > 32, (max(lens), most)
    print("longcode: %d blocks, longest code %d bits, code+value %d bits, %d bytes, %.0f s" % (n, max(lens), most, len(out), time.perf_counter() - t0), flush=True)
    return {"blocks": n, "height": h, "width": w, "quality": 50, "coeffs_sha256": sha(np.ascontiguousarray(zz.astype("<i2")).tobytes()),
            "max_code_bits": max(lens), "max_symbol_bits": most, "bytes": len(out), "sha256": sha(out), "head": out[:64].hex()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=6)
    args = ap.parse_args()
    t0 = time.perf_counter()
    import tinyimgcodec  # noqa: F401

    res = {"generator": "tests/golden/gen/make_goldens_adaptive.py", "numpy": np.__version__}
    res["tables"] = crafted_tables()
    with Pool(args.procs) as pool:
        lc = pool.apply_async(longcode)
        res["cases"] = pool.map(image_case, image_jobs(), chunksize=1)
        print("image cases done, %.0f s" % (time.perf_counter() - t0), flush=True)
        jobs = [(i, q) for i in range(1, 50) for q in QUALITIES]
        res["benchmark"] = pool.map(bench_case, jobs, chunksize=1)
        print("benchmark pairs done, %.0f s" % (time.perf_counter() - t0), flush=True)
        res["longcode"] = lc.get()
    with open(os.path.join(GOLD, "adaptive_streams.json"), "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote adaptive_streams.json, %.0f s" % (time.perf_counter() - t0))


if __name__ == "__main__":
    main()
