#!/usr/bin/env python3
"""Fixtures of the adaptive batch encoder (compress_batch_adaptive): compress(image, q, auto_generate_huffman_table=True) of the
UNMODIFIED reference for a small set of frames of different shapes and qualities, run with the import recipe of
make_goldens_adaptive.py (stand-ins for the two absent pure-container packages; every line of codec logic is the reference's own).

    python tests/golden/gen/make_goldens_adaptive_batch.py

Writes tests/golden/adaptive_batch.json (data only): per frame its recipe ("kind", "seed"), shape and quality, the stream (hex up to
4096 bytes, else length and sha256 alone) and "decoded_sha256" = pixels of the reference's decode(encode(img, q)) (what the stream
holds).  The frames sit around the encoder's workgroup of 256 blocks (255, 256, 257 blocks), include one-symbol tables with an empty
payload (flat frames) and DC categories 12-13 (the 0/255 checker at q = 97).  "longcode" names the coefficient frame of
adaptive_streams.json (made by make_goldens_adaptive.py) by reference: the tests take it from that file.
"""
import hashlib
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "standins"))
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

INLINE_MAX = 4096

# (kind, height, width, quality); kind "noise": default_rng(seed) with seed = 1000 + position in this list
FRAMES = (("noise", 1, 1, 50), ("flat0", 8, 8, 50), ("flat255", 8, 8, 50), ("noise", 13, 21, 75), ("noise", 8, 2040, 50),
          ("noise", 8, 2048, 90), ("noise", 8, 2056, 5), ("noise", 7, 4100, 20), ("flat128", 32, 32, 50), ("noise", 64, 64, 50),
          ("checker", 64, 64, 97))


def sha(b):
    return hashlib.sha256(b).hexdigest()


def make_frame(kind, seed, h, w):
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    if kind.startswith("flat"):
        return np.full((h, w), int(kind[4:]), np.uint8)
    if kind == "checker":  # 8x8 blocks alternating between 0 and 255 (raster order)
        by, bx = np.indices(((h + 7) // 8, (w + 7) // 8))
        return np.kron(np.where((by + bx) % 2 == 0, 0, 255).astype(np.uint8), np.ones((8, 8), np.uint8))[:h, :w]
    raise KeyError(kind)


def main():
    import tinyimgcodec as ref

    frames = []
    for k, (kind, h, w, q) in enumerate(FRAMES):
        img = make_frame(kind, 1000 + k, h, w)
        out = ref.compress(img, quality=q, auto_generate_huffman_table=True)
        info = ref.encode(img, q)
        info["scaled_dct"] = False
        dec = ref.decode(info)
        e = {"kind": kind, "seed": 1000 + k, "height": h, "width": w, "quality": q, "bytes": len(out), "sha256": sha(out),
             "decoded_sha256": sha(np.ascontiguousarray(dec).tobytes())}
        if len(out) <= INLINE_MAX:
            e["stream"] = out.hex()
        frames.append(e)
        print("%-8s %4d x %4d q %2d: %6d bytes" % (kind, h, w, q, len(out)), flush=True)
    res = {"generator": "tests/golden/gen/make_goldens_adaptive_batch.py", "numpy": np.__version__, "frames": frames,
           "longcode": {"file": "adaptive_streams.json", "key": "longcode"}}
    with open(os.path.join(GOLD, "adaptive_batch.json"), "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
