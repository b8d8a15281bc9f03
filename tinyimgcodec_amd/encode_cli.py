#!/usr/bin/env python3
"""Command-line counterpart of the reference's encode.py (encode.py:1-19): image in, .img stream out.

    python -m tinyimgcodec_amd.encode_cli input.(gif|png|jpg|npy|raw) output.img [--quality 50] [--shape H W] [--scaled {best,high,med,low}]

Prints "<n> bytes" and "Compression Ratio: <w*h/n>:1" exactly as the reference does.  Inputs: anything Pillow
opens (converted to "L" as the reference does), a .npy array, or headerless 8-bit gray (.raw with --shape) so that
a box without Pillow can still feed it.  Runs on the MI355X path (no CPU fallback).

--scaled SETTING writes the stream of the reference's standalone C encoder instead (c/encode.c: `encode <width> <height> <setting>`
reading raw pixels; header flag 1 << 30); --quality is then ignored, and height and width must be multiples of 8."""
import argparse
import sys

import numpy as np


def load_gray(path, shape=None):
    if path.endswith(".npy"):
        return np.load(path)
    if path.endswith(".raw"):
        if shape is None:
            raise SystemExit(".raw input needs --shape H W")
        return np.fromfile(path, dtype=np.uint8).reshape(shape)
    from PIL import Image

    return np.asarray(Image.open(path).convert("L"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--quality", type=int, default=50)
    ap.add_argument("--shape", type=int, nargs=2, metavar=("H", "W"))
    ap.add_argument("--scaled", choices=("best", "high", "med", "low"), help="write the integer encoder's stream (c/encode.c) at this setting")
    args = ap.parse_args(argv)
    from . import compress, compress_scaled

    im = load_gray(args.input, args.shape)
    out = compress_scaled(im, args.scaled) if args.scaled else compress(im, args.quality, auto_generate_huffman_table=False)
    byte_size = len(out)
    print(f"{byte_size} bytes")
    print(f"Compression Ratio: {im.shape[1] * im.shape[0] / byte_size}:1")
    with open(args.output, "wb") as f:
        f.write(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
