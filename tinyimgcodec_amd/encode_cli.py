#!/usr/bin/env python3
"""Command-line counterpart of the reference's encode.py (encode.py:1-19): image in, .img stream out.

    python -m tinyimgcodec_amd.encode_cli input.(gif|png|jpg|npy|raw) output.img [--quality 50] [--shape H W] [--scaled {best,high,med,low}]
                                         [--adaptive] [--max-bytes N | --min-psnr DB [--min-quality 1] [--max-quality 99]]
                                         [--also INPUT OUTPUT]...

Prints "<n> bytes" and "Compression Ratio: <w*h/n>:1" exactly as the reference does.  Inputs: anything Pillow
opens (converted to "L" as the reference does), a .npy array, or headerless 8-bit gray (.raw with --shape) so that
a box without Pillow can still feed it.  Runs on the MI355X path (no CPU fallback).

--scaled SETTING writes the stream of the reference's standalone C encoder instead (c/encode.c: `encode <width> <height> <setting>`
reading raw pixels; header flag 1 << 30); --quality is then ignored, and height and width must be multiples of 8.

--max-bytes N writes the stream of the best quality in --min-quality .. --max-quality that fits N bytes (compress_to_size) and prints
"Quality: <q>" as a third line; it cannot be combined with --scaled or an explicit --quality.

--adaptive writes the stream with the image's own Huffman tables (compress_adaptive: the reference's compress(...,
auto_generate_huffman_table=True)); with --max-bytes N the stream of compress_adaptive_to_size - the same search over the smaller
streams, so the same budget buys a higher quality.  Not with --scaled, --min-psnr or --also.

--min-psnr DB writes the smallest stream of that range whose round trip reaches DB decibels (compress_to_psnr) and prints "Quality: <q>"
and "PSNR: <dB>" as third and fourth lines; the same restrictions, and not together with --max-bytes.

--also INPUT OUTPUT (repeatable) codes further files in the same call: all images, of whatever sizes, go through ONE compress_batch() at --quality,
and the two lines are printed per file.  With --scaled SETTING they go through ONE compress_batch_scaled() at that setting instead.  Not
with --max-bytes or --min-psnr."""
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
    ap.add_argument("--quality", type=int, default=None, help="default 50")
    ap.add_argument("--shape", type=int, nargs=2, metavar=("H", "W"))
    ap.add_argument("--scaled", choices=("best", "high", "med", "low"), help="write the integer encoder's stream (c/encode.c) at this setting")
    ap.add_argument("--adaptive", action="store_true", help="write the stream with the image's own Huffman tables (compress_adaptive)")
    target = ap.add_mutually_exclusive_group()
    target.add_argument("--max-bytes", type=int, metavar="N", help="write the best quality whose stream fits N bytes")
    target.add_argument("--min-psnr", type=float, metavar="DB", help="write the smallest stream whose round trip reaches DB decibels")
    ap.add_argument("--min-quality", type=int, default=None, help="with --max-bytes / --min-psnr: lowest quality tried (default 1)")
    ap.add_argument("--max-quality", type=int, default=None, help="with --max-bytes / --min-psnr: highest quality tried (default 99)")
    ap.add_argument("--also", nargs=2, action="append", metavar=("INPUT", "OUTPUT"), help="a further file, coded in the same compress_batch() / compress_batch_scaled() call (repeatable)")
    args = ap.parse_args(argv)
    searching = args.max_bytes is not None or args.min_psnr is not None
    if searching and (args.scaled or args.quality is not None):
        ap.error("--max-bytes / --min-psnr cannot be combined with --scaled or --quality")
    if not searching and (args.min_quality is not None or args.max_quality is not None):
        ap.error("--min-quality / --max-quality need --max-bytes or --min-psnr")
    if args.also and searching:
        ap.error("--also takes a plain --quality or --scaled only")
    if args.adaptive and (args.scaled or args.min_psnr is not None or args.also):
        ap.error("--adaptive cannot be combined with --scaled, --min-psnr or --also")
    from . import (compress, compress_adaptive, compress_adaptive_to_size, compress_batch, compress_batch_scaled, compress_scaled, compress_to_psnr,
                   compress_to_size)

    im = load_gray(args.input, args.shape)
    if args.also:
        paths = [(args.input, args.output)] + [tuple(p) for p in args.also]
        images = [im] + [load_gray(p[0], args.shape) for p in paths[1:]]
        if args.scaled:
            outs = compress_batch_scaled(images, args.scaled)
        else:
            outs = compress_batch(images, [50 if args.quality is None else args.quality] * len(images))
        for (_, dst), a, out in zip(paths, images, outs):
            print(f"{len(out)} bytes")
            print(f"Compression Ratio: {a.shape[1] * a.shape[0] / len(out)}:1")
            with open(dst, "wb") as f:
                f.write(out)
        return 0
    chosen = reached = None
    qrange = (1 if args.min_quality is None else args.min_quality, 99 if args.max_quality is None else args.max_quality)
    if args.adaptive and args.max_bytes is not None:
        out, chosen = compress_adaptive_to_size(im, args.max_bytes, *qrange)
    elif args.adaptive:
        out = compress_adaptive(im, 50 if args.quality is None else args.quality)
    elif args.max_bytes is not None:
        out, chosen = compress_to_size(im, args.max_bytes, *qrange)
    elif args.min_psnr is not None:
        out, chosen, reached = compress_to_psnr(im, args.min_psnr, *qrange)
    elif args.scaled:
        out = compress_scaled(im, args.scaled)
    else:
        out = compress(im, 50 if args.quality is None else args.quality, auto_generate_huffman_table=False)
    byte_size = len(out)
    print(f"{byte_size} bytes")
    print(f"Compression Ratio: {im.shape[1] * im.shape[0] / byte_size}:1")
    if chosen is not None:
        print(f"Quality: {chosen}")
    if reached is not None:
        print(f"PSNR: {reached}")
    with open(args.output, "wb") as f:
        f.write(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
