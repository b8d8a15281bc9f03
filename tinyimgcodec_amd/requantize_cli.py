#!/usr/bin/env python3
"""Rewrites a stored .img stream at a lower quality, or within a byte budget, without going through pixels.

    python -m tinyimgcodec_amd.requantize_cli input.img output.img (--quality Q | --max-bytes N) [--adaptive]

--quality Q: the stream's coefficients dequantised with its own quality's divisors and quantised with those of Q (requantize).
--max-bytes N: the highest quality, no higher than the stream's own, at which the requantised stream has at most N bytes
(requantize_to_size); the file is left unwritten and the exit status is 1 when not even quality 1 fits.
--adaptive: the output carries its image's own Huffman tables (with --quality only: the budget search writes default tables).

The input is a default-table stream (retable_cli --to default makes one of a stream with an embedded table, losslessly).  Prints
"<in> -> <out> bytes (<saving> %) at quality <q>".  Runs on the MI355X path (no CPU fallback)."""
import argparse
import sys


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("input")
    ap.add_argument("output")
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument("--quality", type=int, help="the target quality, 1..99")
    how.add_argument("--max-bytes", type=int, help="the byte budget of the output")
    ap.add_argument("--adaptive", action="store_true", help="write the image's own Huffman tables (with --quality)")
    args = ap.parse_args(argv)
    if args.adaptive and args.max_bytes is not None:
        ap.error("--adaptive goes with --quality: the budget search writes default tables")
    from . import requantize, requantize_to_size

    with open(args.input, "rb") as f:
        data = f.read()
    if args.quality is not None:
        out, q = requantize(data, args.quality, adaptive=args.adaptive), args.quality
    else:
        try:
            out, q = requantize_to_size(data, args.max_bytes)
        except ValueError as e:
            print(f"{args.input}: {e}", file=sys.stderr)
            return 1
    print(f"{len(data)} -> {len(out)} bytes ({100.0 * (len(data) - len(out)) / len(data):.1f} %) at quality {q}")
    with open(args.output, "wb") as f:
        f.write(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
