#!/usr/bin/env python3
"""Rewrites a stored .img stream with the other Huffman table family, losslessly (what jpegtran -optimize does for JPEG, and back).

    python -m tinyimgcodec_amd.retable_cli input.img output.img [--to adaptive|default]

--to adaptive (the default): a default-table stream gets its image's own Huffman tables (retable_adaptive).
--to default: a stream with an embedded table goes back to the default tables (retable_default).

The coefficients are the stream's own: nothing is transformed or quantised again, and the way there and back returns the bytes of a
stream our encoders wrote.  Prints "<in> -> <out> bytes (<saving> %)".  Runs on the MI355X path (no CPU fallback)."""
import argparse
import sys


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--to", choices=("adaptive", "default"), default="adaptive", help="the table family of the output (default adaptive)")
    args = ap.parse_args(argv)
    from . import retable_adaptive, retable_default

    with open(args.input, "rb") as f:
        data = f.read()
    out = (retable_adaptive if args.to == "adaptive" else retable_default)(data)
    print(f"{len(data)} -> {len(out)} bytes ({100.0 * (len(data) - len(out)) / len(data):.1f} %)")
    with open(args.output, "wb") as f:
        f.write(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
