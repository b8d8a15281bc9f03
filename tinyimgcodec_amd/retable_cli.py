#!/usr/bin/env python3
"""Rewrites a stored .img stream with the other Huffman table family, losslessly (what jpegtran -optimize does for JPEG, and back).

    python -m tinyimgcodec_amd.retable_cli input.img output.img [--to adaptive|default] [--also INPUT OUTPUT]...

--to adaptive (the default): a default-table stream gets its image's own Huffman tables (retable_adaptive).
--to default: a stream with an embedded table goes back to the default tables (retable_default).
--also INPUT OUTPUT (repeatable) rewrites further files in the same call: all streams, of whatever sizes, go through ONE
retable_adaptive_batch() / retable_default_batch() - an archive of small streams pays the per-call cost once per 64 files, not per file.

The coefficients are the stream's own: nothing is transformed or quantised again, and the way there and back returns the bytes of a
stream our encoders wrote.  Prints "<in> -> <out> bytes (<saving> %)" per file.  With --also a file that cannot be rewritten is reported
on stderr, the others are written, and the exit status is 1.  Runs on the MI355X path (no CPU fallback)."""
import argparse
import sys


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--to", choices=("adaptive", "default"), default="adaptive", help="the table family of the output (default adaptive)")
    ap.add_argument("--also", nargs=2, action="append", metavar=("INPUT", "OUTPUT"), help="a further file, rewritten in the same batch call (repeatable)")
    args = ap.parse_args(argv)
    from . import retable_adaptive, retable_adaptive_batch, retable_default, retable_default_batch

    def report(data, out, name=""):
        print(f"{name}{len(data)} -> {len(out)} bytes ({100.0 * (len(data) - len(out)) / len(data):.1f} %)")

    if not args.also:
        with open(args.input, "rb") as f:
            data = f.read()
        out = (retable_adaptive if args.to == "adaptive" else retable_default)(data)
        report(data, out)
        with open(args.output, "wb") as f:
            f.write(out)
        return 0
    paths = [(args.input, args.output)] + [tuple(p) for p in args.also]
    datas = []
    for src, _ in paths:
        with open(src, "rb") as f:
            datas.append(f.read())
    outs = (retable_adaptive_batch if args.to == "adaptive" else retable_default_batch)(datas, errors="return")
    failed = 0
    for (src, dst), data, out in zip(paths, datas, outs):
        if isinstance(out, Exception):
            print(f"{src}: {type(out).__name__}: {out}", file=sys.stderr)
            failed += 1
            continue
        report(data, out, src + ": ")
        with open(dst, "wb") as f:
            f.write(out)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
