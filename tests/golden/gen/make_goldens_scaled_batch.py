#!/usr/bin/env python3
"""Fixture for the integer encoder's batch forms (compress_batch_scaled / rd_points_scaled_batch): length and sha256 of the stream of the
reference's integer encoder for the loop of tests/cbenchmark.py over image x setting, on the whole benchmark set - the 49 images of
benchmark_set.npz at the four settings - and Lenna at the four settings.  The stream is the one make_goldens_scaled_enc.py defines and
obtains (reference_case: the unmodified C program compiled into oracle/_ref/ref_c_encode, read back with the reference's own bit reader).
Only recorded results are stored; the images are the ones benchmark_set.npz / lenna.npz already hold.

    make -C oracle ref && python tests/golden/gen/make_goldens_scaled_batch.py [--procs 8] [--every K]

scaled_batch.json: {"generator", "subset": which images of the set are recorded ("all", or the list of indices with --every K: every K-th
image plus indices 0 and 46, cbenchmark's own), "bench": {"<index>": {setting: {"bytes", "sha256"}}}, "lenna": {setting: {"bytes",
"sha256"}}}.  Lenna's four entries must equal scaled_encode.json's (checked here)."""
import argparse
import hashlib
import json
import multiprocessing
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

SETTINGS = ("best", "high", "med", "low")


def image_of(index):
    if index < 0:
        return np.load(os.path.join(GOLD, "lenna.npz"))["img"]
    return np.load(os.path.join(GOLD, "benchmark_set.npz"))["pixels"][index]


def one(job):
    from make_goldens_scaled_enc import reference_case

    index, setting = job
    stream = reference_case(image_of(index), setting, False)[0]
    return index, setting, len(stream), hashlib.sha256(stream).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--every", type=int, default=1, help="record every K-th image of the set (plus indices 0 and 46)")
    args = ap.parse_args()
    n = int(np.load(os.path.join(GOLD, "benchmark_set.npz"))["pixels"].shape[0])
    indices = sorted(set(range(0, n, args.every)) | {0, 46})
    jobs = [(i, s) for i in [-1] + indices for s in SETTINGS]
    with multiprocessing.Pool(args.procs) as pool:
        results = pool.map(one, jobs, chunksize=1)
    doc = {"generator": "tests/golden/gen/make_goldens_scaled_batch.py", "subset": "all" if len(indices) == n else indices, "bench": {}, "lenna": {}}
    for index, setting, size, digest in results:
        entry = doc["lenna"] if index < 0 else doc["bench"].setdefault(str(index), {})
        entry[setting] = {"bytes": size, "sha256": digest}
    pinned = json.load(open(os.path.join(GOLD, "scaled_encode.json")))["cases"]
    for s in SETTINGS:
        assert doc["lenna"][s] == {"bytes": pinned["lenna512_" + s]["bytes"], "sha256": pinned["lenna512_" + s]["sha256"]}, s
    for i in indices:
        print("bench %2d  " % i + "  ".join("%s %6d" % (s, doc["bench"][str(i)][s]["bytes"]) for s in SETTINGS))
    with open(os.path.join(GOLD, "scaled_batch.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote scaled_batch.json (%d images of the set x %d settings, Lenna x %d)" % (len(indices), len(SETTINGS), len(SETTINGS)))


if __name__ == "__main__":
    main()
