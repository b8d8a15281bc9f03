"""What a second quantisation costs: the table of README.md beside requantize().  CPU only - the oracle and the plain numpy model of
tests/requantize_common.py; no GPU, no library call but psnr_from_sse.

For the 49 benchmark images and the pairs 90 -> 50 and 50 -> 10: the bytes and the exact round-trip PSNR against the ORIGINAL image of
  requantize(s, q)              the stream's coefficients through the model, the oracle's writer
  compress(decompress(s), q)    through pixels
  compress(image, q)            from the original, which an archive owner no longer has
Usage: python tools/requantize_quality_table.py   (about two minutes)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import requantize_common as RC  # noqa: E402
from oracle import pyoracle as O  # noqa: E402
from tinyimgcodec_amd.codec import psnr_from_sse  # noqa: E402

px = np.load(os.path.join(ROOT, "tests", "golden", "benchmark_set.npz"))["pixels"]


def sse(a, b):
    return int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum())


for q1, q2 in ((90, 50), (50, 10)):
    tot = {k: [0, 0] for k in ("requantize(s, q)", "compress(decompress(s), q)", "compress(image, q)")}
    src = 0
    for img in px:
        h, w = img.shape
        s = O.compress(img, q1)
        src += len(s)
        info = RC.requantized_info(O.encode_zz16(img, q1), {"height": h, "width": w, "quality": q1}, q2)
        streams = (O.entropy_encode(info["dc"], info["ac"], h, w, q2), O.compress(O.decompress(s), q2), O.compress(img, q2))
        for k, st in zip(tot, streams):
            tot[k][0] += len(st)
            tot[k][1] += sse(O.decompress(st), img)
    print("%d -> %d: source %d bytes" % (q1, q2, src))
    for k, (b, e) in tot.items():
        print("  %-28s %9d bytes  %.3f dB" % (k, b, psnr_from_sse(e, px.size)))
