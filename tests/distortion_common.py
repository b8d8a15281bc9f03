"""Shared by tests/test_distortion_cpu.py and tests/test_distortion_gpu.py: the fixture tests/golden/distortion.json (round-trip error of
the unmodified reference, written by tests/golden/gen/make_goldens_distortion.py), the oracle's round trip, and the two sums.  No test
lives here."""
import json
import os

import numpy as np

import inverse_edges as IE
from test_rate_control_cpu import fixture_image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETTINGS = ("best", "high", "med", "low")
_cache = {}


def load_distortion():
    if "fx" not in _cache:
        with open(os.path.join(GOLDEN, "distortion.json")) as f:
            _cache["fx"] = json.load(f)
    return _cache["fx"]


def scaled_image(name):
    """The pixels of an entry of the fixture's "scaled" part (its "pixels" field says the same in words)."""
    if name == "lenna":
        return fixture_image("lenna")
    return np.load(os.path.join(GOLDEN, "benchmark_set.npz"))["pixels"][int(name[5:]) - 1]


def sums(a, b):
    """(sum of d * d, sum of (d * d) mod 256) over two equally shaped uint8 arrays."""
    assert a.shape == b.shape and a.dtype == b.dtype == np.uint8
    d = a.astype(np.int64) - b.astype(np.int64)
    e = d * d
    return int(e.sum()), int((e & 255).sum())


def block_route(oracle, img, q):
    """decode() of encode(img, q)'s coefficients without a stream in between: the oracle's divisors and inverse transform block by block
    (inverse_edges.pixels_block_idct) - what stands in where compress() has no Huffman code for a coefficient."""
    if "ie" not in _cache:
        _cache["ie"] = IE.Fixture()
    h, w = img.shape
    return IE.pixels_block_idct(_cache["ie"], oracle, oracle.encode_zz16(img, q).astype(np.int64), h, w, q, 0)


def oracle_roundtrip(oracle, img, q):
    """The oracle's decompress(compress(img, q)); the block route where compress() raises for a coefficient without a code."""
    try:
        return oracle.decompress(oracle.compress(img, q))
    except oracle.OracleError:
        return block_route(oracle, img, q)


def oracle_sums(oracle, img, q):
    return sums(img, oracle_roundtrip(oracle, img, q))
