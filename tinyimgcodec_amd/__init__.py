"""tinyimgcodec_amd - MI355X-native drop-in for tinyimgcodec's encode/decode/compress/decompress.

Mirrors tinyimgcodec/__init__.py:1-5 of the reference (same four names); see codec.py for the mapping, and for compress_adaptive /
decompress_adaptive (the reference's per-image Huffman tables).
"""
from ._native import Context, NativeError, NativeUnavailable
from .codec import (compress, compress_adaptive, compress_batch, dctq, decode, decompress, decompress_adaptive, decompress_batch, encode,
                    entropy_encode, entropy_encode_adaptive, parse_header)

__version__ = "0.1.0"
__all__ = ["encode", "decode", "compress", "decompress"]
