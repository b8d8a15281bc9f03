"""tinyimgcodec_amd - MI355X-native drop-in for tinyimgcodec's encode/decode/compress/decompress.

Mirrors tinyimgcodec/__init__.py:1-5 of the reference (same four names); see codec.py for the mapping, for compress_adaptive /
decompress_adaptive (the reference's per-image Huffman tables) and for compress_scaled / dctq_scaled / entropy_encode_scaled (the
reference's standalone integer encoder, c/img.c).
"""
from ._native import Context, NativeError, NativeUnavailable
from .codec import (compress, compress_adaptive, compress_batch, compress_scaled, dctq, dctq_scaled, decode, decompress, decompress_adaptive,
                    decompress_batch, encode, entropy_encode, entropy_encode_adaptive, entropy_encode_scaled, parse_header)

__version__ = "0.1.0"
__all__ = ["encode", "decode", "compress", "decompress"]
