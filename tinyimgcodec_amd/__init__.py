"""tinyimgcodec_amd - MI355X-native drop-in for tinyimgcodec's encode/decode/compress/decompress.

Mirrors tinyimgcodec/__init__.py:1-5 of the reference (same four names); see codec.py for the mapping, for compress_adaptive /
decompress_adaptive and their batch forms compress_batch_adaptive / decompress_batch_adaptive (the reference's per-image Huffman tables) and for compress_scaled / dctq_scaled / entropy_encode_scaled (the
reference's standalone integer encoder, c/img.c) with its batch forms compress_batch_scaled and rd_points_scaled_batch (a list of images at a
setting each; the length and round-trip error of every image x setting pair), and for rate control: compressed_size / compressed_sizes (the length of compress()'s
stream without producing it), compress_to_size (the best quality within a byte budget), their batch forms compressed_sizes_batch and
compress_batch_to_size (a list of images of any shapes in one call, a byte budget per frame) and entropy_size; and for rate-distortion
control: rd_points (size and exact round-trip error per quality), roundtrip_psnr, compress_to_psnr (the smallest stream at no less
than a PSNR), their batch forms rd_points_batch and compress_batch_to_psnr (a list of images of any shapes in one call, a PSNR target per
frame), roundtrip_sse_scaled and psnr_from_sse; and for rate control of the adaptive family: compressed_size_adaptive /
compressed_sizes_adaptive (the length of compress_adaptive()'s stream without producing it), compress_adaptive_to_size (the best quality
within a byte budget, with the image's own tables), compressed_sizes_adaptive_batch (a list of images of any shapes in one call) and
entropy_size_adaptive (the same length from coefficients, on the host); and for the way back from a stream to its coefficients:
entropy_decode (the dictionary the reference's decompress() hands to decode()), entropy_decode_zz (the int16 [N, 64] layout the entropy_*
functions take), entropy_decode_adaptive, and lossless re-tabling of stored streams, retable_adaptive / retable_default, with their batch forms
entropy_decode_zz_batch, retable_adaptive_batch and retable_default_batch (a list of streams in one call: an archive of small streams); and
for a stored stream at another quality or within a byte budget, without pixels: requantize, requantize_zz (the coefficients alone),
requantized_sizes (the length per quality, the stream read once) and requantize_to_size.
"""
from ._native import Context, NativeError, NativeUnavailable
from .codec import (compress, compress_adaptive, compress_batch, compress_batch_adaptive, compress_batch_to_psnr, compress_batch_scaled, compress_batch_to_size, compress_scaled, compress_to_psnr, compress_to_size,
                    compressed_size, compressed_sizes, compressed_sizes_batch, dctq, dctq_scaled, decode, decompress, decompress_adaptive, decompress_batch, decompress_batch_adaptive, encode, entropy_encode,
                    entropy_encode_adaptive, entropy_encode_adaptive_batch, entropy_encode_scaled, entropy_size, max_sse_for_psnr, parse_header, psnr_from_sse, rd_points, rd_points_batch, rd_points_scaled_batch,
                    roundtrip_psnr, roundtrip_sse_scaled)
from .codec import compress_adaptive_to_size, compressed_size_adaptive, compressed_sizes_adaptive, compressed_sizes_adaptive_batch, entropy_size_adaptive
from .codec import entropy_decode, entropy_decode_adaptive, entropy_decode_zz, retable_adaptive, retable_default
from .codec import entropy_decode_zz_batch, last_transcode_batch, retable_adaptive_batch, retable_default_batch
from .codec import last_requantize, requantize, requantize_to_size, requantize_zz, requantized_sizes

__version__ = "0.1.0"
__all__ = ["encode", "decode", "compress", "decompress"]
