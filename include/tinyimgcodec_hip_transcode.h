/* tinyimgcodec_hip_transcode.h - from a stream back to its coefficients, and from one Huffman table family to the other without a
 * second quantisation.
 *
 * The reference's decompress() (codec.py:167-188) is two halves: a reader that fills info["dc"] and info["ac"] from the stream, and
 * decode(info) (codec.py:46-70).  tic_idctq is the second half; the functions here are the first.  Re-tabling is that reader followed by
 * the writer of compress() (codec.py:133-164) on the very dictionary the reader made: the coefficients are the stream's own, nothing is
 * transformed or quantised again (what jpegtran -optimize does for JPEG, and back).
 *
 * A header of its own beside tinyimgcodec_hip.h, which it includes, for the reason tinyimgcodec_hip_adaptive_rate.h gives: the main
 * header's functions are pinned name by name by the test suite; these are bound from a third table (TRANSCODE_SIGNATURES of the
 * Python mirror).  Same library, same conventions.
 *
 * Coefficients are in the zz16 layout of tic_dctq / tic_entropy_encode: int16 [N][64], zig-zag order, absolute DC, N = tic_num_blocks(h, w). */
#ifndef TINYIMGCODEC_HIP_TRANSCODE_H
#define TINYIMGCODEC_HIP_TRANSCODE_H

#include "tinyimgcodec_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The reader of decompress() (codec.py:167-188: read_header, the block loop of decode_huffman / decode_run_length) for default-table and
 * scaled_dct streams, with np.cumsum of the DC differences (codec.py:53) applied: the reference's reading, as tic_decompress reads - long
 * streams on the device, short or unusual ones on the host, the same retry ladder.  *h, *w, *quality and *flag (bit 30: scaled_dct, then
 * *quality is the exponent) are the header's fields (any may be null).  cap_blocks < N: TIC_E_SPACE before any byte is written; a frame
 * without blocks: TIC_OK, nothing written.  A running DC outside int16 - which the layout cannot hold and tic_idctq's callers cannot pass -
 * TIC_E_RANGE.  Header refusals as tic_decompress.  Sets tic_last_decode_path / _giveup / _range as tic_decompress does. */
int tic_entropy_decode(tic_ctx *ctx, const uint8_t *data, size_t len, int16_t *coeffs_zz, size_t cap_blocks, int *h, int *w, int *quality,
                       uint32_t *flag);
/* ... with stream and coefficients resident in device memory: the stream at any address, d_coeffs_zz 16-byte aligned.  The header is read
 * (16 bytes); tic_decompress_dev's header guess is neither used nor changed. */
int tic_entropy_decode_dev(tic_ctx *ctx, const void *d_stream, size_t len, void *d_coeffs_zz, size_t cap_blocks, int *h, int *w, int *quality,
                           uint32_t *flag);
/* Times the device reader's two launches on a resident stream: `warm` untimed runs, an event, `iters` timed runs, an event, one submission
 * (as tic_idct_dev_timed).  *ms_total = elapsed milliseconds for the `iters` runs.  The device route only: a stream the device reader does
 * not take, a stream address that is not 4-byte aligned, or a run that flags anything gives TIC_E_ARG. */
int tic_entropy_decode_dev_timed(tic_ctx *ctx, const void *d_stream, size_t len, void *d_coeffs_zz, size_t cap_blocks, int warm, int iters,
                                 float *ms_total);
/* The reader of decompress() for streams with an embedded table (codec.py:167-188 with read_huffman_table, codec.py:87-106): what
 * tic_decompress_adaptive decodes before its inverse stage, with its checks, verdicts and messages (TIC_E_STREAM, "adaptive stream: ..."). */
int tic_entropy_decode_adaptive(tic_ctx *ctx, const uint8_t *data, size_t len, int16_t *coeffs_zz, size_t cap_blocks, int *h, int *w,
                                int *quality);

/* A default-table stream rewritten with its image's own Huffman tables: the reader above, then the writer of
 * compress(..., auto_generate_huffman_table=True) (codec.py:133-164) on the same coefficients - for a stream of tic_compress the bytes of
 * tic_compress_adaptive of the same image and quality.  The coefficients stay on the device when the device reader took the stream.
 * scaled_dct streams (the flag word has room for one family), header qualities outside 1..99 and negative sizes: TIC_E_STREAM before any GPU
 * work; a frame without blocks TIC_E_ARG, as tic_compress_adaptive; a running DC outside int16 TIC_E_RANGE; TIC_E_SPACE with the needed
 * length in *out_len, as tic_compress_adaptive. */
int tic_retable_adaptive(tic_ctx *ctx, const uint8_t *data, size_t len, uint8_t *out, size_t cap, size_t *out_len);
/* ... and back: the adaptive reader, then the default-table writer of compress() (codec.py:133-164).  Header checks as
 * tic_decompress_adaptive; a symbol without a default code TIC_E_RANGE (the reference raises KeyError); a frame without blocks gives the
 * 16-byte header; TIC_E_SPACE with the needed length in *out_len, as tic_entropy_encode. */
int tic_retable_default(tic_ctx *ctx, const uint8_t *data, size_t len, uint8_t *out, size_t cap, size_t *out_len);

#ifdef __cplusplus
}
#endif
#endif /* TINYIMGCODEC_HIP_TRANSCODE_H */
