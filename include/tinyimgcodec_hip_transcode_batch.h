/* tinyimgcodec_hip_transcode_batch.h - the batch forms of tinyimgcodec_hip_transcode.h: many streams back to their coefficients, or from one
 * Huffman table family to the other, in one call.
 *
 * An archive is many small streams, and a single transcoding call of a small stream is almost all per-call cost (uploads, launches, read-backs,
 * synchronisations: profiles/transcode.txt).  Here the streams of a CHUNK (up to 64 frames) go up in one copy, one launch per kernel of the
 * readers' and writers' descriptor forms works on all of them, the coefficients stay on the device between the reader of one family and the
 * writer of the other, and the results come down in one copy.
 *
 * In every call frame i's result is exactly what the single call gives for that stream: bytes, length and result code.  A frame the batch
 * kernels do not take (too short for the device reader, without blocks, a header the single call refuses), give up on or flag (a damaged
 * stream, a running DC outside int16, a symbol without a default code) goes through the single call behind the batch; the single call alone
 * words errors.  One bad stream never costs an archive its other frames: only null or negative arguments fail the whole call before any work
 * (TIC_E_ARG).
 *
 * rcs (may be null): rcs[i] = the code the single call returns for frame i.  Return value: TIC_OK when every frame succeeded, else the code of
 * the lowest failing index, tic_last_error() = "frame %d: " + that call's message.  n == 0: TIC_OK.  n == 1: the single call.
 * The calls leave tic_last_decode_path / _giveup / _range, tic_last_batch_phases and tic_decompress_dev's header guess as they found them.
 *
 * A header of its own because the test suite pins tinyimgcodec_hip_transcode.h name by name; bound from a fourth table
 * (TRANSCODE_BATCH_SIGNATURES of the Python mirror).  Same library, same conventions. */
#ifndef TINYIMGCODEC_HIP_TRANSCODE_BATCH_H
#define TINYIMGCODEC_HIP_TRANSCODE_BATCH_H

#include "tinyimgcodec_hip_transcode.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tic_entropy_decode of n default-table or scaled_dct streams: frame i's coefficients (zz16 layout) to coeffs[i], which holds cap_blocks[i]
 * blocks; hs / ws / qualities / flags (each may be null) receive the header's fields as tic_entropy_decode returns them, for every frame whose
 * header the single call accepts.  Nothing is written behind block tic_num_blocks(h, w) of any coeffs[i]. */
int tic_entropy_decode_batch(tic_ctx *ctx, const uint8_t *const *streams, const size_t *lens, int n, int16_t *const *coeffs, const size_t *cap_blocks,
                             int *hs, int *ws, int *qualities, uint32_t *flags, int *rcs);
/* tic_retable_adaptive of n default-table streams: frame i's stream with its own tables to outs[i] (caps[i] bytes), its length to out_lens[i] -
 * the needed length where rcs[i] is TIC_E_SPACE, as the single call sets it. */
int tic_retable_adaptive_batch(tic_ctx *ctx, const uint8_t *const *streams, const size_t *lens, int n, uint8_t *const *outs, const size_t *caps,
                               size_t *out_lens, int *rcs);
/* tic_retable_default of n streams with embedded tables, the same way. */
int tic_retable_default_batch(tic_ctx *ctx, const uint8_t *const *streams, const size_t *lens, int n, uint8_t *const *outs, const size_t *caps,
                              size_t *out_lens, int *rcs);
/* How the last of the three calls above went: frames the batch kernels finished, frames that took the single call, chunks.  Any pointer may be
 * null. */
int tic_last_transcode_batch(tic_ctx *ctx, int *batch_frames, int *single_frames, int *chunks);

#ifdef __cplusplus
}
#endif
#endif /* TINYIMGCODEC_HIP_TRANSCODE_BATCH_H */
