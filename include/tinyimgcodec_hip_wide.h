/* tinyimgcodec_hip_wide.h - the entropy stage of compress() for integer images outside 0..255.
 *
 * tic_encode_wide returns what the reference's encode() returns for such an image: int32 DC DIFFERENCES and int32 AC values.  The
 * reference's compress() (codec.py:133-164) codes exactly those arrays, so a stream exists whenever every difference and every AC value
 * has a Huffman code (|difference| < 2,048, |AC| < 1,024) - whatever the running DC adds up to.  tic_entropy_encode takes the zz16 layout
 * with its absolute int16 DC and cannot express a running DC beyond +-32,767 (a ramp of 12-bit flat blocks passes it within a few
 * blocks); the function here takes the differences themselves.  The decoders read such streams already (tic_entropy.h: DcWide).
 *
 * A header of its own beside tinyimgcodec_hip.h, which it includes, for the reason tinyimgcodec_hip_adaptive_rate.h gives: the main
 * header's functions are pinned name by name by the test suite; this one is bound from a table of its own (WIDE_SIGNATURES of the Python
 * mirror).  Same library, same conventions.  Host code only: no context, no device. */
#ifndef TINYIMGCODEC_HIP_WIDE_H
#define TINYIMGCODEC_HIP_WIDE_H

#include "tinyimgcodec_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* compress()'s writer on the arrays of tic_encode_wide / tic_encode: dc int32 [N] (differences, first block raw), ac int32 [N][63],
 * N = tic_num_blocks(h, w); the 16-byte header and the default-table payload, byte for byte the reference's stream.  cap as
 * tic_entropy_encode (tic_compress_bound(h, w) always suffices).  TIC_E_RANGE where the reference raises KeyError: a difference of
 * magnitude 2,048 or more, an AC value of magnitude 1,024 or more; TIC_E_QUALITY outside 1..99; TIC_E_SPACE when cap is short. */
int tic_entropy_encode_dpcm(const int32_t *dc, const int32_t *ac, int h, int w, int quality, uint8_t *out, size_t cap, size_t *out_len);

#ifdef __cplusplus
}
#endif
#endif /* TINYIMGCODEC_HIP_WIDE_H */
