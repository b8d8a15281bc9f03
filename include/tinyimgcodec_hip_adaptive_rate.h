/* tinyimgcodec_hip_adaptive_rate.h - rate control for streams with per-image Huffman tables (tic_compress_adaptive, the
 * reference's compress(..., auto_generate_huffman_table=True)): sizes without a stream, and the best quality within a byte budget.
 *
 * A header of its own beside tinyimgcodec_hip.h, which it includes: the functions of that header are pinned, name by name, by the
 * binding table and by the context-state records of the test suite; these functions are bound from a second table
 * (RATE_ADAPTIVE_SIGNATURES of the Python mirror) until the two are merged.  Same library, same conventions.
 *
 * The length of such a stream is a function of its symbol statistics alone: the table (HuffmanTree, huffman.py:137-194;
 * write_huffman_table, codec.py:73-84) comes from symbol counts and first-occurrence order, the payload is
 * sum over symbols of count x (code length + value bits), and the stream is 16 header bytes + ceil((table bits + payload bits) / 8). */
#ifndef TINYIMGCODEC_HIP_ADAPTIVE_RATE_H
#define TINYIMGCODEC_HIP_ADAPTIVE_RATE_H

#include "tinyimgcodec_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The length of the stream whose tables tic_huffman_table_build makes from these statistics (same arrays: DC categories 0..15, AC
 * symbols (run << 4) | size): 16 + ceil((table bits + sum of count[s] x (len[s] + value bits of s)) / 8), value bits = the category for
 * DC and s & 15 for AC.  TIC_E_ARG and TIC_E_RANGE exactly where the table build returns them.  Host, no GPU.  Every encoder of the
 * adaptive family takes its stream's length from this expression. */
int tic_adaptive_stream_size(const uint64_t *dc_count, const uint64_t *dc_first, const uint64_t *ac_count, const uint64_t *ac_first,
                             size_t *bytes);
/* The adaptive twin of tic_entropy_size: the length tic_entropy_encode_adaptive would write for these coefficients (int16 [N][64]
 * zig-zag, absolute DC), from a host walk of the symbols (DPCM, run lengths, a ZRL per 16 zeros, an EOB behind every block, trailing
 * zeros silent) and the function above.  A frame without blocks TIC_E_ARG; a DC category or AC size above 15 TIC_E_RANGE.  Host, no GPU. */
int tic_entropy_size_adaptive(const int16_t *coeffs_zz, int h, int w, size_t *bytes);

/* The statistics kernels alone, synchronous: nprobes (1..64) probes resident back to back at d_coeffs_zz, probe k of nblocks[k] >= 1
 * blocks (the DPCM restarts at every probe), in ONE launch.  kernel 0: adaptive_stats_probe_kernel_v (8 lanes per block); kernel 1:
 * adaptive_stats_v_kernel (a thread per block: the encoders' kernel).  max_groups 0: the plan's workgroups per probe; n > 0: at most n,
 * so that waves stride on small inputs (kernel 0 only).  count and first: uint64 [nprobes][272] - AC symbols at 0..255, DC categories at
 * 256..271; first = ~0 where a symbol does not occur -, err: uint32 [nprobes] (1: a DC category or AC size above 15).  Both kernels
 * give the same numbers. */
int tic_adaptive_stats_v_dev(tic_ctx *ctx, const void *d_coeffs_zz, int nprobes, const size_t *nblocks, int kernel, int max_groups,
                             uint64_t *count, uint64_t *first, uint32_t *err);
/* Times them: `warm` untimed rounds, an event, `iters` timed rounds, an event, one submission (as tic_entropy_size_dev_timed); a round is
 * the reset of the statistics and the launch.  *ms_total = elapsed milliseconds for the `iters` rounds.  Nothing is read back. */
int tic_adaptive_stats_v_dev_timed(tic_ctx *ctx, const void *d_coeffs_zz, int nprobes, const size_t *nblocks, int kernel, int max_groups,
                                   int warm, int iters, float *ms_total);

/* sizes[i] = the length tic_compress_adaptive would report at qualities[i], or -1 where it returns TIC_E_RANGE - without writing a
 * stream: per quality a transform into the rate workspace, one statistics launch per 64 probes, ONE read-back of the probes'
 * statistics with no host wait before it; tables and lengths are built on the host.  A quality outside 1..99 gives TIC_E_QUALITY
 * before anything is queued; a frame without blocks TIC_E_ARG. */
int tic_adaptive_sizes_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, const int *qualities, int nq,
                           long long *sizes);
/* ... for an image in host memory: one upload, then the above. */
int tic_adaptive_sizes(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, const int *qualities, int nq,
                       long long *sizes);
/* The bisection of tic_compress_to_size, verbatim, where fits(q) means "tic_compress_adaptive at q succeeds with a length <=
 * max_bytes"; the same look-ahead (several steps' middles per submission).  On success `out` holds exactly the *out_len bytes
 * tic_compress_adaptive(..., lo, ...) produces: the stream comes from that encoder at the quality found.  Failures as
 * tic_compress_to_size, nothing written to `out`: qmin without a stream TIC_E_RANGE; qmin too large TIC_E_SPACE with *out_len = its
 * length; the stream does not fit cap TIC_E_SPACE with *out_len = its length (cap < 16: at once); a bad range TIC_E_QUALITY; a frame
 * without blocks TIC_E_ARG. */
int tic_compress_adaptive_to_size(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, size_t max_bytes, int qmin,
                                  int qmax, uint8_t *out, size_t cap, size_t *out_len, int *quality);
/* sizes[i * nq + j] = tic_adaptive_sizes' value for frame i at qualities[j], frames of any shapes in one call: the chunks, uploads and
 * transform runs of tic_stream_sizes_v; per pass one statistics launch per 64 probes, one read-back per chunk.  Frames the batch sets
 * aside go through tic_adaptive_sizes behind it.  Every check before any work ("frame i: ..."); a frame without blocks TIC_E_ARG. */
int tic_adaptive_sizes_v(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides,
                         const int *qualities, int nq, long long *sizes);
/* What the context's last tic_adaptive_sizes[_dev|_v] or tic_compress_adaptive_to_size did (any pointer may be null): probes, times the
 * host waited for the device (the final stream's encoder counts as one), statistics launches. */
int tic_last_adaptive_rate(tic_ctx *ctx, int *probes, int *host_waits, int *stats_launches);

#ifdef __cplusplus
}
#endif
#endif /* TINYIMGCODEC_HIP_ADAPTIVE_RATE_H */
