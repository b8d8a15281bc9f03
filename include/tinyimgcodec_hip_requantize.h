/* tinyimgcodec_hip_requantize.h - a stored stream at another quality, or within a byte budget, without going through pixels.
 *
 * Re-tabling (tinyimgcodec_hip_transcode.h) keeps a stream's coefficients and saves a few per cent.  Requantisation changes them: the
 * reader of decompress() (codec.py:167-188), then block_quantize(block_quantize(c, q1, inverse=True), q2) of the reference (utils.py:48-53)
 * on every coefficient - in float64 and in this order: x = c * ((T * f1) / 100), t = x / ((T * f2) / 100), np.round(t) (half to even) -,
 * then the writer of compress() (codec.py:133-164) with q2 in the header.  No inverse transform, no uint8 clipping between the two
 * quantisers, no forward transform.  Requantising to the stream's own quality returns the stream's coefficients.
 *
 * A header of its own beside tinyimgcodec_hip.h, which it includes, for the reason tinyimgcodec_hip_adaptive_rate.h gives: the main
 * header's functions are pinned name by name by the test suite; these are bound from a table of their own (REQUANT_SIGNATURES of the
 * Python mirror).  Same library, same conventions.  Coefficients are in the zz16 layout of tic_dctq / tic_entropy_decode: int16 [N][64],
 * zig-zag order, absolute DC.
 *
 * Out of scope: streams with embedded tables as INPUT (tic_retable_default makes a default-table stream of one, losslessly), the budget
 * search for adaptive OUTPUT, batch forms, PSNR targets, and TIC_QUALITY_CUSTOM (qualities here are the integers 1..99). */
#ifndef TINYIMGCODEC_HIP_REQUANTIZE_H
#define TINYIMGCODEC_HIP_REQUANTIZE_H

#include "tinyimgcodec_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nblocks blocks of coefficients from from_quality to to_quality, host buffers (out_zz may be coeffs_zz).  A quality outside 1..99:
 * TIC_E_QUALITY before any GPU work.  A result outside int16 - 110 of the 891 pairs of {1,3,7,25,33,50,75,90,99} x 1..99 produce one from
 * |c| <= 1023 - TIC_E_RANGE; out_zz is written all the same, and the elements that left int16 are unspecified there. */
int tic_requantize_zz(tic_ctx *ctx, const int16_t *coeffs_zz, size_t nblocks, int from_quality, int to_quality, int16_t *out_zz);
/* ... with both buffers resident in device memory, 16-byte aligned; the same buffer, or two that do not overlap. */
int tic_requantize_zz_dev(tic_ctx *ctx, const void *d_coeffs_zz, size_t nblocks, int from_quality, int to_quality, void *d_out_zz);
/* The store kernel's descriptor form as it is (what the tests drive it through): a list of jobs on resident buffers, 64 per launch.
 * Job k requantises the nblocks[k] >= 1 blocks from block src_block[k] of d_coeffs_zz
 * (src_blocks blocks; jobs may share their source) from from_quality[k] to to_quality[k]; the results lie back to back in d_out_zz
 * (out_blocks >= the sum of nblocks, else TIC_E_SPACE; it must not overlap the source).  range[k] = 1 where a result of job k leaves int16,
 * else 0; the call's own return value is TIC_OK then.  One host wait for the whole list. */
int tic_requantize_zz_v_dev(tic_ctx *ctx, const void *d_coeffs_zz, size_t src_blocks, int njobs, const size_t *src_block, const size_t *nblocks,
                            const int *from_quality, const int *to_quality, void *d_out_zz, size_t out_blocks, int *range);

/* A default-table stream at quality to_quality: read exactly as tic_entropy_decode reads it (long streams on the device, short or unusual
 * ones on the host, the same retry ladder), requantised on the device - the coefficients never leave it when the device reader took the
 * stream -, written with the default-table writer (adaptive = 0) or with the per-image-table writer of tic_compress_adaptive
 * (adaptive != 0).  The new header carries to_quality.
 * Refusals as tic_retable_adaptive, all before any GPU work: TIC_E_STREAM for a stream shorter than its header, for scaled_dct streams,
 * flag bit 31, a header quality outside 1..99 and negative sizes; TIC_E_QUALITY for to_quality outside 1..99.  A frame without blocks gives
 * the 16-byte header (adaptive: TIC_E_ARG, as tic_compress_adaptive).  TIC_E_RANGE for a running DC or a requantised value outside int16,
 * or a symbol without a Huffman code (the reference's writer raises KeyError).  TIC_E_SPACE with the needed length in *out_len. */
int tic_requantize(tic_ctx *ctx, const uint8_t *data, size_t len, int to_quality, int adaptive, uint8_t *out, size_t cap, size_t *out_len);

/* sizes[i] = the length tic_requantize(..., qualities[i], 0, ...) would give, or -1 where it gives no stream (TIC_E_RANGE), for nq
 * qualities: the stream is read ONCE; per 64 qualities one launch of the measuring kernel, which reads the resident
 * coefficients once and stores nothing, all queued without a host wait in between, one read-back.  Refusals as tic_requantize; a quality outside
 * 1..99 TIC_E_QUALITY before any GPU work.  A frame without blocks: 16 everywhere. */
int tic_requantized_sizes(tic_ctx *ctx, const uint8_t *data, size_t len, const int *qualities, int nq, long long *sizes);

/* The best requantised stream within a byte budget: tic_compress_to_size's contract, with tic_requantize(..., q, 0, ...) in the place of
 * tic_compress(..., q, ...) - the bisection
 *     lo = qmin, hi = qmax;  while (lo < hi) { mid = (lo + hi + 1) / 2;  if (fits(mid)) lo = mid; else hi = mid - 1; }
 * where fits(q) = "tic_requantize succeeds at q and its length <= max_bytes"; the stream of quality lo in out, lo in *quality.
 * qmax = 0 stands for the stream's own quality (the sensible ceiling: above it nothing is gained back).  When not even qmin fits:
 * TIC_E_SPACE with its length in *out_len (TIC_E_RANGE where qmin gives no stream), nothing written.  qmin < 1, qmax > 99 or
 * qmin > qmax: TIC_E_QUALITY.  The stream is read once; every round of the search (several steps of look-ahead, as
 * tic_compress_to_size) is one launch of the measuring kernel on the resident coefficients and one host wait; the chosen quality is
 * then requantised in place by the store kernel and written by the default-table writer. */
int tic_requantize_to_size(tic_ctx *ctx, const uint8_t *data, size_t len, size_t max_bytes, int qmin, int qmax, uint8_t *out, size_t cap,
                           size_t *out_len, int *quality);

/* A measurement aid, as the other *_timed calls: not part of the contract above, and the only caller of the composition (mode 2).
 * Times the kernels alone on nblocks resident blocks (16-byte aligned) at 1..64 target qualities: `warm` untimed runs, an event, `iters`
 * timed runs, an event, one submission (as tic_entropy_size_dev_timed).  mode 0: the store kernel, nq jobs into the probe workspace; mode 1:
 * the measuring kernel (behind the memset of its nq results); mode 2: the composition the measuring kernel replaces - the store kernel as
 * in mode 0, then the size kernel's descriptor form on what it wrote (behind the same memset).  *ms_total = elapsed milliseconds for the
 * `iters` runs.  sizes (may be null): the nq stream lengths of the last run, -1 where there is no stream (mode 0: zeros). */
int tic_requant_kernels_timed(tic_ctx *ctx, const void *d_coeffs_zz, size_t nblocks, int from_quality, const int *qualities, int nq, int mode,
                              int warm, int iters, float *ms_total, long long *sizes);

/* What the last tic_requantize / tic_requantized_sizes / tic_requantize_to_size / tic_requantize_zz* of this context did (any pointer may
 * be null): *route = 1 the device reader took the stream, 2 the host reader did, 0 no stream was read; *measure_launches = launches of the
 * measuring kernel (a search: one per round; tic_requantized_sizes: one per 64 qualities); *store_launches = launches of the store kernel
 * (a stream written: one); *rounds = host waits on measured sizes (a search: its rounds; tic_requantized_sizes: 1). */
int tic_last_requantize(tic_ctx *ctx, int *route, int *measure_launches, int *store_launches, int *rounds);

#ifdef __cplusplus
}
#endif
#endif /* TINYIMGCODEC_HIP_REQUANTIZE_H */
