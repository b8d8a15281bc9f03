/*
 * tinyimgcodec_hip.h - C-ABI of the MI355X-native tinyimgcodec hot path (libtinyimgcodec_hip.so).
 *
 * The reference (clysto/tinyimgcodec) has no FFI of its own: its boundary is the Python function API
 * tinyimgcodec/__init__.py:1-5 -> codec.py (encode/decode/compress/decompress).  Each entry point below names
 * the reference function (file:line under /root/reference) whose work it replaces.  Conventions: plain pointers
 * and sizes, caller-owned buffers, int return codes (0 = ok, negative = error, message via tic_last_error),
 * no exceptions across the ABI, no torch types.  A tic_ctx owns one HIP device + one stream; use one context per
 * host thread (calls on the same context must not overlap).  All device work is issued on the context's own
 * stream.  There is NO CPU fallback for the transform stage: without a usable gfx950 device tic_create fails.
 *
 * Coefficient layout produced by the device stage ("zz16"): int16 [N][64], N = ceil(h/8)*ceil(w/8) blocks in
 * raster order, each block's 64 quantised coefficients in zig-zag scan order (constants.py:23-34); element 0 is
 * the quantised DC *before* DPCM (the DPCM of codec.py:34-35 is applied by the entropy stage / tic_encode).
 */
#ifndef TINYIMGCODEC_HIP_H
#define TINYIMGCODEC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TIC_OK 0
#define TIC_E_ARG -1      /* bad argument (null pointer, negative size, ...) */
#define TIC_E_QUALITY -2  /* quality outside 1..99 (reference: ZeroDivisionError / KeyError / struct.error) */
#define TIC_E_RANGE -3    /* a coefficient has no Huffman code (reference: KeyError in encode_huffman) */
#define TIC_E_SPACE -4    /* output buffer too small */
#define TIC_E_STREAM -5   /* malformed / unsupported stream */
#define TIC_E_HIP -6      /* HIP runtime error (see tic_last_error) */
#define TIC_E_NODEVICE -7 /* no gfx950 device / extension unusable */
#define TIC_E_BUSY -8     /* an asynchronous call has not finished yet (tic_async_result with wait == 0) */

/* kernel variants of the transform stage (all bit-identical in output) */
#define TIC_QUALITY_CUSTOM 0 /* the quality installed with tic_set_custom_quality (any number in [1, 99]) */
#define TIC_KERNEL_AUTO 0
#define TIC_KERNEL_EXACT 1  /* every coefficient in pocketfft float64 operation order */
#define TIC_KERNEL_HYBRID 2 /* fp32 AAN fast path + guard band + exact rational coefficients + exact fallback */

typedef struct tic_ctx tic_ctx;

/* ---- lifecycle -------------------------------------------------------------------------------------- */
const char *tic_version(void);
/* 0 for the shipped library (it reads no environment variable); 1 for the test-hooks build of the same sources
 * (libtinyimgcodec_hip_hooks.so, -DTIC_TEST_HOOKS: csrc/tic_hooks.h lists the variables that build honours). */
int tic_build_has_test_hooks(void);
int tic_device_count(void);
/* Create a context on HIP device `device`.  NULL on failure (tic_last_error(NULL) explains). */
tic_ctx *tic_create(int device);
void tic_destroy(tic_ctx *ctx);
/* Last error message of the context (or of the failed tic_create when ctx == NULL).  Never NULL. */
const char *tic_last_error(const tic_ctx *ctx);
/* Device name / arch string of the context's device, e.g. "gfx950:sramecc+:xnack-". */
const char *tic_device_arch(const tic_ctx *ctx);

/* ---- sizes ------------------------------------------------------------------------------------------ */
/* Number of 8x8 blocks of an h x w image after pad_image (utils.py:56-61); 0 when h == 0 or w == 0. */
size_t tic_num_blocks(int h, int w);
/* Upper bound of the compressed size in bytes (16-byte header + worst-case Huffman payload). */
size_t tic_compress_bound(int h, int w);

/* ---- transform stage: replaces encode() codec.py:26-43 (pad_image utils.py:56-61, level shift codec.py:29,
 *      block_slice utils.py:13-20, block_dct utils.py:32-37, block_quantize utils.py:48-53, zig-zag
 *      codec.py:32-33).  Runs on the GPU. ---------------------------------------------------------------- */

/* Host-buffer convenience form: H2D copy, kernel, D2H copy, synchronous.  image: uint8, row stride in bytes.
 * coeffs_zz: int16[N*64] (layout above). */
int tic_dctq(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, int quality,
             int16_t *coeffs_zz);

/* Same stage, reference output convention: dc int32[N] with DPCM applied (codec.py:34-35), ac int32[N*63]. */
int tic_encode(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, int quality, int32_t *dc,
               int32_t *ac);

/* The same for integer images whose values lie outside 0..255 (the reference casts with astype(int32), codec.py:29, and
 * transforms any integers): int32 pixels (row stride in ELEMENTS), float64 exact operation order on the device, int32
 * coefficients.  A drop-in edge, not a hot path.
 * Domain: exact - the reference's dc / ac, integer for integer - wherever every rounded quotient fits int32, for every int32 pixel.  `- 128`
 * is int32's wrapping subtraction as in the reference (pixels INT32_MIN .. INT32_MIN + 127 wrap to the top of the range), and so is the DC
 * difference (np.diff of an int32 array).  Where a rounded quotient leaves int32 the reference's own result is numpy's invalid cast (a
 * RuntimeWarning; INT32_MIN for either sign where it was tried) while the device's conversion saturates: nothing is promised there.  At
 * quality 10 every int32 image is inside the domain. */
int tic_encode_wide(tic_ctx *ctx, const int32_t *image, int h, int w, ptrdiff_t row_stride_elems, int quality, int32_t *dc,
                    int32_t *ac);
/* encode() / decode() with a non-integral quality (utils.py:50-53 computes with any number; the device holds one constant block
 * per integer quality): installs the constants of `quality`, any number in [1, 99], in the context's spare slot; tic_dctq,
 * tic_encode, tic_encode_wide, tic_dctq_dev and tic_idctq then take quality = TIC_QUALITY_CUSTOM to mean it. */
int tic_set_custom_quality(tic_ctx *ctx, double quality);

/* Device-resident form (what bench.py times): d_image / d_coeffs are device pointers from tic_dev_alloc.
 * Asynchronous on the context's stream; `variant` is one of TIC_KERNEL_*. */
int tic_dev_alloc(tic_ctx *ctx, size_t bytes, void **dptr);
int tic_dev_free(tic_ctx *ctx, void *dptr);
int tic_host_alloc_pinned(tic_ctx *ctx, size_t bytes, void **hptr);
int tic_host_free_pinned(tic_ctx *ctx, void *hptr);
/* Pins memory the caller already holds (hipHostRegister / hipHostUnregister).  tic_compress_batch and tic_dctq_batch copy frames
 * that lie in pinned or registered memory with rows back to back (row_stride == w, w a multiple of 8) to the device from where
 * they are; other frames are staged through the pipeline's own pinned slots (one extra host copy). */
int tic_host_register(tic_ctx *ctx, void *hptr, size_t bytes);
int tic_host_unregister(tic_ctx *ctx, void *hptr);
/* Host side of the batch pipeline and NUMA ("own pinned buffers / NUMA node" per GPU): *node = NUMA node of
 * the context's device (-1: unknown), *ncpus = CPUs of that node the process may run on.  The threads the pipeline creates
 * (staging, read-back, hand-out) bind themselves to those CPUs - never the caller's thread - unless tic_set_numa_binding(ctx, 0);
 * the pinned staging slots are placed on the device's node by hipHostMalloc itself. */
int tic_numa_info(tic_ctx *ctx, int *node, int *ncpus);
int tic_set_numa_binding(tic_ctx *ctx, int enable);
/* How the last batch call took its input: frames copied from the caller's pinned/registered memory / frames staged. */
int tic_last_batch_input_path(tic_ctx *ctx, int *direct_frames, int *staged_frames);
/* Where the last tic_compress_batch / tic_dctq_batch call spent its time: ms8[0] staging copies into pinned memory (pageable
 * input) or registration of the caller's frames, [1] enqueueing (H2D copy, kernels, length copies), [2] waiting for chunks,
 * [3] stream read-back, [4] hand-out into the caller's buffers, [5] waiting for a free slot; [6], [7] unused.  Sums over the
 * call per pipeline thread (0, 1, 5: the submitting thread; 2, 3: the reading thread; 4: the hand-out thread): they overlap. */
int tic_last_batch_phases(tic_ctx *ctx, double *ms8);
/* Pageable frames handed to the batch entry points are pinned IN PLACE for the duration of the call (one hipHostRegister over
 * the address range of the batch, or of a chunk, when the frames lie close together; unregistered before the call returns) and
 * read by the copy engine where they lie; frames that lie scattered, and ranges that cannot be registered, are staged through the
 * pipeline's pinned slots by copy threads.  enable = 0 stages everything (rounds 1-3).  tic_last_batch_auto_registered: how
 * many frames of the last batch call took the registered route (they also count as "direct" in tic_last_batch_input_path). */
int tic_set_auto_register(tic_ctx *ctx, int enable);
int tic_last_batch_auto_registered(tic_ctx *ctx, int *frames);
int tic_memcpy_h2d(tic_ctx *ctx, void *dst, const void *src, size_t bytes);
int tic_memcpy_d2h(tic_ctx *ctx, void *dst, const void *src, size_t bytes);
int tic_memset_dev(tic_ctx *ctx, void *dst, int value, size_t bytes);
int tic_sync(tic_ctx *ctx);
/* Test hook of the hooks build (the shipped library returns TIC_E_ARG and touches nothing): waits for the context's streams and fills
 * every buffer the context holds as scratch - any content is legal when a call begins - with `byte` (0..255); buffers that carry an
 * invariant between calls are left alone; tic_last_error then says how many buffers and bytes it filled and how many it kept.
 * TIC_E_BUSY while a tic_compress_dev_async or tic_decompress_dev_async ticket is open. */
int tic_test_poison(tic_ctx *ctx, int byte);
/* Test hook of the hooks build (the shipped library returns -1 and counts nothing): how many buffers the contexts of this process
 * own at the moment - counted where one is allocated and where one is freed, so that a closed context must give all of its back. */
int tic_test_live_buffers(void);
int tic_dctq_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, int quality,
                 void *d_coeffs_zz, int variant);
/* Batch form: `nframes` equally sized frames in ONE launch (grid row per frame).  Frame f starts at
 * d_images + f*frame_stride bytes and its coefficients at d_coeffs_zz + f*coeff_frame_stride bytes. */
int tic_dctq_dev_frames(tic_ctx *ctx, const void *d_images, int nframes, int h, int w, ptrdiff_t row_stride,
                        ptrdiff_t frame_stride, int quality, void *d_coeffs_zz, ptrdiff_t coeff_frame_stride,
                        int variant);
/* Times `iters` back-to-back launches of the transform kernel with HIP events recorded on the context's stream
 * (the stream the kernel is launched on).  *ms_total = elapsed milliseconds for all `iters` launches. */
int tic_dctq_dev_timed(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, int quality,
                       void *d_coeffs_zz, int variant, int iters, float *ms_total);
/* bench.py's form ("hipEvent time of the DCT+quant kernel only, >= 20 iterations after warm-up"): `warm`
 * untimed launches, an event, `iters` timed launches, an event, all in ONE submission - the first event is stamped when the last
 * warm-up launch retires with the timed launches already queued behind it (recorded on an idle stream it is stamped at once and the
 * interval opens with the first launch's submission latency).  per_launch_ms: NULL, or room for 2 * iters floats - then every timed
 * launch carries a start and a stop event on its own dispatch packet (no marker packets between the launches) and
 * per_launch_ms[2i] = duration of launch i, per_launch_ms[2i+1] = start of the first timed launch .. end of launch i. */
int tic_dctq_dev_timed_warm(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, int quality,
                            void *d_coeffs_zz, int variant, int warm, int iters, float *ms_total, float *per_launch_ms);
/* The same for the batch form (nframes frames per launch). */
int tic_dctq_dev_frames_timed(tic_ctx *ctx, const void *d_images, int nframes, int h, int w, ptrdiff_t row_stride,
                              ptrdiff_t frame_stride, int quality, void *d_coeffs_zz, ptrdiff_t coeff_frame_stride,
                              int variant, int iters, float *ms_total);
/* Cold-cache timing: launch i works on pair i % npairs of (d_images[k], d_coeffs_zz[k]); with pairs totalling well over
 * the 256 MiB Infinity Cache every launch streams from and to HBM (bench.py's roofline.cold). */
int tic_dctq_dev_timed_rotating(tic_ctx *ctx, const void *const *d_images, void *const *d_coeffs_zz, int npairs, int h,
                                int w, ptrdiff_t row_stride, int quality, int variant, int iters, float *ms_total);
/* Diagnostics: with stats enabled the HYBRID kernel counts (with a global atomic, which costs time - keep it off
 * when measuring) the blocks it had to redo on the exact path; tic_last_fallback_blocks returns the count
 * accumulated since the previous call and resets it. */
int tic_set_stats(tic_ctx *ctx, int enable);
/* Device entropy stage: which packing kernel.  max_quality < 1 (default): 8 lanes per block for every frame.  max_quality >= 1: a
 * lane per block (a wave = 64 blocks) for qualities up to it; a frame in which a block needs more than 512 bits is transparently
 * packed again with the 8-lane kernel (and the limit then drops below that quality).  Same bytes either way. */
int tic_set_entropy_lane_kernel(tic_ctx *ctx, int max_quality);
int tic_last_fallback_blocks(tic_ctx *ctx, unsigned long long *count);
/* ... and the strip kernel's other rare paths over the same launches (reset by either call): stats[0] = blocks settled in float64 by
 * the batch pass (= tic_last_fallback_blocks), [1] = strips whose rational coefficients were recomputed in the loop (a .5 tie of
 * (0,0) (0,4) (4,0) (4,4) somewhere in the strip), [2] = strips redone as a whole in the exact operation order (batch full, or all
 * eight blocks tripped), [3] = the largest batch any wave carried.  Diagnostics: no counterpart in the reference. */
int tic_last_rare_path_stats(tic_ctx *ctx, unsigned long long stats[4]);
/* What the launcher decided for the last transform launch through tic_dctq_dev / tic_dctq_dev_frames on this context: info[0] = 0 when the
 * strip kernel did not run (the exact kernel took the whole frame), 1 when it ran rows first, 2 columns first; [1] = schedule kind (0 rows
 * form: strided or team, 1 chunked, 2 round-interleaved); [2] = team count (0: no team schedule); [3], [4] = grid x, y; [5] = strips a
 * wave advances by; [6], [7] = the fast rectangle in strips, x and y.  Host bookkeeping, no device work.  Diagnostics: no counterpart
 * in the reference. */
int tic_last_strip_launch(tic_ctx *ctx, int info[8]);

/* ---- entropy stage (host): replaces the per-block loops of compress() codec.py:133-164:
 *      DC DPCM codec.py:34-35, encode_run_length huffman.py:12-33, encode_huffman huffman.py:41-63,
 *      BitBuffer bitbuffer.py:5-72, make_header codec.py:102-114. -------------------------------------------- */
int tic_entropy_encode(const int16_t *coeffs_zz, int h, int w, int quality, uint8_t *out, size_t cap,
                       size_t *out_len);

/* Entropy stage on the device (same stream bytes as tic_entropy_encode): coefficients in HBM -> stream in HBM.
 * Bits per block, a 64-bit offset scan and parallel bit packing; synchronous; cap >= tic_compress_bound(). */
int tic_entropy_encode_dev(tic_ctx *ctx, const void *d_coeffs_zz, int h, int w, int quality, void *d_out, size_t cap,
                           size_t *out_len);

/* ---- whole codec ------------------------------------------------------------------------------------- */
/* compress() with image and stream both resident in HBM: transform kernels + device entropy stage. */
int tic_compress_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, int quality, void *d_out,
                     size_t cap, size_t *out_len);
/* The same, asynchronously: the frame's launches are queued and the call returns with a ticket; up to 64 tickets may be open per
 * context.  For callers that compress resident frames back to back (compress() in a loop, /root/reference/tests/benchmark.py:12-23):
 * submission and completion are paid once per burst, not once per frame, and the transform and packing of a frame run beside the
 * packing and placing of the frame before it (two lanes inside the context).  The streams are WRITTEN in ticket order (the placing
 * kernels run on the context's stream, so anything queued on the context afterwards sees them); until a ticket is collected its input
 * must not be modified and its output not read.  tic_async_result delivers the frame's length or its error (same codes as
 * tic_compress_dev) and closes the ticket; with wait == 0 it returns TIC_E_BUSY while the frame is still in flight (tic_sync waits for
 * everything queued). */
int tic_compress_dev_async(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, int quality, void *d_out,
                           size_t cap, long long *ticket);
int tic_async_result(tic_ctx *ctx, long long ticket, int wait, size_t *out_len);
/* compress() codec.py:133 with auto_generate_huffman_table=False, host buffers: upload, GPU transform stage, GPU
 * entropy stage, download of the finished stream. */
int tic_compress(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, int quality, uint8_t *out,
                 size_t cap, size_t *out_len);

/* ---- rate control: how large a stream would be, and the best quality within a byte budget ------------------------------
 *      No counterpart in the reference, where a size is len(compress(image, q)) (codec.py:133-164; tests/benchmark.py tabulates
 *      six of them per image).  The length of a default-table stream (flag 0) is a function of the coefficients alone: the code
 *      lengths of encode_huffman (huffman.py:41-63) summed - DC category code + category bits, ZRLs, (run, size) code + size bits,
 *      the EOB that closes every block (huffman.py:12-33) - rounded up to a byte (bitbuffer.py:17-18), plus the 16-byte header. */
/* The length tic_entropy_encode would write for these coefficients (same layout: int16 [N][64] zig-zag, absolute DC), from a walk
 * that only sums lengths; TIC_E_RANGE exactly where tic_entropy_encode returns it.  Host, no GPU. */
int tic_entropy_size(const int16_t *coeffs_zz, int h, int w, size_t *bytes);
/* The same for coefficients resident in device memory, by the size kernel: one read of the coefficients, no workspace, nothing
 * written but the result.  Synchronous.  Equals the out_len of tic_entropy_encode_dev for the same buffer. */
int tic_entropy_size_dev(tic_ctx *ctx, const void *d_coeffs_zz, int h, int w, size_t *bytes);
/* Times the size kernel alone: `warm` untimed launches, an event, `iters` timed launches, an event, one submission (as
 * tic_dctq_dev_timed_warm); *ms_total = elapsed milliseconds for the `iters` launches. */
int tic_entropy_size_dev_timed(tic_ctx *ctx, const void *d_coeffs_zz, int h, int w, int warm, int iters, float *ms_total);
/* sizes[i] = the length tic_compress_dev would report at qualities[i], or -1 where it would return TIC_E_RANGE - without writing a
 * stream: per quality the transform into a workspace of the context and the size kernel, all queued on the context's stream with
 * no host wait in between, then one read-back of the nq results.  A quality outside 1..99 gives TIC_E_QUALITY before anything is
 * queued. */
int tic_stream_sizes_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, const int *qualities, int nq,
                         long long *sizes);
/* ... for an image in host memory: one upload, then the above. */
int tic_stream_sizes(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, const int *qualities, int nq,
                     long long *sizes);
/* The stream of the quality this bisection ends at, where fits(q) means "tic_compress_dev at q succeeds with a length <= max_bytes":
 *     if not fits(qmin): fail
 *     lo, hi = qmin, qmax
 *     while lo < hi: mid = (lo + hi + 1) / 2;  if fits(mid): lo = mid  else: hi = mid - 1
 *     *quality = lo
 * Where sizes do not decrease with the quality (every image measured so far; no theorem) that is the largest fitting quality of the
 * range; a quality without a code (TIC_E_RANGE) counts as not fitting.  On success d_out holds exactly the *out_len bytes
 * tic_compress_dev(..., lo, ...) produces, and no byte behind them is written.  Failures write nothing to d_out: qmin fits no code
 * TIC_E_RANGE; qmin is too large TIC_E_SPACE with *out_len = its length; the stream does not fit cap TIC_E_SPACE with *out_len = its
 * length (cap < 16: TIC_E_SPACE at once); qmin > qmax or either outside 1..99 TIC_E_QUALITY.  The search probes with
 * tic_stream_sizes_dev's machinery and may probe ahead - the middles of the next two or three steps in one submission - so the host
 * waits a few times, not once per step; the result is the bisection's. */
int tic_compress_to_size_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, size_t max_bytes, int qmin, int qmax,
                             void *d_out, size_t cap, size_t *out_len, int *quality);
/* ... with image and stream in host memory. */
int tic_compress_to_size(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, size_t max_bytes, int qmin, int qmax,
                         uint8_t *out, size_t cap, size_t *out_len, int *quality);
/* What the context's last tic_compress_to_size[_dev] did (either pointer may be null): qualities probed, and times the host waited
 * for the device (the probe submissions plus the one for the final stream). */
int tic_last_rate_search(tic_ctx *ctx, int *probes, int *host_waits);

/* ---- rate-distortion: the exact round-trip error, and the smallest stream at no more than a given error ----------------
 *      The reference's benchmark is a loop of compress -> decompress -> psnr (tests/benchmark.py:12-23, tests/cbenchmark.py:20-31).
 *      The decoder here reproduces the reference's pixels bit for bit, so the squared error between an image and
 *      decompress(compress(image, q)) is an exact integer, a function of the quantised coefficients and the image alone: the measuring
 *      kernel runs the inverse transform on resident coefficients and, instead of storing pixels, sums over the h x w pixels of the frame
 *          sums[0] = sum of d * d            d = original - decoded             (the true squared error)
 *          sums[1] = sum of (d * d) & 255    what the reference's tests/psnr.py sums: it subtracts and squares uint8 arrays
 *      No stream, no entropy stage, no decoded frame.  PSNR = 20 log10(255 / sqrt(sum / (h * w))). */
/* The kernel alone, synchronous: coefficients in the device layout (int16 [N][64] zig-zag, absolute DC), the original frame d_image
 * with its own row stride (bytes of a row behind w are never read).  scaled_exponent < 0: the float codec at `quality` (1..99, or
 * TIC_QUALITY_CUSTOM); scaled_exponent 0..62: a scaled-DCT frame as tic_idctq_scaled decodes it (`quality` is ignored; above 62
 * TIC_E_QUALITY).  Neither buffer is written.  No blocks: both sums 0. */
int tic_distortion_dev(tic_ctx *ctx, const void *d_coeffs_zz, const void *d_image, int h, int w, ptrdiff_t row_stride, int quality,
                       int scaled_exponent, uint64_t sums[2]);
/* Times the measuring kernel alone: `warm` untimed launches, an event, `iters` timed launches, an event, one submission (as
 * tic_entropy_size_dev_timed); *ms_total = elapsed milliseconds for the `iters` launches. */
int tic_distortion_dev_timed(tic_ctx *ctx, const void *d_coeffs_zz, const void *d_image, int h, int w, ptrdiff_t row_stride, int quality,
                             int scaled_exponent, int warm, int iters, float *ms_total);
/* Times idct_kernel alone the same way, on the same kind of coefficients, storing its pixels to d_out (uint8 [h][out_stride], device):
 * the launch the measuring kernel stands beside (tools/distortion_timing.py). */
int tic_idct_dev_timed(tic_ctx *ctx, const void *d_coeffs_zz, void *d_out, int h, int w, ptrdiff_t out_stride, int quality, int scaled_exponent,
                       int warm, int iters, float *ms_total);
/* Rate and distortion at every quality of a list: sizes[i] as tic_stream_sizes_dev (-1 where a coefficient has no Huffman code; the
 * sums are reported there all the same - the coefficients exist, only the entropy coder has no code for one), sse[i] / sse_wrapped[i]
 * the two sums of decompress(compress(image, qualities[i])) against the image.  One memset clears the nq results; per quality the
 * transform into the context's coefficient workspace, the size kernel and the measuring kernel are queued back to back on the
 * context's stream; one read-back.  Argument checks and their order: tic_stream_sizes_dev's (a null sse or sse_wrapped with nq > 0 is
 * TIC_E_ARG). */
int tic_rd_points_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, const int *qualities, int nq, long long *sizes,
                      uint64_t *sse, uint64_t *sse_wrapped);
/* ... for an image in host memory: one upload, then the above. */
int tic_rd_points(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, const int *qualities, int nq, long long *sizes,
                  uint64_t *sse, uint64_t *sse_wrapped);
/* The mirror of tic_compress_to_size_dev: the stream of the quality this bisection ends at, where meets(q) means "tic_compress_dev at q
 * succeeds and the squared error of its round trip is <= max_sse":
 *     if not meets(qmax): fail
 *     lo, hi = qmin, qmax
 *     while lo < hi: mid = (lo + hi) / 2;  if meets(mid): hi = mid  else: lo = mid + 1
 *     *quality = lo, *sse = its squared error
 * Where the error does not grow with the quality that is the smallest quality of the range that meets the bound - the smallest stream
 * at no less than the PSNR max_sse stands for.  On success d_out holds exactly the *out_len bytes tic_compress_dev(..., lo, ...)
 * produces, and no byte behind them is written.  Failures write nothing to d_out: qmax has a coefficient without a code TIC_E_RANGE;
 * qmax misses the bound TIC_E_SPACE (the target is out of reach) - both with *quality = qmax and *sse = its squared error, and the
 * latter with *out_len = 0; the stream does not fit cap TIC_E_SPACE with *out_len = its length, at least 16 - so *out_len tells the two
 * TIC_E_SPACE apart (cap < 16: TIC_E_SPACE at once, nothing written to any of the three); qmin > qmax or either outside 1..99
 * TIC_E_QUALITY.  Probes (transform, size kernel, measuring kernel) are queued several bisection steps ahead per submission, to the
 * depth per frame size of the size search; tic_last_rate_search reports this search too.  No blocks: the header at qmin, *sse = 0. */
int tic_compress_to_psnr_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, uint64_t max_sse, int qmin, int qmax,
                             void *d_out, size_t cap, size_t *out_len, int *quality, uint64_t *sse);
/* ... with image and stream in host memory. */
int tic_compress_to_psnr(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, uint64_t max_sse, int qmin, int qmax,
                         uint8_t *out, size_t cap, size_t *out_len, int *quality, uint64_t *sse);
/* The distortion column of the reference's tests/cbenchmark.py: the two sums of decompress(stream of the integer encoder at setting qf)
 * against the image - tic_dctq_scaled's kernel followed by the measuring kernel at exponent qf.  Arguments as tic_dctq_scaled. */
int tic_roundtrip_sse_scaled(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, int qf, uint64_t sums[2]);

/* Batch of n independent frames of identical geometry (BASELINE config 3): pinned staging buffers, two HIP
 * streams (the H2D copy of chunk c+1 overlaps the kernels of chunk c and the read-back of chunk c-1).
 * threads <= 0: entropy stage on the device (only finished streams cross PCIe); threads > 0: coefficients are
 * read back and entropy-coded on that many host worker threads.  images[i] / outs[i] are host pointers;
 * out_lens[i] receives each size. */
int tic_compress_batch(tic_ctx *ctx, const uint8_t *const *images, int n, int h, int w, ptrdiff_t row_stride,
                       int quality, uint8_t *const *outs, const size_t *caps, size_t *out_lens, int threads);
/* A batch of one chunk (up to 64 small frames) whose outs[] are the rows of one block of memory (equal distances, 8-byte aligned: a pool of
 * n x cap bytes) has its streams stored straight into that block by the read-back kernel (the block is pinned for the call; off with
 * tic_set_auto_register(ctx, 0)); bytes of outs[i] behind out_lens[i], up to the chunk's longest stream, are then NOT preserved.
 * *streams = how many streams of the last tic_compress_batch went that way. */
int tic_last_batch_zero_copy(tic_ctx *ctx, int *streams);

/* compress() (codec.py:133-164 of the reference) of n frames of ANY sizes and qualities in one call - the whole loop over image x quality of
 * the reference's tests/benchmark.py:12-23 is one call, and so is a folder of photographs of different sizes.  Frame i is hs[i] x ws[i] with
 * rows row_strides[i] bytes apart, coded at qualities[i] into outs[i] (caps[i] bytes; tic_compress_bound(hs[i], ws[i]) always suffices);
 * out_lens[i] receives its size.  Every stream is byte for byte what tic_compress gives for that frame, whatever the order of the frames.
 * Entropy stage on the device.  All arguments are checked before any work: a bad size, stride or quality, a null image or buffer is reported
 * for the first offending frame ("frame i: ...") and nothing is written.  Frames without blocks get the header-only stream; frames the batch
 * kernels do not take (more than 8,192^2 pixels, or more pixels than a chunk holds) are coded one by one behind the batch.  A coefficient
 * without a Huffman code in any frame fails the call with TIC_E_RANGE; a stream longer than caps[i] fails it with TIC_E_SPACE naming frame i
 * (other frames may have been written by then). */
int tic_compress_batch_v(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides,
                         const int *qualities, uint8_t *const *outs, const size_t *caps, size_t *out_lens);
/* How the last tic_compress_batch_v went: frames through the batch kernels / frames coded one by one / chunks / transform launches (one per
 * run of neighbouring frames of one width and quality whose heights are multiples of 8).  Any pointer may be NULL. */
int tic_last_compress_batch_v(tic_ctx *ctx, int *batch_frames, int *single_frames, int *chunks, int *transform_launches);

/* ---- rate control for a batch ------------------------------------------------------------------------------------------------------
 * tic_stream_sizes of n frames of ANY sizes in one call: sizes[i * nq + j] is what tic_stream_sizes gives for frame i at qualities[j]
 * (-1 where a coefficient has no Huffman code, 16 for a frame without blocks) - the reference's whole benchmark table
 * (tests/benchmark.py: 49 images x 6 qualities) is one call.  All arguments are checked before any work ("frame i: ..." for the first
 * offending frame, as tic_compress_batch_v).  The frames are cut into tic_compress_batch_v's chunks (64 frames, 32 MB of pixels), ordered
 * by (width, height); per chunk one upload, every probe queued - a transform launch per probe, neighbours of equal width at one quality
 * whose heights are multiples of 8 in one launch, and one launch of the size kernel's descriptor form per 64 probes - and one read-back.
 * Frames the batch does not take (tic_compress_batch_v's) go through tic_stream_sizes behind it. */
int tic_stream_sizes_v(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides,
                       const int *qualities, int nq, long long *sizes);
/* tic_compress_to_size of n frames of ANY sizes, each within its own budget max_bytes[i], over one quality range: frame i gets exactly
 * what tic_compress_to_size(image i, max_bytes[i], qmin, qmax) gives - outs[i] (caps[i] bytes), out_lens[i], qualities[i] - and status[i]:
 *     TIC_OK        the stream, its length and its quality are set; no byte of outs[i] behind out_lens[i] is written
 *     TIC_E_SPACE   qmin exceeds the budget: out_lens[i] = its length at qmin; or the chosen stream exceeds caps[i]: out_lens[i] = its length
 *     TIC_E_RANGE   qmin has a coefficient without a Huffman code
 * outs[i] is untouched on every failure.  The call returns the first non-OK status in frame order (tic_last_error: that frame's message,
 * "frame i: ..."); the other frames are delivered all the same.  Argument errors (a bad range TIC_E_QUALITY; a bad size or stride, a null
 * image, buffer or array TIC_E_ARG) are found before any work and write nothing.
 * Phase 1, per chunk of the plan above: one upload, then the bisections of all its frames in lockstep - every round one submission of
 * each unsettled frame's next middles (1 to 3 steps ahead, by the chunk's size), one read-back, one wait: at most 7 rounds for 1..99.
 * Phase 2: the streams of all fitting frames from tic_compress_batch_v at the qualities found (their pixels are uploaded a second time);
 * a length that contradicts its probe is TIC_E_HIP.  Frames the batch does not take go through tic_compress_to_size behind it. */
int tic_compress_batch_to_size(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides,
                               const size_t *max_bytes, int qmin, int qmax, uint8_t *const *outs, const size_t *caps, size_t *out_lens,
                               int *qualities, int *status);
/* How the last tic_stream_sizes_v / tic_compress_batch_to_size went: frames through the batch / frames handled one by one behind it /
 * chunks / probes queued / host waits of phase 1 (one per chunk for the sizes, one per round of a chunk for the search) / launches of the
 * size kernel's descriptor form.  Any pointer may be NULL. */
int tic_last_rate_batch(tic_ctx *ctx, int *batch_frames, int *single_frames, int *chunks, int *probes, int *search_waits, int *size_launches);

/* ---- rate-distortion for a batch ---------------------------------------------------------------------------------------------------
 * tic_rd_points of n frames of ANY sizes in one call: sizes / sse / sse_wrapped[i * nq + j] are what tic_rd_points gives for frame i at
 * qualities[j] (size -1 where a coefficient has no Huffman code, the sums reported all the same; 16 / 0 / 0 for a frame without blocks) -
 * the reference's benchmark loop compress -> decompress -> psnr over 49 images x 6 qualities (tests/benchmark.py) is one call.  Argument
 * checks and their order are tic_stream_sizes_v's; a null sse or sse_wrapped with work to do is TIC_E_ARG.  The route is
 * tic_stream_sizes_v's: per chunk one upload, one memset of both result arrays, every probe queued quality by quality - per pass over the
 * workspace the transforms, then per 64 probes one launch of the size kernel's descriptor form and one of the measuring kernel's - one
 * read-back, one wait.  Frames the batch does not take go through tic_rd_points behind it ("frame i: ..." on error). */
int tic_rd_points_v(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides,
                    const int *qualities, int nq, long long *sizes, uint64_t *sse, uint64_t *sse_wrapped);
/* tic_compress_to_psnr of n frames of ANY sizes, each against its own bound max_sse[i], over one quality range: frame i gets exactly what
 * tic_compress_to_psnr(image i, max_sse[i], qmin, qmax) gives - outs[i] (caps[i] bytes), out_lens[i], qualities[i], sse[i] - and status[i]:
 *     TIC_OK        the stream, its length, its quality and its squared error are set; no byte of outs[i] behind out_lens[i] is written
 *                   (a frame without blocks: the header at qmin, sse[i] = 0)
 *     TIC_E_RANGE   qmax has a coefficient without a Huffman code: qualities[i] = qmax, sse[i] = its error, out_lens[i] = 0
 *     TIC_E_SPACE   qmax misses the bound: qualities[i] = qmax, sse[i] = its error, out_lens[i] = 0; or the chosen stream exceeds caps[i]:
 *                   out_lens[i] = its length (at least 16), sse[i] = its error
 * outs[i] is untouched on every failure.  The call returns the first non-OK status in frame order (tic_last_error: that frame's message,
 * "frame i: ..."); the other frames are delivered all the same.  Argument errors are tic_compress_batch_to_size's, found before any work.
 * Phase 1, per chunk: one upload, then the bisections of all its frames in lockstep - every round one submission of each unsettled frame's
 * next middles (1 to 3 steps ahead, by the chunk's size; the first round qmax as well), one read-back, one wait: at most 1 + ceil(7 / depth)
 * rounds.  Phase 2: the streams of the frames that ended well from tic_compress_batch_v at the qualities found; a length that contradicts
 * its probe is TIC_E_HIP.  Frames the batch does not take go through tic_compress_to_psnr behind it. */
int tic_compress_batch_to_psnr(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides,
                               const uint64_t *max_sse, int qmin, int qmax, uint8_t *const *outs, const size_t *caps, size_t *out_lens,
                               int *qualities, uint64_t *sse, int *status);
/* tic_last_rate_batch reports the two calls above as well (size_launches stays the size launches); *sse_launches: launches of the measuring
 * kernel's descriptor form by the last of them, or by the last tic_distortion_v_dev.  The pointer may be NULL. */
int tic_last_rd_batch(tic_ctx *ctx, int *sse_launches);
/* The measuring kernel's descriptor form alone, synchronous, on n probes: probe i is the hs[i] x ws[i] frame d_images[i] (a host array of
 * device pointers; rows row_strides[i] bytes apart) against coefficients of the float codec at qualities[i].  The coefficients of all
 * probes lie back to back at d_coeffs_zz (device layout, tic_num_blocks(hs[i], ws[i]) blocks each).  sums[2 * i], sums[2 * i + 1]: probe
 * i's two sums (0, 0 without blocks).  One launch per 64 probes with blocks.  Checks as tic_distortion_dev, per probe ("probe i: ..."). */
int tic_distortion_v_dev(tic_ctx *ctx, const void *d_coeffs_zz, const void *const *d_images, int n, const int *hs, const int *ws,
                         const ptrdiff_t *row_strides, const int *qualities, uint64_t *sums);
/* Times those launches alone, as tic_distortion_dev_timed times its one: *ms_total = elapsed milliseconds for `iters` rounds of them. */
int tic_distortion_v_dev_timed(tic_ctx *ctx, const void *d_coeffs_zz, const void *const *d_images, int n, const int *hs, const int *ws,
                               const ptrdiff_t *row_strides, const int *qualities, int warm, int iters, float *ms_total);

/* The same batch spread over nctx contexts - one per GPU of the node - by ONE process: a host thread per context, contiguous
 * shards of ceil(n / nctx) frames in frame order, no exchange between the shards; out_lens in frame order.  What a caller that
 * loops over images (/root/reference/tests/benchmark.py:12-23) gets from a multi-GPU node without a launcher.  Returns the first
 * failing shard's code; *failed_ctx (may be null) = that context's index (-1: none).  Contexts must be distinct; two may share a
 * device. */
int tic_compress_batch_multi(tic_ctx *const *ctxs, int nctx, const uint8_t *const *images, int n, int h, int w,
                             ptrdiff_t row_stride, int quality, uint8_t *const *outs, const size_t *caps, size_t *out_lens,
                             int threads, int *failed_ctx);

/* Host threads the batch pipeline may use to stage pageable frames into its pinned slots (default 0: min(8, cores / 2)).  A node
 * that runs one process per GPU sets cores_of_node / local_world_size / 2 here, so that 8 ranks do not start 64 copy threads. */
int tic_set_stage_threads(tic_ctx *ctx, int threads);
int tic_get_stage_threads(tic_ctx *ctx);
/* PCI bus id of the context's device ("0000:c1:00.0"); never NULL. */
const char *tic_pci_bus_id(const tic_ctx *ctx);

/* Same batch, transform stage only (what the metric counts): per-frame coefficients land in coeffs[i]
 * (int16[N*64], host).  If coeffs == NULL the coefficients stay on the device and are discarded. */
int tic_dctq_batch(tic_ctx *ctx, const uint8_t *const *images, int n, int h, int w, ptrdiff_t row_stride,
                   int quality, int16_t *const *coeffs);

/* parse_header() codec.py:117-130 */
int tic_parse_header(const uint8_t *data, size_t len, int *h, int *w, int *quality, uint32_t *flag);

/* decode() codec.py:46-70 from coefficients: coeffs_zz int16[N*64] zig-zag with the DC already integrated
 * (np.cumsum, codec.py:53); GPU dequantise (utils.py:52) + inverse DCT in scipy's operation order
 * (utils.py:40-45) + clip + truncating uint8 cast + crop.  out: uint8[h*w], cap >= h*w. */
int tic_idctq(tic_ctx *ctx, const int16_t *coeffs_zz, int h, int w, int quality, uint8_t *out, size_t cap);

/* decode()'s scaled_dct branch, codec.py:59-62 (coefficients of the reference's C encoder, header flag 1<<30, codec.py:127-128):
 * coeffs / ANNSCALES (constants.py:37-51) * 2**exponent, inverse quantiser of quality 50, then as tic_idctq.  exponent = the
 * stream's quality field, 0..62. */
int tic_idctq_scaled(tic_ctx *ctx, const int16_t *coeffs_zz, int h, int w, int exponent, uint8_t *out, size_t cap);

/* decompress() codec.py:167-189 + decode() codec.py:46-70 for default-table streams, including those of the reference's C
 * encoder (header flag 1<<30 -> scaled_dct branch): host Huffman/RLE decode (huffman.py:36-38,66-98), GPU dequantise +
 * inverse DCT (utils.py:40-45,52) + clip + truncating uint8 cast.  out: uint8[h*w]. */
int tic_decompress(tic_ctx *ctx, const uint8_t *data, size_t len, uint8_t *out, size_t cap);
/* decompress() codec.py:167-189 of `n` streams in one call - the mirror of tic_compress_batch; what the loop of the reference's own
 * benchmark does one stream at a time (tests/benchmark.py:12-23).  Frame i: exactly what tic_decompress(ctx, streams[i], lens[i], outs[i],
 * caps[i]) gives; hs[i] / ws[i] (either array may be null) receive its geometry.  The streams of a chunk go up in one copy, are decoded by
 * ONE launch of each of the device decoder's two kernels, and their pixels come down in one copy (straight into outs[] where the frames
 * follow each other in memory).  Frames the batch kernels do not take - short or damaged streams, C-encoder streams - are decoded by
 * tic_decompress itself behind the batch.  Headers are checked before any work (first bad frame's error, nothing decoded); a decode
 * error is the first failing frame's, all other frames are complete. */
int tic_decompress_batch(tic_ctx *ctx, const uint8_t *const *streams, const size_t *lens, int n, uint8_t *const *outs, const size_t *caps,
                         int *hs, int *ws);
/* How the last tic_decompress_batch went (any pointer may be null): frames decoded by the batch kernels, frames that took the
 * single-frame call, chunks, frames whose pixels were copied straight into the caller's memory. */
int tic_last_decompress_batch(tic_ctx *ctx, int *batch_frames, int *single_frames, int *chunks, int *direct_frames);
/* ... and the work buffer of the last chunk it handed to the batch kernels' launcher (any pointer may be null): the chunk's range - the
 * stream bits one lane walks, the largest of its frames' choices -, the bytes the launcher carves out for the chunk, the bytes the
 * context held.  All zero when the call formed no chunk. */
int tic_last_decompress_batch_work(tic_ctx *ctx, int *range_bits, size_t *work_used, size_t *work_held);
/* Diagnostics: the bytes of work buffer the device decoder's launchers carve out for nframes streams with total_ranges ranges of
 * range_bits stream bits (an odd number of 32-bit words, 288 ... 2016; a stream of b bits has ceil((b - 128) / range_bits) ranges) and
 * total_blocks blocks in all.  0 for a range the decoder does not take. */
size_t tic_decode_work_bytes(size_t nframes, size_t total_ranges, size_t total_blocks, int range_bits);
/* decompress() with stream and pixels both resident in device memory - the counterpart of tic_compress_dev (decompress()
 * codec.py:167-189 between two device buffers).  d_out receives h rows of w pixels, out_stride bytes apart (out_cap: bytes of
 * the buffer); *h / *w (may be null) receive the geometry of the header.  Long streams never leave the device; short ones and
 * anything the device decoder hands to the host decoder (tic_last_decode_path / _giveup) make the round trip through host memory. */
int tic_decompress_dev(tic_ctx *ctx, const void *d_stream, size_t len, void *d_out, ptrdiff_t out_stride, size_t out_cap, int *h,
                       int *w);
/* Which Huffman decoder the context's last tic_decompress used: 1 = the device decoder (streams of >= 16,384 blocks: only the
 * stream crosses PCIe upwards, only the pixels downwards), 2 = the host decoder (short streams; any long stream in which the
 * device decoder met something unusual - the host's bit-serial path reproduces the reference's behaviour on malformed streams). */
int tic_last_decode_path(tic_ctx *ctx);
/* ... and, when the device decoder handed a long stream to the host decoder, why (0: it did not; bit 1 an incident in the stream's
 * first range, 4 a range without a synchronisation point, 8 / 16 / 32 an incident on the true chain, 2 trace overflow, 64 no block
 * produced, 128 a look-back that timed out, 256 a block that reaches behind the stream's end, 512 a running DC outside int16).
 * Bit 512: the reference integrates the DC differences as int32 (np.cumsum, codec.py:53) and transforms whatever the sum holds, so a
 * well-formed default-table or scaled_dct stream may carry a DC the int16 coefficient layout cannot (differences of +-2047 leave
 * int16 within 17 blocks; no encoder of this library or of the reference writes such a stream).  The device decoder hands the stream
 * over, and the host route gives the inverse stage the true DC in an int32 side array: tic_decompress, tic_decompress_batch (behind
 * the batch) and tic_decompress_dev decode such a stream to the reference's pixels.  The int16 layout of tic_idctq / tic_idctq_scaled
 * is unchanged and cannot express it.  Out of scope: a running DC beyond int32 (np.cumsum wraps there), and adaptive streams with a
 * DC outside int16, which stay TIC_E_STREAM (tic_decompress_adaptive). */
int tic_last_decode_giveup(tic_ctx *ctx);
/* ... and the stream bits per lane the device decoder's last run worked with (2 average blocks, 288 ... 2,016; 1,056 at least for nearly flat streams), and how many runs the
 * last long stream took: 2 = the first choice met a range without a synchronisation point and the longest range was tried.
 * Either pointer may be null.  (No counterpart in the reference: huffman.py:77-98 decodes bit by bit.) */
int tic_last_decode_range(tic_ctx *ctx, int *range_bits, int *tries);
/* tic_decompress_dev launches a long stream on a GUESS of its 16-byte header (the header of the stream this context decoded last: the
 * frames of a sequence, the images of a batch; only after two equal headers in a row) instead of reading it from device memory first;
 * the kernels echo the real header and a wrong guess costs a second decode - and nothing else: a run on a wrong guess writes no pixel
 * (the kernel that stores pixels compares the stream's first 16 bytes with the header its geometry came from), so no byte of d_out outside the real h x w is ever touched.  Returns 1 when the last tic_decompress_dev's guess held, -1 when it did not (the stream was
 * decoded again with its own header), 0 when no guess was made.  (No counterpart in the reference: decompress() codec.py:133-164 reads
 * the header from host memory.) */
int tic_last_decode_guess(tic_ctx *ctx);
/* A guess is made only after two streams in a row came with the same header, so alternating geometries never pay for one; enable = 0
 * turns the guessing off altogether for this context (every tic_decompress_dev reads the header first, tic_decompress_dev_async runs
 * synchronously), 1 (the default) back on. */
int tic_set_decode_guess(tic_ctx *ctx, int enable);
/* tic_decompress_dev, asynchronously (the counterpart of tic_compress_dev_async for decompress() in a loop,
 * /root/reference/tests/benchmark.py:19): a long stream is launched on the guess of its header on a stream of the ticket's own and the
 * call returns; up to 4 tickets may be open per context and their frames overlap on the device.  tic_decompress_async_result waits
 * (wait == 0: TIC_E_BUSY while in flight), checks what the kernels reported and, when the guess did not hold or the stream is anything
 * but a whole well-formed one, decodes it again synchronously: a ticket's outcome is always tic_decompress_dev's for the same arguments.
 * The destination must not be read before the result is collected; d_stream must stay valid until then.  Launches are ordered behind
 * everything queued on the context's stream at the time of the call; tic_sync waits for them too. */
int tic_decompress_dev_async(tic_ctx *ctx, const void *d_stream, size_t len, void *d_out, ptrdiff_t out_stride, size_t out_cap,
                             long long *ticket);
int tic_decompress_async_result(tic_ctx *ctx, long long ticket, int wait, int *h_out, int *w_out);

/* ---- per-image Huffman tables: compress(image, quality, auto_generate_huffman_table=True), codec.py:133-164 ----------------
 *      Stream: the 16-byte header with the flag word written most significant bit first (write_uint(1 << 31, 32), codec.py:111: bytes
 *      80 00 00 00), the table of write_huffman_table (codec.py:73-84: DC u16 count, per entry category:4 length:4 code; AC u16 count,
 *      per entry run:4 size:4 length:8 code; entries in the tree's depth-first leaf order), not byte-aligned, then the payload of
 *      encode_huffman (huffman.py:41-63) with the frame's own codes, zero-padded to a byte.  The tree is HuffmanTree's
 *      (huffman.py:137-194): leaves in first-occurrence order into heapq, ties broken by the heap's mechanics.  A code plus its value
 *      bits may take up to 64 bits; a deeper tree gives TIC_E_RANGE, as does a DC category or AC size above 15 (which
 *      write_huffman_table cannot store).  An image without blocks is TIC_E_ARG (the reference raises IndexError in
 *      calc_huffman_table, huffman.py:101-108).  The reference's own decompress() misreads these streams (it reads the flag
 *      little-endian, codec.py:119); tic_decompress keeps that behaviour, tic_decompress_adaptive reads them as written. */
/* Upper bound of an adaptive stream's size. */
size_t tic_compress_adaptive_bound(int h, int w);
/* Host buffers, as tic_compress: GPU transform stage, GPU symbol statistics, the table built on the host (one read-back of the
 * statistics), GPU packing with the table, download of the stream.  TIC_E_SPACE when the stream does not fit `cap` (*out_len then
 * receives the bytes needed; nothing is written). */
int tic_compress_adaptive(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, int quality, uint8_t *out,
                          size_t cap, size_t *out_len);
/* The same from int16 [N][64] zig-zag coefficients with absolute DC (the layout of tic_dctq; DPCM as codec.py:34-35): the adaptive twin
 * of tic_entropy_encode, on the GPU. */
int tic_entropy_encode_adaptive(tic_ctx *ctx, const int16_t *coeffs_zz, int h, int w, int quality, uint8_t *out, size_t cap,
                                size_t *out_len);
/* Adaptive streams for a batch of frames of any sizes, a quality each, in one call: outs[i] receives what
 * tic_compress_adaptive(images[i], hs[i], ws[i], row_strides[i], qualities[i]) writes, byte for byte.  The frames go through the mixed
 * batch's plan and pipeline (tic_compress_batch_v) in chunks of up to 64: per chunk one statistics launch, one read-back of the chunk's
 * statistics, the tables on the host, one upload, one launch each of the three packing kernels.  A frame larger than a chunk is coded
 * by tic_compress_adaptive behind the batch.
 * Every argument is checked before any work ("frame %d: ..." in tic_last_error): TIC_E_ARG for null arrays or pointers, bad geometry,
 * or a frame without blocks (the reference raises IndexError there), TIC_E_QUALITY for a quality outside 1..99.
 * A frame whose stream is longer than caps[i] is not packed and nothing is written to outs[i]; out_lens[i] receives the size needed,
 * every other frame is coded as usual, and the call returns TIC_E_SPACE at its end: out_lens[i] > caps[i] marks exactly the unwritten
 * frames.  TIC_E_RANGE (naming the frame) as tic_compress_adaptive. */
int tic_compress_batch_adaptive_v(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws,
                                  const ptrdiff_t *row_strides, const int *qualities, uint8_t *const *outs, const size_t *caps,
                                  size_t *out_lens);
/* The coefficient-domain twin: coeffs[i] = int16 [N_i][64] zig-zag coefficients with absolute DC (tic_entropy_encode_adaptive's layout);
 * the same chunks and kernels without upload of pixels or transform. */
int tic_entropy_encode_adaptive_batch(tic_ctx *ctx, const int16_t *const *coeffs, int n, const int *hs, const int *ws,
                                      const int *qualities, uint8_t *const *outs, const size_t *caps, size_t *out_lens);
/* What the last of these two calls did: frames coded in chunks, frames coded one by one behind them, chunks (null pointers are skipped). */
int tic_last_compress_batch_adaptive(tic_ctx *ctx, int *batch_frames, int *single_frames, int *chunks);
/* The table alone, on the host (calc_huffman_table huffman.py:101-108 + write_huffman_table codec.py:73-84): per symbol its count and
 * first-occurrence key (DC: index = size category, key = block; AC: index = (run << 4) | size, key = block * 64 + ordinal of the symbol
 * in the block's run-length list) -> per symbol codeword (right-aligned) and length (0 for symbols that do not occur, and for the
 * single symbol of a one-symbol tree), and the serialized table bits (MSB first, zero-padded; *table_bits = their number).
 * TIC_E_ARG when either histogram is empty, TIC_E_RANGE for a code too long (see above), TIC_E_SPACE when table_cap is short
 * (2,610 bytes always suffice). */
int tic_huffman_table_build(const uint64_t *dc_count /*16*/, const uint64_t *dc_first /*16*/, const uint64_t *ac_count /*256*/,
                            const uint64_t *ac_first /*256*/, uint64_t *dc_code /*16*/, uint8_t *dc_len /*16*/, uint64_t *ac_code /*256*/,
                            uint8_t *ac_len /*256*/, uint8_t *table, size_t table_cap, size_t *table_bits);
/* decompress() codec.py:167-189 for streams with an embedded table, read as written: Huffman decode (codes up to 64 bits), GPU
 * dequantise + inverse DCT as tic_decompress.  Strict where the reference is not: a malformed table (not a prefix code, counts out of
 * range, a code the payload meets without a symbol), a truncated stream, a block of more than 63 AC coefficients or a DC outside int16
 * give TIC_E_STREAM.  out: uint8[h*w].
 * The Huffman decode runs on the device (the table is parsed on the host and goes up as look-up tables; the coefficients never cross
 * PCIe) for every stream of >= 16,384 blocks, and for shorter ones from 1,024 blocks and 262,144 payload bits on, unless a code of its
 * tables has length zero (a flat frame's one-symbol tree).  All other streams, and any stream in which the device decoder meets
 * something unusual, take the host's bit-serial decoder, which alone decides between pixels and TIC_E_STREAM.  tic_last_decode_path
 * (1 device, 2 host) and tic_last_decode_giveup (bits: 4 the chain did not settle, 8 a window without a code or a block of more than
 * 63 AC entries, 16 the stream ends before the last block, 32 a DC outside int16) tell which. */
int tic_decompress_adaptive(tic_ctx *ctx, const uint8_t *data, size_t len, uint8_t *out, size_t cap);
/* The same with stream and pixels both resident in device memory, arguments as tic_decompress_dev: only the stream's first 2.6 KB
 * (header and table) come down; d_out receives h rows of w pixels, out_stride bytes apart, and no other byte of it is written;
 * *h / *w (may be null) receive the header's geometry.  TIC_E_SPACE (nothing written) when out_cap is short.  A stream the host decoder
 * takes makes the round trip through host memory.  A stream at a 4-byte aligned address is decoded where it lies and read in 32-bit
 * words: up to 3 bytes behind `len`, to the next 4-byte boundary, are read (and masked); any other address is copied first. */
int tic_decompress_adaptive_dev(tic_ctx *ctx, const void *d_stream, size_t len, void *d_out, ptrdiff_t out_stride, size_t out_cap, int *h,
                                int *w);
/* tic_decompress_adaptive of MANY streams in one call; arguments as tic_decompress_batch.  Frame i: what tic_decompress_adaptive(ctx,
 * streams[i], lens[i], outs[i], caps[i]) gives, geometry in hs[i] / ws[i] (either may be null).  The frames the batch kernels take - at
 * least one block, a table that parses and has no code of length zero, bit positions that fit 32 bits; no size threshold - are cut into
 * chunks in the caller's order; a chunk goes up in ONE copy (descriptors, a look-up table per frame, the streams), is decoded by one
 * launch per kernel (three rounds of the stitch with the passes and the inverse transform behind them; sixteen more rounds, once, when a
 * frame of the chunk has not settled) and comes down in ONE copy - straight into the caller's memory where the frames are dense and
 * follow each other there, else through a pinned buffer.  Every frame not taken, and every frame the kernels give up on, goes through
 * tic_decompress_adaptive afterwards, in index order; fewer than two taken frames make the whole call a loop of single calls (n == 1 is
 * exactly the single call).  Errors: the header checks of tic_decompress_adaptive run for every frame before any work (the first
 * offending frame's error, prefixed "frame %d:", nothing decoded); an error while decoding is the first one met, and every frame that
 * did not itself fail is complete.  n == 0: TIC_OK. */
int tic_decompress_batch_adaptive(tic_ctx *ctx, const uint8_t *const *streams, const size_t *lens, int n, uint8_t *const *outs,
                                  const size_t *caps, int *hs, int *ws);
/* How the last such call went: frames decoded by the batch kernels, frames that took the single call, chunks (null pointers are skipped). */
int tic_last_decompress_batch_adaptive(tic_ctx *ctx, int *batch_frames, int *single_frames, int *chunks);
/* ... and the frames of its chunks whose pixels came down straight into the caller's memory (0: every chunk went through the pinned buffer). */
int tic_last_decompress_batch_adaptive_direct(tic_ctx *ctx);
/* The device decoder's geometry for an adaptive stream of `len` bytes whose payload starts at bit `payload_bit` (128 + table bits) and
 * holds `nblocks` blocks: stream bits per lane and the number of such ranges (a workgroup walks 256 of them).  Pure arithmetic, no
 * context; TIC_E_ARG for a stream the device decoder cannot address.  Either pointer may be null. */
int tic_adaptive_decode_geometry(size_t len, size_t payload_bit, size_t nblocks, int *range_bits, size_t *nranges);

/* ---- the reference's integer encoder: c/img.c + c/encode.c, the standalone C program ("scaled DCT" streams) ------------------------
 *      The stream is what the library calls IMG_init -> IMG_encodeHeader -> IMG_encodeBlock per block in raster order ->
 *      IMG_encodeComplete produce (img.c:157-253), NOT what the command-line program writes: encode.c:47 loops on feof and appends the
 *      code of w/8 blocks of uninitialised stack behind the last strip, and its 8 KiB FIFO overwrites itself on wide frames.
 *      Header (img.c:183-192): height, width, setting qf (0 best .. 3 low), flag 1 << 30, four little-endian u32.  Per block
 *      (img.c:207-249): pixel ^ 0x80 as int8, IMG_fdct (img.c:47-125: AAN butterflies with the 8-bit constants 181, 98, 139, 334, every
 *      output of either pass truncated to int16; the AAN scale factors stay in the coefficients), IMG_quantize (img.c:194-205:
 *      sign(d) * (((QUANT >> 1) + |d|) * (65536 / (QUANT << qf)) >> 16)), DC difference, zig-zag, run lengths, the default tables, EOB after
 *      every block.  End (BB_flushBits, img.h:36-40): one byte with the 0..7 pending bits behind the last whole byte - a zero byte when the
 *      payload ends on a byte boundary: 16 + floor(P / 8) + 1 bytes for P payload bits; an image without blocks is 17 bytes.
 *      Heights and widths must be multiples of 8 (encode.c:37): anything else is TIC_E_ARG.  qf outside 0..3 is TIC_E_QUALITY.  An AC
 *      magnitude above 1,023 (possible at best only: the reference reads past AC_HUFF_TABLE[run][10] there, undefined behaviour) or a DC
 *      difference above category 11 is TIC_E_RANGE.  tic_decompress and its siblings read these streams (flag 1 << 30). */
#define TIC_SCALED_BEST 0
#define TIC_SCALED_HIGH 1
#define TIC_SCALED_MED 2
#define TIC_SCALED_LOW 3
/* Upper bound of a scaled-DCT stream's size: tic_compress_bound + the flush byte. */
size_t tic_compress_scaled_bound(int h, int w);
/* IMG_fdct + IMG_quantize (img.c:47-125, 194-205) + zig-zag of every block on the GPU, host buffers: coeffs_zz int16[N*64] in the zz16
 * layout (absolute DC), as tic_dctq. */
int tic_dctq_scaled(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, int qf, int16_t *coeffs_zz);
/* The same between device buffers, asynchronous on the context's stream (as tic_dctq_dev).  Writes exactly N * 128 bytes. */
int tic_dctq_scaled_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, int qf, void *d_coeffs_zz);
/* ... for `nframes` equally sized frames in one launch (grid row per frame), strides as tic_dctq_dev_frames; coeff_frame_stride a
 * multiple of 16. */
int tic_dctq_scaled_dev_frames(tic_ctx *ctx, const void *d_images, int nframes, int h, int w, ptrdiff_t row_stride, ptrdiff_t frame_stride,
                               int qf, void *d_coeffs_zz, ptrdiff_t coeff_frame_stride);
/* tic_dctq_dev_timed_warm for this kernel: `warm` untimed launches, an event, `iters` timed launches, an event, one submission;
 * per_launch_ms as there (NULL, or 2 * iters floats). */
int tic_dctq_scaled_dev_timed_warm(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, int qf, void *d_coeffs_zz, int warm,
                                   int iters, float *ms_total, float *per_launch_ms);
/* IMG_encodeHeader + the entropy half of IMG_encodeBlock (img.c:217-248) + IMG_encodeComplete from zz16 coefficients, on the host (no
 * GPU): the twin of tic_entropy_encode. */
int tic_entropy_encode_scaled(const int16_t *coeffs_zz, int h, int w, int qf, uint8_t *out, size_t cap, size_t *out_len);
/* The whole encoder (what `encode <width> <height> <setting>` of c/encode.c is meant to write), host buffers, every stage on the GPU. */
int tic_compress_scaled(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, int qf, uint8_t *out, size_t cap,
                        size_t *out_len);
/* ... with image and stream both resident in device memory.  cap >= tic_compress_scaled_bound(): d_out must be 16-byte aligned and
 * receives the stream straight from the placing kernel (bytes behind the stream, up to the next 16-byte unit, may be written).  A smaller
 * buffer gets exactly the stream's bytes, and nothing at all when the stream does not fit (TIC_E_SPACE). */
int tic_compress_scaled_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, int qf, void *d_out, size_t cap,
                            size_t *out_len);

/* tic_compress_scaled of n frames of ANY sizes and settings in one call (the loop of the reference's tests/cbenchmark.py over image x
 * setting): out_lens[i] bytes at outs[i] are byte for byte what tic_compress_scaled gives for frame i at qfs[i], whatever the order of the
 * frames.  Semantics as tic_compress_batch_v: every argument is checked before any work - the first offender is named "frame i: ..." and
 * nothing is written (TIC_E_ARG for a size that is no multiple of 8, a bad stride, a null image or buffer; TIC_E_QUALITY for a setting
 * outside 0..3); a frame without blocks gets the host's 17-byte stream; tic_compress_scaled_bound(hs[i], ws[i]) always suffices as caps[i];
 * a coefficient without a Huffman code fails the call with TIC_E_RANGE, a stream longer than caps[i] with TIC_E_SPACE naming frame i.
 * Frames are ordered by (setting, width, height) and travel in chunks of up to 64 frames and 32 MB of pixels: per chunk one upload, ONE
 * transform launch (the integer kernel's descriptor form), one packing and one placing launch, one read-back.  Frames a chunk cannot hold
 * go through tic_compress_scaled behind the batch. */
int tic_compress_batch_scaled_v(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides,
                                const int *qfs, uint8_t *const *outs, const size_t *caps, size_t *out_lens);
/* How the last tic_compress_batch_scaled_v went: frames through the batch kernels / frames coded one by one / chunks / transform launches
 * (one per chunk).  Any pointer may be NULL. */
int tic_last_compress_batch_scaled(tic_ctx *ctx, int *batch_frames, int *single_frames, int *chunks, int *transform_launches);
/* The integer kernel's descriptor form alone, synchronous, frames resident: d_images is a host array of n device pointers (rows
 * row_strides[i] bytes apart, any alignment); the coefficients of all frames lie back to back at d_coeffs_zz (16-byte aligned, device
 * layout, tic_num_blocks(hs[i], ws[i]) blocks each, in the caller's order).  One launch per 64 frames. */
int tic_dctq_scaled_v_dev(tic_ctx *ctx, const void *const *d_images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides,
                          const int *qfs, void *d_coeffs_zz);
/* The table of tests/cbenchmark.py in one call: for frame i and setting qfs[j], sizes[i * nq + j] is the length of tic_compress_scaled's
 * stream (-1 where a coefficient has no Huffman code; 17 for a frame without blocks) and sse[i * nq + j], sse_wrapped[i * nq + j] are the two
 * sums of tic_roundtrip_sse_scaled (reported for a -1 entry too; 0 for a frame without blocks).  Any of the three may be NULL.  Argument
 * checks as above.  Per chunk one upload, one memset of the results, and per 64 probes (a probe is a frame x setting pair) ONE transform
 * launch - a record per probe, the nq records of a frame naming the same pixels -, one launch of the size kernel and one of the measuring
 * kernel, then one read-back.  Frames a chunk cannot hold go through the single-frame calls behind the batch. */
int tic_rd_points_scaled_v(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides,
                           const int *qfs, int nq, long long *sizes, uint64_t *sse, uint64_t *sse_wrapped);
/* How the last tic_rd_points_scaled_v went.  Any pointer may be NULL. */
int tic_last_rd_scaled_batch(tic_ctx *ctx, int *batch_frames, int *single_frames, int *chunks, int *transform_launches, int *size_launches,
                             int *sse_launches);

/* ---- multi-GPU (the reference has no counterpart: it is single-process, codec.py:133-164 runs one image
 *      at a time).  One process per GPU; a batch shards by independent frames (frame i -> rank i / ceil(B/G)) with no
 *      data-path collective.  The one exchange is an all-gather of per-frame compressed sizes, so that every rank knows every
 *      frame's offset in the concatenated output: RCCL over xGMI, opened lazily (world == 1 never loads librccl).
 *      Rendezvous: rank 0 publishes the RCCL unique id as the file `rendezvous_path`, the others poll for it; pass a name
 *      unique to the launch and to the communicator (e.g. /tmp/tic_rdv_<MASTER_PORT>_<launcher pid>_<launcher start>_<seq>).
 *      RCCL with more than one rank needs one GPU per rank: it has run with a single rank only so far (no multi-GPU box
 *      was available to the build); the multi-rank flow is covered by world_size-2 tests over gloo. ---------------------- */
typedef struct tic_comm tic_comm;
int tic_comm_create(tic_ctx *ctx, int rank, int world, const char *rendezvous_path, tic_comm **out);
/* The same with the reader's acceptance window spelled out: not_before_ns = the oldest publication time (CLOCK_REALTIME) a
 * reader believes - pass the LAUNCHER's start time when ranks may start long after rank 0 published (staggered launchers, a
 * restarted worker); 0 = the calling process's own start (tic_comm_create), 1 = any age (names inside a directory that is
 * private to the launch).  timeout_ms <= 0 = two minutes. */
int tic_comm_create_ex(tic_ctx *ctx, int rank, int world, const char *rendezvous_path, uint64_t not_before_ns, int timeout_ms,
                       tic_comm **out);
int tic_comm_destroy(tic_comm *comm);
int tic_comm_rank(const tic_comm *comm);
/* NCCL_VERSION_CODE of the RCCL library the communicator runs on (0: single rank, no library loaded).  tic_comm_create refuses a
 * library whose major version is not 2: the RCCL entry points are bound through hand-written RCCL 2.x prototypes. */
int tic_comm_rccl_version(const tic_comm *comm);
int tic_comm_world(const tic_comm *comm);
const char *tic_comm_last_error(const tic_comm *comm);
/* all[r * n_mine + k] = size k of rank r (every rank passes the same n_mine; pad short shards). */
int tic_gather_sizes(tic_comm *comm, const uint64_t *mine, int n_mine, uint64_t *all);
/* In-place element-wise maximum over the ranks (also serves as a barrier: bench.py's max-over-ranks timing). */
int tic_comm_allreduce_max(tic_comm *comm, double *vals, int n);
/* The rendezvous file of tic_comm_create, usable on its own (no GPU involved): publish = exclusive creation (O_EXCL|O_NOFOLLOW,
 * 0600) under a temporary name + rename, after removing leftovers of the same name; wait = poll (timeout_ms) for a complete
 * file OWNED BY THE CALLER'S EFFECTIVE USER with `bytes` of payload published no earlier than not_before_ns (CLOCK_REALTIME;
 * 0 = the calling process's start: a file an earlier launch left behind is ignored; 1 = any age).  The poll interval doubles
 * from 50 us to 20 ms.  tinyimgcodec_amd/distributed.py builds its torch-free control channel (FileComm) on these two. */
int tic_rdv_publish(const char *path, const void *payload, size_t bytes);
int tic_rdv_wait(const char *path, void *payload, size_t bytes, int timeout_ms, uint64_t not_before_ns);

/* ---- diagnostics (not part of the drop-in surface) ------------------------------------------------------------- */
/* Runs the in-register 8x8 byte transpose used by the kernels (DPP + v_perm) and a shuffle-based formulation of
 * the same permutation on `nthreads` x 8 bytes (nthreads multiple of 256); the two outputs must be identical. */
int tic_selftest_transpose(tic_ctx *ctx, const void *host_in, void *host_dpp, void *host_ref, int nthreads);

#ifdef __cplusplus
}
#endif
#endif /* TINYIMGCODEC_HIP_H */
