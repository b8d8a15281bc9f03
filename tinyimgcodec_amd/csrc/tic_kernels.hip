// tic_kernels.hip - CDNA4 (gfx950) kernels of the tinyimgcodec transform stage.
//
// Replaces, on the GPU, the body of encode() (codec.py:26-43 of the reference): pad_image (utils.py:56-61),
// level shift (codec.py:29), 8x8 tiling (utils.py:13-20), 2-D DCT (utils.py:32-37), quantisation (utils.py:48-53)
// and the zig-zag gather (codec.py:32-33); and of decode() (codec.py:46-70): dequantise, inverse DCT, clip, cast.
//
// Work decomposition (wave64): one wavefront owns a strip of 8 horizontally adjacent 8x8 blocks (64x8 pixels); 8 lanes serve a block.
// Every wave-level store of coefficients is 1 KiB contiguous (8 blocks x 128 B, zig-zag order established in LDS).  No MFMA: the
// stage is a byte-in / int16-out streaming stencil, bounded by HBM (3 B per pixel).
//
// Two arithmetic paths, bit-identical results:
//   exact : float64, scipy/pocketfft operation order for all 64 coefficients (tic_math.h dct8_exact): dctq_exact_kernel - padding
//           strips, the reference kernel of the tests, the last resort of the production kernel.
//   strip : the production kernel (dctq_strip_kernel<kCols>): float32 AAN butterflies, every rounding accepted only outside a rigorous
//           guard band around the .5 ties.  Ties of the four rational coefficients are settled inside the loop in the reference's
//           float64 operation order (columns first: from the fast path's own exact column sums, rational_quad; rows first: from the
//           pixels, rational_slim); blocks with an irrational coefficient inside its band join a wave-local batch that is settled
//           behind the loop in float64 (wave_redo_block / second_level_8), and only what that cannot decide takes the exact order.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>

#include "tic_hooks.h"
#include "tic_kernels.h"
#include "tic_rd_plan.h"
#include "tic_strip_plan.h"
#include "tic_strip_lds.h"
#include "tic_math.h"

namespace tic {

// ---- cross-lane helpers ---------------------------------------------------------------------------------
// DPP controls (gfx9 encoding): quad_perm = p0 | p1<<2 | p2<<4 | p3<<6 ; row_shl:n = 0x100+n ; row_shr:n = 0x110+n
#define TIC_DPP_QP_XOR1 0xB1 /* quad_perm [1,0,3,2] */
#define TIC_DPP_QP_XOR2 0x4E /* quad_perm [2,3,0,1] */
#define TIC_DPP_ROW_SHL4 0x104 /* lane i reads lane i+4 */
#define TIC_DPP_ROW_SHR4 0x114 /* lane i reads lane i-4 */

__device__ __forceinline__ uint32_t perm_b32(uint32_t hi_src, uint32_t lo_src, uint32_t sel) {
    return __builtin_amdgcn_perm(hi_src, lo_src, sel);
}

// 8x8 byte transpose across the 8 lanes of a block.  In: lane i holds row i as (lo = px 0..3, hi = px 4..7).
// Out: lane i holds column i as (lo = rows 0..3, hi = rows 4..7).  10 VALU ops, no LDS.
__device__ __forceinline__ void transpose8x8_bytes(uint32_t &lo, uint32_t &hi, int i) {
    // stage A: exchange 4x4 byte blocks between lanes i and i^4
    uint32_t nhi = (uint32_t)__builtin_amdgcn_update_dpp((int)hi, (int)lo, TIC_DPP_ROW_SHL4, 0xf, 0x5, false);
    uint32_t nlo = (uint32_t)__builtin_amdgcn_update_dpp((int)lo, (int)hi, TIC_DPP_ROW_SHR4, 0xf, 0xa, false);
    lo = nlo;
    hi = nhi;
    // stage B: exchange 2x2 byte blocks between lanes i and i^2
    uint32_t selB = (i & 2) ? 0x03020706u : 0x05040100u;
    uint32_t plo = (uint32_t)__builtin_amdgcn_mov_dpp((int)lo, TIC_DPP_QP_XOR2, 0xf, 0xf, true);
    uint32_t phi = (uint32_t)__builtin_amdgcn_mov_dpp((int)hi, TIC_DPP_QP_XOR2, 0xf, 0xf, true);
    lo = perm_b32(plo, lo, selB);
    hi = perm_b32(phi, hi, selB);
    // stage C: exchange single bytes between lanes i and i^1
    uint32_t selC = (i & 1) ? 0x03070105u : 0x06020400u;
    plo = (uint32_t)__builtin_amdgcn_mov_dpp((int)lo, TIC_DPP_QP_XOR1, 0xf, 0xf, true);
    phi = (uint32_t)__builtin_amdgcn_mov_dpp((int)hi, TIC_DPP_QP_XOR1, 0xf, 0xf, true);
    lo = perm_b32(plo, lo, selC);
    hi = perm_b32(phi, hi, selC);
}

// Reference implementation of the same transpose with ds_bpermute shuffles (used by the self-test kernel).
__device__ __forceinline__ void transpose8x8_bytes_shfl(uint32_t &lo, uint32_t &hi, int i) {
    uint32_t row[2] = {lo, hi};
    uint32_t col_lo = 0, col_hi = 0;
    int base = (threadIdx.x & 63) & ~7;
    for (int r = 0; r < 8; r++) {
        uint32_t l = __shfl(row[0], base + r, 64), h = __shfl(row[1], base + r, 64);
        uint32_t w = (i < 4) ? l : h;
        uint32_t byte = (w >> (8 * (i & 3))) & 0xffu;
        if (r < 4)
            col_lo |= byte << (8 * r);
        else
            col_hi |= byte << (8 * (r - 4));
    }
    lo = col_lo;
    hi = col_hi;
}

// Wave-private LDS hand-off: the LDS pipeline executes one wave's DS instructions in order, so a compiler-level
// fence is all that is needed between a write phase and a read phase of the same wave.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// np.pad(..., "reflect") index (utils.py:56-61): no edge repeat, period 2(n-1); n == 1 degenerates to edge.
__device__ __forceinline__ int reflect_index(int i, int n) {
    if (i < n) return i;
    if (n >= 8) return 2 * (n - 1) - i; // padding is at most 7 samples: a single reflection
    if (n == 1) return 0;
    int p = 2 * (n - 1), j = i;
    while (j >= p) j -= p; // tiny axes only
    return j < n ? j : p - j;
}

constexpr int kWavesPerWG = 4;      // (8-wave workgroups, three per CU, measured level: profiles/r02_ab_wg8.txt)
static_assert(kWavesPerWG == kStripWavesPerWG, "tic_strip_plan.h plans for this workgroup");
constexpr int kLdsStrideDw = 68;    // dwords per block in the transpose buffer (64 + 4 pad; bank analysis in DESIGN.md)
constexpr int kZzStrideB = 144;     // bytes per block in the zig-zag staging buffer (128 + 16 pad)
constexpr int kLdsWaveBytes = 8 * kLdsStrideDw * 4; // 2176 B per wave (>= 8*144)

struct Strip {
    int by, bx;   // block coordinates of this lane's block
    bool valid;   // lane's block exists
    size_t oblk;  // raster index of the block
};

// Loads row i of the lane's block as 8 bytes (reflect padding at the right/bottom borders).
__device__ __forceinline__ void load_block_row(const uint8_t *__restrict__ img, int h, int w, long stride, bool aligned8,
                                               const Strip &s, int i, uint32_t &lo, uint32_t &hi) {
    lo = 0;
    hi = 0;
    if (!s.valid) return;
    int y = reflect_index(s.by * 8 + i, h);
    int x0 = s.bx * 8;
    const uint8_t *p = img + (long)y * stride + x0;
    if (aligned8 && x0 + 8 <= w) {
        uint2 v = *reinterpret_cast<const uint2 *>(p);
        lo = v.x;
        hi = v.y;
    } else {
        const uint8_t *rowp = img + (long)y * stride;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            uint32_t b = rowp[reflect_index(x0 + k, w)];
            if (k < 4)
                lo |= b << (8 * k);
            else
                hi |= b << (8 * (k - 4));
        }
    }
}

// Transposes 8 dwords per lane across the 8 lanes of each block through the wave's LDS buffer:
// in: lane (b,c) holds v[u] = M[u][c]; out: lane (b,u) holds v[c] = M[u][c].
__device__ __forceinline__ void transpose8x8_dwords(uint32_t *lds, int b, int i, uint32_t v[8]) {
    uint32_t *blk = lds + b * kLdsStrideDw;
#pragma unroll
    for (int u = 0; u < 8; u++) blk[u * 8 + i] = v[u];
    wave_lds_fence();
    const uint4 *rp = reinterpret_cast<const uint4 *>(blk + i * 8);
    uint4 a = rp[0], c = rp[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = c.x; v[5] = c.y; v[6] = c.z; v[7] = c.w;
    wave_lds_fence();
}

// Exact path for the lane's block: float64, pocketfft order, true IEEE division, round-half-even.
// colLo/colHi: the lane's pixel column (8 bytes).  Out: q[v] = quantised coefficient (u = i, v) as int.
__device__ __forceinline__ void exact_block(uint32_t colLo, uint32_t colHi, uint32_t *lds, int b, int i,
                                         const DctqConsts *__restrict__ C, int q[8]) {
    double c[8];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        c[r] = (double)((int)((colLo >> (8 * r)) & 0xffu) - 128);
        c[r + 4] = (double)((int)((colHi >> (8 * r)) & 0xffu) - 128);
    }
    dct8_exact(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]); // axis -2: down the column
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = (uint32_t)__double2loint(c[k]);
    transpose8x8_dwords(lds, b, i, w);
    uint32_t wh[8];
#pragma unroll
    for (int k = 0; k < 8; k++) wh[k] = (uint32_t)__double2hiint(c[k]);
    transpose8x8_dwords(lds, b, i, wh);
#pragma unroll
    for (int k = 0; k < 8; k++) c[k] = __hiloint2double((int)wh[k], (int)w[k]);
    dct8_exact(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]); // axis -1: along frequency row u = i
    const double *div = C->div + i * 8;
#pragma unroll
    for (int v = 0; v < 8; v++) {
        q[v] = (int)rint(c[v] / div[v]); // np.round(X / div): IEEE divide, half-even
        __builtin_amdgcn_sched_barrier(0); // one division at a time: keeps the register footprint of the 8 expansions small
    }
}

// Writes the lane's 8 coefficients (natural positions i*8+v) into zig-zag order in LDS, then each lane stores
// 16 bytes: a wave writes its 8 blocks as one contiguous 1 KiB segment.
__device__ __forceinline__ void store_zigzag(uint32_t *lds, int b, int i, const uint16_t zz[8], const int q[8],
                                             int16_t *__restrict__ out, const Strip &s) {
    char *blk = reinterpret_cast<char *>(lds) + b * kZzStrideB;
#pragma unroll
    for (int v = 0; v < 8; v++) *reinterpret_cast<int16_t *>(blk + zz[v]) = (int16_t)q[v];
    wave_lds_fence();
    uint4 val = *reinterpret_cast<const uint4 *>(blk + i * 16);
    wave_lds_fence();
    if (s.valid) *reinterpret_cast<uint4 *>(out + s.oblk * 64 + i * 8) = val;
}

__device__ __forceinline__ Strip make_strip(int tile, int ntiles, int tiles_x, int bw, int b) {
    Strip s;
    int ty = tile / tiles_x;
    int tx = tile - ty * tiles_x;
    s.by = ty;
    s.bx = tx * 8 + b;
    s.valid = (tile < ntiles) && (s.bx < bw);
    s.oblk = (size_t)ty * bw + s.bx;
    return s;
}

// ---------------------------------------------------------------------------------------------------------
// Kernel 1: exact path for every block.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWavesPerWG * 64) void dctq_exact_kernel(DctqArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[kWavesPerWG][kLdsWaveBytes / 4];
    a.img += (long)blockIdx.y * a.frame_stride_in; // batch: one grid row per frame
    a.out = reinterpret_cast<int16_t *>(reinterpret_cast<char *>(a.out) + (long)blockIdx.y * a.frame_stride_out);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane >> 3, i = lane & 7;
    uint32_t *lds = lds_all[wave];
    int tile = blockIdx.x * kWavesPerWG + wave;
    int ntiles = a.ntiles;
    if (a.rem_mode) { // enumerate only the strips outside the hybrid kernel's rectangle
        const int bh = a.ntiles / a.tiles_x, rw = a.tiles_x - a.fast_tx;
        const int n_right = bh * rw, n_bottom = (bh - a.fast_ty) * a.fast_tx;
        ntiles = 0;
        if (tile < n_right) {
            tile = (tile / rw) * a.tiles_x + a.fast_tx + tile % rw;
            ntiles = a.ntiles;
        } else if (tile < n_right + n_bottom) {
            const int k = tile - n_right;
            tile = (a.fast_ty + k / a.fast_tx) * a.tiles_x + k % a.fast_tx;
            ntiles = a.ntiles;
        }
    }
    Strip s = make_strip(tile, ntiles, a.tiles_x, a.bw, b);
    uint32_t lo, hi;
    load_block_row(a.img, a.h, a.w, a.stride, a.aligned8, s, i, lo, hi);
    transpose8x8_bytes(lo, hi, i);
    int q[8];
    exact_block(lo, hi, lds, b, i, a.consts, q);
    const uint4 zzv = *reinterpret_cast<const uint4 *>(a.consts->zzofs + i * 8);
    uint16_t zz[8] = {(uint16_t)zzv.x, (uint16_t)(zzv.x >> 16), (uint16_t)zzv.y, (uint16_t)(zzv.y >> 16),
                      (uint16_t)zzv.z, (uint16_t)(zzv.z >> 16), (uint16_t)zzv.w, (uint16_t)(zzv.w >> 16)};
    store_zigzag(lds, b, i, zz, q, a.out, s);
}

// ---------------------------------------------------------------------------------------------------------
// Kernel 2: the production kernel (dctq_strip_kernel below): float32 fast path behind a guard band, rational ties settled inside the
// loop from the fast path's own exact column sums, wave-local batch pass for the irrational trips.
//
// Persistent waves, each walking its strips (strip = 8 horizontally adjacent blocks) in the order the launcher chose:
// team schedule when the grid fits the chip at once, chunked schedule for larger grids (launch_dctq).
// Main loop, per strip (unrolled x3, the landing registers of the pixel loads rotate by name):
//   load   : lane 8*r + b reads the 8 bytes of pixel row r of block b -> every 8 lanes read 64 contiguous bytes; inline
//            assembly + hand-counted vmcnt keep two strips in flight.
//   xpose 0: the 8 bytes go to wave-private LDS straight out of the landing registers (one ds_write_b64 behind the counted wait);
//            lane 8*b + c reads pixel column c of block b back with eight ds_read_u8 - a byte transpose without a vector instruction.
//   pass 1 : float32 AAN DOWN the pixel column held by the lane - the reference's pass order (utils.py:33-37: axis -2 first).  Outputs
//            0 and 4 are the column's sum and alternating sum: exact integers, the very numbers the reference's float64 row pass
//            starts from for the four rational coefficients (0,0) (0,4) (4,0) (4,4).  The level shift is folded into output 0.
//   xpose 1: 8x8 dword transpose per block through wave-private LDS: eight lane-linear planes, one per output of pass 1, written with
//            ds_write_addtid_b32 (no address register) and read back 32 contiguous bytes per lane, conflict-free (tic_strip_lds.h);
//            lane 8*b + u then holds frequency row u.
//   pass 2 : float32 AAN along that row; quantise with the magic-number rounding trick; the guard test is the largest distance
//            to the rounded value per lane against three per-row thresholds.
//   ties   : if one of the four rational coefficients tripped anywhere in the strip (an exact .5 tie: 2.2 % of random blocks at q = 50,
//            most blocks of posterised, two-level and flat content), ALL 32 rational coefficients of the strip are recomputed in the
//            reference's float64 operation order by the 64 lanes at once (rational_quad: column sums re-read from xpose 1's buffer,
//            two DPP exchanges, one division) and written over the fast path's values in the zig-zag staging.  ~40 instructions;
//            rounds 2-4 took the pixels through a byte transpose, v_sad_u8 and three DPP butterflies per tie block after the loop.
//   store  : int16 results packed two to a dword, four lane-linear stores into staging planes, the lane that stores chunk k of the
//            block gathers its eight scan positions with eight ds_read_u16 (rows first: scattered to zig-zag order in LDS, read back
//            16 B per lane); 16 B per lane, 1 KiB contiguous per wave.
//   trips  : blocks in which one of the 60 irrational coefficients tripped its guard band (0.2 % of random blocks at q = 50, 0.9 % at
//            q = 90) join the wave's batch and are settled after the loop in float64.
// ---------------------------------------------------------------------------------------------------------
constexpr int kTWaveBytes = kTPlaneWaveBytes;     // 2448 B: transpose buffer.  Columns first: eight lane-linear planes (tic_strip_lds.h);
                                                  // rows first: two halves of 256 dwords; the rare paths behind the loop: 8 x 68 dwords
static_assert(kTWaveBytes >= kLdsWaveBytes && kTWaveBytes % 16 == 0, "transpose8x8_dwords keeps its own layout in the same buffer");
constexpr int kZzWaveBytes = 8 * kZzStrideB;      // 1152 B zig-zag staging per wave (columns first: four planes, 1052 B; store_zigzag behind the
                                                  // loop: 8 x 144 B); its first 640 B double as the byte-transpose buffer
static_assert(kZPlaneWaveBytes <= kZzWaveBytes, "the staging planes fit the zig-zag buffer");
constexpr int kPxBlkBytes = 80;                   // byte-transpose buffer: 64 pixel bytes per block + 16 (bank spread of the b64 writes)
constexpr int kChunkStrips = 8;                   // chunked schedule: strips per wave (a workgroup streams 32 adjacent strips).  With the
                                                  // sc1 nt stores 8 beats round 2's 16: 256 x 1080p 270 against 288 us, 8192^2 37.3 against
                                                  // 38.4, 16384^2 120 against 121 (profiles/r03_ab_chunk.txt)

// Quantiser of the fast path: s = RN(z*mul + magic) is rint(z*mul) of the EXACT product (one rounding, half-even; adding
// kMagic = 1.5 * 2^23 puts the integer's two's complement into the low mantissa bits: no v_rndne / v_cvt), d = RN(z*mul - rint(z*mul))
// is the distance that feeds the guard-band test.  Three instructions per coefficient (v_fmaak, v_sub, v_fmac); the product is
// never rounded on its own, which is what tools/fastpath_error_bound.py's "multiplier" term assumes.
__device__ __forceinline__ void quant_fma(float z, float mul, uint32_t &bits, float &d) {
    const float s = fmaf(z, mul, kMagic);
    bits = __float_as_uint(s);
    const float nr = kMagic - s; // -rint(z*mul), exact
    d = fmaf(z, mul, nr);
}

// Coefficient stores: 16 B per lane, write-through and non-temporal (`sc1 nt`).  Write-through: the launch does not end with a
// write-back of 33 MB of dirty L2 lines (plain stores: +1.5-1.8 us per 4096^2 launch).  Non-temporal on top of it: with plain
// `sc1` the kernel took 13.0 us on data that is not already in the Infinity Cache against 9.7 us (16384^2: 150 against 127 us;
// profiles/r03_ablate_cold.txt, r03_microbench7_cold_floors.txt); replaying one cache-resident frame the two are level.
__device__ __forceinline__ void store16_wt_nt(void *p, const uint4 &v) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 d = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1 nt" : : "v"(p), "v"(d) : "memory");
}
// The same store with a scalar base and a 32-bit lane offset: the strip's address arithmetic stays on the scalar unit (the 64-bit
// vector add per strip and its register pair are gone).
__device__ __forceinline__ void store16_wt_nt(const void *sbase, uint32_t voff, const uint4 &v) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 d = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, %2 sc1 nt" : : "v"(voff), "v"(d), "s"(sbase) : "memory");
}

constexpr int kBatch = 8;                              // entries of the wave's batch
constexpr int kBatchWaveBytes = kBatch * (128 + 64) + 64; // images, pixel rows, ids

// A double through DPP: lane i reads the value of the lane the control word names.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// The four rational coefficients (0,0) (0,4) (4,0) (4,4) of all eight blocks of a strip in the reference's float64 operation order
// (same arithmetic as dct8_exact restricted to outputs 0 and 4 of both passes).  The column pass of the
// reference turns the integer column sums S_c (level-shifted) and alternating sums A_c = (x0+x7+x3+x4) - (x1+x2+x5+x6) into
// y0_c = fl(S_c * SQ2H/2), y4_c = fl(A_c * TW3/2) - one rounding each, everything before the constant is exact.  Those integers are
// pass 1's outputs 0 and 4 of the fast path and sit in the transpose buffer as exact floats: row u = 0 and row u = 4 of every block.
// The row pass adds the eight y in pocketfft's order: A = (y0+y7) + (y3+y4), B = (y1+y2) + (y5+y6), output 0 = fl((A+B) * SQ2H/2),
// output 4 = fl((A-B) * TW3/2) (the power-of-two scalings are exact and commute with the roundings).
// Lane 8*b + i works for block b: w = i >> 2 picks the frequency row u = 4w, k = i & 3 the pair (0,7) (3,4) (1,2) (5,6) whose two
// values the lane converts, scales and adds; one quad_perm exchange gives A (lanes k = 0,1) and B (k = 2,3), a second brings the
// other half over; lane k = 0 finishes v = 0, lane k = 1 finishes v = 4.  Returns the quantised coefficient (true IEEE division,
// half-even) in the lanes i = 0, 1, 4, 5 - (0,0) (0,4) (4,0) (4,4) at scan positions 0, 14, 10, 39.
__device__ __forceinline__ int rational_quad(const uint32_t *ldsT, int b, int i, const double *cst_rat) {
#pragma clang fp contract(off)
    const int w = i >> 2, k = i & 3;
    const uint32_t ca = (0x05010300u >> (8 * k)) & 0xffu, cb = (0x06020407u >> (8 * k)) & 0xffu;
    const uint32_t *row = ldsT + w * (4 * kTPlaneQ[4]) + 8 * b; // frequency row u = 4w of block b: plane 4w, eight contiguous dwords
    const float fa = __uint_as_float(row[ca]);                  // (planes 0 and 4 share banks: these two reads are 2-way conflicted)
    const float fb = __uint_as_float(row[cb]);
    const double K = w ? (kTW3 * 0.5) : (kSq2h * 0.5);
    const double ya = (double)fa * K, yb = (double)fb * K;
    const double p = ya + yb;                                   // y0+y7 | y3+y4 | y1+y2 | y5+y6
    const double s2 = p + dpp_f64<TIC_DPP_QP_XOR1>(p);          // A (k = 0, 1) | B (k = 2, 3)
    const double o = dpp_f64<TIC_DPP_QP_XOR2>(s2);              // the other half
    const double E = (k & 1) ? s2 - o : s2 + o;                 // k = 0: A + B, k = 1: A - B
    const double X = E * ((k & 1) ? (kTW3 * 0.5) : (kSq2h * 0.5));
    const double div = cst_rat[2 * w + (k & 1)], rdiv = cst_rat[4 + 2 * w + (k & 1)];
    return (int)rint(div_rn(X, div, rdiv)); // np.round(X / div): the correctly rounded quotient (tic_math.h div_rn: five multiply-adds), half-even
}

// Exact float64 sub-path of the four rational coefficients, 8 lanes per block, no LDS: rowLo/rowHi = pixel row i of the lane's
// block.  The row's bytes are first reordered (0,7,3,4,1,2,5,6) so that, after the byte transpose, neighbouring lanes hold the
// columns pocketfft adds first: the 8-point sums of SURVEY Appendix A become three DPP butterflies (xor 1, xor 2, +4).
// Column sums come from v_sad_u8.  Lanes 0..3 of the block return (0,0), (0,4), (4,0), (4,4) - one coefficient, one division at
// most, per lane.  Used by the rows-first instantiation, whose fast path has no column sums.
__device__ __forceinline__ int rational_slim(uint32_t rowLo, uint32_t rowHi, int i, const double *cst_rat) {
#pragma clang fp contract(off)
    uint32_t lo = perm_b32(rowHi, rowLo, 0x04030700u); // x0 x7 x3 x4
    uint32_t hi = perm_b32(rowHi, rowLo, 0x06050201u); // x1 x2 x5 x6
    transpose8x8_bytes(lo, hi, i);                     // lane i: column (0,7,3,4,1,2,5,6)[i], bytes = rows 0..7
    const uint32_t tot = __builtin_amdgcn_sad_u8(lo, 0u, __builtin_amdgcn_sad_u8(hi, 0u, 0u));
    const uint32_t sa = __builtin_amdgcn_sad_u8(lo & 0xff0000ffu, 0u, __builtin_amdgcn_sad_u8(hi & 0xff0000ffu, 0u, 0u)); // rows 0,3,4,7
    const int e0 = (int)tot - 1024, e4 = 2 * (int)sa - (int)tot;
    double y0 = (double)e0 * (kSq2h * 0.5);
    double y4 = (double)e4 * (kTW3 * 0.5);
    y0 = y0 + dpp_f64<TIC_DPP_QP_XOR1>(y0); // a0+a7 | a3+a4 | a1+a2 | a5+a6
    y4 = y4 + dpp_f64<TIC_DPP_QP_XOR1>(y4);
    y0 = y0 + dpp_f64<TIC_DPP_QP_XOR2>(y0); // A = p07 + p34 (lanes 0..3) | B = p12 + p56 (lanes 4..7)
    y4 = y4 + dpp_f64<TIC_DPP_QP_XOR2>(y4);
    const double b0 = dpp_f64<TIC_DPP_ROW_SHL4>(y0), b4 = dpp_f64<TIC_DPP_ROW_SHL4>(y4); // lanes 0..3 read B
    const double A = (i & 2) ? y4 : y0, B = (i & 2) ? b4 : b0;       // lanes 0,1: frequency row u = 0; lanes 2,3: u = 4
    const double E = (i & 1) ? A - B : A + B;                         // v = 0 | v = 4
    const double X = E * ((i & 1) ? (kTW3 * 0.5) : (kSq2h * 0.5));
    const double div = cst_rat[i & 3], rdiv = cst_rat[4 + (i & 3)];
    return (int)rint(div_rn(X, div, rdiv)); // (round 5: the reciprocal product, and the compiler's division when a lane sat near a tie - in a tie strip one always does)
}
// A block redone by the whole wave in float64 straight from the definition (lane 8*u + c: t[u][c] = sum_r M[u][r] x[r][c], then
// X[u][v = c] = sum_k M[v][k] t[u][k]; error ~1e-13, the reference's own is ~1e-12).  A rounding is decided when no .5 tie lies
// within 1e-9 of X * (1/div); decided values go to their place in the block's 128-byte zig-zag image.  The four rational
// coefficients are left alone: the image already holds their exact values (fast path outside the guard band, rational_quad inside).
// Returns the lanes that stayed undecided.  ~450 cycles for one block.
__device__ __forceinline__ unsigned long long wave_redo_block(const uint8_t *px /* 64 pixels, LDS */, double *tbuf /* 64 doubles, LDS */,
                                                              const double *cosm, const double *rdiv, const uint16_t *zzofs, int16_t *img16,
                                                              int lane) {
    const int u = lane >> 3, c = lane & 7;
    // (two accumulators per sum and 16-byte table reads: the pass runs on the launch's tail, one wave alone on its SIMD - what counts is
    //  the length of the dependent chain, not the instruction count; the 1e-9 test below does not care about the order of the additions)
    typedef double d2 __attribute__((ext_vector_type(2)));
    const d2 *mu = reinterpret_cast<const d2 *>(cosm + u * 8), *mc = reinterpret_cast<const d2 *>(cosm + c * 8);
    const d2 m0 = mu[0], m1 = mu[1], m2 = mu[2], m3 = mu[3];
    double x[8];
#pragma unroll
    for (int r = 0; r < 8; r++) x[r] = (double)((int)px[r * 8 + c] - 128);
    double ta = m0.x * x[0], tb = m0.y * x[1];
    ta = fma(m1.x, x[2], ta); tb = fma(m1.y, x[3], tb);
    ta = fma(m2.x, x[4], ta); tb = fma(m2.y, x[5], tb);
    ta = fma(m3.x, x[6], ta); tb = fma(m3.y, x[7], tb);
    tbuf[u * 8 + c] = ta + tb;
    const d2 n0 = mc[0], n1 = mc[1], n2 = mc[2], n3 = mc[3]; // (requested in front of the fence: they do not depend on it)
    wave_lds_fence();
    const d2 *tu = reinterpret_cast<const d2 *>(tbuf + u * 8);
    const d2 y0 = tu[0], y1 = tu[1], y2 = tu[2], y3 = tu[3];
    double xa = n0.x * y0.x, xb = n0.y * y0.y;
    xa = fma(n1.x, y1.x, xa); xb = fma(n1.y, y1.y, xb);
    xa = fma(n2.x, y2.x, xa); xb = fma(n2.y, y2.y, xb);
    xa = fma(n3.x, y3.x, xa); xb = fma(n3.y, y3.y, xb);
    const double X = xa + xb;
    const double tq = X * rdiv[lane], rq = rint(tq);
    const bool rational = (lane & 0x1b) == 0; // (u,v) in {0,4} x {0,4}
    const bool decided = fabs(tq - rq) < 0.5 - 1e-9;
    if (decided && !rational) img16[zzofs[lane] >> 1] = (int16_t)(int)rq;
    const unsigned long long und = __ballot(!decided && !rational);
    wave_lds_fence();
    return und;
}

// Second level, 8 lanes per block (up to eight blocks at once): the fast path's butterflies in float64 (error ~1e-13 against the
// reference's ~1e-12).  colLo/colHi: the lane's pixel column.  q[v] = rounding of (u = i, v) where no .5 tie lies within 1e-9 of the
// quotient; the return value has bit v set where it does (undecided: the caller goes to the exact operation order - or, for the four
// rational coefficients, keeps what the image already holds).  ~1,000 cycles, against ~450 per block for wave_redo_block: the batch
// pass takes this one from three entries on, and so do the strips the batch had no room for.
__device__ __forceinline__ uint32_t second_level_8(uint32_t colLo, uint32_t colHi, uint32_t *lds, int b, int i, const double *mul64, int q[8]) {
    double c[8];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        c[r] = (double)(int)((colLo >> (8 * r)) & 0xffu);
        c[r + 4] = (double)(int)((colHi >> (8 * r)) & 0xffu);
    }
    dct8_aan(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]); // down the column
    c[0] -= 1024.0;
    uint32_t w[8], wh[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = (uint32_t)__double2loint(c[k]);
    transpose8x8_dwords(lds, b, i, w);
#pragma unroll
    for (int k = 0; k < 8; k++) wh[k] = (uint32_t)__double2hiint(c[k]);
    transpose8x8_dwords(lds, b, i, wh);
#pragma unroll
    for (int k = 0; k < 8; k++) c[k] = __hiloint2double((int)wh[k], (int)w[k]);
    dct8_aan(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]); // along frequency row u = i
    uint32_t und = 0;
#pragma unroll
    for (int v = 0; v < 8; v++) {
        const double t = c[v] * mul64[i * 8 + v], r = rint(t);
        q[v] = (int)r;
        if (!(fabs(t - r) < 0.5 - 1e-9)) und |= 1u << v;
    }
    return und;
}

// The strip kernel's arguments as they lie in the kernel-argument segment (every argument at its natural alignment, in order).
struct StripKernargs {
    const uint8_t *img;
    const DctqConsts *consts;
    StripHead hd;
    StripWarm w;
    DctqArgs a;
};
static_assert(offsetof(StripKernargs, hd) == 16 && sizeof(StripHead) == 40 && offsetof(StripKernargs, w) == 64, "leading scalars, then one line");

// An LDS pointer as the 32-bit address the ds instructions take, and back.
template <class T>
__device__ __forceinline__ uint32_t lds_addr(T *p) {
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)(p);
}
template <class T>
__device__ __forceinline__ T *lds_ptr(uint32_t v) {
    return (T *)(__attribute__((address_space(3))) T *)(uintptr_t)v;
}

// kCols: the pass order of the fast path.  true  - columns first, byte transpose through LDS, ties from the exact column sums (rational_quad):
//                 grids that fit the chip at once, where every wave owns its strips in advance and the launch ends with the unluckiest one;
//        false - rows first, the pixels converted straight out of the landing registers (no byte transpose: 22 LDS cycles and a dependent
//                 LDS round trip less per strip), ties from the pixels (rational_slim, ~75 instructions per tie strip): grids of several
//                 rounds (16384^2, batches), where workgroups are dispatched as others finish and what counts is the average cost per
//                 strip - 16384^2 at q = 10 / 50 / 90: 107 / 119 / 127 us rows first against 123 / 130 / 137 us columns first
//                 (profiles/r05_config5.json, r04_config5.json).  Same results, bit for bit (tests run both orders on every rare-path frame).
//
// Arguments: the image, the constants and the schedule words of StripHead (tic_strip_plan.h) come first, as scalars - 14 dwords, which
// the file is compiled to preload (-mllvm -amdgpu-kernarg-preload-count=11, csrc/Makefile: they arrive in user SGPRs s[2:15] at wave
// launch where the firmware preloads, and through the compiler's compatibility prologue at the kernel's entry where it does not).  The
// constant-block load, both pixel loads and the walk's start state need nothing else, so no scalar-memory wait stands in front of
// them.  `w` is the one 64-byte line of what the start needs next (block indices, the output pointer); `a` is read by the rare paths only.
template <bool kCols>
__global__ __launch_bounds__(kWavesPerWG * 64, 6) __attribute__((amdgpu_num_vgpr(72))) void dctq_strip_kernel(
    const uint8_t *img, const DctqConsts *consts, unsigned long long hd_split, uint32_t hd_stride, uint32_t hd_misc, uint32_t hd_tstep,
    uint32_t hd_nfast, uint32_t hd_fast_tx, uint32_t hd_magic_fast_tx, uint32_t hd_in_step32, uint32_t hd_step_tx, StripWarm w, DctqArgs a) {
    const StripHead hd = {hd_split, hd_stride, hd_misc, hd_tstep, hd_nfast, hd_fast_tx, hd_magic_fast_tx, hd_in_step32, hd_step_tx};
    __shared__ __attribute__((aligned(16))) uint32_t ldsT_all[kWavesPerWG][kTWaveBytes / 4];
    __shared__ __attribute__((aligned(16))) uint32_t ldsZ_all[kWavesPerWG][kZzWaveBytes / 4];
    __shared__ __attribute__((aligned(16))) unsigned char cst_blk[kStripBlkBytes]; // constants, shared by the workgroup
    __shared__ __attribute__((aligned(16))) uint32_t bat_all[kWavesPerWG][kBatchWaveBytes / 4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t *ldsT = ldsT_all[wave];
    char *ldsZ = reinterpret_cast<char *>(ldsZ_all[wave]);
    const uint16_t *cst_zz = reinterpret_cast<const uint16_t *>(cst_blk + kBlkZz);  // [64] index u*8+v
    const double *cst_rat = reinterpret_cast<const double *>(cst_blk + kBlkRat);    // div of (0,0) (0,4) (4,0) (4,4)
    uint4 *bat_img = reinterpret_cast<uint4 *>(bat_all[wave]);                      // [kBatch][8] 16-byte pieces: zig-zag images
    uint2 *bat_pix = reinterpret_cast<uint2 *>(bat_all[wave] + kBatch * 32);        // [kBatch][8] pixel rows
    uint32_t *bat_id = bat_all[wave] + kBatch * 48;                                 // [kBatch] block index
    const DctqConsts *__restrict__ C = consts;
    const uint8_t *img_s = img;
    if (__builtin_expect(blockIdx.z != 0, 0)) { // batch of frames: one grid plane per frame (a branch: plane 0 does not wait for the stride)
        asm volatile("" : : : "memory");
        img_s += (long)blockIdx.z * w.frame_stride_in;
    }

    const int lr = lane >> 3, lb = lane & 7; // load phase: pixel row lr of block lb
    const int b = lane >> 3, i = lane & 7;   // compute phase: pixel column c = i of block b (pass 1), frequency row u = i (pass 2)
    unsigned long long mask_exact = 0;       // strips of this wave's walk to redo in the exact order (wave-uniform)
    uint32_t n_second = 0, n_quad = 0;       // blocks recomputed in float64, strips through rational_quad (statistics)
    int nE = 0;                              // entries in the batch (wave-uniform)
    int t_first, n_my;
    int16_t *out_f; // the plane's output
    uint32_t st_off = (uint32_t)lane * 16u; // lane offset inside a strip's 1 KiB output
    {
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        f32x4 m0, m1;
        f32x4 thr;
        u32x4 zzv;
        // Constants: the workgroup copies the quality's block (kStripBlkBytes = 2,624 bytes: tic_math.h) into LDS, 41 lanes of every wave
        // one 16-byte piece each (the first version let every lane load its own multipliers, thresholds and offsets - 8, then 12 wave-wide
        // loads per wave in front of the first pixel load: four such loads more cost 0.67 us on a 4096^2 launch).
        // Every VMEM instruction from here to the end of the loop is issued by hand and counted (see TIC_TAKE).
        u32x4 c_fill;
        {
            constexpr int kPpw = kStripBlkPieces / kWavesPerWG; // 41 pieces of 16 bytes per wave
            static_assert(kPpw * kWavesPerWG == kStripBlkPieces && kPpw <= 64, "constant block must split evenly over the waves");
            const uint32_t piece = lane < kPpw ? (uint32_t)(wave * kPpw + lane) : (uint32_t)kStripBlkPieces - 1u;
            const uint32_t fo = piece * 16u;
            asm volatile("global_load_dwordx4 v[76:79], %0, %1" : : "v"(fo), "s"(C->strip_blk) : "memory", "v76", "v77", "v78", "v79"); // (lands in reserved registers: see TIC_LOAD)
        }
        const uint32_t ld_off = (uint32_t)lr * hd.stride + (uint32_t)lb * 8u; // lane offset from the strip's first pixel

        // Strip walk: one scalar cursor (that of the prefetch).  Its start state is strip_cursor (tic_strip_plan.h, walked on the host by
        // tests/native/strip_plan_selftest.cpp) over preloaded words: no scalar-memory wait, no division in the rows and chunk schedules,
        // no per-workgroup memory.  Counts of the shipped binary: DESIGN.md 5.1.  (Measured in round 1: a prologue of ~250 scalar
        // instructions per wave - four integer divisions - made the last of a CU's five workgroups issue its first load 3,000 cycles
        // after the first, the 20 waves of a CU share one scalar unit; a table of per-wave start states read with s_load was as slow:
        // the scalar cache serves misses to distinct lines one by one.)
        const StripCursor cur = strip_cursor(hd, w, blockIdx.x, blockIdx.y, (uint32_t)wave);
        n_my = cur.n_my;
        t_first = (int)cur.t_first;
        uint32_t txp = cur.txp, in_off = cur.in_off, oblk;
        const uint32_t in_wrap32 = strip_in_wrap(hd);
        uint32_t src_off = 0; // a load past the end of the walk re-reads the wave's last strip (strip 0 if it has none)
        int n_issued = 0;
        // Pixel loads land in RESERVED registers v72..v79: the kernel is compiled with amdgpu_num_vgpr(72), so the compiler
        // allocates v0..v71 only, and the asm statements below name v72.. explicitly (declared as clobbers, which makes the
        // kernel descriptor cover them: 80 registers, six waves per SIMD).  The compiler never sees a loaded value: it goes from the
        // landing pair to LDS behind the counted wait, inside the same asm statement.  (Rounds 1-2 gave the asm load a "=v" output: the
        // compiler then believes the value exists from that statement on and is free to copy it - a phi move, a coalescing with a
        // register tuple - before it has landed, and to reuse a register that a load in flight will still write.  It happened not
        // to; tools/microbench7.hip faulted exactly that way.  Accumulator registers would do too, but the compiler then splits the
        // 80 registers 40:40 and spills.)  amdgpu_num_vgpr is a budget the allocator aims for, NOT a wall (a rare-path change once
        // made it put float64 division temporaries into v72..v77): the guarantee is csrc/lint_strip_kernel.py (run by the Makefile
        // behind the link and by tests/test_host_cpu.py), which checks in the disassembly of the shipped binary that no instruction
        // outside these statements touches v72..v79.  Keep it green.
#define TIC_RSV_CLOBBER "memory", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79"
#define TIC_LOAD(R, OB)                                                                                      \
    do {                                                                                                     \
        src_off = n_issued < n_my ? in_off : src_off;                                                        \
        OB = oblk;                                                                                           \
        asm volatile("global_load_dwordx2 v[" R "], %0, %1" : : "v"(ld_off), "s"(img_s + src_off) : TIC_RSV_CLOBBER); \
        n_issued++;                                                                                          \
        strip_step(txp, in_off, oblk, hd.step_tx, hd.fast_tx, hd.in_step32, in_wrap32, w);                   \
    } while (0)
    // the first two loads: the pixel offsets alone (the block indices need `w`, which must not be waited for in front of a load)
#define TIC_LOAD_HEAD(R, WRAP)                                                                               \
    do {                                                                                                     \
        src_off = n_issued < n_my ? in_off : src_off;                                                        \
        asm volatile("global_load_dwordx2 v[" R "], %0, %1" : : "v"(ld_off), "s"(img_s + src_off) : TIC_RSV_CLOBBER); \
        n_issued++;                                                                                          \
        WRAP = strip_step_in(txp, in_off, hd.step_tx, hd.fast_tx, hd.in_step32, in_wrap32);                  \
    } while (0)
    // waits until all but the N youngest vector-memory operations are done, then sends the strip's pixel rows from the landing pair
    // v[R] (which keeps the strip's bytes until the pair is loaded again, two strips later: the batch fetches the raw words from
    // there, raw_words) to the byte-transpose buffer
#define TIC_TAKE_COLS(R, N) asm volatile("s_waitcnt vmcnt(" #N ")\n\tds_write_b64 %0, v[" R "]" : : "v"(px_wr) : TIC_RSV_CLOBBER)
    // columns first, dword transpose: pass 1's eight outputs go to the eight lane-linear planes with ds_write_addtid_b32 (address =
    // m0 + offset + 4 * lane: no address register to move, 2 cycles a store against 6 for a ds_write2_b32 of two of them).  m0 belongs to
    // nobody between statements: it is set here, in front of its eight readers (one wait state between an SALU write of m0 and an
    // add-TID access), and csrc/lint_strip_kernel.py checks that nothing else in the kernel writes or reads it.  The stores stand
    // ahead of the compiler's reads in program order, which is all a wave's own LDS traffic needs (as TIC_TAKE_COLS).
#define TIC_PUT_PLANES(D0, D1, D2, D3, D4, D5, D6, D7)                                                                            \
    asm volatile("s_mov_b32 m0, %8\n\ts_nop 0\n\tds_write_addtid_b32 %0 offset:%9\n\tds_write_addtid_b32 %1 offset:%10\n\t"         \
                 "ds_write_addtid_b32 %2 offset:%11\n\tds_write_addtid_b32 %3 offset:%12\n\tds_write_addtid_b32 %4 offset:%13\n\t" \
                 "ds_write_addtid_b32 %5 offset:%14\n\tds_write_addtid_b32 %6 offset:%15\n\tds_write_addtid_b32 %7 offset:%16"     \
                 : : "v"(D0), "v"(D1), "v"(D2), "v"(D3), "v"(D4), "v"(D5), "v"(D6), "v"(D7), "s"(t_base),                          \
                     "n"(16 * kTPlaneQ[0]), "n"(16 * kTPlaneQ[1]), "n"(16 * kTPlaneQ[2]), "n"(16 * kTPlaneQ[3]),                   \
                     "n"(16 * kTPlaneQ[4]), "n"(16 * kTPlaneQ[5]), "n"(16 * kTPlaneQ[6]), "n"(16 * kTPlaneQ[7]) : TIC_RSV_CLOBBER)
    // columns first, zig-zag staging: the lane's four packed dwords to the four staging planes, same form
#define TIC_PUT_ZPLANES(W0, W1, W2, W3)                                                                                           \
    asm volatile("s_mov_b32 m0, %4\n\ts_nop 0\n\tds_write_addtid_b32 %0 offset:%5\n\tds_write_addtid_b32 %1 offset:%6\n\t"          \
                 "ds_write_addtid_b32 %2 offset:%7\n\tds_write_addtid_b32 %3 offset:%8"                                            \
                 : : "v"(W0), "v"(W1), "v"(W2), "v"(W3), "s"(z_base),                                                              \
                     "n"(4 * kZPlaneDw[0]), "n"(4 * kZPlaneDw[1]), "n"(4 * kZPlaneDw[2]), "n"(4 * kZPlaneDw[3]) : TIC_RSV_CLOBBER)
    // rows first: waits, then converts the strip's eight pixels straight out of the landing registers v[R0], v[R1]
#define TIC_TAKE_ROWS(D, R0, R1, N)                                                                          \
    asm volatile("s_waitcnt vmcnt(" #N ")\n\tv_cvt_f32_ubyte0 %0, v" #R0 "\n\tv_cvt_f32_ubyte1 %1, v" #R0 "\n\tv_cvt_f32_ubyte2 %2, v" #R0 \
                 "\n\tv_cvt_f32_ubyte3 %3, v" #R0 "\n\tv_cvt_f32_ubyte0 %4, v" #R1 "\n\tv_cvt_f32_ubyte1 %5, v" #R1                       \
                 "\n\tv_cvt_f32_ubyte2 %6, v" #R1 "\n\tv_cvt_f32_ubyte3 %7, v" #R1                                                       \
                 : "=v"(D[0]), "=v"(D[1]), "=v"(D[2]), "=v"(D[3]), "=v"(D[4]), "=v"(D[5]), "=v"(D[6]), "=v"(D[7]) : : TIC_RSV_CLOBBER)
        uint32_t ob0, ob1, ob2;
        uint32_t kstrip = 0; // ordinal of the strip in this wave's walk
        bool wrap0, wrap1;
        uint32_t ty0 = cur.ty, tx0 = cur.txp;
        TIC_LOAD_HEAD("72:73", wrap0);
        TIC_LOAD_HEAD("74:75", wrap1);
        // (the words of the round schedule are named here so that they stay live up to this point on every path: the compiler requests
        //  the whole line of `w` at the kernel's entry, and a path that let a requested register die would have to wait for the line
        //  before it could reuse the register - in front of the loads)
        asm volatile("; block indices: behind the loads" : "+s"(ty0), "+s"(tx0) : "s"(w.round_wgs), "s"(w.round_span), "s"(w.magic_round_wgs) : TIC_RSV_CLOBBER);
        oblk = strip_oblk(ty0, tx0, w);
        ob0 = oblk;
        strip_step_blk(oblk, wrap0, w);
        ob1 = oblk;
        strip_step_blk(oblk, wrap1, w);
        // While the three loads fly: every address of the loop that does not depend on the constants.  (The empty statement pins the
        // values in front of the wait - statements of this kind keep their order; left alone, the compiler computes them behind the barrier.)
        // LDS layouts of the loop (conflict-free: tools/lds_bank_model.py)
        //   byte transpose : block lb's pixel row lr at lb*80 + lr*8; lane (b, c) reads byte r*8 + c of block b, r = 0..7
        //   dword transpose, columns first: value (u, c) of block b at dword 4*kTPlaneQ[u] + 8*b + c (tic_strip_lds.h): the writer's
        //                    own lane index inside plane u, stored without an address register (TIC_PUT_PLANES); the reader's eight
        //                    dwords are 32 contiguous bytes
        //   dword transpose, rows first: value (v, r) of block b at dword (r>>2)*256 + v*32 + 4*(b ^ s(v)) + (r&3), s(v) = 4 for v in {2,3,6,7}
        //   zig-zag staging, columns first: value (u, v) of block b is a halfword of dword kZPlaneDw[p] + 8*b + u, p the plane of v's pair
        //                    (tic_strip_lds.h): four packed dwords per lane, stored like the transpose's (TIC_PUT_ZPLANES); the lane that
        //                    stores chunk k gathers its eight scan positions with eight ds_read_u16 (8 conflict cycles per strip remain)
        //   zig-zag staging, rows first: scan position p of block b at byte (p>>3)*128 + 16*(b ^ f(p>>3)) + 2*(p&7), f(c) = 4 * bit 1 of c:
        //                    eight ds_write_b16, one ds_read_b128
        // (pass 1 runs in the compute layout - lane 8*b + c - columns first, in the load layout - lane 8*r + b - rows first)
        constexpr int kHalf = 256; // rows first: dword offset of the half that holds rows 4..7
        uint32_t px_wr = lds_addr(ldsZ + lb * kPxBlkBytes + lr * 8);
        uint32_t o_px_rd = lds_addr(ldsZ + b * kPxBlkBytes + i);
        uint32_t o_twA = lds_addr(ldsT + (lr >> 2) * kHalf + (lr & 3) + 4 * lb);       // rows first, outputs {0,1,4,5}: + k*32 dwords
        uint32_t o_twB = lds_addr(ldsT + (lr >> 2) * kHalf + (lr & 3) + 4 * (lb ^ 4)); // rows first, outputs {2,3,6,7}
        const uint32_t t_base = lds_addr(ldsT);                                        // columns first: the planes' base (wave-uniform)
        // (the two 16-byte reads are pinned as indices of 16-byte pieces: the pointers keep the alignment ds_read_b128 needs)
        uint32_t q_tr = kCols ? (uint32_t)(kTPlaneStepQ * (i >> 1) + kTPlaneOddQ * (i & 1) + 2 * b)   // plane u = i, block b; the second piece follows
                              : (uint32_t)(i * 8 + (b ^ (4 * ((i >> 1) & 1))));                      // first half; the second kHalf dwords on
        uint32_t q_zr = (uint32_t)(i * 8 + (b ^ (4 * ((i >> 1) & 1)))); // rows first: the lane's chunk of the staging
        uint32_t o_zb = lds_addr(ldsZ); // the staging's base
        const uint32_t z_base = lds_addr(ldsZ); // columns first: the staging planes' base (wave-uniform)
        if constexpr (kCols)
            asm volatile("; addresses of the loop" : "+v"(px_wr), "+v"(o_px_rd), "+v"(q_tr), "+v"(o_zb), "+v"(st_off) : : TIC_RSV_CLOBBER);
        else
            asm volatile("; addresses of the loop" : "+v"(px_wr), "+v"(o_px_rd), "+v"(o_twA), "+v"(o_twB), "+v"(q_tr), "+v"(q_zr), "+v"(o_zb), "+v"(st_off) : : TIC_RSV_CLOBBER);
        const uint8_t *px_rd = lds_ptr<const uint8_t>(o_px_rd);
        uint32_t *twA = lds_ptr<uint32_t>(o_twA), *twB = lds_ptr<uint32_t>(o_twB);
        const uint4 *tr = reinterpret_cast<const uint4 *>(__builtin_assume_aligned(ldsT, 16)) + q_tr;
        const uint4 *zr = reinterpret_cast<const uint4 *>(__builtin_assume_aligned(ldsZ, 16)) + q_zr;
        char *zb = lds_ptr<char>(o_zb);
        // batch of frames: the plane's output
        out_f = reinterpret_cast<int16_t *>(reinterpret_cast<char *>(w.out) + (long)blockIdx.z * w.frame_stride_out);
        // the constant piece is older than the pixel loads: it has landed when only those are in flight.  (Issuing the second
        // pixel load behind the barrier instead: +0.13 us, profiles/r02_ab_opt_switches.txt.)
        asm volatile("s_waitcnt vmcnt(2)\n\tv_mov_b32 %0, v76\n\tv_mov_b32 %1, v77\n\tv_mov_b32 %2, v78\n\tv_mov_b32 %3, v79"
                     : "=v"(c_fill.x), "=v"(c_fill.y), "=v"(c_fill.z), "=v"(c_fill.w) : : "memory", "v76", "v77", "v78", "v79");
        if (lane < kStripBlkPieces / kWavesPerWG) *reinterpret_cast<u32x4 *>(cst_blk + (wave * (kStripBlkPieces / kWavesPerWG) + lane) * 16) = c_fill;
        // workgroup barrier by hand (the compiler's would also wait for the pixel loads it does not know about)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" : : : "memory");
        // pass 2's lane holds frequency row u = i (columns first) or frequency column v = i (rows first): its eight multipliers, its
        // three accept thresholds (groups {1,2,3} | {5,6,7} | {0,4} of the other index), its eight offsets in the zig-zag image
        m0 = *reinterpret_cast<const f32x4 *>(cst_blk + (kCols ? kBlkMul : kBlkMulT) + i * 32);
        m1 = *reinterpret_cast<const f32x4 *>(cst_blk + (kCols ? kBlkMul : kBlkMulT) + i * 32 + 16);
        thr = *reinterpret_cast<const f32x4 *>(cst_blk + (kCols ? kBlkThr : kBlkThrT) + i * 16);
        zzv = *reinterpret_cast<const u32x4 *>(cst_blk + (kCols ? kBlkZz : kBlkZzT) + i * 16);
        // rows first: the eight scatter addresses of the lane's coefficients in the zig-zag staging
        auto zz_ptr = [&](uint32_t ofs) { // ofs = 2 * scan position of the coefficient
            const uint32_t c = ofs >> 4; // (the chunk's swizzle: found by search, tools/lds_bank_model.py)
            return reinterpret_cast<int16_t *>(zb + c * 128 + (ofs & 15) + 16 * (b ^ (4 * ((c >> 1) & 1))));
        };
        int16_t *zp0 = zz_ptr(zzv.x & 0xffff), *zp1 = zz_ptr(zzv.x >> 16), *zp2 = zz_ptr(zzv.y & 0xffff), *zp3 = zz_ptr(zzv.y >> 16);
        int16_t *zp4 = zz_ptr(zzv.z & 0xffff), *zp5 = zz_ptr(zzv.z >> 16), *zp6 = zz_ptr(zzv.w & 0xffff), *zp7 = zz_ptr(zzv.w >> 16);
        wave_lds_fence();
        // columns first: the lane that stores chunk i of block b gathers scan positions 8i .. 8i+7 out of the staging planes.  Where they sit
        // is the inverse of zzv: lane (b, u = i) writes the staging offset of each of its (u, v) to an inverse table at the value's scan position
        // (in the transpose buffer, free until the loop starts; the eight blocks write the same 128 bytes) and reads its chunk's eight back.
        const uint16_t *zg0 = nullptr, *zg1 = nullptr, *zg2 = nullptr, *zg3 = nullptr, *zg4 = nullptr, *zg5 = nullptr, *zg6 = nullptr, *zg7 = nullptr;
        if constexpr (kCols) {
            char *inv = reinterpret_cast<char *>(ldsT);
            auto put = [&](uint32_t ofs, int v) { *reinterpret_cast<uint16_t *>(inv + ofs) = (uint16_t)(strip_zstage_byte(0, v) + 4 * i); };
            put(zzv.x & 0xffff, 0); put(zzv.x >> 16, 1); put(zzv.y & 0xffff, 2); put(zzv.y >> 16, 3);
            put(zzv.z & 0xffff, 4); put(zzv.z >> 16, 5); put(zzv.w & 0xffff, 6); put(zzv.w >> 16, 7);
            wave_lds_fence();
            const uint4 gv = reinterpret_cast<const uint4 *>(__builtin_assume_aligned(ldsT, 16))[i];
            wave_lds_fence();
            const char *gb = zb + 32 * b;
            auto at = [&](uint32_t ofs) { return reinterpret_cast<const uint16_t *>(gb + ofs); };
            zg0 = at(gv.x & 0xffff); zg1 = at(gv.x >> 16); zg2 = at(gv.y & 0xffff); zg3 = at(gv.y >> 16);
            zg4 = at(gv.z & 0xffff); zg5 = at(gv.z >> 16); zg6 = at(gv.w & 0xffff); zg7 = at(gv.w >> 16);
        }

        int left = n_my;
        // raw pixel words of the strip in work, out of its landing registers (batch entries only)
        auto raw_words = [&](auto tag, uint32_t &lo, uint32_t &hi) {
            constexpr int R = decltype(tag)::value;
            static_assert(R == 72 || R == 74 || R == 76, "landing register pair");
            if constexpr (R == 72) asm volatile("v_mov_b32 %0, v72\n\tv_mov_b32 %1, v73" : "=v"(lo), "=v"(hi) : : "memory");
            else if constexpr (R == 74) asm volatile("v_mov_b32 %0, v74\n\tv_mov_b32 %1, v75" : "=v"(lo), "=v"(hi) : : "memory");
            else asm volatile("v_mov_b32 %0, v76\n\tv_mov_b32 %1, v77" : "=v"(lo), "=v"(hi) : : "memory");
        };
        auto process = [&](auto tag, const float (&pxr)[8], const uint32_t ob) {
            float d0, d1, d2, d3, d4, d5, d6, d7;
            if constexpr (kCols) { // byte transpose: pixel column c = i of block b, rows 0..7 (written by TIC_TAKE_COLS)
                d0 = (float)px_rd[0]; d1 = (float)px_rd[8]; d2 = (float)px_rd[16]; d3 = (float)px_rd[24];
                d4 = (float)px_rd[32]; d5 = (float)px_rd[40]; d6 = (float)px_rd[48]; d7 = (float)px_rd[56];
            } else {               // pixel row lr of block lb, converted by TIC_TAKE_ROWS
                d0 = pxr[0]; d1 = pxr[1]; d2 = pxr[2]; d3 = pxr[3]; d4 = pxr[4]; d5 = pxr[5]; d6 = pxr[6]; d7 = pxr[7];
            }
            // ---- pass 1: down the pixel column | along the pixel row -----------------------------------------------------
            dct8_aan(d0, d1, d2, d3, d4, d5, d6, d7);
            d0 -= 1024.0f;
            if constexpr (kCols) {
                TIC_PUT_PLANES(d0, d1, d2, d3, d4, d5, d6, d7);
            } else {
                twA[0 * 32] = __float_as_uint(d0); twA[1 * 32] = __float_as_uint(d1); twB[2 * 32] = __float_as_uint(d2);
                twB[3 * 32] = __float_as_uint(d3); twA[4 * 32] = __float_as_uint(d4); twA[5 * 32] = __float_as_uint(d5);
                twB[6 * 32] = __float_as_uint(d6); twB[7 * 32] = __float_as_uint(d7);
            }
            wave_lds_fence();
            const uint4 ra = tr[0], rb = tr[kCols ? 1 : kHalf / 4];
            wave_lds_fence();
            float e0 = __uint_as_float(ra.x), e1 = __uint_as_float(ra.y), e2 = __uint_as_float(ra.z), e3 = __uint_as_float(ra.w);
            float e4 = __uint_as_float(rb.x), e5 = __uint_as_float(rb.y), e6 = __uint_as_float(rb.z), e7 = __uint_as_float(rb.w);
            // ---- pass 2: along the frequency row u = i -------------------------------------------------------------------
            dct8_aan(e0, e1, e2, e3, e4, e5, e6, e7);
            uint32_t q0, q1, q2, q3, q4, q5, q6, q7;
            float r0, r1, r2, r3, r4, r5, r6, r7;
            quant_fma(e0, m0.x, q0, r0); quant_fma(e1, m0.y, q1, r1); quant_fma(e2, m0.z, q2, r2); quant_fma(e3, m0.w, q3, r3);
            quant_fma(e4, m1.x, q4, r4); quant_fma(e5, m1.y, q5, r5); quant_fma(e6, m1.z, q6, r6); quant_fma(e7, m1.w, q7, r7);
            // guard test: three groups per row, v in {1,2,3} | {5,6,7} | {0,4} (tic_math.h thrR)
            const float mA1 = fmaxf(fmaxf(fabsf(r1), fabsf(r2)), fabsf(r3)); // v_max3_f32 with |.| modifiers
            const float mA2 = fmaxf(fmaxf(fabsf(r5), fabsf(r6)), fabsf(r7));
            const float mB = fmaxf(fabsf(r0), fabsf(r4));
            const unsigned long long cA = __ballot(mA1 > thr.x) | __ballot(mA2 > thr.y); // lanes whose guard band tripped: v in 1,2,3,5,6,7
            const unsigned long long cB = __ballot(mB > thr.z);                           // ... v in 0,4
            if constexpr (kCols) { // the low halves of the magic-number floats, two to a dword (v_perm_b32), four lane-linear stores
                const uint32_t qq[8] = {q0, q1, q2, q3, q4, q5, q6, q7};
                const uint32_t w0 = perm_b32(qq[kZPairHi[0]], qq[kZPairLo[0]], 0x05040100u), w1 = perm_b32(qq[kZPairHi[1]], qq[kZPairLo[1]], 0x05040100u);
                const uint32_t w2 = perm_b32(qq[kZPairHi[2]], qq[kZPairLo[2]], 0x05040100u), w3 = perm_b32(qq[kZPairHi[3]], qq[kZPairLo[3]], 0x05040100u);
                TIC_PUT_ZPLANES(w0, w1, w2, w3);
            } else {
                *zp0 = (int16_t)q0; *zp1 = (int16_t)q1; *zp2 = (int16_t)q2; *zp3 = (int16_t)q3;
                *zp4 = (int16_t)q4; *zp5 = (int16_t)q5; *zp6 = (int16_t)q6; *zp7 = (int16_t)q7;
            }
            const unsigned long long kRat = 0x1111111111111111ull; // lanes i in {0,4}: their coefficients 0 and 4 are the rational ones (either order)
            // ---- a rational coefficient sits on a tie somewhere in the strip (one strip in six at q = 50 on noise; every strip of
            //      posterised, two-level or flat content): the exact values of all 32, over the fast path's ------------------------
            if (__builtin_expect((cB & kRat) != 0ull, 0)) {
                n_quad++;
                if constexpr (kCols) {
                    const int rq = rational_quad(ldsT, b, i, cst_rat);
                    // lanes i = 0, 1, 4, 5 hold (u, v) = (4 (i >> 2), 4 (i & 1)): its halfword in the staging planes of block b, by arithmetic
                    // (as nested selects the compiler built three exec-mask regions out of the four offsets, inside the tie path)
                    constexpr int kV0 = strip_zstage_byte(0, 0), kV4 = strip_zstage_byte(0, 4);
                    if ((i & 2) == 0) *reinterpret_cast<int16_t *>(zb + kV0 + (kV4 - kV0) * (i & 1) + 16 * (i >> 2) + 32 * b) = (int16_t)rq;
                } else { // rows first: no column sums at hand - from the pixels (load layout -> a row per lane of the block, through LDS)
                    uint32_t lo0, hi0;
                    raw_words(tag, lo0, hi0);
                    uint2 *pb = reinterpret_cast<uint2 *>(ldsT);
                    pb[lb * 8 + lr] = make_uint2(lo0, hi0);
                    wave_lds_fence();
                    const uint2 rowv = pb[lane]; // row i of block b
                    wave_lds_fence();
                    const int rq = rational_slim(rowv.x, rowv.y, i, cst_rat); // lanes 0..3 of a block: (0,0), (0,4), (4,0), (4,4)
                    if (i < 4) *zz_ptr(i == 0 ? 0u : (i == 1 ? 28u : (i == 2 ? 20u : 78u))) = (int16_t)rq;
                }
            }
            wave_lds_fence();
            uint4 val;
            if constexpr (kCols) { // eight ds_read_u16 (zero-extending: not the d16 forms), two halves to a dword
                const uint32_t h0 = *zg0, h1 = *zg1, h2 = *zg2, h3 = *zg3, h4 = *zg4, h5 = *zg5, h6 = *zg6, h7 = *zg7;
                val = make_uint4(h0 | (h1 << 16), h2 | (h3 << 16), h4 | (h5 << 16), h6 | (h7 << 16));
            } else
                val = *zr;
            wave_lds_fence();
            const char *dst = reinterpret_cast<const char *>(out_f) + ((unsigned long long)ob << 7); // (scalar: the strip's 1 KiB)
            // ---- an irrational coefficient inside its guard band (one strip in seventy at q = 50, one in fourteen at q = 90) ------
            const unsigned long long mG = cA | (cB & ~kRat);
            if (__builtin_expect(mG != 0ull, 0)) {
                // per block: lane l answers for block l & 7 (byte l & 7 of the lane mask); the low byte of the ballot is the 8-bit
                // block mask (folding the bytes on the scalar unit took ~40 dependent scalar instructions per tripped strip)
                const uint32_t gm = (uint32_t)__ballot(((mG >> (8u * (uint32_t)i)) & 0xffull) != 0ull) & 0xffu;
                const int nnew = __builtin_popcount(gm);
                if (nE + nnew <= kBatch && gm != 0xffu) {
                    // the blocks join the batch: id, pixel rows (in the load layout this lane holds row lr of block lb), staged image
                    uint32_t lo0, hi0;
                    raw_words(tag, lo0, hi0);
                    const uint32_t below = (1u << b) - 1u, lbelow = (1u << lb) - 1u;
                    const bool mine = (gm >> b) & 1u;
                    const int e = nE + __builtin_popcount(gm & below);
                    if (mine) bat_img[e * 8 + i] = val;
                    if (mine && i == 0) bat_id[e] = ob + (uint32_t)b;
                    if ((gm >> lb) & 1u) bat_pix[(nE + __builtin_popcount(gm & lbelow)) * 8 + lr] = make_uint2(lo0, hi0);
                    // the tripped blocks leave with the batch pass; the others now (at least one lane stores: the strip's one
                    // vector-memory instruction is issued on every path, which the counted waits rely on)
                    if (!mine) store16_wt_nt(dst, st_off, val);
                    nE += nnew;
                    n_second += (uint32_t)nnew;
                } else {
                    // no room (or all eight blocks tripped): the whole strip is redone in the exact order after the loop
                    mask_exact |= 1ull << kstrip;
                    store16_wt_nt(dst, st_off, val);
                }
            } else
                store16_wt_nt(dst, st_off, val); // 16 B per lane, 1 KiB contiguous per wave
            left--;
            kstrip++;
        };
        // Two strips ahead: strip j is consumed after L(j+2) is issued; in steady state the instructions younger than
        // L(j) are S(j-2) L(j+1) S(j-1) L(j+2) -> vmcnt(4); the first two strips see 2 and 3.  (A rare branch issues at most
        // the same single store per strip.  Three strips ahead: no faster, profiles/r02_ab_prefetch_depth.txt, r03_ablate_cold.txt.)
        float pxf[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#define TIC_STEP(RLOAD, OBL, RTAKE, R0, R1, OBP, N)                                                          \
        TIC_LOAD(RLOAD, OBL);                                                                                \
        if constexpr (kCols) { TIC_TAKE_COLS(RTAKE, N); } else { TIC_TAKE_ROWS(pxf, R0, R1, N); }            \
        process(std::integral_constant<int, R0>(), pxf, OBP)
        do {
            if (left == 0) break;
            TIC_STEP("76:77", ob2, "72:73", 72, 73, ob0, 2);
            if (left == 0) break;
            TIC_STEP("72:73", ob0, "74:75", 74, 75, ob1, 3);
            while (left != 0) {
                TIC_STEP("74:75", ob1, "76:77", 76, 77, ob2, 4);
                if (left == 0) break;
                TIC_STEP("76:77", ob2, "72:73", 72, 73, ob0, 4);
                if (left == 0) break;
                TIC_STEP("72:73", ob0, "74:75", 74, 75, ob1, 4);
            }
        } while (0);
#undef TIC_STEP
        // Loads past the end of the walk (clamped addresses) may still be in flight: they land in v72..v79, which nothing behind
        // the loop names (the compiler never allocates them), so nothing waits for them - nor for the acknowledgement of the
        // strip stores, which is what rounds 1-3's `s_waitcnt vmcnt(1)` here really waited for (~580 cycles at the head of every
        // batch pass; profiles/r04_tail_experiments.txt).  The statement stays as a scheduling fence with the same clobbers.
        asm volatile("; end of the strip walk" : : : TIC_RSV_CLOBBER);
#undef TIC_LOAD
#undef TIC_LOAD_HEAD
#undef TIC_TAKE_COLS
#undef TIC_PUT_PLANES
#undef TIC_PUT_ZPLANES
#undef TIC_TAKE_ROWS
#undef TIC_RSV_CLOBBER
    }
    // The rare paths behind the loop read DctqArgs.  They ask for it HERE, through the kernel-argument pointer (passed through an empty
    // statement: the compiler cannot move the requests in front of it) - read as `a.field`, every field is requested at the kernel's
    // entry, and the start's one scalar wait then stands for four more lines of kernel arguments, served one after the other.
    typedef const __attribute__((address_space(4))) char *kernarg_ptr;
    kernarg_ptr kargs = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("; rare paths: DctqArgs from here on" : "+s"(kargs));
    const __attribute__((address_space(4))) DctqArgs *ca = reinterpret_cast<const __attribute__((address_space(4))) DctqArgs *>(kargs + offsetof(StripKernargs, a));
    (void)a;
    // ---- the batch pass: blocks with an irrational coefficient inside its guard band ----------------------------------------
    if (nE != 0) {
        const double *cst_cos = reinterpret_cast<const double *>(cst_blk + kBlkCos);   // orthonormal DCT-II matrix, index k*8+n
        const double *cst_rdiv = reinterpret_cast<const double *>(cst_blk + kBlkRdiv); // 1/div, index u*8+v
        // (1) float64 recompute: whole wave, one block at a time - or, when the wave met a cluster of trips (three entries and more),
        // all entries at once, 8 lanes each
        uint32_t m_exact = 0; // entries that need the exact operation order
        if (nE < 3) {
            for (int ee = 0; ee < nE; ee++) {
                const unsigned long long und = wave_redo_block(reinterpret_cast<const uint8_t *>(bat_pix + ee * 8), reinterpret_cast<double *>(ldsT), cst_cos,
                                                               cst_rdiv, cst_zz, reinterpret_cast<int16_t *>(bat_img + ee * 8), lane);
                if (und != 0ull) m_exact |= 1u << ee;
            }
        } else {
            const bool have2 = b < nE;
            const int e2 = have2 ? b : 0;
            const uint2 rowv = bat_pix[e2 * 8 + i];
            uint32_t lo = rowv.x, hi = rowv.y;
            transpose8x8_bytes(lo, hi, i);
            int qs[8];
            uint32_t und = second_level_8(lo, hi, ldsT, b, i, reinterpret_cast<const double *>(cst_blk + kBlkMul64), qs);
            if ((i & 3) == 0) und &= ~0x11u; // the rational coefficients (u, v in {0,4}): the image holds their exact values
            const uint4 zo = *reinterpret_cast<const uint4 *>(cst_zz + i * 8);
            const uint32_t zw[4] = {zo.x, zo.y, zo.z, zo.w};
            int16_t *img2 = reinterpret_cast<int16_t *>(bat_img + e2 * 8);
            if (have2) {
#pragma unroll
                for (int v = 0; v < 8; v++)
                    if (!((und >> v) & 1u) && !((i & 3) == 0 && (v & 3) == 0)) img2[((zw[v >> 1] >> (16 * (v & 1))) & 0xffffu) >> 1] = (int16_t)qs[v];
            }
            const unsigned long long um = __ballot(have2 && und != 0u);
            for (int ee = 0; ee < nE; ee++)
                if ((um >> (8 * ee)) & 0xffull) m_exact |= 1u << ee;
        }
        // (2) 8 lanes per entry: the exact order where even float64 from the definition could not decide (a true tie of an
        // irrational coefficient - practically never)
        const bool have = b < nE;
        const int e = have ? b : 0;
        const uint32_t blk = bat_id[e];
        if (m_exact != 0u) {
            const uint2 rowv = bat_pix[e * 8 + i]; // pixel row i of the block
            int16_t *img16 = reinterpret_cast<int16_t *>(bat_img + e * 8);
            uint32_t lo = rowv.x, hi = rowv.y;
            transpose8x8_bytes(lo, hi, i); // -> pixel column i
            const uint4 zo = *reinterpret_cast<const uint4 *>(cst_zz + i * 8); // byte offsets in the image of (u = i, v = 0..7)
            const uint32_t zw[4] = {zo.x, zo.y, zo.z, zo.w};
            int qx[8];
            exact_block(lo, hi, ldsT, b, i, C, qx);
            if (have && ((m_exact >> e) & 1u)) {
#pragma unroll
                for (int v = 0; v < 8; v++) img16[((zw[v >> 1] >> (16 * (v & 1))) & 0xffffu) >> 1] = (int16_t)qx[v];
            }
        }
        wave_lds_fence();
        const uint4 val = bat_img[e * 8 + i];
        if (have) store16_wt_nt(reinterpret_cast<char *>(out_f) + ((unsigned long long)blk << 7) + (uint32_t)i * 16u, val);
    }
    if (ca->fallback_count != nullptr && lane == 0) { // diagnostics (tic_set_stats): never in a timed launch
        if (n_second != 0) atomicAdd(ca->fallback_count, (unsigned long long)n_second);
        if (n_quad != 0) atomicAdd(ca->fallback_count + 1, (unsigned long long)n_quad);
        if (mask_exact != 0ull) atomicAdd(ca->fallback_count + 2, (unsigned long long)__builtin_popcountll(mask_exact));
        if (nE != 0) atomicMax(ca->fallback_count + 3, (unsigned long long)nE);
    }
    // ---- strips the batch had no room for: the exact operation order, whole strip ---------------------------------------
    if (mask_exact == 0ull) return;
    asm volatile("s_waitcnt vmcnt(0)" : : : "memory"); // the wave's fast-path stores to these strips must have landed
    const uint4 zzn = *reinterpret_cast<const uint4 *>(cst_zz + i * 8);
    const uint16_t zz[8] = {(uint16_t)zzn.x, (uint16_t)(zzn.x >> 16), (uint16_t)zzn.y, (uint16_t)(zzn.y >> 16),
                            (uint16_t)zzn.z, (uint16_t)(zzn.z >> 16), (uint16_t)zzn.w, (uint16_t)(zzn.w >> 16)};
    for (unsigned long long todo = mask_exact; todo != 0ull; todo &= todo - 1ull) {
        const int k = __builtin_ctzll(todo);
        const long t = (long)t_first + (long)k * ca->tstep; // strip index inside the fast rectangle
        const int ty = (int)(t / ca->fast_tx), tx = (int)(t - (long)ty * ca->fast_tx);
        Strip s;
        s.by = ty;
        s.bx = tx * 8 + b;
        s.valid = true;
        s.oblk = (size_t)ty * ca->bw + s.bx;
        uint32_t lo, hi;
        load_block_row(img_s, ca->h, ca->w, ca->stride, true, s, i, lo, hi);
        transpose8x8_bytes(lo, hi, i);
        int q[8];
        // the second level for the whole strip; the exact order only if it leaves something undecided (a tie of a rational
        // coefficient included: this path has no column sums at hand)
        const uint32_t und = second_level_8(lo, hi, ldsT, b, i, reinterpret_cast<const double *>(cst_blk + kBlkMul64), q);
        if (__ballot(und != 0u) != 0ull) exact_block(lo, hi, ldsT, b, i, C, q);
        store_zigzag(reinterpret_cast<uint32_t *>(ldsZ), b, i, zz, q, out_f, s);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Kernel 1b: exact path for integer images outside 0..255 (the reference transforms any integers: codec.py:29 is
// `astype(int32) - 128`).  int32 pixels in, int32 coefficients out (zig-zag order), float64 in pocketfft's order throughout.
// A drop-in edge, not a hot path: lane 8*b + i gathers pixel column i of block b itself (reflect padding as pad_image).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWavesPerWG * 64) void dctq_exact_wide_kernel(WideArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[kWavesPerWG][kLdsWaveBytes / 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane >> 3, i = lane & 7;
    uint32_t *lds = lds_all[wave];
    const int tile = blockIdx.x * kWavesPerWG + wave;
    Strip s = make_strip(tile, a.ntiles, a.tiles_x, a.bw, b);
    double c[8];
#pragma unroll
    for (int r = 0; r < 8; r++) c[r] = 0.0;
    if (s.valid) {
        const int x = reflect_index(s.bx * 8 + i, a.w);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int y = reflect_index(s.by * 8 + r, a.h);
            // codec.py:29 subtracts in int32, so INT32_MIN .. INT32_MIN + 127 wrap to the top of the range; the conversion is exact
            c[r] = (double)(int32_t)((uint32_t)a.img[(long)y * a.stride + x] - 128u);
        }
    }
    dct8_exact(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]); // axis -2: down the column
    uint32_t w[8], wh[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = (uint32_t)__double2loint(c[k]);
    transpose8x8_dwords(lds, b, i, w);
#pragma unroll
    for (int k = 0; k < 8; k++) wh[k] = (uint32_t)__double2hiint(c[k]);
    transpose8x8_dwords(lds, b, i, wh);
#pragma unroll
    for (int k = 0; k < 8; k++) c[k] = __hiloint2double((int)wh[k], (int)w[k]);
    dct8_exact(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]); // axis -1: along frequency row u = i
    if (!s.valid) return;
    const double *div = a.consts->div + i * 8;
    const uint16_t *zz = a.consts->zzofs + i * 8; // byte offset of (u = i, v) in an int16 zig-zag block = 2 * scan position
    int32_t *ob = a.out + s.oblk * 64;
#pragma unroll
    for (int v = 0; v < 8; v++) {
        ob[zz[v] >> 1] = (int32_t)rint(c[v] / div[v]); // np.round(X / div).astype(int32)
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Kernel 3: decode side - dequantise (utils.py:52), inverse DCT (utils.py:40-45, exact order), +128, clip,
// truncating cast (codec.py:68-70), crop.  Input: int16 [N][64] zig-zag, DC already integrated (np.cumsum).
// ---------------------------------------------------------------------------------------------------------
// constants.py:37-51: ANNSCALES = this integer table / 2048 - the scale the reference's C encoder leaves in its coefficients
// (8 * a_u * a_v of the AAN factorisation, 14-bit fixed point).  decode()'s scaled_dct branch divides by it.
__constant__ int kAnnScalesInt[64] = {
    16384, 22725, 21407, 19266, 16384, 12873, 8867,  4520,  22725, 31521, 29692, 26722, 22725, 17855, 12299, 6270,
    21407, 29692, 27969, 25172, 21407, 16819, 11585, 5906,  19266, 26722, 25172, 22654, 19266, 15137, 10426, 5315,
    16384, 22725, 21407, 19266, 16384, 12873, 8867,  4520,  12873, 17855, 16819, 15137, 12873, 10114, 6967,  3552,
    8867,  12299, 11585, 10426, 8867,  6967,  4799,  2446,  4520,  6270,  5906,  5315,  4520,  3552,  2446,  1247};

// The loads of the measuring instantiations go through pointers TYPED as global.  A pointer that is a kernel argument is known to be one; a
// pointer that a kernel loaded from a record in memory (idct_sse_kernel_v) is a generic one to the compiler, and every access through it a
// flat load, which counts on the LDS counter too: the eight scatter stores of a tile then wait for memory one by one.  The store kernels keep
// their plain pointers (and with them their assembly); the choice is one of type, by kMeasure, the expressions are the same.
#define TIC_GLOBAL __attribute__((address_space(1)))
typedef uint32_t tic_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t tic_u32x4 __attribute__((ext_vector_type(4)));

// The measuring epilogue, in two halves that idct_sse_kernel (one tile per wave) and idct_sse_kernel_v (a walk of tiles per wave) share.
// Sum widths: a tile's eight pixels per lane are at most 8 * 255^2 = 520,200, summed in 32 bits; the lane's running sums over a walk,
// and everything that leaves the lane - the wave reduction, the LDS words, the atomic's operand - are 64 bits, so no length of walk can
// wrap them and the plan enforces no bound on it.  (32-bit workgroup sums, the single-tile kernel's first form, wrap from a walk of 32
// tiles: 2,048 pixels * 255^2 is 2^27.)  Integer sums: the order of arrival does not change the result.
struct SseAcc {
    unsigned long long sq = 0, sw = 0; // sum of d * d, sum of (d * d) & 255
};

// Accumulate this tile: lane i of block b holds decoded row y = 8 by + i, pixels x0 .. x0 + 7 in px[]; it reads the same eight pixels of the
// original (one 8-byte load where that is aligned and whole, byte loads otherwise: the store path's split) and sums over the pixels INSIDE
// the frame - what lies beyond h or w (the decoder's cropped padding; in the original whatever the row pitch leaves there) is neither read
// nor counted.
__device__ __forceinline__ void sse_accumulate_tile(const Strip &s, int i, int h, int w, const SseArgs &m, const uint32_t px[8], SseAcc &acc) {
    uint32_t sq = 0, sw = 0;
    const int y = s.by * 8 + i, x0 = s.bx * 8;
    if (s.valid && y < h) {
        const TIC_GLOBAL uint8_t *p = (const TIC_GLOBAL uint8_t *)m.img + (long)y * m.stride + x0;
        uint32_t lo = 0, hi = 0;
        if (m.aligned8 && x0 + 8 <= w) {
            const tic_u32x2 v = *(const TIC_GLOBAL tic_u32x2 *)p;
            lo = v.x;
            hi = v.y;
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (x0 + k < w) {
                    const uint32_t bt = p[k];
                    if (k < 4) lo |= bt << (8 * k); else hi |= bt << (8 * (k - 4));
                }
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int d = (int)px[k] - (int)(((k < 4 ? lo : hi) >> (8 * (k & 3))) & 0xffu);
            const uint32_t e = x0 + k < w ? (uint32_t)(d * d) : 0u;
            sq += e;
            sw += e & 255u;
        }
    }
    acc.sq += sq;
    acc.sw += sw;
}

// Reduce and add: the workgroup's sums, ONE 64-bit vector atomic per non-zero sum on `res`.  Every lane of the workgroup must arrive.
__device__ __forceinline__ void sse_reduce_add(SseAcc acc, DistortionResult *res) {
    __shared__ unsigned long long wsum[kWavesPerWG][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc.sq += __shfl_xor(acc.sq, off, 64);
        acc.sw += __shfl_xor(acc.sw, off, 64);
    }
    if (lane == 0) {
        wsum[wave][0] = acc.sq;
        wsum[wave][1] = acc.sw;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tq = 0, tw = 0;
#pragma unroll
        for (int k = 0; k < kWavesPerWG; k++) {
            tq += wsum[k][0];
            tw += wsum[k][1];
        }
        if (tq) atomicAdd(&res->sse, tq); // (tw != 0 implies tq != 0)
        if (tw) atomicAdd(&res->sse_wrapped, tw);
    }
}

// kWideDc: the DC comes from a.dc32 (IdctArgs: a stream whose running DC left int16), everything else as ever
// kMeasure: the measuring epilogue (idct_sse_kernel, idct_sse_kernel_v): the decoded pixels are compared with the frame `m` describes
// instead of being stored, the tile's sums added to `acc`; the caller ends in sse_reduce_add
template <bool kWideDc, bool kMeasure = false>
__device__ __forceinline__ void idct_body(const IdctArgs &a, int wg_tile0, const SseArgs *m = nullptr, SseAcc *acc = nullptr) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[kWavesPerWG][kLdsWaveBytes / 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane >> 3, i = lane & 7;
    uint32_t *lds = lds_all[wave];
    const int tile = wg_tile0 + wave; // (wg_tile0: the workgroup's first tile)
    using ConstsPtr = std::conditional_t<kMeasure, const TIC_GLOBAL DctqConsts *, const DctqConsts *>;
    const ConstsPtr __restrict__ C = (ConstsPtr)a.consts;
    Strip s = make_strip(tile, a.ntiles, a.tiles_x, a.bw, b);
    if (a.first_block >= 0) { // block-range form: 8 consecutive blocks of the raster order per wave
        const long blk = a.first_block + (long)tile * 8 + b;
        s.valid = blk < a.first_block + a.nblocks_sel;
        s.by = (int)(blk / a.bw);
        s.bx = (int)(blk - (long)s.by * a.bw);
        s.oblk = (size_t)blk;
    }

    // lane i of block b loads zig-zag entries 8i..8i+7 (16 B), scatters them to natural order in LDS
    uint4 val = make_uint4(0, 0, 0, 0);
    if constexpr (kMeasure) {
        if (s.valid) {
            const tic_u32x4 v = *(const TIC_GLOBAL tic_u32x4 *)((const TIC_GLOBAL int16_t *)a.coeffs + s.oblk * 64 + i * 8);
            val = make_uint4(v.x, v.y, v.z, v.w);
        }
    } else {
        if (s.valid) val = *reinterpret_cast<const uint4 *>(a.coeffs + s.oblk * 64 + i * 8);
    }
    char *blk = reinterpret_cast<char *>(lds) + b * kZzStrideB;
    {
        uint32_t wv[4] = {val.x, val.y, val.z, val.w};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            int nat = C->zznat[i * 8 + k]; // natural index of scan position 8i+k
            int16_t cv = (int16_t)((wv[k >> 1] >> (16 * (k & 1))) & 0xffffu);
            *reinterpret_cast<int16_t *>(blk + nat * 2) = cv;
        }
    }
    wave_lds_fence();
    // lane i takes column v = i of the natural 8x8 coefficient matrix: X[u][i], u = 0..7
    double c[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
        int16_t cv = *reinterpret_cast<const int16_t *>(blk + (u * 8 + i) * 2);
        if (a.scaled) // codec.py:60-62: (coeffs / ANNSCALES) * 2**quality, then the inverse quantiser of quality 50: three roundings
            c[u] = (((double)cv / ((double)kAnnScalesInt[u * 8 + i] / 2048.0)) * a.pow2) * C->div[u * 8 + i];
        else
            c[u] = (double)cv * C->div[u * 8 + i]; // coeffs * (Q*factor/100)
    }
    if (kWideDc && i == 0 && s.valid) { // the same expressions on the int32 value (exact in float64, like the int16 one)
        const double dcv = (double)a.dc32[s.oblk];
        c[0] = a.scaled ? ((dcv / ((double)kAnnScalesInt[0] / 2048.0)) * a.pow2) * C->div[0] : dcv * C->div[0];
    }
    wave_lds_fence();
    idct8_exact(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]); // axis -2
    uint32_t w[8], wh[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = (uint32_t)__double2loint(c[k]);
    transpose8x8_dwords(lds, b, i, w);
#pragma unroll
    for (int k = 0; k < 8; k++) wh[k] = (uint32_t)__double2hiint(c[k]);
    transpose8x8_dwords(lds, b, i, wh);
#pragma unroll
    for (int k = 0; k < 8; k++) c[k] = __hiloint2double((int)wh[k], (int)w[k]);
    idct8_exact(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]); // axis -1: lane i holds pixel row i
    uint32_t px[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        double v = c[k] + 128.0;
        v = v < 0.0 ? 0.0 : v;
        v = v > 255.0 ? 255.0 : v;
        px[k] = (uint32_t)(int)v; // truncation toward zero, as astype(np.uint8) on a clipped value
    }
    if constexpr (kMeasure) { // round-trip error instead of pixels (nothing above returns: every lane reaches the caller's reduction)
        sse_accumulate_tile(s, i, a.h, a.w, *m, px, *acc);
        return;
    }
    if (!s.valid) return;
    int y = s.by * 8 + i;
    if (y >= a.h) return;
    int x0 = s.bx * 8;
    uint8_t *p = a.out + (long)y * a.stride + x0;
    if (a.aligned8 && x0 + 8 <= a.w) {
        uint2 o;
        o.x = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
        o.y = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
        *reinterpret_cast<uint2 *>(p) = o;
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (x0 + k < a.w) p[k] = (uint8_t)px[k];
    }
}
__global__ __launch_bounds__(kWavesPerWG * 64) void idct_kernel(IdctArgs a) { idct_body<false>(a, blockIdx.x * kWavesPerWG); }
__global__ __launch_bounds__(kWavesPerWG * 64) void idct_wide_dc_kernel(IdctArgs a) { idct_body<true>(a, blockIdx.x * kWavesPerWG); }
// The measuring instantiation: decode and compare, no pixel written (tic_distortion_dev, tic_rd_points_dev, tic_compress_to_psnr_dev).
__global__ __launch_bounds__(kWavesPerWG * 64) void idct_sse_kernel(IdctArgs a, SseArgs m) {
    SseAcc acc;
    idct_body<false, true>(a, blockIdx.x * kWavesPerWG, &m, &acc);
    sse_reduce_add(acc, m.res);
}
// The descriptor form: the frames of a chunk in one launch (tic_decompress_batch_adaptive).  Workgroup g transforms the kWavesPerWG tiles from
// wgs[g].y on of frame wgs[g].x, whose arguments are args[wgs[g].x]; a frame has ceil(ntiles / kWavesPerWG) workgroups.
__global__ __launch_bounds__(kWavesPerWG * 64) void idct_batch_kernel(const IdctArgs *__restrict__ args, const uint2 *__restrict__ wgs) {
    const uint2 e = wgs[blockIdx.x];
    const IdctArgs a = args[e.x];
    idct_body<false>(a, (int)e.y);
}
// The measuring kernel's descriptor form: up to kSseMaxProbes PROBES - a frame's coefficients at one quality against that frame's pixels,
// any block counts - in ONE launch (tic_rd_points_v, tic_compress_batch_to_psnr, tic_distortion_v_dev).  A workgroup finds its probe as
// stream_size_kernel_v does: lane l loads first_group[l] (0xffffffff behind the last probe), the wave counts the entries <= blockIdx.x; the
// count is a scalar, so the record comes by scalar loads and is uniform across the workgroup.  Group g of a probe walks the probe's
// workgroup-tiles g, g + ngroups, ... - the stride is the probe's own group count (capped on the host: tic_rd_plan.h), never the grid's -
// sums in registers across the walk (SseAcc: 64-bit lane sums, no bound on the walk) and ends in one atomic per non-zero sum on the probe's
// own result: a 4096^2 probe issues at most 1,024 atomics per sum, where idct_sse_kernel issues 8,192.
// LDS across the walk: a wave's region of lds_all is reused by every tile.  All of it is wave-private and one wave's DS instructions execute
// in order, so what is needed between the last transposing read of one tile and the first scatter of the next is a compiler-level fence:
// transpose8x8_dwords ends in one behind its reads, and the loop closes with another.  No workgroup barrier inside the walk: the trip count
// is uniform across the workgroup (it depends on blockIdx.x and the record alone), so every wave reaches the barrier of sse_reduce_add.
// kScaledProbes: a table that may hold probes of the integer encoder (tic_rd_points_scaled_v) - the record's exponent word decides per probe,
// and idct_body branches on a.scaled at run time.  A table of float probes alone takes the instantiation without the branch (measured: the
// branch costs a 4096^2 float probe 1.6 of 40.4 us).
static_assert(kWavesPerWG == kSseWavesPerWG, "tic_rd_plan.h counts a probe's workgroups by this workgroup");
template <bool kScaledProbes>
__global__ __launch_bounds__(kWavesPerWG * 64) void idct_sse_kernel_v(const SseProbeTable *__restrict__ pt, DistortionResult *__restrict__ res) {
    const int lane = threadIdx.x & 63;
    const uint32_t first = pt->first_group[lane];
    const int probe = __builtin_amdgcn_readfirstlane(__popcll(__ballot(first <= blockIdx.x)) - 1);
    const SseProbeRec &r = pt->rec[probe];
    IdctArgs a;
    a.coeffs = r.coeffs;
    a.out = nullptr;
    a.h = r.h, a.w = r.w;
    a.stride = 0;
    a.bw = r.bw, a.tiles_x = r.tiles_x, a.ntiles = r.ntiles;
    a.aligned8 = 0;
    a.consts = static_cast<const DctqConsts *>(r.consts);
    if constexpr (kScaledProbes) {
        a.scaled = r.scaled_exp1 != 0u;
        a.pow2 = __hiloint2double((int)((1022u + r.scaled_exp1) << 20), 0); // 2 ** (scaled_exp1 - 1); 0.5 for a float probe, which never reads it
    }
    SseArgs m;
    m.img = r.img;
    m.stride = (long)r.stride;
    m.aligned8 = r.aligned8;
    m.res = res + r.result;
    const uint32_t wg_tiles = ((uint32_t)r.ntiles + kWavesPerWG - 1) / kWavesPerWG, ngroups = r.ngroups;
    SseAcc acc;
    for (uint32_t t = blockIdx.x - r.first_group; t < wg_tiles; t += ngroups) {
        idct_body<false, true>(a, (int)(t * kWavesPerWG), &m, &acc);
        wave_lds_fence();
    }
    sse_reduce_add(acc, m.res);
}

// ---------------------------------------------------------------------------------------------------------
// Self-test kernel: checks the DPP byte transpose against the shuffle formulation on arbitrary data.
// ---------------------------------------------------------------------------------------------------------
__global__ void selftest_transpose_kernel(const uint2 *in, uint2 *out_dpp, uint2 *out_ref) {
    int lane = threadIdx.x & 63, i = lane & 7;
    uint2 v = in[blockIdx.x * blockDim.x + threadIdx.x];
    uint32_t lo = v.x, hi = v.y;
    transpose8x8_bytes(lo, hi, i);
    out_dpp[blockIdx.x * blockDim.x + threadIdx.x] = make_uint2(lo, hi);
    lo = v.x;
    hi = v.y;
    transpose8x8_bytes_shfl(lo, hi, i);
    out_ref[blockIdx.x * blockDim.x + threadIdx.x] = make_uint2(lo, hi);
}

// ---- launchers ---------------------------------------------------------------------------------------------
static inline int grid_for(int ntiles) { return (ntiles + kWavesPerWG - 1) / kWavesPerWG; }

// Schedule knobs of the strip kernel's launcher.  The product uses the defaults below; the environment is consulted only behind
// the test-hook gate (tic_hooks.h, TIC_TEST_HOOKS=1: tests/test_gpu_parity.py::test_strip_schedules_are_equivalent drives every
// schedule against the exact kernel) - read once, or at every launch while TIC_TUNE is set too (it may be set at any time).
struct Tunables {
    int max_wgs, sched, chunk, order;
    int split[8];
};
static Tunables read_tunables() {
    auto geti = [](const char *k, int d) { const char *v = test_hook(k); return v ? atoi(v) : d; };
    Tunables t;
    t.max_wgs = geti("TIC_MAX_WGS", 0);             // persistent grid size (0: resident workgroups of the chip)
    t.sched = geti("TIC_SCHED", 1);                 // grids larger than the chip: 0 strided, 1 chunked (default), 2 round-interleaved
    t.chunk = geti("TIC_CHUNK", kChunkStrips);      // strips per wave of schedules 1 and 2
    t.order = geti("TIC_ORDER", -1);                // pass order of the strip kernel: -1 by grid (default), 0 rows first, 1 columns first
    // per-round row weights of the team schedule ("0" disables it): the six workgroups of a CU reach their first pixel
    // 1,400 ... 6,200 cycles after their own entry (profiles/r03_stamps_tail.txt), later rounds get fewer strip rows.  Round 5: the
    // first round gives a row to the last (4096^2: 9,8,6,4,3,2 rows instead of round 3's 10,8,6,4,3,1 - a wave's rare work grows with
    // its strips, and the launch ends with the unluckiest wave: 9.9-10.0 against 10.2-10.3 us, profiles/r05_split_weights.txt)
    const char *sp = test_hook("TIC_SPLIT") ? test_hook("TIC_SPLIT") : "15,13,10,7,5,3";
    for (int k = 0; k < 8; k++) t.split[k] = 0;
    for (int k = 0; k < 8 && sp && *sp; k++) {
        t.split[k] = atoi(sp);
        sp = strchr(sp, ',');
        if (sp) sp++;
    }
    return t;
}
static Tunables tunables() {
    // TIC_TUNE is looked up at every launch (rounds 1-6 latched it with the first launch of the process: a test that set it later - every
    // one of the suite's, behind an earlier test's launch - forced nothing).  The shipped build reads no environment: test_hook is a
    // constant nullptr there and this is `once`.
    static const Tunables once = read_tunables();
    return test_hook("TIC_TUNE") != nullptr ? read_tunables() : once;
}

int dctq_kernel_id(int abi_variant) { // (TIC_KERNEL_AUTO 0, TIC_KERNEL_EXACT 1, TIC_KERNEL_HYBRID 2: include/tinyimgcodec_hip.h)
    return abi_variant == 1 ? 1 : ((abi_variant == 0 || abi_variant == 2) ? 2 : -1);
}

// variant 1: the exact kernel for every block; variant 2: the strip kernel on the rectangle of complete 64x8 strips with 8-byte
// aligned rows, the exact kernel on what is left (right / bottom padding).
hipError_t launch_dctq(DctqArgs a, int variant, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop, StripLaunchInfo *info) {
    if (info) *info = StripLaunchInfo{};
    if (a.ntiles <= 0) return hipSuccess;
    if (variant != 1 && variant != 2) return hipErrorInvalidValue;
    dim3 block(kWavesPerWG * 64);
    a.nwaves = a.step_ty = a.step_tx = 0;
    a.fast_ty = a.fast_tx = 0;
    a.rem_mode = 0;
    a.dbg = nullptr;
    const int nf = a.nframes > 0 ? a.nframes : 1;
    if (variant == 1) {
        hipLaunchKernelGGL(dctq_exact_kernel, dim3(grid_for(a.ntiles), nf), block, 0, stream, a);
        return hipGetLastError();
    }
    // The strip walk keeps 32-bit pixel offsets: a frame of 4 GiB or more is transformed in bands of whole block rows, one launch
    // per band (the stage has no dependency between block rows: the DC is not differenced here).  Round 2 sent such frames to
    // the exact kernel as a whole.  (TIC_BAND_BYTES, a test hook, lowers the limit so that the banding can be tested on small frames.)
    {
        long limit = 1L << 32;
        if (const char *e = test_hook("TIC_BAND_BYTES")) limit = atol(e) > 0 ? atol(e) : limit;
        if (a.aligned8 && nf == 1 && a.w >= 64 && (long)a.h * a.stride >= limit) {
            const long band = (limit - 1) / a.stride / 8 * 8; // pixel rows per band
            if (band >= 8) {
                for (long y0 = 0; y0 < a.h; y0 += band) {
                    DctqArgs b = a;
                    b.h = (int)((long)a.h - y0 < band ? (long)a.h - y0 : band);
                    b.img = a.img + y0 * a.stride;
                    b.out = a.out + (y0 / 8) * (long)a.bw * 64;
                    b.ntiles = ((b.h + 7) / 8) * b.tiles_x;
                    const hipError_t e = launch_dctq(b, variant, stream, nullptr, nullptr, info); // (the report: the last band's)
                    if (e != hipSuccess) return e;
                }
                return hipSuccess;
            }
        }
    }
    const int bh = a.ntiles / a.tiles_x;
    // persistent grid = exactly the workgroups the chip holds at once (CUs x resident workgroups per CU): a larger
    // grid runs in two uneven rounds, a smaller one leaves wave slots empty (measured: 15.0 us at 1280 workgroups
    // vs 16.3 us at 2048 on a 4096^2 frame)
    static int cus = 256;
    static const int resident = [] {
        int dev = 0, per_cu = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, dctq_strip_kernel<true>, kWavesPerWG * 64, 0) != hipSuccess || per_cu < 1)
            per_cu = 4;
        // 80 VGPRs and 23 KiB of LDS allow 6 workgroups per CU (7 measured no better when the kernel still fitted them:
        // a seventh lengthens the start ramp by as much as it hides, profiles/r02_ab_occupancy.txt)
        if (per_cu > 6) per_cu = 6;
        return cus * per_cu;
    }();
    const Tunables tune = tunables();
    // the schedule: tic_strip_plan.h (strided, chunked, round-interleaved or team; the words of the kernel's start state)
    StripTune st;
    st.cus = cus, st.resident = resident, st.max_wgs = tune.max_wgs, st.sched = tune.sched, st.chunk = tune.chunk;
    for (int k = 0; k < 8; k++) st.split[k] = tune.split[k];
    const StripFrame fr = {a.h, a.w, a.stride, a.bw, a.aligned8, nf};
    const StripPlan pl = strip_plan(fr, st);
    a.fast_tx = pl.fast_tx;
    a.fast_ty = pl.fast_ty;
    if (pl.launch) {
        // the same schedule in DctqArgs, for the kernel's rare paths (the exact redo of a strip finds it by t_first + k * tstep)
        a.nwaves = pl.nwaves, a.wg_stride = pl.wg_stride, a.tstep = pl.tstep, a.wg_span = pl.wg_span, a.round_wgs = pl.round_wgs;
        a.team_count = pl.team_count, a.step_ty = pl.step_ty, a.step_tx = pl.step_tx;
        for (int k = 0; k < 9; k++) a.split[k] = pl.split[k];
        a.in_step32 = pl.hd.in_step32, a.in_wrap32 = pl.in_wrap32, a.oblk_step = pl.wm.oblk_step, a.oblk_wrap = pl.wm.oblk_wrap;
        a.magic_fast_tx = pl.hd.magic_fast_tx, a.magic_tstep = pl.wm.magic_round_wgs;
        a.split_lo = pl.hd.split, a.split_hi = (pl.hd.misc >> 8) & 0xffu;
        const StripHead &hd = pl.hd;
        StripWarm wm = pl.wm;
        wm.out = a.out, wm.frame_stride_in = a.frame_stride_in, wm.frame_stride_out = a.frame_stride_out;
        const dim3 grid(pl.grid_x, pl.grid_y, nf);
        // pass order: columns first where the whole grid is resident at once (static shares: the tail decides), rows first for grids
        // of several rounds (dynamic dispatch: the average cost per strip decides); TIC_ORDER (test hook) forces one
        const bool cols = tune.order < 0 ? !pl.multi_round : tune.order == 1;
        auto *kern = cols ? dctq_strip_kernel<true> : dctq_strip_kernel<false>;
        if (info) {
            info->order = cols ? 2 : 1, info->kind = (int)(hd.misc & 0xffu), info->team_count = pl.team_count;
            info->grid_x = (int)pl.grid_x, info->grid_y = (int)pl.grid_y, info->tstep = pl.tstep, info->fast_tx = pl.fast_tx, info->fast_ty = pl.fast_ty;
        }
        if (ev_start && ev_stop) // the dispatch packet's own time stamps (tic_dctq_dev_timed_warm's per-launch times)
            hipExtLaunchKernelGGL(kern, grid, block, 0, stream, ev_start, ev_stop, 0, a.img, a.consts, hd.split, hd.stride, hd.misc, hd.tstep, hd.nfast,
                                  hd.fast_tx, hd.magic_fast_tx, hd.in_step32, hd.step_tx, wm, a);
        else
            hipLaunchKernelGGL(kern, grid, block, 0, stream, a.img, a.consts, hd.split, hd.stride, hd.misc, hd.tstep, hd.nfast, hd.fast_tx,
                               hd.magic_fast_tx, hd.in_step32, hd.step_tx, wm, a);
    }
    const int nrem = bh * (a.tiles_x - a.fast_tx) + (bh - a.fast_ty) * a.fast_tx;
    if (nrem > 0) {
        a.rem_mode = 1;
        hipLaunchKernelGGL(dctq_exact_kernel, dim3(grid_for(nrem), nf), block, 0, stream, a);
    }
    return hipGetLastError();
}

hipError_t launch_dctq_wide(const WideArgs &a, hipStream_t stream) {
    if (a.ntiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(dctq_exact_wide_kernel, dim3(grid_for(a.ntiles)), dim3(kWavesPerWG * 64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_idct(const IdctArgs &a, hipStream_t stream) {
    if (a.ntiles <= 0) return hipSuccess;
    dim3 grid(grid_for(a.ntiles)), block(kWavesPerWG * 64);
    if (a.dc32) hipLaunchKernelGGL(idct_wide_dc_kernel, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(idct_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

int idct_batch_wgs(int ntiles) { return grid_for(ntiles); }
int idct_batch_tiles_per_wg() { return kWavesPerWG; }
hipError_t launch_idct_batch(const IdctArgs *d_args, const uint2 *d_wgs, size_t nwgs, hipStream_t stream) {
    if (!d_args || !d_wgs || nwgs == 0 || nwgs > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(idct_batch_kernel, dim3((uint32_t)nwgs), dim3(kWavesPerWG * 64), 0, stream, d_args, d_wgs);
    return hipGetLastError();
}

hipError_t launch_idct_sse(const IdctArgs &a, const SseArgs &m, hipStream_t stream) {
    if (a.ntiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(idct_sse_kernel, dim3(grid_for(a.ntiles)), dim3(kWavesPerWG * 64), 0, stream, a, m);
    return hipGetLastError();
}

hipError_t launch_idct_sse_v(const SseProbeTable *d_probes, size_t ngroups, DistortionResult *d_res, hipStream_t stream, bool scaled_probes) {
    if (ngroups == 0) return hipSuccess;
    if (!d_probes || !d_res || ngroups > (size_t)kSseMaxProbes * kSseMaxGroups) return hipErrorInvalidValue;
    if (scaled_probes)
        hipLaunchKernelGGL(idct_sse_kernel_v<true>, dim3((unsigned)ngroups), dim3(kWavesPerWG * 64), 0, stream, d_probes, d_res);
    else
        hipLaunchKernelGGL(idct_sse_kernel_v<false>, dim3((unsigned)ngroups), dim3(kWavesPerWG * 64), 0, stream, d_probes, d_res);
    return hipGetLastError();
}

hipError_t launch_selftest_transpose(const void *in, void *out_dpp, void *out_ref, int nthreads, hipStream_t stream) {
    hipLaunchKernelGGL(selftest_transpose_kernel, dim3(nthreads / 256), dim3(256), 0, stream, (const uint2 *)in,
                       (uint2 *)out_dpp, (uint2 *)out_ref);
    return hipGetLastError();
}

} // namespace tic
