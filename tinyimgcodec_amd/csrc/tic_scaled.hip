// tic_scaled.hip - gfx950 kernel of the integer forward transform: the transform stage of the reference's standalone C encoder
// (c/img.c:207-217: level shift, IMG_fdct, IMG_quantize), uint8 pixels -> zz16 (int16 [N][64], zig-zag order, absolute DC), so that the
// entropy stage behind it is the one every other encoder here uses.
//
// Memory shape of dctq_strip_kernel (tic_kernels.hip), none of its floating point: a wave owns a strip of 8 horizontally
// adjacent blocks (64 x 8 pixels); lane 8*r + b loads the 8 bytes of pixel row r of block b, so every 8 lanes read 64 contiguous bytes;
// the wave's 8 blocks leave as one contiguous 1 KiB of coefficients, 16 bytes per lane, one writer per line.  In between, per lane:
//   row pass   : IMG_fdct's row butterflies on the lane's own pixel row, straight out of the loaded registers (pixel ^ 0x80 as int8);
//   transpose  : the eight int16 results go to wave-private LDS transposed (the int16 store IS the reference's truncation); lane 8*b + c
//                reads column c of block b back as one 16-byte piece;
//   column pass: the same butterflies down that column; int16 truncation; multiply-and-shift quantiser with the setting's reciprocals
//                (eight table words per lane, loaded once per wave);
//   zig-zag    : int16 scatter into the block's 128-byte image in LDS, read back 16 bytes per lane, stored.
// Waves are persistent over a grid-stride walk of the strips; the next strip's pixels are requested before the current one is worked
// on.  No fast path, no guard band, no rare path, no counters: 32-bit integer VALU from end to end.
// fdctq_scaled_kernel_v is the same walk in descriptor form: one launch for frames of any sizes and settings (tic_scaled_frames.h).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "tic_hooks.h"
#include "tic_scaled.h"
#include "tic_scaled_math.h"

namespace tic {

namespace {

constexpr int kWaves = 4;     // waves per workgroup
constexpr int kBlkB = 144;    // bytes per block in the LDS staging buffers (128 + 16 pad: the 8 blocks start in different banks)
constexpr int kMaxGroups = 2048; // workgroups that are resident at once on 256 CUs (8 per CU): larger frames are walked, not tiled

__device__ const ScaledTab kScaledTabDev = make_scaled_tab();

__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 16 bytes per lane, write-through and non-temporal, as the strip kernel's coefficient stores (a vector store: one address per lane)
__device__ __forceinline__ void store16_stream(void *p, const uint4 &v) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 d = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1 nt" : : "v"(p), "v"(d) : "memory");
}

__device__ __forceinline__ int sx8(uint32_t w, int k) { return (int)(int8_t)(w >> (8 * k)); }

// pixel row lr of block lb of strip `tile` (zeros for a strip past the walk or a block past the frame's right edge)
__device__ __forceinline__ uint2 load_strip_row(const ScaledArgs &a, const uint8_t *img, int tile, int lr, int lb) {
    uint2 v = make_uint2(0u, 0u);
    if (tile >= a.ntiles) return v;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int bx = tx * 8 + lb;
    if (bx >= a.bw) return v;
    const uint8_t *p = img + (long)(ty * 8 + lr) * a.stride + (long)bx * 8;
    if (a.aligned8) return *reinterpret_cast<const uint2 *>(p);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v.x |= (uint32_t)p[k] << (8 * k);
        v.y |= (uint32_t)p[k + 4] << (8 * k);
    }
    return v;
}

__global__ __launch_bounds__(kWaves * 64) void fdctq_scaled_kernel(ScaledArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char ldsT_all[kWaves][8 * kBlkB]; // transposed row-pass results
    __shared__ __attribute__((aligned(16))) unsigned char ldsZ_all[kWaves][8 * kBlkB]; // zig-zag images
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned char *ldsT = ldsT_all[wave], *ldsZ = ldsZ_all[wave];
    const uint8_t *img = a.img + (long)blockIdx.y * a.frame_stride_in; // one grid row per frame
    char *out = reinterpret_cast<char *>(a.out) + (long)blockIdx.y * a.frame_stride_out;
    const int lr = lane >> 3, lb = lane & 7; // load phase and row pass: pixel row lr of block lb
    const int b = lane >> 3, i = lane & 7;   // column pass: column i of block b; store: 16-byte piece i of block b
    uint32_t tab[8];                         // reciprocal | QUANT >> 1 | scan position of coefficient (u, i), u = 0..7
#pragma unroll
    for (int u = 0; u < 8; u++) tab[u] = kScaledTabDev.w[a.qf][u * 8 + i];
    int16_t *tw = reinterpret_cast<int16_t *>(ldsT + lb * kBlkB + lr * 2);          // + 16 bytes per column
    const uint4 *tr = reinterpret_cast<const uint4 *>(ldsT + b * kBlkB + i * 16);
    unsigned char *zblk = ldsZ + b * kBlkB;
    const uint4 *zr = reinterpret_cast<const uint4 *>(zblk + i * 16);

    const int nwaves = (int)gridDim.x * kWaves;
    int tile = __builtin_amdgcn_readfirstlane((int)blockIdx.x * kWaves + wave);
    uint2 cur = load_strip_row(a, img, tile, lr, lb);
    for (; tile < a.ntiles; tile += nwaves) {
        const uint2 nxt = load_strip_row(a, img, tile + nwaves, lr, lb); // in flight while this strip is worked on
        // ---- row pass (img.c:55-88) ---------------------------------------------------------------------------------------
        const uint32_t lo = cur.x ^ 0x80808080u, hi = cur.y ^ 0x80808080u;
        int s0 = sx8(lo, 0), s1 = sx8(lo, 1), s2 = sx8(lo, 2), s3 = sx8(lo, 3);
        int s4 = sx8(hi, 0), s5 = sx8(hi, 1), s6 = sx8(hi, 2), s7 = sx8(hi, 3);
        fdct8_scaled(s0, s1, s2, s3, s4, s5, s6, s7);
        tw[0 * 8] = (int16_t)s0; tw[1 * 8] = (int16_t)s1; tw[2 * 8] = (int16_t)s2; tw[3 * 8] = (int16_t)s3;
        tw[4 * 8] = (int16_t)s4; tw[5 * 8] = (int16_t)s5; tw[6 * 8] = (int16_t)s6; tw[7 * 8] = (int16_t)s7;
        wave_fence();
        const uint4 col = *tr;
        wave_fence();
        // ---- column pass (img.c:91-124) -----------------------------------------------------------------------------------
        s0 = (int)(col.x << 16) >> 16; s1 = (int)col.x >> 16; s2 = (int)(col.y << 16) >> 16; s3 = (int)col.y >> 16;
        s4 = (int)(col.z << 16) >> 16; s5 = (int)col.z >> 16; s6 = (int)(col.w << 16) >> 16; s7 = (int)col.w >> 16;
        fdct8_scaled(s0, s1, s2, s3, s4, s5, s6, s7);
        // ---- quantiser (img.c:194-205) and zig-zag --------------------------------------------------------------------------
        const int s[8] = {s0, s1, s2, s3, s4, s5, s6, s7};
#pragma unroll
        for (int u = 0; u < 8; u++)
            *reinterpret_cast<int16_t *>(zblk + ((tab[u] >> 23) & 0x7eu)) = (int16_t)quant_scaled((int)(int16_t)s[u], tab[u]);
        wave_fence();
        const uint4 val = *zr;
        wave_fence();
        const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
        const int bx = tx * 8 + b;
        if (bx < a.bw) store16_stream(out + ((size_t)ty * (size_t)a.bw + (size_t)bx) * 128 + (size_t)i * 16, val);
        cur = nxt;
    }
}

// ---- descriptor form: the strips of up to kScaledMaxFrames frames of any sizes and settings in ONE launch --------------------------------
// The walk is the one above over the launch's global strip index; what the kernel above takes from its arguments a wave takes from the
// record the strip belongs to.  A record is found by a ballot over one table entry per lane (loaded once per wave), so its index is
// wave-uniform and its fields arrive by scalar loads; a wave looks again only when its walk leaves the record's strips.
struct StripRec { // wave-uniform: the record the wave is in
    const uint8_t *img;
    char *out;        // the frame's first output block
    long pitch;
    int bw, tiles_x;
    int first, end;   // the record's strips, in the launch's count
    int qf, aligned8;
};

__device__ __forceinline__ void find_strip_rec(const ScaledFrameTable *__restrict__ t, uint32_t my_first, int g, StripRec &s) {
    const int f = __builtin_amdgcn_readfirstlane(__popcll(__ballot(my_first <= (uint32_t)g)) - 1);
    const ScaledFrameRec &r = t->rec[f];
    s.img = reinterpret_cast<const uint8_t *>(t->img_base + r.img_off);
    s.out = reinterpret_cast<char *>(t->out_base + r.first_block * 128ull);
    s.pitch = (long)r.pitch;
    s.bw = (int)r.bw, s.tiles_x = (int)r.tiles_x;
    s.first = (int)r.first_strip, s.end = (int)(r.first_strip + r.nstrips);
    s.qf = r.qf, s.aligned8 = (int)r.aligned8;
}

// pixel row lr of block lb of strip g, which lies in record s (zeros for a block past the frame's right edge)
__device__ __forceinline__ uint2 load_strip_row_v(const StripRec &s, int g, int lr, int lb) {
    uint2 v = make_uint2(0u, 0u);
    const int tile = g - s.first;
    const int ty = tile / s.tiles_x, tx = tile - ty * s.tiles_x;
    const int bx = tx * 8 + lb;
    if (bx >= s.bw) return v;
    const uint8_t *p = s.img + (long)(ty * 8 + lr) * s.pitch + (long)bx * 8;
    if (s.aligned8) return *reinterpret_cast<const uint2 *>(p);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v.x |= (uint32_t)p[k] << (8 * k);
        v.y |= (uint32_t)p[k + 4] << (8 * k);
    }
    return v;
}

__global__ __launch_bounds__(kWaves * 64) void fdctq_scaled_kernel_v(const ScaledFrameTable *__restrict__ t, int nstrips) {
    __shared__ __attribute__((aligned(16))) unsigned char ldsT_all[kWaves][8 * kBlkB]; // transposed row-pass results
    __shared__ __attribute__((aligned(16))) unsigned char ldsZ_all[kWaves][8 * kBlkB]; // zig-zag images
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned char *ldsT = ldsT_all[wave], *ldsZ = ldsZ_all[wave];
    const int lr = lane >> 3, lb = lane & 7; // load phase and row pass: pixel row lr of block lb
    const int b = lane >> 3, i = lane & 7;   // column pass: column i of block b; store: 16-byte piece i of block b
    int16_t *tw = reinterpret_cast<int16_t *>(ldsT + lb * kBlkB + lr * 2);          // + 16 bytes per column
    const uint4 *tr = reinterpret_cast<const uint4 *>(ldsT + b * kBlkB + i * 16);
    unsigned char *zblk = ldsZ + b * kBlkB;
    const uint4 *zr = reinterpret_cast<const uint4 *>(zblk + i * 16);

    const int nwaves = (int)gridDim.x * kWaves;
    int g = __builtin_amdgcn_readfirstlane((int)blockIdx.x * kWaves + wave);
    if (g >= nstrips) return;
    const uint32_t my_first = t->first_strip[lane]; // the wave's copy of the search column
    StripRec rc;
    find_strip_rec(t, my_first, g, rc);
    uint2 cur = load_strip_row_v(rc, g, lr, lb);
    uint32_t tab[8]; // reciprocal | QUANT >> 1 | scan position of coefficient (u, i), u = 0..7, at setting tab_qf
    int tab_qf = -1;
    for (; g < nstrips; g += nwaves) {
        // the next strip, perhaps another record's: in flight while this strip is worked on
        const int gn = g + nwaves;
        StripRec rn = rc;
        uint2 nxt = make_uint2(0u, 0u);
        if (gn < nstrips) {
            if (gn >= rn.end) find_strip_rec(t, my_first, gn, rn);
            nxt = load_strip_row_v(rn, gn, lr, lb);
        }
        if (rc.qf != tab_qf) { // eight table words per lane, again only where the setting changes between two strips of the walk
            tab_qf = rc.qf;
#pragma unroll
            for (int u = 0; u < 8; u++) tab[u] = kScaledTabDev.w[tab_qf][u * 8 + i];
        }
        // ---- row pass (img.c:55-88) ---------------------------------------------------------------------------------------
        const uint32_t lo = cur.x ^ 0x80808080u, hi = cur.y ^ 0x80808080u;
        int s0 = sx8(lo, 0), s1 = sx8(lo, 1), s2 = sx8(lo, 2), s3 = sx8(lo, 3);
        int s4 = sx8(hi, 0), s5 = sx8(hi, 1), s6 = sx8(hi, 2), s7 = sx8(hi, 3);
        fdct8_scaled(s0, s1, s2, s3, s4, s5, s6, s7);
        tw[0 * 8] = (int16_t)s0; tw[1 * 8] = (int16_t)s1; tw[2 * 8] = (int16_t)s2; tw[3 * 8] = (int16_t)s3;
        tw[4 * 8] = (int16_t)s4; tw[5 * 8] = (int16_t)s5; tw[6 * 8] = (int16_t)s6; tw[7 * 8] = (int16_t)s7;
        wave_fence();
        const uint4 col = *tr;
        wave_fence();
        // ---- column pass (img.c:91-124) -----------------------------------------------------------------------------------
        s0 = (int)(col.x << 16) >> 16; s1 = (int)col.x >> 16; s2 = (int)(col.y << 16) >> 16; s3 = (int)col.y >> 16;
        s4 = (int)(col.z << 16) >> 16; s5 = (int)col.z >> 16; s6 = (int)(col.w << 16) >> 16; s7 = (int)col.w >> 16;
        fdct8_scaled(s0, s1, s2, s3, s4, s5, s6, s7);
        // ---- quantiser (img.c:194-205) and zig-zag --------------------------------------------------------------------------
        const int s[8] = {s0, s1, s2, s3, s4, s5, s6, s7};
#pragma unroll
        for (int u = 0; u < 8; u++)
            *reinterpret_cast<int16_t *>(zblk + ((tab[u] >> 23) & 0x7eu)) = (int16_t)quant_scaled((int)(int16_t)s[u], tab[u]);
        wave_fence();
        const uint4 val = *zr;
        wave_fence();
        const int tile = g - rc.first;
        const int ty = tile / rc.tiles_x, tx = tile - ty * rc.tiles_x;
        const int bx = tx * 8 + b;
        if (bx < rc.bw) store16_stream(rc.out + ((size_t)ty * (size_t)rc.bw + (size_t)bx) * 128 + (size_t)i * 16, val);
        cur = nxt;
        rc = rn;
    }
}

} // namespace

hipError_t launch_fdctq_scaled_v(const ScaledFrameTable *d_table, uint32_t total_strips, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop) {
    if (total_strips == 0) return hipSuccess;
    if (!d_table || total_strips > 0x7fffffffu) return hipErrorInvalidValue;
    unsigned groups = (total_strips + kWaves - 1) / kWaves;
    if (groups > (unsigned)kMaxGroups) groups = (unsigned)kMaxGroups;
    if (const char *e = test_hook("TIC_SCALED_V_GROUPS")) // (tests: few waves walk strips of several frames at tiny shapes)
        if (atoi(e) >= 1 && (unsigned)atoi(e) < groups) groups = (unsigned)atoi(e);
    const dim3 grid(groups), block(kWaves * 64);
    if (ev_start && ev_stop)
        hipExtLaunchKernelGGL(fdctq_scaled_kernel_v, grid, block, 0, stream, ev_start, ev_stop, 0, d_table, (int)total_strips);
    else
        hipLaunchKernelGGL(fdctq_scaled_kernel_v, grid, block, 0, stream, d_table, (int)total_strips);
    return hipGetLastError();
}

hipError_t launch_fdctq_scaled(const ScaledArgs &a, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop) {
    if (a.ntiles <= 0 || a.nframes <= 0) return hipSuccess;
    if (a.qf < 0 || a.qf > 3) return hipErrorInvalidValue;
    int groups = (a.ntiles + kWaves - 1) / kWaves;
    const int cap = kMaxGroups / a.nframes > 0 ? kMaxGroups / a.nframes : 1;
    if (groups > cap) groups = cap;
    const dim3 grid((unsigned)groups, (unsigned)a.nframes), block(kWaves * 64);
    if (ev_start && ev_stop)
        hipExtLaunchKernelGGL(fdctq_scaled_kernel, grid, block, 0, stream, ev_start, ev_stop, 0, a);
    else
        hipLaunchKernelGGL(fdctq_scaled_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

} // namespace tic
