// tic_size_gpu.hip - how long would the stream be?  The payload bits of a default-table stream from its coefficients, without
// producing the stream: one read of the int16 coefficients, a sum per lane, one vector atomic per workgroup.
//
// The length of compress()'s stream (codec.py:133-164) is a pure function of the coefficients: per block the DC category code and its
// value bits (huffman.py:41-63 on the DPCM of codec.py:34-35), per non-zero AC entry the ZRLs of its zero run, the (run, size) code and
// the size bits (huffman.py:12-33), the EOB that closes every block; rounded up to a byte (bitbuffer.py:17-18) behind the 16-byte header.
// The packing kernels of tic_entropy_gpu.hip find these bits on the way to placing them; this kernel only adds them up, which leaves
// out everything that makes packing expensive: no bit strings in LDS, no staging slots, no offsets, no placing launch.
//
// Decomposition, as the packers': 8 lanes per block, lane k owns zig-zag entries 8k .. 8k + 7 (one 16-byte load); a wave takes CHUNKS
// of 8 consecutive blocks (1 KB, contiguous) and keeps kSizeUnroll of them in flight.  What a lane needs from its neighbours is the
// zero run carried into it (the packers' carry-through scan over the 8 lanes of a block, by DPP) and, in lane 0 of a block, the DC of
// the block before (lane - 8; the wave's first block reads it from memory, the frame's first block differences against 0).
// Every entry then costs one LDS look-up in a table indexed by (zero run in front of it, size category): tic_size_gpu.h.  The DC goes
// through the same look-up (row 63, which also carries the block's EOB), a zero entry finds 0 there, an entry without a code finds
// 2^16: a lane's sum of eight look-ups holds the bits below and the "no code" count above bit 16, with no branch in the walk.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "tic_entropy_gpu.h"
#include "tic_size_gpu.h"

namespace tic {

void build_size_tab(SizeTabDev *t) {
    HuffDev hd;
    build_huff_dev(&hd); // ac_bits / dc_bits: code length + size bits, 0 = no code
    const uint32_t zrl = hd.ac_bits[0xF0], eob = hd.ac_bits[0];
    for (int run = 0; run < kSizeTabRuns; run++)
        for (int sz = 0; sz < kSizeTabSizes; sz++) {
            uint32_t v;
            if (run == kSizeDcRow) {
                v = (sz <= 11 && hd.dc_bits[sz]) ? hd.dc_bits[sz] + eob : kSizeNoCode;
            } else if (sz == 0) {
                v = 0;
            } else {
                const uint32_t b = sz <= 15 ? hd.ac_bits[((run & 15) << 4) | sz] : 0u;
                v = b ? (uint32_t)(run >> 4) * zrl + b : kSizeNoCode;
            }
            t->len[run * kSizeTabSizes + sz] = v;
        }
}

namespace {

constexpr int kSizeWaves = 4;      // waves per workgroup
constexpr int kSizeUnroll = 4;     // chunks a wave loads before it walks the first: 4 KB in flight per wave
constexpr int kSizeMaxGroups = 1024; // workgroups per frame at most (4 per CU): each ends in ONE atomic on the frame's result

// Size category of a coefficient: its bit length, 0 for 0.  The exponent of the float is exact for |v| <= 65535.
__device__ __forceinline__ int size_category(int v) {
    int e;
    (void)frexpf((float)v, &e);
    return e;
}

template <int N>
__device__ __forceinline__ int dpp_row_shr(int v) {
    return __builtin_amdgcn_update_dpp(0, v, 0x110 + N, 0xf, 0xf, false);
}

// The bits of one lane's eight entries (k = lane & 7: entries 8k .. 8k + 7 of its block); prev_dc: the DC of the block before (used by
// k == 0), 0 for the frame's first block.  Bits below bit 16, entries without a code counted above it.
__device__ __forceinline__ uint32_t lane_bits(const uint4 v, int k, int prev_dc, const uint32_t *tab) {
    int c[8];
    c[0] = (int)(int16_t)(v.x & 0xffff); c[1] = (int)v.x >> 16; c[2] = (int)(int16_t)(v.y & 0xffff); c[3] = (int)v.y >> 16;
    c[4] = (int)(int16_t)(v.z & 0xffff); c[5] = (int)v.z >> 16; c[6] = (int)(int16_t)(v.w & 0xffff); c[7] = (int)v.w >> 16;
    // zero run that ends with this lane's last entry (tz) and whether the lane holds nothing else (az); the DC position is no AC zero
    int nz_mask = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) nz_mask |= (c[j] != 0 && !(k == 0 && j == 0)) ? (1 << j) : 0;
    int az = nz_mask == 0;
    int tz = az ? (k == 0 ? 7 : 8) : (__clz(nz_mask) - 24);
    // carry-through scan over the 8 lanes of the block (a lane only uses lanes of its own block: k >= D)
#define TIC_CARRY_STEP(D)                                          \
    {                                                              \
        const int pa = dpp_row_shr<D>(az), pt = dpp_row_shr<D>(tz); \
        if (k >= D) {                                              \
            tz = az ? pt + tz : tz;                                \
            az = az & pa;                                          \
        }                                                          \
    }
    TIC_CARRY_STEP(1)
    TIC_CARRY_STEP(2)
    TIC_CARRY_STEP(4)
#undef TIC_CARRY_STEP
    int run = dpp_row_shr<1>(tz); // the zero run in front of this lane's first entry (at most 55)
    if (k == 0) {
        run = kSizeDcRow;    // the DC difference takes the table's DC row ...
        c[0] = c[0] - prev_dc;
    }
    uint32_t acc = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        acc += tab[run * kSizeTabSizes + size_category(c[j])];
        run = c[j] != 0 ? 0 : run + 1;
        if (j == 0 && k == 0) run = 0; // ... and the AC run starts behind it
    }
    return acc;
}

__global__ __launch_bounds__(kSizeWaves * 64) void stream_size_kernel(const int16_t *__restrict__ zz, const SizeTabDev *__restrict__ tabdev,
                                                                      unsigned long long blocks_per_frame, unsigned long long chunks_per_frame,
                                                                      SizeResult *__restrict__ res) {
    __shared__ uint32_t tab[kSizeTabRuns * kSizeTabSizes];
    __shared__ unsigned long long wsum[kSizeWaves];
    __shared__ uint32_t wbad[kSizeWaves];
    for (int i = threadIdx.x; i < kSizeTabRuns * kSizeTabSizes; i += kSizeWaves * 64) tab[i] = tabdev->len[i];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = lane & 7;
    const unsigned long long frame = blockIdx.y;
    const int16_t *fz = zz + frame * blocks_per_frame * 64ull;
    const unsigned long long nwaves = (unsigned long long)gridDim.x * kSizeWaves;
    const unsigned long long gw = (unsigned long long)blockIdx.x * kSizeWaves + (unsigned long long)wave;
    uint32_t bits = 0, bad = 0; // (a lane adds at most 480 bits per chunk: 2^32 is out of reach of any frame the block count allows)
    __syncthreads();
    for (unsigned long long base = gw; base < chunks_per_frame; base += nwaves * kSizeUnroll) {
        uint4 v[kSizeUnroll];
        int p0[kSizeUnroll];
        bool valid[kSizeUnroll];
#pragma unroll
        for (int u = 0; u < kSizeUnroll; u++) { // every load of the round, back to back
            const unsigned long long ch = base + (unsigned long long)u * nwaves;
            const unsigned long long blk = ch * 8ull + (unsigned long long)(lane >> 3);
            valid[u] = ch < chunks_per_frame && blk < blocks_per_frame;
            v[u] = valid[u] ? *reinterpret_cast<const uint4 *>(fz + blk * 64ull + (unsigned long long)(k * 8)) : make_uint4(0u, 0u, 0u, 0u);
            p0[u] = (lane == 0 && valid[u] && ch != 0ull) ? (int)fz[(ch * 8ull - 1ull) * 64ull] : 0; // DC of the block before the wave's first
        }
#pragma unroll
        for (int u = 0; u < kSizeUnroll; u++) {
            int prev = __shfl_up((int)(int16_t)(v[u].x & 0xffff), 8, 64); // DC of the block before: lane - 8 ...
            if (lane == 0) prev = p0[u];                                   // ... or the last block of the chunk before (frame start: 0)
            const uint32_t acc = lane_bits(v[u], k, prev, tab);
            bits += valid[u] ? (acc & 0xffffu) : 0u;
            bad |= valid[u] ? (acc >> 16) : 0u;
        }
    }
    unsigned long long t = bits;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    const int any_bad = __any(bad != 0u);
    if (lane == 0) {
        wsum[wave] = t;
        wbad[wave] = any_bad ? 1u : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        uint32_t b = 0;
        for (int i = 0; i < kSizeWaves; i++) {
            s += wsum[i];
            b |= wbad[i];
        }
        if (s) atomicAdd(&res[frame].bits, s);
        if (b) atomicOr(&res[frame].nocode, 1u);
    }
}

} // namespace

hipError_t stream_size_gpu(const int16_t *d_zz, size_t blocks_per_frame, int nframes, const SizeTabDev *d_tab, SizeResult *d_res,
                           hipStream_t stream) {
    if (blocks_per_frame == 0 || nframes <= 0) return hipSuccess;
    if (nframes > 65535) return hipErrorInvalidValue;
    const size_t chunks = (blocks_per_frame + 7) / 8;
    size_t groups = (chunks + (size_t)(kSizeWaves * kSizeUnroll) - 1) / (size_t)(kSizeWaves * kSizeUnroll);
    if (groups > (size_t)kSizeMaxGroups) groups = (size_t)kSizeMaxGroups;
    hipLaunchKernelGGL(stream_size_kernel, dim3((unsigned)groups, (unsigned)nframes), dim3(kSizeWaves * 64), 0, stream, d_zz, d_tab,
                       (unsigned long long)blocks_per_frame, (unsigned long long)chunks, d_res);
    return hipGetLastError();
}

} // namespace tic
