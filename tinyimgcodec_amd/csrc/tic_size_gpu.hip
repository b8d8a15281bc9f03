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
#include "tic_size_walk.h"

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
static_assert(kSizeGroupChunks == (size_t)(kSizeWaves * kSizeUnroll), "a workgroup's round is what the probe table counts groups by");

// What a wave walks: a run of blocks whose DPCM starts against 0 - a frame of the uniform launch, a probe of the descriptor form.
struct SizeSpan {
    const int16_t *fz;              // its first block
    unsigned long long nblocks, nchunks;
    unsigned long long first_chunk; // of this wave: its index among the waves that share the span ...
    unsigned long long nwaves;      // ... and their number: the stride of its loop
};

// The walk both kernels share: the wave's chunks, kSizeUnroll in flight.  Every index is the span's own: the `valid` test of a partial last
// chunk, the `ch != 0` guard on the DC in front of the wave's first block, the DPCM start.  Bits below bit 16 summed into `bits`, "no code"
// into `bad`.
__device__ __forceinline__ void size_walk(const SizeSpan &s, int lane, int k, const uint32_t *tab, uint32_t &bits, uint32_t &bad) {
    const int16_t *fz = s.fz;
    for (unsigned long long base = s.first_chunk; base < s.nchunks; base += s.nwaves * kSizeUnroll) {
        uint4 v[kSizeUnroll];
        int p0[kSizeUnroll];
        bool valid[kSizeUnroll];
#pragma unroll
        for (int u = 0; u < kSizeUnroll; u++) { // every load of the round, back to back
            const unsigned long long ch = base + (unsigned long long)u * s.nwaves;
            const unsigned long long blk = ch * 8ull + (unsigned long long)(lane >> 3);
            valid[u] = ch < s.nchunks && blk < s.nblocks;
            v[u] = valid[u] ? *reinterpret_cast<const uint4 *>(fz + blk * 64ull + (unsigned long long)(k * 8)) : make_uint4(0u, 0u, 0u, 0u);
            p0[u] = (lane == 0 && valid[u] && ch != 0ull) ? (int)fz[(ch * 8ull - 1ull) * 64ull] : 0; // DC of the block before the wave's first
        }
#pragma unroll
        for (int u = 0; u < kSizeUnroll; u++) {
            int prev = __shfl_up((int)(int16_t)(v[u].x & 0xffff), 8, 64); // DC of the block before: lane - 8 ...
            if (lane == 0) prev = p0[u];                                   // ... or the last block of the chunk before (span start: 0)
            const uint32_t acc = lane_bits(v[u], k, prev, tab);
            bits += valid[u] ? (acc & 0xffffu) : 0u;
            bad |= valid[u] ? (acc >> 16) : 0u;
        }
    }
}

// The workgroup's sum: ONE vector atomic add (and one or, where a coefficient had no code) on the span's result.
__device__ __forceinline__ void size_reduce(uint32_t bits, uint32_t bad, int lane, int wave, unsigned long long *wsum, uint32_t *wbad, SizeResult *dst) {
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
        if (s) atomicAdd(&dst->bits, s);
        if (b) atomicOr(&dst->nocode, 1u);
    }
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
    const SizeSpan s = {zz + frame * blocks_per_frame * 64ull, blocks_per_frame, chunks_per_frame,
                        (unsigned long long)blockIdx.x * kSizeWaves + (unsigned long long)wave, (unsigned long long)gridDim.x * kSizeWaves};
    uint32_t bits = 0, bad = 0; // (a lane adds at most 480 bits per chunk: 2^32 is out of reach of any frame the block count allows)
    __syncthreads();
    size_walk(s, lane, k, tab, bits, bad);
    size_reduce(bits, bad, lane, wave, wsum, wbad, res + frame);
}

// The descriptor form: up to kSizeMaxProbes PROBES - a frame's coefficients at one quality, any block count each, back to back in zz - in ONE
// launch.  A workgroup finds its probe the way the entropy stage's descriptor form finds its frame (find_frame, tic_entropy_gpu.hip): lane l
// loads first_group[l] (0xffffffff behind the last probe), the wave counts the entries <= blockIdx.x; the count is a scalar, so the record
// comes by scalar loads and the span stays wave-uniform.  The wave stride is the probe's own group count, not the grid's; the result entry
// (and with it the "no code" flag) is the probe's.
__global__ __launch_bounds__(kSizeWaves * 64) void stream_size_kernel_v(const int16_t *__restrict__ zz, const SizeTabDev *__restrict__ tabdev,
                                                                        const SizeProbeTable *__restrict__ pt, SizeResult *__restrict__ res) {
    __shared__ uint32_t tab[kSizeTabRuns * kSizeTabSizes];
    __shared__ unsigned long long wsum[kSizeWaves];
    __shared__ uint32_t wbad[kSizeWaves];
    for (int i = threadIdx.x; i < kSizeTabRuns * kSizeTabSizes; i += kSizeWaves * 64) tab[i] = tabdev->len[i];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = lane & 7;
    const uint32_t first = pt->first_group[lane];
    const int probe = __builtin_amdgcn_readfirstlane(__popcll(__ballot(first <= blockIdx.x)) - 1);
    const SizeProbeRec &r = pt->rec[probe];
    const SizeSpan s = {zz + r.first_block * 64ull, r.nblocks, (r.nblocks + 7ull) / 8ull,
                        (unsigned long long)(blockIdx.x - r.first_group) * kSizeWaves + (unsigned long long)wave, (unsigned long long)r.ngroups * kSizeWaves};
    uint32_t bits = 0, bad = 0;
    __syncthreads();
    size_walk(s, lane, k, tab, bits, bad);
    size_reduce(bits, bad, lane, wave, wsum, wbad, res + r.result);
}

} // namespace

hipError_t stream_size_gpu(const int16_t *d_zz, size_t blocks_per_frame, int nframes, const SizeTabDev *d_tab, SizeResult *d_res,
                           hipStream_t stream) {
    if (blocks_per_frame == 0 || nframes <= 0) return hipSuccess;
    if (nframes > 65535) return hipErrorInvalidValue;
    const size_t chunks = (blocks_per_frame + 7) / 8;
    const size_t groups = size_probe_groups(blocks_per_frame);
    hipLaunchKernelGGL(stream_size_kernel, dim3((unsigned)groups, (unsigned)nframes), dim3(kSizeWaves * 64), 0, stream, d_zz, d_tab,
                       (unsigned long long)blocks_per_frame, (unsigned long long)chunks, d_res);
    return hipGetLastError();
}

hipError_t stream_size_gpu_v(const int16_t *d_zz, const SizeProbeTable *d_probes, size_t ngroups, const SizeTabDev *d_tab, SizeResult *d_res,
                             hipStream_t stream) {
    if (ngroups == 0) return hipSuccess;
    if (ngroups > (size_t)kSizeMaxProbes * kSizeMaxGroups) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_size_kernel_v, dim3((unsigned)ngroups), dim3(kSizeWaves * 64), 0, stream, d_zz, d_tab, d_probes, d_res);
    return hipGetLastError();
}

} // namespace tic
