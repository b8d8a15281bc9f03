// tic_requant_gpu.hip - a stored stream's coefficients at another quality, without pixels: dequantise with the divisors of the quality the
// stream was written at, quantise with those of the new one.
//
// The stage is defined by the reference: block_quantize(block_quantize(c, q1, inverse=True), q2) (utils.py:48-53) on the coefficients the
// stream's reader returns - per coefficient, in float64 and in this order,
//     x = c * ((T * f1) / 100)        t = x / ((T * f2) / 100)        np.round(t)   (half to even)
// The table value T cancels in exact arithmetic but not in float64: the rounded product is divided, and exact ties (50 -> 25 halves every
// coefficient) sit beside quotients that the two roundings in front of np.round move across a half.  So the kernel reproduces the three
// float64 operations one by one - the divisors are DctqConsts::div, the very numbers the forward quantiser divides by (build_consts), the
// division is the compiler's correctly rounded IEEE one (div_rn of tic_math.h is proven for the forward quantiser's numerators only), the
// rounding is rint - with contraction off, as everywhere in this library.
//
// Decomposition, as the size kernel's (tic_size_gpu.hip): 8 lanes per block, lane k owns zig-zag entries 8k .. 8k + 7 (one 16-byte load,
// one 16-byte store); a wave takes CHUNKS of 8 consecutive blocks (1 KB, contiguous).  A lane needs nothing from its neighbours: its 16
// divisors (8 of each quality, reached from its zig-zag positions through DctqConsts::zznat) are loaded once per workgroup, whose job -
// and with it the pair of qualities - is uniform.  Zero coefficients are the majority of any stored frame and requantise to zero at any
// pair of qualities: a lane whose eight entries are all zero stores them as they are, and where that holds for every lane of the wave
// the float64 instructions are branched over (the compiler's execz skip of the divergent region).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tic_requant_gpu.h"
#include "tic_size_walk.h"

namespace tic {

namespace {

// (kRequantWaves, kRequantUnroll and the chunk arithmetic of a wave's walk: tic_requant_plan.h, where the host self-test walks with them too)

// One coefficient: the reference's three float64 operations.  `bad`: the result does not fit int16.
__device__ __forceinline__ int requant_one(int c, double d_from, double d_to, bool &bad) {
#pragma clang fp contract(off)
    const double x = (double)c * d_from;
    const double t = x / d_to;
    const double r = rint(t);
    bad |= !(r >= -32768.0 && r <= 32767.0);
    return (int)r; // (|r| < 2^30 for every int16 c and every pair of qualities: 32768 x 6050 / 0.2)
}

__global__ __launch_bounds__(kRequantWaves * 64) void requant_kernel_v(const int16_t *src, int16_t *dst, // (no __restrict__: a job may be in place)
                                                                       const RequantJobTable *__restrict__ jt,
                                                                       const DctqConsts *__restrict__ consts, uint32_t *__restrict__ flags) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = lane & 7;
    // the workgroup's job: lane l compares first_group[l] with the workgroup's index (entries behind the last job are 0xffffffff)
    const uint32_t first = jt->first_group[lane];
    const int job = __builtin_amdgcn_readfirstlane(__popcll(__ballot(first <= blockIdx.x)) - 1);
    const RequantJobRec &r = jt->rec[job];
    const RequantWalk wk = requant_walk(r.nblocks, blockIdx.x - r.first_group, r.ngroups, wave);
    const int16_t *sz = src + r.src_block * 64ull;
    int16_t *dz = dst + r.dst_block * 64ull;
    const DctqConsts *cf = consts + r.q_from, *ct = consts + r.q_to;
    double d_from[8], d_to[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int nat = cf->zznat[k * 8 + j]; // natural index of zig-zag position 8k + j
        d_from[j] = cf->div[nat];
        d_to[j] = ct->div[nat];
    }
    bool bad = false;
    for (unsigned long long base = wk.first_chunk; base < wk.nchunks; base += requant_round_stride(wk)) {
        uint4 v[kRequantUnroll];
        bool valid[kRequantUnroll];
        unsigned long long at[kRequantUnroll];
#pragma unroll
        for (int u = 0; u < kRequantUnroll; u++) { // every load of the round, back to back
            unsigned long long ch, blk;
            valid[u] = requant_lane_block(wk, base, u, lane, &ch, &blk);
            at[u] = blk * 64ull + (unsigned long long)(k * 8);
            v[u] = valid[u] ? *reinterpret_cast<const uint4 *>(sz + at[u]) : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < kRequantUnroll; u++) {
            uint4 o = v[u];
            if ((v[u].x | v[u].y | v[u].z | v[u].w) != 0u) { // (an invalid lane holds zeros)
                int c[8];
                c[0] = (int)(int16_t)(v[u].x & 0xffff); c[1] = (int)v[u].x >> 16; c[2] = (int)(int16_t)(v[u].y & 0xffff); c[3] = (int)v[u].y >> 16;
                c[4] = (int)(int16_t)(v[u].z & 0xffff); c[5] = (int)v[u].z >> 16; c[6] = (int)(int16_t)(v[u].w & 0xffff); c[7] = (int)v[u].w >> 16;
#pragma unroll
                for (int j = 0; j < 8; j++) c[j] = c[j] != 0 ? requant_one(c[j], d_from[j], d_to[j], bad) : 0;
                o.x = ((uint32_t)c[0] & 0xffffu) | ((uint32_t)c[1] << 16);
                o.y = ((uint32_t)c[2] & 0xffffu) | ((uint32_t)c[3] << 16);
                o.z = ((uint32_t)c[4] & 0xffffu) | ((uint32_t)c[5] << 16);
                o.w = ((uint32_t)c[6] & 0xffffu) | ((uint32_t)c[7] << 16);
            }
            if (valid[u]) *reinterpret_cast<uint4 *>(dz + at[u]) = o;
        }
    }
    // the job's range flag: one vector atomic per wave that saw a result outside int16
    if (__any(bad ? 1 : 0) && lane == 0) atomicOr(flags + r.flag, 1u);
}

// ---- the measuring instance ------------------------------------------------------------------------------------------------------------
// The same walk with the size kernel's lane sum (lane_bits, tic_size_walk.h) in the place of the store: a wave holds a round of four chunks
// in registers and takes them through its workgroup's qualities one after the other - the divisors of all of them lie in LDS, in zig-zag
// order (8 consecutive doubles per lane and quality: four 16-byte reads) -, so the frame is read once however many qualities are measured.
// What a lane needs from its neighbours is lane_bits' own (the zero run carried into it, the DC of the block before: lane - 8, or for the
// wave's first block the source DC in front of the chunk, requantised by lane 0, whose first divisor is the DC's).
// Sums: a quality's bits of a round are reduced over the wave at once (one 32-bit reduction: bits below bit 20, values without a code or
// outside int16 counted above it - a round is at most 4 x 64 x 8 values of at most 27 bits) and kept per wave in LDS; the workgroup ends in
// ONE atomic add per quality (and one or, where a value had no code), as idct_sse_kernel_v and the size kernel do.
// LDS: 32 KB of divisors for 64 qualities, the 4.3 KB size table, 3 KB of sums - four workgroups per CU.
__global__ __launch_bounds__(kRequantWaves * 64) void requant_size_kernel_v(const int16_t *__restrict__ src, unsigned long long nblocks,
                                                                            const RequantQualities qs, unsigned split,
                                                                            const DctqConsts *__restrict__ consts,
                                                                            const SizeTabDev *__restrict__ tabdev, SizeResult *__restrict__ res) {
    __shared__ uint32_t tab[kSizeTabRuns * kSizeTabSizes];
    __shared__ __attribute__((aligned(16))) double dto[kSizeMaxProbes * 64];
    __shared__ unsigned long long wsum[kRequantWaves][kSizeMaxProbes];
    __shared__ uint32_t wbad[kRequantWaves][kSizeMaxProbes];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = lane & 7;
    // this workgroup's qualities: i = blockIdx.y + li * split, li = 0 .. nlocal - 1
    const int nlocal = ((int)qs.nq - (int)blockIdx.y + (int)split - 1) / (int)split;
    for (int i = threadIdx.x; i < kSizeTabRuns * kSizeTabSizes; i += kRequantWaves * 64) tab[i] = tabdev->len[i];
    for (int i = threadIdx.x; i < nlocal * 64; i += kRequantWaves * 64) {
        const DctqConsts *ct = consts + qs.q_to[blockIdx.y + (unsigned)(i >> 6) * split];
        dto[i] = ct->div[ct->zznat[i & 63]];
    }
    for (int i = threadIdx.x; i < kRequantWaves * kSizeMaxProbes; i += kRequantWaves * 64) (&wsum[0][0])[i] = 0ull, (&wbad[0][0])[i] = 0u;
    const DctqConsts *cf = consts + qs.q_from;
    double d_from[8];
#pragma unroll
    for (int j = 0; j < 8; j++) d_from[j] = cf->div[cf->zznat[k * 8 + j]];
    const RequantWalk wk = requant_walk(nblocks, blockIdx.x, gridDim.x, wave);
    __syncthreads();
    for (unsigned long long base = wk.first_chunk; base < wk.nchunks; base += requant_round_stride(wk)) {
        uint4 v[kRequantUnroll];
        int p0[kRequantUnroll];
        bool valid[kRequantUnroll];
#pragma unroll
        for (int u = 0; u < kRequantUnroll; u++) { // every load of the round, back to back
            unsigned long long ch, blk;
            valid[u] = requant_lane_block(wk, base, u, lane, &ch, &blk);
            v[u] = valid[u] ? *reinterpret_cast<const uint4 *>(src + blk * 64ull + (unsigned long long)(k * 8)) : make_uint4(0u, 0u, 0u, 0u);
            p0[u] = (lane == 0 && valid[u] && ch != 0ull) ? (int)src[(ch * 8ull - 1ull) * 64ull] : 0; // source DC of the block before the wave's first
        }
        for (int li = 0; li < nlocal; li++) {
            double d_to[8];
#pragma unroll
            for (int j = 0; j < 8; j++) d_to[j] = dto[li * 64 + k * 8 + j];
            uint32_t round_sum = 0;
#pragma unroll
            for (int u = 0; u < kRequantUnroll; u++) {
                uint4 o = v[u];
                bool bad = false;
                if ((v[u].x | v[u].y | v[u].z | v[u].w) != 0u) {
                    int c[8];
                    c[0] = (int)(int16_t)(v[u].x & 0xffff); c[1] = (int)v[u].x >> 16; c[2] = (int)(int16_t)(v[u].y & 0xffff); c[3] = (int)v[u].y >> 16;
                    c[4] = (int)(int16_t)(v[u].z & 0xffff); c[5] = (int)v[u].z >> 16; c[6] = (int)(int16_t)(v[u].w & 0xffff); c[7] = (int)v[u].w >> 16;
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        bool b = false;
                        c[j] = c[j] != 0 ? requant_one(c[j], d_from[j], d_to[j], b) : 0;
                        if (b) c[j] = 0; // (lane_bits' look-up holds sizes up to 16: the value is counted as one without a code instead)
                        bad |= b;
                    }
                    o.x = ((uint32_t)c[0] & 0xffffu) | ((uint32_t)c[1] << 16);
                    o.y = ((uint32_t)c[2] & 0xffffu) | ((uint32_t)c[3] << 16);
                    o.z = ((uint32_t)c[4] & 0xffffu) | ((uint32_t)c[5] << 16);
                    o.w = ((uint32_t)c[6] & 0xffffu) | ((uint32_t)c[7] << 16);
                }
                int prev = __shfl_up((int)(int16_t)(o.x & 0xffff), 8, 64); // requantised DC of the block before: lane - 8 ...
                if (lane == 0) {                                            // ... or of the last block of the chunk before (frame start: 0)
                    bool b = false;
                    prev = p0[u] != 0 ? requant_one(p0[u], d_from[0], d_to[0], b) : 0;
                    if (b) prev = 0; // (that block's own lane counts it)
                }
                const uint32_t acc = lane_bits(o, k, prev, tab);
                round_sum += valid[u] ? (acc & 0xffffu) + ((acc >> 16) << 20) + (bad ? (1u << 20) : 0u) : 0u;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) round_sum += __shfl_xor(round_sum, off, 64);
            if (lane == 0) {
                wsum[wave][li] += round_sum & 0xfffffu;
                wbad[wave][li] |= round_sum >> 20;
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nlocal) {
        unsigned long long s = 0;
        uint32_t b = 0;
        for (int w = 0; w < kRequantWaves; w++) {
            s += wsum[w][threadIdx.x];
            b |= wbad[w][threadIdx.x];
        }
        SizeResult *dst = res + blockIdx.y + threadIdx.x * split;
        if (s) atomicAdd(&dst->bits, s);
        if (b) atomicOr(&dst->nocode, 1u);
    }
}

} // namespace

hipError_t requant_size_gpu_v(const int16_t *d_src, size_t nblocks, const RequantQualities &qs, const DctqConsts *d_consts, const SizeTabDev *d_tab,
                              SizeResult *d_res, hipStream_t stream) {
    if (nblocks == 0 || qs.nq < 1 || qs.nq > kSizeMaxProbes || qs.q_from < 1 || qs.q_from > 99 || (((uintptr_t)d_src) & 15u)) return hipErrorInvalidValue;
    for (int i = 0; i < qs.nq; i++)
        if (qs.q_to[i] < 1 || qs.q_to[i] > 99) return hipErrorInvalidValue;
    const size_t split = requant_size_split(nblocks, (size_t)qs.nq);
    hipLaunchKernelGGL(requant_size_kernel_v, dim3((unsigned)size_probe_groups(nblocks), (unsigned)split), dim3(kRequantWaves * 64), 0, stream, d_src,
                       (unsigned long long)nblocks, qs, (unsigned)split, d_consts, d_tab, d_res);
    return hipGetLastError();
}

hipError_t requant_gpu_v(const int16_t *d_src, int16_t *d_dst, const RequantJobTable *d_jobs, size_t ngroups, const DctqConsts *d_consts,
                         uint32_t *d_flags, hipStream_t stream) {
    if (ngroups == 0) return hipSuccess;
    if (ngroups > (size_t)kSizeMaxProbes * kSizeMaxGroups) return hipErrorInvalidValue;
    if ((((uintptr_t)d_src) | ((uintptr_t)d_dst)) & 15u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(requant_kernel_v, dim3((unsigned)ngroups), dim3(kRequantWaves * 64), 0, stream, d_src, d_dst, d_jobs, d_consts, d_flags);
    return hipGetLastError();
}

} // namespace tic
