// tic_adaptive_stats_gpu.hip - the symbol statistics of per-image Huffman tables as a PROBE: what adaptive_stats_v_kernel
// (tic_adaptive_gpu.hip) leaves for the same coefficients - counts, first-occurrence keys, the error word, bit for bit - from a walk in
// the size kernel's decomposition (tic_size_gpu.hip) instead of one thread per block.
//
// The length of an adaptive stream is a function of these statistics alone (adaptive_stream_size, tic_adaptive.cpp), so a rate search
// over the adaptive family is a transform and this kernel per probe.
//
// Decomposition: 8 lanes per block, lane k owns zig-zag entries 8k .. 8k + 7 (one 16-byte load); a wave takes chunks of 8 consecutive
// blocks and keeps kUnroll of them in flight; probes are found through a SizeProbeTable (tic_rate_plan.h), a probe's workgroups are capped
// and stride.  A lane needs from its neighbours
//   the zero run carried into it      the size kernel's carry-through scan over the 8 lanes of a block (row_shr DPP, lanes of one block only);
//   the DC of the block before        lane - 8; the wave's first block reads it from memory, a probe's first block differences against 0;
//   the symbols emitted below it      an exclusive prefix over the 8 lanes of the block, by the same DPP steps: a non-zero entry behind a run
//                                     of r zeros emits r >> 4 ZRLs and one (run, size) symbol; the first ZRL has the ordinal in front of the
//                                     entry, the (run, size) symbol comes r >> 4 later, EOB's ordinal is the block's count.
// Histogram: counts in LDS, kCopies copies (one per k: lanes of a wave that hit one bin in one instruction are at most 8), first keys
// once, pre-tested before atomicMin as stats_group does.  The EOB occurs once per block: lane 7 keeps count and smallest key in registers
// and adds them once, behind the walk.  The DC occurs once per block too: its one histogram update per block comes from lane 0.  A
// workgroup ends in one global atomicAdd / atomicMin per non-empty bin: sums and minima, so no result depends on the order of workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tic_adaptive.h"
#include "tic_adaptive_stats_gpu.h"

namespace tic {
namespace {

constexpr int kWaves = 4;  // waves per workgroup
constexpr int kUnroll = 4; // chunks a wave loads before it walks the first
static_assert(kSizeGroupChunks == (size_t)(kWaves * kUnroll), "a workgroup's round is what the probe table counts groups by");
constexpr int kCopies = 8;       // count histograms per workgroup, one per lane position in a block
constexpr int kCopyStride = 273; // words between them: copy c starts 17 c banks further

template <int N>
__device__ __forceinline__ int dpp_row_shr(int v) {
    return __builtin_amdgcn_update_dpp(0, v, 0x110 + N, 0xf, 0xf, false);
}

__device__ __forceinline__ int bit_len(int v) { // utils.py:9-10 of |v|
    const uint32_t a = (uint32_t)(v < 0 ? -v : v);
    return a ? 32 - __clz((int)a) : 0;
}

// One symbol (n of them for a ZRL run: consecutive ordinals, the first one's key) into the workgroup's histogram.
__device__ __forceinline__ void hit(uint32_t *cnt, unsigned long long *first, int bin, uint32_t n, unsigned long long key) {
    atomicAdd(&cnt[bin], n);
    if (key < first[bin]) atomicMin(&first[bin], key);
}

// What lane 7 of a block keeps of its blocks' EOBs.
struct Eob {
    uint32_t count;
    unsigned long long key;
};

// The symbols of one lane's eight entries (k = lane & 7: entries 8k .. 8k + 7 of block `blk` of its span); prev_dc: the DC of the block
// before (used by k == 0), 0 for the span's first block.  Every lane of the wave calls it (the DPP steps read neighbours); only `valid`
// lanes count.
__device__ __forceinline__ void lane_symbols(const uint4 v, int k, int prev_dc, bool valid, unsigned long long blk, uint32_t *cnt,
                                             unsigned long long *first, uint32_t &err, Eob &eob) {
    int c[8];
    c[0] = (int)(int16_t)(v.x & 0xffff); c[1] = (int)v.x >> 16; c[2] = (int)(int16_t)(v.y & 0xffff); c[3] = (int)v.y >> 16;
    c[4] = (int)(int16_t)(v.z & 0xffff); c[5] = (int)v.z >> 16; c[6] = (int)(int16_t)(v.w & 0xffff); c[7] = (int)v.w >> 16;
    // non-zero AC entries of the lane (the DC position is no AC entry), the zero run that ends with its last entry (tz) and whether it
    // holds nothing else (az)
    int nz_mask = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) nz_mask |= (c[j] != 0 && !(k == 0 && j == 0)) ? (1 << j) : 0;
    int az = nz_mask == 0;
    int tz = az ? (k == 0 ? 7 : 8) : (__clz(nz_mask) - 24);
    // carry-through scan over the 8 lanes of the block (a lane only uses lanes of its own block: k >= D)
#define TIC_CARRY_STEP(D)                                           \
    {                                                               \
        const int pa = dpp_row_shr<D>(az), pt = dpp_row_shr<D>(tz); \
        if (k >= D) {                                               \
            tz = az ? pt + tz : tz;                                 \
            az = az & pa;                                           \
        }                                                           \
    }
    TIC_CARRY_STEP(1)
    TIC_CARRY_STEP(2)
    TIC_CARRY_STEP(4)
#undef TIC_CARRY_STEP
    int run0 = dpp_row_shr<1>(tz); // the zero run in front of this lane's first entry (at most 55)
    if (k == 0) run0 = 0;          // the AC run starts behind the DC
    // symbols the lane emits, and those its block emits in the lanes below it
    int nsym = 0;
    {
        int r = run0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const bool nz = (nz_mask >> j) & 1;
            nsym += nz ? (r >> 4) + 1 : 0;
            r = nz ? 0 : r + 1;
            if (j == 0 && k == 0) r = 0;
        }
    }
    int incl = nsym;
#define TIC_PREFIX_STEP(D)                   \
    {                                        \
        const int p = dpp_row_shr<D>(incl);  \
        if (k >= D) incl += p;               \
    }
    TIC_PREFIX_STEP(1)
    TIC_PREFIX_STEP(2)
    TIC_PREFIX_STEP(4)
#undef TIC_PREFIX_STEP
    if (!valid) return;
    const unsigned long long kb = blk * 64ull;
    if (k == 0) { // the DC category: its key is the block
        const int sz = bit_len(c[0] - prev_dc);
        err |= sz > 15 ? 1u : 0u;
        hit(cnt, first, kAdaptDcBin + (sz & 15), 1u, blk);
    }
    if (k == 7) { // the EOB behind the block's last symbol
        eob.count++;
        const unsigned long long key = kb + (unsigned long long)incl;
        eob.key = key < eob.key ? key : eob.key;
    }
    int ord = incl - nsym, r = run0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if ((nz_mask >> j) & 1) {
            const int zrl = r >> 4;
            if (zrl) hit(cnt, first, 0xF0, (uint32_t)zrl, kb + (unsigned long long)ord);
            ord += zrl;
            const int sz = bit_len(c[j]);
            err |= sz > 15 ? 1u : 0u;
            hit(cnt, first, ((r & 15) << 4) | (sz & 15), 1u, kb + (unsigned long long)ord);
            ord++;
            r = 0;
        } else {
            r++;
        }
        if (j == 0 && k == 0) r = 0;
    }
}

__global__ __launch_bounds__(kWaves * 64) void adaptive_stats_probe_kernel_v(const int16_t *__restrict__ zz, const SizeProbeTable *__restrict__ pt,
                                                                             AdaptStats *__restrict__ stats) {
    __shared__ uint32_t s_count[kCopies * kCopyStride];
    __shared__ unsigned long long s_first[kAdaptBins];
    __shared__ uint32_t s_err;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, k = lane & 7;
    for (int i = tid; i < kCopies * kCopyStride; i += kWaves * 64) s_count[i] = 0u;
    for (int i = tid; i < kAdaptBins; i += kWaves * 64) s_first[i] = ~0ull;
    if (tid == 0) s_err = 0u;
    // the workgroup's probe (stream_size_kernel_v): one load per lane of the prefix table and a ballot; the record comes by scalar loads
    const uint32_t fg = pt->first_group[lane];
    const int probe = __builtin_amdgcn_readfirstlane(__popcll(__ballot(fg <= blockIdx.x)) - 1);
    const SizeProbeRec &rec = pt->rec[probe];
    const int16_t *fz = zz + rec.first_block * 64ull;
    const unsigned long long nblocks = rec.nblocks, nchunks = (rec.nblocks + 7ull) / 8ull;
    const unsigned long long first_chunk = (unsigned long long)(blockIdx.x - rec.first_group) * kWaves + (unsigned long long)wave;
    const unsigned long long nwaves = (unsigned long long)rec.ngroups * kWaves;
    AdaptStats *st = stats + rec.result;
    __syncthreads();

    uint32_t *cnt = s_count + k * kCopyStride;
    uint32_t err = 0u;
    Eob eob = {0u, ~0ull};
    for (unsigned long long base = first_chunk; base < nchunks; base += nwaves * kUnroll) {
        uint4 v[kUnroll];
        int p0[kUnroll];
        bool valid[kUnroll];
        unsigned long long blk[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) { // every load of the round, back to back
            const unsigned long long ch = base + (unsigned long long)u * nwaves;
            blk[u] = ch * 8ull + (unsigned long long)(lane >> 3);
            valid[u] = ch < nchunks && blk[u] < nblocks;
            v[u] = valid[u] ? *reinterpret_cast<const uint4 *>(fz + blk[u] * 64ull + (unsigned long long)(k * 8)) : make_uint4(0u, 0u, 0u, 0u);
            p0[u] = (lane == 0 && valid[u] && ch != 0ull) ? (int)fz[(ch * 8ull - 1ull) * 64ull] : 0; // DC of the block before the wave's first
        }
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            int prev = __shfl_up((int)(int16_t)(v[u].x & 0xffff), 8, 64); // DC of the block before: lane - 8 ...
            if (lane == 0) prev = p0[u];                                   // ... or the last block of the chunk before (probe start: 0)
            lane_symbols(v[u], k, prev, valid[u], blk[u], cnt, s_first, err, eob);
        }
    }
    if (eob.count) hit(cnt, s_first, 0, eob.count, eob.key);
    if (__any(err != 0u) && lane == 0) atomicOr(&s_err, 1u);
    __syncthreads();
    for (int i = tid; i < kAdaptBins; i += kWaves * 64) {
        uint32_t n = 0;
#pragma unroll
        for (int c = 0; c < kCopies; c++) n += s_count[c * kCopyStride + i];
        if (n) {
            atomicAdd(&st->count[i], (unsigned long long)n);
            atomicMin(&st->first[i], s_first[i]);
        }
    }
    if (tid == 0 && s_err) atomicOr(&st->err, 1u);
}

// Empty statistics for `count` entries: counts and error zero, first keys ~0.
__global__ __launch_bounds__(256) void adaptive_stats_probe_reset_kernel(AdaptStats *__restrict__ st) {
    AdaptStats *s = st + blockIdx.x;
    for (int i = (int)threadIdx.x; i < kAdaptBins; i += 256) {
        s->count[i] = 0ull;
        s->first[i] = ~0ull;
    }
    if (threadIdx.x == 0) s->err = 0u;
}

} // namespace

hipError_t adaptive_stats_probe_reset(AdaptStats *d_stats, int count, hipStream_t stream) {
    if (count < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(adaptive_stats_probe_reset_kernel, dim3((unsigned)count), dim3(256), 0, stream, d_stats);
    return hipGetLastError();
}

hipError_t adaptive_stats_probe_v(const int16_t *d_zz, const SizeProbeTable *d_probes, size_t ngroups, AdaptStats *d_stats, hipStream_t stream) {
    if (ngroups == 0 || ngroups > (size_t)kSizeMaxProbes * kSizeMaxGroups) return hipErrorInvalidValue;
    hipLaunchKernelGGL(adaptive_stats_probe_kernel_v, dim3((unsigned)ngroups), dim3(kWaves * 64), 0, stream, d_zz, d_probes, d_stats);
    return hipGetLastError();
}

} // namespace tic
