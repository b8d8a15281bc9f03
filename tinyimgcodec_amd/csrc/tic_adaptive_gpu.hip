// tic_adaptive_gpu.hip - device half of the per-image Huffman tables (compress(..., auto_generate_huffman_table=True), codec.py:133-164
// of the reference): symbol statistics of a frame, then packing with the frame's own codes (up to 64 bits per codeword).
//
// A thread owns a block: the workgroup's 256 blocks are loaded coalesced into LDS (rows of 33 words, so that the 64 lanes of a wave,
// each reading its own block, hit different banks) and every thread walks its block's symbols with block_symbols() - the one
// definition of DPCM, run lengths, ZRL and EOB (huffman.py:12-33) the three kernels share:
//   adaptive_stats_kernel   counts per symbol and first-occurrence keys into LDS (integer atomics), then one global atomicAdd /
//                           atomicMin per non-empty bin per workgroup: the result does not depend on the order of the workgroups.
//   adaptive_bits_kernel    bits per block with the frame's table, and their sum per workgroup;
//   adaptive_scan_kernel    one workgroup: exclusive prefix of the workgroup sums;
//   adaptive_write_kernel   the block's bit offset (a prefix inside the workgroup on top of the workgroup's), then its symbols as
//                           big-endian 32-bit words: words the block shares with a neighbour (its first and last) by atomicOr into
//                           the zeroed stream, the words between by plain stores.
// The table itself is built on the host between the statistics and the packing (tic_adaptive.cpp): one read-back of 4.4 KB.
//
// Every kernel is written once, as the work of ONE workgroup on ONE frame (stats_group, bits_group, scan_groups, write_group), and
// launched in two forms: for a single frame (the workgroup's index is its group), and in descriptor form for the frames of a chunk
// (adaptive_*_v_kernel: the workgroup finds its frame in an AdaptFrameTable, tic_adaptive_frames.h, and works on that frame's blocks,
// statistics, table, sums and stream area with frame-local indices - block 0 of every frame is raw, no read reaches a neighbour).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tic_adaptive.h"

namespace tic {
namespace {

constexpr int kThreads = 256; // blocks per workgroup
static_assert(kThreads == (int)kAdaptGroupBlocks, "the host plan counts workgroups of this many blocks");
constexpr int kRow = 33;      // LDS words per block (32 + 1 against bank conflicts)

__device__ __forceinline__ int bit_len(uint32_t a) { return a ? 32 - __clz((int)a) : 0; } // utils.py:9-10

__device__ __forceinline__ int coef(const uint32_t *row, int k) {
    const uint32_t w = row[k >> 1];
    return (int)(int16_t)((k & 1) ? (w >> 16) : (w & 0xffffu));
}

// The workgroup's blocks [b0, b0 + 256) of zz into LDS rows (blocks past n: zeros).
__device__ __forceinline__ void load_blocks(const int16_t *__restrict__ zz, unsigned long long n, unsigned long long b0, uint32_t *blk) {
    const uint4 *src = reinterpret_cast<const uint4 *>(zz);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int i = (int)threadIdx.x + kThreads * j; // uint4 i of the group: block i / 8, part i % 8
        const int bl = i >> 3, part = i & 7;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (b0 + (unsigned long long)bl < n) v = src[(b0 + (unsigned long long)bl) * 8ull + (unsigned long long)part];
        uint32_t *d = blk + bl * kRow + part * 4;
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
    }
}

// DPCM of the block's DC (codec.py:34-35: the first block raw, the others minus the previous block's DC).
__device__ __forceinline__ int dc_diff(const int16_t *__restrict__ zz, const uint32_t *blk, unsigned long long b) {
    const int t = (int)threadIdx.x;
    const int dc = coef(blk + t * kRow, 0);
    if (b == 0) return dc;
    const int prev = t ? coef(blk + (t - 1) * kRow, 0) : (int)zz[(b - 1) * 64ull];
    return dc - prev;
}

// The symbols of one block in stream order (huffman.py:12-33 and :41-63): fn(bin, value bits, size, ordinal) for the DC category
// (bin kAdaptDcBin + category), every AC (run, size) symbol with ZRL = (15, 0) per 16 zeros, and EOB = (0, 0); the ordinal counts
// the block's run-length list (the DC has ordinal 0 of its own list).  Returns false when a DC category or an AC size exceeds 15:
// write_huffman_table has 4 bits for them (codec.py:73-84).
template <typename F>
__device__ __forceinline__ bool block_symbols(const uint32_t *row, int diff, F &&fn) {
    bool ok = true;
    {
        const uint32_t a = (uint32_t)(diff < 0 ? -diff : diff);
        const int sz = bit_len(a);
        ok = sz <= 15;
        fn(kAdaptDcBin + (sz & 15), (uint32_t)(diff + (diff >> 31)) & ((1u << sz) - 1u), sz, 0);
    }
    int last = 63;
    while (last > 0 && coef(row, last) == 0) last--; // trailing zeros: no symbols (huffman.py:16-17)
    int run = 0, ord = 0;
    for (int k = 1; k <= last; k++) {
        const int v = coef(row, k);
        if (v == 0) {
            run++;
            continue;
        }
        while (run >= 16) { // ZRL (huffman.py:24-28)
            fn(0xF0, 0u, 0, ord++);
            run -= 16;
        }
        const uint32_t a = (uint32_t)(v < 0 ? -v : v);
        const int sz = bit_len(a);
        ok = ok && sz <= 15;
        fn((run << 4) | (sz & 15), (uint32_t)(v + (v >> 31)) & ((1u << sz) - 1u), sz, ord++);
        run = 0;
    }
    fn(0, 0u, 0, ord); // EOB (huffman.py:33)
    return ok;
}

// Workgroup g of a frame of n blocks at zz: its statistics into st.
__device__ __forceinline__ void stats_group(const int16_t *__restrict__ zz, unsigned long long n, unsigned long long g, AdaptStats *__restrict__ st) {
    __shared__ uint32_t blk[kThreads * kRow];
    __shared__ uint32_t s_count[kAdaptBins];
    __shared__ unsigned long long s_first[kAdaptBins];
    __shared__ uint32_t s_err;
    const int t = (int)threadIdx.x;
    for (int i = t; i < kAdaptBins; i += kThreads) {
        s_count[i] = 0u;
        s_first[i] = ~0ull;
    }
    if (t == 0) s_err = 0u;
    const unsigned long long b0 = g * kThreads, b = b0 + (unsigned long long)t;
    load_blocks(zz, n, b0, blk);
    __syncthreads();
    if (b < n) {
        const bool ok = block_symbols(blk + t * kRow, dc_diff(zz, blk, b), [&](int bin, uint32_t, int, int ord) {
            atomicAdd(&s_count[bin], 1u);
            const unsigned long long key = bin >= kAdaptDcBin ? b : b * 64ull + (unsigned long long)ord;
            if (key < s_first[bin]) atomicMin(&s_first[bin], key);
        });
        if (!ok) atomicOr(&s_err, 1u);
    }
    __syncthreads();
    for (int i = t; i < kAdaptBins; i += kThreads)
        if (s_count[i]) {
            atomicAdd(&st->count[i], (unsigned long long)s_count[i]);
            atomicMin(&st->first[i], s_first[i]);
        }
    if (t == 0 && s_err) atomicOr(&st->err, 1u);
}
__global__ __launch_bounds__(kThreads) void adaptive_stats_kernel(const int16_t *__restrict__ zz, unsigned long long n,
                                                                  AdaptStats *__restrict__ st) {
    stats_group(zz, n, blockIdx.x, st);
}

// Workgroup g of a frame: bits per block into bbits (the frame's), their sum into *gsum (the workgroup's).
__device__ __forceinline__ void bits_group(const int16_t *__restrict__ zz, unsigned long long n, unsigned long long g,
                                           const HuffWide *__restrict__ tab, uint32_t *__restrict__ bbits, unsigned long long *__restrict__ gsum) {
    __shared__ uint32_t blk[kThreads * kRow];
    __shared__ uint32_t s_len[kAdaptBins];
    __shared__ unsigned long long s_sum[kThreads / 64];
    const int t = (int)threadIdx.x;
    for (int i = t; i < kAdaptBins; i += kThreads) s_len[i] = tab->len[i];
    const unsigned long long b0 = g * kThreads, b = b0 + (unsigned long long)t;
    load_blocks(zz, n, b0, blk);
    __syncthreads();
    uint32_t bits = 0;
    if (b < n) {
        (void)block_symbols(blk + t * kRow, dc_diff(zz, blk, b), [&](int bin, uint32_t, int size, int) { bits += s_len[bin] + (uint32_t)size; });
        bbits[b] = bits;
    }
    unsigned long long s = bits;
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((t & 63) == 0) s_sum[t >> 6] = s;
    __syncthreads();
    if (t == 0) {
        unsigned long long sum = 0;
        for (int i = 0; i < kThreads / 64; i++) sum += s_sum[i];
        *gsum = sum;
    }
}
__global__ __launch_bounds__(kThreads) void adaptive_bits_kernel(const int16_t *__restrict__ zz, unsigned long long n,
                                                                 const HuffWide *__restrict__ tab, uint32_t *__restrict__ bbits,
                                                                 unsigned long long *__restrict__ gsum) {
    bits_group(zz, n, blockIdx.x, tab, bbits, gsum + blockIdx.x);
}

// Exclusive prefix of gsum[0, groups) in place, one workgroup.
__device__ __forceinline__ void scan_groups(unsigned long long *__restrict__ gsum, unsigned long long groups) {
    __shared__ unsigned long long s[1024];
    __shared__ unsigned long long carry;
    const int t = (int)threadIdx.x;
    if (t == 0) carry = 0ull;
    __syncthreads();
    for (unsigned long long base = 0; base < groups; base += 1024) {
        const unsigned long long i = base + (unsigned long long)t;
        const unsigned long long v = i < groups ? gsum[i] : 0ull;
        s[t] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const unsigned long long x = t >= off ? s[t - off] : 0ull;
            __syncthreads();
            s[t] += x;
            __syncthreads();
        }
        const unsigned long long c = carry;
        if (i < groups) gsum[i] = c + s[t] - v;
        __syncthreads();
        if (t == 1023) carry = c + s[1023];
        __syncthreads();
    }
}
__global__ __launch_bounds__(1024) void adaptive_scan_kernel(unsigned long long *__restrict__ gsum, unsigned long long groups) {
    scan_groups(gsum, groups);
}

// MSB-first bits into big-endian 32-bit words from bit `pos` of the stream on.  The first word (shared with what lies before) and the
// last, partial one (shared with what follows) are ORed in atomically; a word is never written at or past `nwords`.
struct WordWriter {
    uint32_t *out;
    unsigned long long wi, nwords;
    unsigned long long acc; // pending bits, left-aligned
    uint32_t nacc;
    bool first;
    uint32_t *err;
    __device__ __forceinline__ void store(uint32_t word, bool shared) {
        if (wi >= nwords) {
            atomicOr(err, 1u);
        } else if (shared) {
            atomicOr(out + wi, __builtin_bswap32(word));
        } else {
            out[wi] = __builtin_bswap32(word);
        }
    }
    __device__ __forceinline__ void put32(uint32_t v, uint32_t n) { // n <= 32, v < 2^n
        if (n == 0) return;
        acc |= ((unsigned long long)v) << (64u - nacc - n);
        nacc += n;
        if (nacc >= 32u) {
            store((uint32_t)(acc >> 32), first);
            first = false;
            wi++;
            acc <<= 32;
            nacc -= 32u;
        }
    }
    __device__ __forceinline__ void put(unsigned long long v, uint32_t n) { // n <= 64
        if (n > 32u) {
            put32((uint32_t)(v >> 32), n - 32u);
            put32((uint32_t)v, 32u);
        } else {
            put32((uint32_t)v, n);
        }
    }
    __device__ __forceinline__ void finish() {
        if (nacc) store((uint32_t)(acc >> 32), true);
    }
};

// Workgroup g of a frame: its blocks' symbols into the frame's stream `out` behind base_bits + goff (the workgroup's offset) bits.
__device__ __forceinline__ void write_group(const int16_t *__restrict__ zz, unsigned long long n, unsigned long long g,
                                            const HuffWide *__restrict__ tab, const uint32_t *__restrict__ bbits, unsigned long long goff,
                                            uint32_t *__restrict__ out, unsigned long long base_bits, unsigned long long out_words,
                                            uint32_t *__restrict__ err) {
    __shared__ uint32_t blk[kThreads * kRow];
    __shared__ unsigned long long s_code[kAdaptBins];
    __shared__ uint32_t s_len[kAdaptBins];
    __shared__ unsigned long long s_scan[kThreads];
    const int t = (int)threadIdx.x;
    for (int i = t; i < kAdaptBins; i += kThreads) {
        s_code[i] = tab->code[i];
        s_len[i] = tab->len[i];
    }
    const unsigned long long b0 = g * kThreads, b = b0 + (unsigned long long)t;
    load_blocks(zz, n, b0, blk);
    const uint32_t mine = b < n ? bbits[b] : 0u;
    s_scan[t] = mine;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        const unsigned long long x = t >= off ? s_scan[t - off] : 0ull;
        __syncthreads();
        s_scan[t] += x;
        __syncthreads();
    }
    if (b >= n || mine == 0u) return;
    const unsigned long long pos = base_bits + goff + s_scan[t] - mine;
    WordWriter wr{out, pos >> 5, out_words, 0ull, (uint32_t)(pos & 31ull), true, err};
    (void)block_symbols(blk + t * kRow, dc_diff(zz, blk, b), [&](int bin, uint32_t value, int size, int) {
        wr.put(s_code[bin], s_len[bin]);
        wr.put32(value, (uint32_t)size);
    });
    wr.finish();
}
__global__ __launch_bounds__(kThreads) void adaptive_write_kernel(const int16_t *__restrict__ zz, unsigned long long n,
                                                                  const HuffWide *__restrict__ tab, const uint32_t *__restrict__ bbits,
                                                                  const unsigned long long *__restrict__ goff, uint32_t *__restrict__ out,
                                                                  unsigned long long base_bits, unsigned long long out_words,
                                                                  uint32_t *__restrict__ err) {
    write_group(zz, n, blockIdx.x, tab, bbits, goff[blockIdx.x], out, base_bits, out_words, err);
}

// ---- descriptor form: the frames of a chunk in one launch per kernel ---------------------------------------------------------------------
// The frame of workgroup `idx`: the last one whose first workgroup is not behind idx (find_frame of tic_entropy_gpu.hip: one load per lane
// of the 64-entry prefix table, 0xffffffff behind the last frame, and a ballot; the result is wave-uniform).  The kernels call it first,
// with whole waves.
__device__ __forceinline__ int find_frame(const uint32_t *__restrict__ first, uint32_t idx) {
    const uint32_t v = first[threadIdx.x & 63];
    return __builtin_amdgcn_readfirstlane(__popcll(__ballot(v <= idx)) - 1);
}

// The chunk's statistics start empty: counts left by the slot's previous chunk would be added to.
__global__ __launch_bounds__(kThreads) void adaptive_stats_reset_kernel(AdaptStats *__restrict__ st) {
    AdaptStats *s = st + blockIdx.x;
    for (int i = (int)threadIdx.x; i < kAdaptBins; i += kThreads) {
        s->count[i] = 0ull;
        s->first[i] = ~0ull;
    }
    if (threadIdx.x == 0) s->err = 0u;
}

__global__ __launch_bounds__(kThreads) void adaptive_stats_v_kernel(const int16_t *__restrict__ zz, const AdaptFrameTable *__restrict__ ft,
                                                                    AdaptStats *__restrict__ st) {
    const int f = find_frame(ft->first_group, blockIdx.x);
    const AdaptFrameRec &r = ft->rec[f];
    stats_group(zz + r.first_block * 64ull, r.nblocks, blockIdx.x - r.first_group, st + f);
}

__global__ __launch_bounds__(kThreads) void adaptive_bits_v_kernel(const int16_t *__restrict__ zz, const AdaptFrameTable *__restrict__ ft,
                                                                   const HuffWide *__restrict__ tabs, uint32_t *__restrict__ bbits,
                                                                   unsigned long long *__restrict__ gsum) {
    const int f = find_frame(ft->first_group, blockIdx.x);
    const AdaptFrameRec &r = ft->rec[f];
    if (r.skip) return;
    bits_group(zz + r.first_block * 64ull, r.nblocks, blockIdx.x - r.first_group, tabs + f, bbits + r.first_block, gsum + blockIdx.x);
}

// One workgroup per frame: the frame's header and table into its (zeroed) area - whole words up to base_bits; the blocks around that bit
// OR theirs in behind this launch - and the exclusive prefix of the frame's own workgroup sums.
__global__ __launch_bounds__(1024) void adaptive_scan_v_kernel(const AdaptFrameTable *__restrict__ ft, const uint8_t *__restrict__ heads,
                                                               unsigned long long *__restrict__ gsum, unsigned char *__restrict__ streams) {
    const AdaptFrameRec &r = ft->rec[blockIdx.x];
    if (r.skip) return;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(heads + (size_t)blockIdx.x * kAdaptHeadStride);
    uint32_t *dst = reinterpret_cast<uint32_t *>(streams + r.out_off);
    const unsigned long long head_words = ((unsigned long long)r.base_bits + 31ull) / 32ull;
    for (unsigned long long i = threadIdx.x; i < head_words && i < r.out_words; i += 1024) dst[i] = src[i];
    scan_groups(gsum + r.first_group, r.ngroups);
}

__global__ __launch_bounds__(kThreads) void adaptive_write_v_kernel(const int16_t *__restrict__ zz, const AdaptFrameTable *__restrict__ ft,
                                                                    const HuffWide *__restrict__ tabs, const uint32_t *__restrict__ bbits,
                                                                    const unsigned long long *__restrict__ goff, unsigned char *__restrict__ streams,
                                                                    uint32_t *__restrict__ err) {
    const int f = find_frame(ft->first_group, blockIdx.x);
    const AdaptFrameRec &r = ft->rec[f];
    if (r.skip) return;
    write_group(zz + r.first_block * 64ull, r.nblocks, blockIdx.x - r.first_group, tabs + f, bbits + r.first_block, goff[blockIdx.x],
                reinterpret_cast<uint32_t *>(streams + r.out_off), r.base_bits, r.out_words, err);
}

inline unsigned long long groups_of(size_t n) { return (n + kThreads - 1) / kThreads; }
inline size_t bbits_bytes(size_t n) { return (n * 4 + 255) / 256 * 256; }

} // namespace

size_t adaptive_work_bytes(size_t nblocks) { return bbits_bytes(nblocks) + groups_of(nblocks) * 8; }

hipError_t adaptive_stats(const int16_t *d_zz, size_t nblocks, AdaptStats *d_stats, hipStream_t stream) {
    if (nblocks == 0) return hipSuccess;
    adaptive_stats_kernel<<<dim3((unsigned)groups_of(nblocks)), dim3(kThreads), 0, stream>>>(d_zz, nblocks, d_stats);
    return hipGetLastError();
}

hipError_t adaptive_pack(const int16_t *d_zz, size_t nblocks, const HuffWide *d_tab, void *d_work, uint32_t *d_out,
                         unsigned long long base_bits, unsigned long long out_words, unsigned int *d_err, hipStream_t stream) {
    if (nblocks == 0) return hipSuccess;
    const unsigned long long groups = groups_of(nblocks);
    uint32_t *bbits = (uint32_t *)d_work;
    unsigned long long *gsum = (unsigned long long *)((char *)d_work + bbits_bytes(nblocks));
    adaptive_bits_kernel<<<dim3((unsigned)groups), dim3(kThreads), 0, stream>>>(d_zz, nblocks, d_tab, bbits, gsum);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    adaptive_scan_kernel<<<dim3(1), dim3(1024), 0, stream>>>(gsum, groups);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    adaptive_write_kernel<<<dim3((unsigned)groups), dim3(kThreads), 0, stream>>>(d_zz, nblocks, d_tab, bbits, gsum, d_out, base_bits,
                                                                                   out_words, d_err);
    return hipGetLastError();
}

hipError_t adaptive_stats_v(const int16_t *d_zz, const AdaptFrameTable *d_frames, int count, size_t ngroups, AdaptStats *d_stats,
                            hipStream_t stream) {
    if (count < 1 || count > kEntropyMaxFrames || ngroups == 0 || ngroups > 0x7fffffffu) return hipErrorInvalidValue;
    adaptive_stats_reset_kernel<<<dim3((unsigned)count), dim3(kThreads), 0, stream>>>(d_stats);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    adaptive_stats_v_kernel<<<dim3((unsigned)ngroups), dim3(kThreads), 0, stream>>>(d_zz, d_frames, d_stats);
    return hipGetLastError();
}

hipError_t adaptive_pack_v(const int16_t *d_zz, const AdaptFrameTable *d_frames, int count, size_t ngroups, const HuffWide *d_tabs,
                           const uint8_t *d_heads, uint32_t *d_bbits, unsigned long long *d_gsum, void *d_streams, unsigned int *d_err,
                           hipStream_t stream) {
    if (count < 1 || count > kEntropyMaxFrames || ngroups == 0 || ngroups > 0x7fffffffu) return hipErrorInvalidValue;
    adaptive_bits_v_kernel<<<dim3((unsigned)ngroups), dim3(kThreads), 0, stream>>>(d_zz, d_frames, d_tabs, d_bbits, d_gsum);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    adaptive_scan_v_kernel<<<dim3((unsigned)count), dim3(1024), 0, stream>>>(d_frames, d_heads, d_gsum, (unsigned char *)d_streams);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    adaptive_write_v_kernel<<<dim3((unsigned)ngroups), dim3(kThreads), 0, stream>>>(d_zz, d_frames, d_tabs, d_bbits, d_gsum,
                                                                                     (unsigned char *)d_streams, d_err);
    return hipGetLastError();
}

} // namespace tic
