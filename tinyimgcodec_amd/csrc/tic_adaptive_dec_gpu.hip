// tic_adaptive_dec_gpu.hip - Huffman + run-length decode of a stream with an embedded (per-image) table on the GPU: the device twin
// of adaptive_decode (tic_adaptive.cpp; decode_huffman huffman.py:77-98, decode_run_length huffman.py:36-38, np.cumsum of the DC
// differences codec.py:53).  The method is that of tic_entropy_dec_gpu.hip (read its header comment) in its plainest form, with
// tables that come from the stream instead of the default ones:
//   measure and stitch   a lane per RANGE of payload bits.  Launch 0: every lane walks the symbols from its range's first bit as if a
//             block started there, one symbol per look-up in a 64-bit window, and leaves where its walk left the range (its EXIT: the
//             first block start at or behind the range's end).  Then lane t takes lane t-1's exit as its ENTRY and, if that is not
//             the bit it walked from last, walks again - inside the launch through LDS among the 256 lanes of a workgroup, until
//             no exit of the workgroup moves; across workgroups from launch to launch.  Range 0 starts on a true block start; a
//             Huffman walk falls in step with the true chain within a block or two, so nearly every exit of the first walks already
//             is the true chain's, the second walks are the true chain, and a launch that moves no exit proves it: entries are then
//             true by induction over t.  No traces are kept (a block start carries no state: a walk from a true entry IS the true
//             chain), so none can overflow, and a block longer than a range - up to 30 + 63 x 64 = 4,062 bits - is no special case:
//             the chain passes over the range, whose lane counts no block.  Where walks do NOT fall in step (runs of one repeated
//             symbol, as in the long-code fixture: a walk out of step stays out of step) the true chain advances a workgroup
//             per launch.  A chain that has not settled after kAdaptDecMaxRounds launches is "no synchronisation point": give up.
//   block positions   exclusive sum of the ranges' block counts (one workgroup; a range count per 2 average blocks), then every lane
//             walks its range once more from its true entry and writes the first bit of each of its blocks.
//   decode    a lane per block zeroes its row of the int16 [N][64] array and writes its coefficients (zig-zag order) and its DC
//             difference; one workgroup sums the differences into the rows (np.cumsum).
// Every walk is bounded: a symbol advances at least one bit, a walk that meets a window without a code goes on one bit further, one
// that meets a block of more than 63 AC entries starts a block behind it, and a walk ends at its range's or the stream's end.
// Anything unusual ON THE CHAIN before block N - such an incident, the stream's end, a running DC outside int16 - sets a give-up bit:
// the caller then runs the host decoder, which alone words errors.  Bits behind block N are ignored, as on the host.
// Stream words are read from memory (L2-resident: 64 lanes a range apart), the tables from LDS.
//
// DESCRIPTOR FORM (adaptive_decode_gpu_batch, the kernels named *_v): the same five kernels for the frames of a chunk
// (tic_adaptive_decode_plan.h), one launch each.  Every workgroup looks its frame up in an uploaded table (a workgroup of the range and
// block grids) or is its frame's own (the two sums: grid = frames), reads the frame's descriptor and stages THAT frame's tables in LDS.
// Nothing crosses a frame: a workgroup's 256 lanes are consecutive ranges (or blocks) of one frame, the first lane of a frame's first
// workgroup starts at the frame's payload_bit, the DC sum starts over with every frame, and a frame's Stream is its own words, word
// count and last-word mask inside the chunk's stream buffer - window() never reads another frame's bytes, nor the padding between them.
// Exits, walked-from bits, counts and incidents lie in chunk-wide arrays at the frame's range0, block positions, DC differences and
// coefficients at its blk0.  Status is per frame (give-up bits, blocks on the chain, exits moved per round) plus ONE count per round
// for the chunk, so that the host reads one word to know whether every frame has settled.
// ROUNDS PROTOCOL of a chunk (decided here and in tic_api.hip adbatch_decode, nowhere else):
//   1. rounds 0..2, the passes and the inverse transform are launched at once; one status read-back, one synchronisation - the single
//      call's optimistic path;
//   2. if round 2 moved an exit anywhere in the chunk, rounds 3..18 are launched and nothing else (a workgroup of a frame whose last
//      round moved none of its exits leaves at once: a fixed point stays one);
//   3. a frame round 18 still moved is marked kAdaptGiveupNoSync by the caller - its single call has all kAdaptDecMaxRounds rounds;
//   4. the passes and the inverse transform run once more for the whole chunk: settled frames get the same result again, the frames that
//      settled in rounds 3..18 their first true one.
// So one pathological frame (the long-code fixture: its chain advances a workgroup per launch) holds a chunk for 16 launches, not 512.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "tic_adaptive.h"

namespace tic {
static_assert(sizeof(AdaptDecTab) == kAdaptDecTabBytes && kAdaptDecTabSlot >= kAdaptDecTabBytes && kAdaptDecTabSlot % 256 == 0, "the plan's table slot");
namespace {

constexpr int kThreads = 256, kScanThreads = 1024;
constexpr uint32_t kNone = 0xffffffffu;

struct Stream {
    const uint32_t *words;
    uint32_t nwords, last_mask; // big-endian mask of the last word: the bytes behind the stream's end read as zero
    uint32_t total_bits;
};

__device__ __forceinline__ uint32_t word_be(const Stream &s, uint32_t wi) {
    if (wi >= s.nwords) return 0u;
    const uint32_t v = __builtin_bswap32(s.words[wi]);
    return wi == s.nwords - 1u ? (v & s.last_mask) : v;
}
// the 64 stream bits from bit p on (zeros behind the end)
__device__ __forceinline__ unsigned long long window(const Stream &s, uint32_t p) {
    const uint32_t wi = p >> 5, sh = p & 31u;
    const unsigned long long v = ((unsigned long long)word_be(s, wi) << 32) | word_be(s, wi + 1u);
    return sh ? (v << sh) | (word_be(s, wi + 2u) >> (32u - sh)) : v;
}

// (length << 8) | symbol of the code the window starts with; 0: none
__device__ __forceinline__ uint32_t lookup(const AdaptDecTab &tab, int k, unsigned long long win) {
    const uint32_t e = tab.prim[k][win >> (64 - kAdaptDecK)];
    if (e) return e;
    uint32_t lo = 0, hi = tab.nlong[k]; // the last long code <= win
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab.long_code[k][mid] <= win) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) return 0;
    const uint32_t ls = tab.long_ls[k][lo - 1];
    const uint32_t len = ls >> 8;
    return ((tab.long_code[k][lo - 1] ^ win) >> (64u - len)) == 0 ? ls : 0u;
}

// BitBuffer.read_int (bitbuffer.py:56-66) of the `size` bits behind a code of `len` bits: one's complement for negatives
__device__ __forceinline__ int value_of(unsigned long long win, uint32_t len, uint32_t size) {
    if (size == 0) return 0;
    const unsigned long long bits = (win << len) >> (64u - size); // (len + size <= 64 and size >= 1: len <= 63)
    if ((bits >> (size - 1u)) & 1ull) return (int)bits;
    return -(int)((~bits) & ((1ull << size) - 1ull));
}

enum { kBlockOk = 0, kBlockIncident = 1, kBlockEnd = 2 };
// One block from bit p as adaptive_decode reads it.  kBlockOk: *next = the bit behind its EOB.  kBlockIncident: a window without a code
// (*next = one bit behind it) or more than 63 AC entries (*next = behind the entry that did not fit).  kBlockEnd: a symbol reaches
// past the stream's end.  row (may be null): the block's 64 coefficients, already zero, receive the AC entries; *dc its DC difference.
__device__ __forceinline__ int walk_block(const AdaptDecTab &tab, const Stream &s, uint32_t p, uint32_t *next, int16_t *row, int *dc) {
    unsigned long long win = window(s, p);
    uint32_t e = lookup(tab, 0, win);
    if (!e) {
        *next = p + 1u;
        return p + 1u > s.total_bits ? kBlockEnd : kBlockIncident;
    }
    uint32_t len = e >> 8, size = e & 255u;
    if (p + len + size > s.total_bits) return kBlockEnd;
    if (dc) *dc = value_of(win, len, size);
    p += len + size;
    for (uint32_t pos = 1;;) {
        win = window(s, p);
        e = lookup(tab, 1, win);
        if (!e) {
            *next = p + 1u;
            return p + 1u > s.total_bits ? kBlockEnd : kBlockIncident;
        }
        len = e >> 8;
        const uint32_t sym = e & 255u;
        size = sym & 15u;
        if (p + len + size > s.total_bits) return kBlockEnd;
        p += len + size;
        if (sym == 0) break; // EOB (huffman.py:92-94)
        pos += sym >> 4;
        if (pos > 63u) {
            *next = p;
            return kBlockIncident;
        }
        if (row) row[pos] = (int16_t)value_of(win, len, size);
        pos++;
    }
    *next = p;
    return kBlockOk;
}

// The chain from bit `entry` through a range that ends at `limit`: blocks that start in front of `limit`, the exit, and how many
// blocks were whole before the first incident (kNone: no incident).  pos_out (may be null): the first bit of block i at pos_out[i],
// i < pos_cap.
__device__ __forceinline__ uint32_t walk_range(const AdaptDecTab &tab, const Stream &s, uint32_t entry, uint32_t limit, uint32_t *exit_bit, uint32_t *bad_at,
                                               uint32_t *pos_out, uint32_t pos_cap) {
    uint32_t p = entry, cnt = 0, bad = kNone;
    while (p < limit) {
        uint32_t next = p;
        const int r = walk_block(tab, s, p, &next, nullptr, nullptr);
        if (r == kBlockEnd) {
            if (bad == kNone) bad = cnt;
            p = s.total_bits;
            break;
        }
        if (r == kBlockIncident) {
            if (bad == kNone) bad = cnt;
        } else {
            if (pos_out && cnt < pos_cap) pos_out[cnt] = p;
            cnt++;
        }
        p = next;
    }
    *exit_bit = p;
    *bad_at = bad;
    return cnt;
}

__device__ __forceinline__ void stage_tab(AdaptDecTab *lds, const AdaptDecTab *__restrict__ g) {
    static_assert(sizeof(AdaptDecTab) % 8 == 0, "copied as 64-bit words");
    const unsigned long long *src = (const unsigned long long *)g;
    unsigned long long *dst = (unsigned long long *)lds;
    for (uint32_t i = threadIdx.x; i < sizeof(AdaptDecTab) / 8; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

// Work buffer: five words per range, then a word and an int per block.
struct Work {
    uint32_t *exit_bit[2]; // by round parity: round r reads [r & 1 ^ 1], writes [r & 1]
    uint32_t *from, *count, *bad_at, *first;
    uint32_t *pos;
    int *dcdiff;
};
__host__ __device__ inline Work carve(void *work, size_t nranges, size_t nblocks) {
    Work w;
    uint32_t *p = (uint32_t *)work;
    w.exit_bit[0] = p, p += nranges;
    w.exit_bit[1] = p, p += nranges;
    w.from = p, p += nranges;
    w.count = p, p += nranges;
    w.bad_at = p, p += nranges;
    w.first = p, p += nranges;
    w.pos = p, p += nblocks;
    w.dcdiff = (int *)p;
    return w;
}

struct Geo {
    Stream s;
    uint32_t base, range, nranges, nblocks;
};
__device__ __forceinline__ uint32_t range_limit(const Geo &g, uint32_t t) {
    return t + 1u == g.nranges ? g.s.total_bits : g.base + (t + 1u) * g.range;
}

// One launch of the stitch.  A workgroup's 256 lanes own consecutive ranges: inside the launch they hand their exits on through LDS
// and walk again until no exit of the workgroup moves (at most 256 times: the stretch in which no walk falls in step), so that a
// launch carries the true chain across a whole workgroup at least; the workgroup's first lane takes its entry from the launch before.
__global__ void __launch_bounds__(kThreads) adapt_dec_round(Geo g, const AdaptDecTab *__restrict__ d_tab, void *work, AdaptDecStatus *st, int round) {
    __shared__ AdaptDecTab tab;
    __shared__ uint32_t ex[kThreads];
    __shared__ uint32_t moved;
    stage_tab(&tab, d_tab);
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    const bool valid = t < g.nranges;
    const Work w = carve(work, g.nranges, g.nblocks);
    const uint32_t *in = w.exit_bit[(round & 1) ^ 1];
    uint32_t *out = w.exit_bit[round & 1];
    uint32_t from = kNone, x = 0, cnt = 0, bad = kNone, entry = 0; // (kNone is no bit of a stream)
    bool walked = false;
    if (valid) {
        entry = (round == 0 || t == 0) ? g.base + t * g.range : in[t - 1u];
        if (round != 0) from = w.from[t], x = in[t];
    }
    const uint32_t x0 = x;
    for (int it = 0; it <= kThreads; it++) {
        bool m = false;
        if (valid && entry != from) { // (else: walked from here already)
            uint32_t nx;
            cnt = walk_range(tab, g.s, entry, range_limit(g, t), &nx, &bad, nullptr, 0);
            m = !walked && round == 0 ? true : nx != x;
            from = entry, x = nx, walked = true;
        }
        ex[threadIdx.x] = x;
        if (threadIdx.x == 0) moved = 0u;
        __syncthreads();
        if (m) moved = 1u;
        __syncthreads();
        const bool again = moved != 0u;
        if (valid && threadIdx.x > 0) entry = ex[threadIdx.x - 1u];
        __syncthreads();
        if (!again) break;
    }
    if (!valid) return;
    if (walked) w.from[t] = from, w.count[t] = cnt, w.bad_at[t] = bad;
    out[t] = x;
    if (round == 0)
        st->changed[0] = 1u;
    else if (x != x0)
        atomicAdd(&st->changed[round], 1u); // (few: the walks of round 0 fall in step within their range nearly everywhere)
}

// inclusive sum over the workgroup's kScanThreads values; every thread receives the sum up to and including its own
template <typename T> __device__ __forceinline__ T block_scan(T v, T *lds) {
    for (uint32_t d = 1; d < kScanThreads; d <<= 1) {
        lds[threadIdx.x] = v;
        __syncthreads();
        if (threadIdx.x >= d) v += lds[threadIdx.x - d];
        __syncthreads();
    }
    return v;
}

// first[t] = blocks in front of range t; the chain's incidents and its length against N
__global__ void __launch_bounds__(kScanThreads) adapt_dec_scan(Geo g, void *work, AdaptDecStatus *st) {
    __shared__ uint32_t lds[kScanThreads];
    const Work w = carve(work, g.nranges, g.nblocks);
    const uint32_t per = (g.nranges + kScanThreads - 1u) / kScanThreads;
    const uint32_t t0 = min(threadIdx.x * per, g.nranges), t1 = min(t0 + per, g.nranges);
    uint32_t sum = 0;
    for (uint32_t t = t0; t < t1; t++) sum += w.count[t];
    const uint32_t incl = block_scan(sum, lds);
    uint32_t run = incl - sum;
    bool incident = false;
    for (uint32_t t = t0; t < t1; t++) {
        w.first[t] = run;
        const uint32_t bad = w.bad_at[t];
        if (bad != kNone && (unsigned long long)run + bad < g.nblocks) incident = true;
        run += w.count[t];
    }
    if (incident) atomicOr(&st->giveup, kAdaptGiveupIncident);
    if (threadIdx.x == kScanThreads - 1u) {
        st->blocks = incl;
        if (incl < g.nblocks) atomicOr(&st->giveup, kAdaptGiveupShort);
    }
}

__global__ void __launch_bounds__(kThreads) adapt_dec_positions(Geo g, const AdaptDecTab *__restrict__ d_tab, void *work) {
    __shared__ AdaptDecTab tab;
    stage_tab(&tab, d_tab);
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= g.nranges) return;
    const Work w = carve(work, g.nranges, g.nblocks);
    const uint32_t first = w.first[t];
    if (first >= g.nblocks || w.count[t] == 0) return;
    uint32_t x, bad;
    (void)walk_range(tab, g.s, w.from[t], range_limit(g, t), &x, &bad, w.pos + first, g.nblocks - first);
}

__global__ void __launch_bounds__(kThreads) adapt_dec_blocks(Geo g, const AdaptDecTab *__restrict__ d_tab, void *work, const AdaptDecStatus *st, int16_t *zz) {
    __shared__ AdaptDecTab tab;
    stage_tab(&tab, d_tab);
    const uint32_t b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= g.nblocks) return;
    const Work w = carve(work, g.nranges, g.nblocks);
    int16_t *row = zz + (size_t)b * 64;
    uint4 *row4 = (uint4 *)row;
#pragma unroll
    for (int i = 0; i < 8; i++) row4[i] = make_uint4(0, 0, 0, 0);
    int dc = 0;
    // (a chain that ends before block N has given up already, and so has one the rounds have not settled: whatever such a run leaves
    //  in pos[] is walked within the stream's bounds and written within the row's)
    const uint32_t p = b < st->blocks ? w.pos[b] : g.s.total_bits;
    if (p < g.s.total_bits) {
        uint32_t next;
        (void)walk_block(tab, g.s, p, &next, row, &dc); // (on a settled chain without incident: kBlockOk by the walks before)
    }
    w.dcdiff[b] = dc;
}

// np.cumsum of the DC differences into the rows; a running DC outside int16 gives up
__global__ void __launch_bounds__(kScanThreads) adapt_dec_dc(Geo g, void *work, AdaptDecStatus *st, int16_t *zz) {
    __shared__ long long lds[kScanThreads];
    const Work w = carve(work, g.nranges, g.nblocks);
    const uint32_t per = (g.nblocks + kScanThreads - 1u) / kScanThreads;
    const uint32_t b0 = min(threadIdx.x * per, g.nblocks), b1 = min(b0 + per, g.nblocks);
    long long sum = 0;
    for (uint32_t b = b0; b < b1; b++) sum += w.dcdiff[b];
    long long run = block_scan(sum, lds) - sum;
    bool out_of_range = false;
    for (uint32_t b = b0; b < b1; b++) {
        run += w.dcdiff[b];
        if (run < -32768 || run > 32767) out_of_range = true;
        zz[(size_t)b * 64] = (int16_t)run;
    }
    if (out_of_range) atomicOr(&st->giveup, kAdaptGiveupDc);
}


// ---- descriptor form: the frames of a chunk in one launch per kernel (see the header comment) ---------------------------------------
__device__ __forceinline__ Geo geo_of(const AdaptDecFrame &F, const uint32_t *__restrict__ words_all) {
    Geo g;
    g.s.words = words_all + F.word0, g.s.nwords = F.nwords, g.s.last_mask = F.last_mask, g.s.total_bits = F.total_bits;
    g.base = F.payload_bit, g.range = F.range_bits, g.nranges = F.nranges, g.nblocks = F.nblocks;
    return g;
}
__device__ __forceinline__ const AdaptDecTab *tab_of(const AdaptDecBatch &a, uint32_t f) {
    return (const AdaptDecTab *)(a.tabs + (size_t)f * kAdaptDecTabSlot);
}
// the chunk's work arrays from the frame's first range and block on
__device__ __forceinline__ Work carve_frame(const AdaptDecBatch &a, const AdaptDecFrame &F) {
    Work w = carve(a.work, a.ranges, a.blocks);
    w.exit_bit[0] += F.range0, w.exit_bit[1] += F.range0, w.from += F.range0, w.count += F.range0, w.bad_at += F.range0, w.first += F.range0;
    w.pos += F.blk0, w.dcdiff += F.blk0;
    return w;
}

// adapt_dec_round for the workgroup's frame.  The exits it moved are counted once per workgroup, for the frame and for the chunk.
__global__ void __launch_bounds__(kThreads) adapt_dec_round_v(AdaptDecBatch a, int round) {
    __shared__ AdaptDecTab tab;
    __shared__ uint32_t ex[kThreads];
    __shared__ uint32_t moved;
    const uint32_t f = a.rwg_frame[blockIdx.x];
    AdaptDecFrameStatus *st = a.fs + f;
    if (round >= kAdaptBatchRounds0 && st->changed[round - 1] == 0) return; // (the whole workgroup: this frame has settled, and a fixed point stays one)
    const AdaptDecFrame F = a.frames[f];
    stage_tab(&tab, tab_of(a, f));
    const Geo g = geo_of(F, a.words);
    const Work w = carve_frame(a, F);
    const uint32_t t = (blockIdx.x - F.rwg0) * kThreads + threadIdx.x; // the range inside the frame
    const bool valid = t < g.nranges;
    const uint32_t *in = w.exit_bit[(round & 1) ^ 1];
    uint32_t *out = w.exit_bit[round & 1];
    uint32_t from = kNone, x = 0, cnt = 0, bad = kNone, entry = 0;
    bool walked = false;
    if (valid) {
        entry = (round == 0 || t == 0) ? g.base + t * g.range : in[t - 1u];
        if (round != 0) from = w.from[t], x = in[t];
    }
    const uint32_t x0 = x;
    for (int it = 0; it <= kThreads; it++) {
        bool m = false;
        if (valid && entry != from) {
            uint32_t nx;
            cnt = walk_range(tab, g.s, entry, range_limit(g, t), &nx, &bad, nullptr, 0);
            m = !walked && round == 0 ? true : nx != x;
            from = entry, x = nx, walked = true;
        }
        ex[threadIdx.x] = x;
        if (threadIdx.x == 0) moved = 0u;
        __syncthreads();
        if (m) moved = 1u;
        __syncthreads();
        const bool again = moved != 0u;
        if (valid && threadIdx.x > 0) entry = ex[threadIdx.x - 1u];
        __syncthreads();
        if (!again) break;
    }
    if (valid) {
        if (walked) w.from[t] = from, w.count[t] = cnt, w.bad_at[t] = bad;
        out[t] = x;
    }
    const int n = __syncthreads_count(valid && round != 0 && x != x0);
    if (threadIdx.x != 0) return;
    if (round == 0) {
        st->changed[0] = 1u, a.cs->changed[0] = 1u; // (every workgroup stores the same word)
    } else if (n) {
        atomicAdd(&st->changed[round], (uint32_t)n); // (few: the walks of round 0 fall in step within their range nearly everywhere)
        atomicAdd(&a.cs->changed[round], (uint32_t)n);
    }
}

// adapt_dec_scan, a workgroup per frame.  The frame's give-up bits and block count are written afresh: the passes may run twice.
__global__ void __launch_bounds__(kScanThreads) adapt_dec_scan_v(AdaptDecBatch a) {
    __shared__ uint32_t lds[kScanThreads];
    const AdaptDecFrame F = a.frames[blockIdx.x];
    const Work w = carve_frame(a, F);
    const uint32_t per = (F.nranges + kScanThreads - 1u) / kScanThreads;
    const uint32_t t0 = min(threadIdx.x * per, F.nranges), t1 = min(t0 + per, F.nranges);
    uint32_t sum = 0;
    for (uint32_t t = t0; t < t1; t++) sum += w.count[t];
    const uint32_t incl = block_scan(sum, lds);
    uint32_t run = incl - sum;
    bool incident = false;
    for (uint32_t t = t0; t < t1; t++) {
        w.first[t] = run;
        const uint32_t bad = w.bad_at[t];
        if (bad != kNone && (unsigned long long)run + bad < F.nblocks) incident = true;
        run += w.count[t];
    }
    const bool any = __syncthreads_or(incident) != 0;
    if (threadIdx.x == kScanThreads - 1u) {
        AdaptDecFrameStatus *st = a.fs + blockIdx.x;
        st->blocks = incl;
        st->giveup = (any ? kAdaptGiveupIncident : 0u) | (incl < F.nblocks ? kAdaptGiveupShort : 0u);
    }
}

__global__ void __launch_bounds__(kThreads) adapt_dec_positions_v(AdaptDecBatch a) {
    __shared__ AdaptDecTab tab;
    const uint32_t f = a.rwg_frame[blockIdx.x];
    const AdaptDecFrame F = a.frames[f];
    stage_tab(&tab, tab_of(a, f));
    const uint32_t t = (blockIdx.x - F.rwg0) * kThreads + threadIdx.x;
    if (t >= F.nranges) return;
    const Geo g = geo_of(F, a.words);
    const Work w = carve_frame(a, F);
    const uint32_t first = w.first[t];
    if (first >= F.nblocks || w.count[t] == 0) return;
    uint32_t x, bad;
    (void)walk_range(tab, g.s, w.from[t], range_limit(g, t), &x, &bad, w.pos + first, F.nblocks - first); // (inside the frame's own blocks)
}

__global__ void __launch_bounds__(kThreads) adapt_dec_blocks_v(AdaptDecBatch a) {
    __shared__ AdaptDecTab tab;
    const uint32_t f = a.bwg_frame[blockIdx.x];
    const AdaptDecFrame F = a.frames[f];
    stage_tab(&tab, tab_of(a, f));
    const uint32_t b = (blockIdx.x - F.bwg0) * kThreads + threadIdx.x; // the block inside the frame
    if (b >= F.nblocks) return;
    const Geo g = geo_of(F, a.words);
    const Work w = carve_frame(a, F);
    int16_t *row = a.zz + ((size_t)F.blk0 + b) * 64;
    uint4 *row4 = (uint4 *)row;
#pragma unroll
    for (int i = 0; i < 8; i++) row4[i] = make_uint4(0, 0, 0, 0);
    int dc = 0;
    // (as in adapt_dec_blocks: whatever an unsettled or short chain leaves in pos[] is walked within the frame's stream and written within the row)
    const uint32_t p = b < a.fs[f].blocks ? w.pos[b] : g.s.total_bits;
    if (p < g.s.total_bits) {
        uint32_t next;
        (void)walk_block(tab, g.s, p, &next, row, &dc);
    }
    w.dcdiff[b] = dc;
}

// adapt_dec_dc, a workgroup per frame: the sum starts over with every frame (codec.py:53)
__global__ void __launch_bounds__(kScanThreads) adapt_dec_dc_v(AdaptDecBatch a) {
    __shared__ long long lds[kScanThreads];
    const AdaptDecFrame F = a.frames[blockIdx.x];
    const Work w = carve_frame(a, F);
    int16_t *zz = a.zz + (size_t)F.blk0 * 64;
    const uint32_t per = (F.nblocks + kScanThreads - 1u) / kScanThreads;
    const uint32_t b0 = min(threadIdx.x * per, F.nblocks), b1 = min(b0 + per, F.nblocks);
    long long sum = 0;
    for (uint32_t b = b0; b < b1; b++) sum += w.dcdiff[b];
    long long run = block_scan(sum, lds) - sum;
    bool out_of_range = false;
    for (uint32_t b = b0; b < b1; b++) {
        run += w.dcdiff[b];
        if (run < -32768 || run > 32767) out_of_range = true;
        zz[(size_t)b * 64] = (int16_t)run;
    }
    const bool any = __syncthreads_or(out_of_range) != 0;
    if (any && threadIdx.x == 0) a.fs[blockIdx.x].giveup |= kAdaptGiveupDc; // (this workgroup alone writes the frame's status in this launch)
}

// (a stream of fewer than 2^32 - 8,192 bits, checked by the caller: bit positions are 32-bit, and a walk may step past the end by a symbol)
inline uint32_t ranges_of(size_t len, size_t payload_bit, int range_bits) {
    const size_t payload = len * 8 - payload_bit;
    return (uint32_t)((payload + (size_t)range_bits - 1) / (size_t)range_bits);
}

} // namespace

// Stream bits per lane: two average blocks, 256 at least (a lane's walk is one dependent chain of look-ups: its length is the kernel's
// time), 4,096 at most.
int adaptive_dec_range_bits(size_t len, size_t payload_bit, size_t nblocks) { return adaptive_dec_range_rule(len, payload_bit, nblocks); }

size_t adaptive_dec_work_bytes(size_t len, size_t payload_bit, size_t nblocks, int range_bits) {
    return ((size_t)ranges_of(len, payload_bit, range_bits) * 6 + nblocks * 2) * 4;
}

hipError_t adaptive_decode_gpu(const void *d_stream, size_t len, size_t payload_bit, size_t nblocks, int range_bits, const AdaptDecTab *d_tab,
                               void *d_work, AdaptDecStatus *d_status, int16_t *d_zz, int round0, int nrounds, bool finish, hipStream_t stream) {
    if (((uintptr_t)d_stream & 3u) || len * 8 <= payload_bit || len * 8 + 8192 >= (1ull << 32) || nblocks == 0 || nblocks >= (1ull << 31) ||
        range_bits < 64 || round0 < 0 || nrounds < 0 || round0 + nrounds > kAdaptDecMaxRounds || (nrounds == 0 && !finish))
        return hipErrorInvalidValue;
    Geo g;
    g.s.words = (const uint32_t *)d_stream;
    g.s.nwords = (uint32_t)((len + 3) / 4);
    g.s.last_mask = (len & 3) ? ~0u << (32u - 8u * (uint32_t)(len & 3)) : ~0u;
    g.s.total_bits = (uint32_t)(len * 8);
    g.base = (uint32_t)payload_bit;
    g.range = (uint32_t)range_bits;
    g.nranges = ranges_of(len, payload_bit, range_bits);
    g.nblocks = (uint32_t)nblocks;
    hipError_t e;
    if (round0 == 0) {
        if ((e = hipMemsetAsync(d_status, 0, sizeof(AdaptDecStatus), stream)) != hipSuccess) return e;
    } else if (finish) {
        // the give-up bits and the block count belong to the passes behind the rounds: when those ran on a guess, they run again
        if ((e = hipMemsetAsync(d_status, 0, offsetof(AdaptDecStatus, changed), stream)) != hipSuccess) return e;
    }
    const uint32_t range_grid = (g.nranges + kThreads - 1u) / kThreads, block_grid = (g.nblocks + kThreads - 1u) / kThreads;
    for (int r = round0; r < round0 + nrounds; r++) adapt_dec_round<<<range_grid, kThreads, 0, stream>>>(g, d_tab, d_work, d_status, r);
    if (!finish) return hipGetLastError();
    adapt_dec_scan<<<1, kScanThreads, 0, stream>>>(g, d_work, d_status);
    adapt_dec_positions<<<range_grid, kThreads, 0, stream>>>(g, d_tab, d_work);
    adapt_dec_blocks<<<block_grid, kThreads, 0, stream>>>(g, d_tab, d_work, d_status, d_zz);
    adapt_dec_dc<<<1, kScanThreads, 0, stream>>>(g, d_work, d_status, d_zz);
    return hipGetLastError();
}

// The descriptor form's launcher: rounds [round0, round0 + nrounds) for every frame of the chunk and, with `finish`, the passes behind them.
// round0 = 0 starts a decode and zeroes the status words.  The host-side checks come before the first launch.
hipError_t adaptive_decode_gpu_batch(const AdaptDecBatch &a, int round0, int nrounds, bool finish, hipStream_t stream) {
    if (!a.frames || !a.rwg_frame || !a.bwg_frame || !a.tabs || !a.words || !a.work || !a.cs || !a.fs || !a.zz || ((uintptr_t)a.words & 3u) ||
        ((uintptr_t)a.tabs & 7u) || ((uintptr_t)a.zz & 15u) || a.nframes == 0 || a.ranges == 0 || a.blocks == 0 || a.range_wgs == 0 || a.block_wgs == 0 ||
        round0 < 0 || nrounds < 0 || round0 + nrounds > kAdaptBatchRounds || (nrounds == 0 && !finish))
        return hipErrorInvalidValue;
    hipError_t e;
    if (round0 == 0 && (e = hipMemsetAsync(a.cs, 0, sizeof(AdaptDecChunkStatus) + (size_t)a.nframes * sizeof(AdaptDecFrameStatus), stream)) != hipSuccess) return e;
    for (int r = round0; r < round0 + nrounds; r++) adapt_dec_round_v<<<a.range_wgs, kThreads, 0, stream>>>(a, r);
    if (!finish) return hipGetLastError();
    adapt_dec_scan_v<<<a.nframes, kScanThreads, 0, stream>>>(a);
    adapt_dec_positions_v<<<a.range_wgs, kThreads, 0, stream>>>(a);
    adapt_dec_blocks_v<<<a.block_wgs, kThreads, 0, stream>>>(a);
    adapt_dec_dc_v<<<a.nframes, kScanThreads, 0, stream>>>(a);
    return hipGetLastError();
}

} // namespace tic
