// tic_adaptive_frames.h - the per-frame records of the adaptive encoder's descriptor form (adaptive_stats_v / adaptive_pack_v,
// tic_adaptive_gpu.hip), free of HIP: what the statistics kernel leaves and the packing kernels read per frame, the table a launch finds
// its frames in, and the three functions of the host plan - a chunk's table from the mixed plan (tic_host_pipeline.h), the carving of a
// slot's buffers, and the stream areas from the exact lengths.  tests/native/adaptplan_selftest.cpp sweeps them on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "tic_host_pipeline.h"

namespace tic {

// Symbol bins of the adaptive tables: AC (run << 4) | size at 0..255, DC size category c at kAdaptDcBin + c.
constexpr int kAdaptDcBin = 256, kAdaptBins = 272;
// Longest symbol (code + value bits) the packing kernel and the decoder take.
constexpr int kAdaptMaxSymbolBits = 64;
// Serialized table bits at most: 2 x 16 count bits, 16 DC entries of 8 + 15 bits, 256 AC entries of 16 + 64 bits.
constexpr size_t kAdaptMaxTableBytes = (32 + 16 * 23 + 256 * 80 + 7) / 8;

// What the statistics kernel leaves per frame: symbol counts and first-occurrence keys (DC: block index; AC: block * 64 + ordinal of
// the symbol in the block's run-length list, huffman.py:12-33), and an error word (1: a DC category or AC size above 15, which the
// reference's write_huffman_table cannot store, codec.py:73-84).
struct AdaptStats {
    unsigned long long count[kAdaptBins];
    unsigned long long first[kAdaptBins]; // ~0: the symbol does not occur
    unsigned int err;
};

// The table as the packing kernels use it: codeword (right-aligned, up to 64 bits) and its length per bin.
struct HuffWide {
    unsigned long long code[kAdaptBins];
    unsigned int len[kAdaptBins];
};

constexpr unsigned kAdaptGroupBlocks = 256; // blocks per workgroup of the statistics, bits and write kernels (one thread each)
// A frame's header and serialized table as the host lays them out for ONE upload: a multiple of 16 bytes apart, whole 32-bit words.
constexpr size_t kAdaptHeadStride = (16 + kAdaptMaxTableBytes + 15) / 16 * 16;

// One frame of a launch.  A workgroup owns kAdaptGroupBlocks blocks of ONE frame: a frame's workgroups are rounded up, so first_group is a
// prefix sum of its own and no function of first_block.  The statistics launch reads first_block, nblocks and first_group; the other
// fields are known only behind it (the host builds the frame's table from the statistics) and are filled for the packing launches.
struct AdaptFrameRec {
    unsigned long long first_block; // in d_zz, 64 coefficients each
    unsigned long long nblocks;
    unsigned long long out_off;     // byte offset of the frame's stream area in d_streams, a multiple of 16
    unsigned long long out_words;   // 32-bit words of the stream: nothing is written at or past it
    uint32_t first_group, ngroups;  // workgroups in front of the frame's, and its own
    uint32_t base_bits;             // the payload's first bit: 128 + table bits
    uint32_t skip;                  // 1: the frame is not packed (its stream does not fit the caller's buffer): it has no area
    uint32_t pad[4];
};
static_assert(sizeof(AdaptFrameRec) == 64, "a record is 64 bytes");

// The table a launch reads, found the way EntropyFrameTable is: lane l compares first_group[l] with the workgroup's index; entries behind
// the last frame are 0xffffffff.
struct AdaptFrameTable {
    uint32_t first_group[kEntropyMaxFrames];
    AdaptFrameRec rec[kEntropyMaxFrames];
};

// Fills `t` for frames of nblocks[k] blocks (k < n <= kEntropyMaxFrames, every one >= 1), coefficients back to back; the stream fields are
// zero.  *nblk, *ngroups: the launch's totals.  False when n is out of range, a frame is empty or the grid leaves 31 bits.
inline bool fill_adaptive_table(AdaptFrameTable *t, int n, const size_t *nblocks, size_t *nblk, size_t *ngroups) {
    if (n < 1 || n > kEntropyMaxFrames) return false;
    for (int k = 0; k < kEntropyMaxFrames; k++) {
        t->first_group[k] = 0xffffffffu;
        t->rec[k] = AdaptFrameRec();
    }
    size_t blk = 0, grp = 0;
    for (int k = 0; k < n; k++) {
        if (nblocks[k] == 0) return false;
        const size_t groups = (nblocks[k] + kAdaptGroupBlocks - 1) / kAdaptGroupBlocks;
        if (grp + groups > 0x7fffffffu) return false;
        AdaptFrameRec &r = t->rec[k];
        r.first_block = blk, r.nblocks = nblocks[k];
        r.first_group = (uint32_t)grp, r.ngroups = (uint32_t)groups;
        t->first_group[k] = (uint32_t)grp;
        blk += nblocks[k], grp += groups;
    }
    *nblk = blk, *ngroups = grp;
    return true;
}
// ... of chunk `c` of a mixed plan: the plan's order, its frames' coefficients at MixedFrame::first_block.
inline bool adaptive_chunk_table(const MixedPlan &p, const MixedChunk &c, AdaptFrameTable *t, size_t *nblk, size_t *ngroups) {
    size_t nb[kEntropyMaxFrames];
    if (c.count < 1 || c.count > kEntropyMaxFrames) return false;
    for (int k = 0; k < c.count; k++) nb[k] = p.frames[(size_t)(c.first + k)].nblk;
    return fill_adaptive_table(t, c.count, nb, nblk, ngroups);
}

// Stream areas from the exact lengths: frame k's stream has total_bits[k] bits (header and table included) of which the first
// base_bits[k] are header and table; total_bits[k] == 0 marks a frame that is not packed.  Areas lie back to back in table order, each a
// multiple of 16 bytes (whole words of the stream, rounded up).  *stream_bytes: their sum.
inline void assign_adaptive_streams(AdaptFrameTable *t, int n, const unsigned long long *total_bits, const uint32_t *base_bits, size_t *stream_bytes) {
    size_t off = 0;
    for (int k = 0; k < n; k++) {
        AdaptFrameRec &r = t->rec[k];
        r.skip = total_bits[k] == 0;
        r.out_off = off;
        r.out_words = (total_bits[k] + 31) / 32;
        r.base_bits = r.skip ? 0u : base_bits[k];
        off += ((size_t)r.out_words * 4 + 15) / 16 * 16;
    }
    *stream_bytes = off;
}

// How a chunk of `count` frames, nblk blocks and ngroups workgroups carves a slot's device buffer (and, up to `upload_end`, its pinned
// mirror): the statistics the first launch leaves; then what ONE upload brings behind them - an error word (uploaded as zero), the
// read-back's offsets, the frame table, the frames' code tables, their headers and serialized tables -; then bits per block and the
// workgroup sums.  Every piece starts at a multiple of 256.
struct AdaptSlotLayout {
    size_t stats, err, rb_frames, frames, tabs, heads, upload_end, bbits, gsum, end;
};
inline AdaptSlotLayout adaptive_slot_layout(size_t count, size_t nblk, size_t ngroups) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    AdaptSlotLayout l;
    l.stats = 0;
    l.err = up(l.stats + count * sizeof(AdaptStats));
    l.rb_frames = l.err + 256;
    l.frames = up(l.rb_frames + sizeof(EntropyFrameTable));
    l.tabs = up(l.frames + sizeof(AdaptFrameTable));
    l.heads = up(l.tabs + count * sizeof(HuffWide));
    l.upload_end = up(l.heads + count * kAdaptHeadStride);
    l.bbits = l.upload_end;
    l.gsum = up(l.bbits + nblk * 4);
    l.end = up(l.gsum + ngroups * 8);
    return l;
}

} // namespace tic
