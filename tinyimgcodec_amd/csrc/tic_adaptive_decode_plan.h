// tic_adaptive_decode_plan.h - the plan of tic_decompress_batch_adaptive (tic_api.hip), free of HIP and of the context, modelled on
// tic_decode_plan.h: which frames go into which chunk, the descriptor the kernels of tic_adaptive_dec_gpu.hip read for each of them (where its
// words, ranges and blocks lie in the chunk's buffers, its own range, its first workgroup in the two grids), where its pixels and its table
// lie, the chunk's totals and work-buffer bytes, and the byte layout of the one buffer a chunk uploads.  All of it is a function of the
// frames' geometries, stream lengths and payload starts and of five limits; tests/native/adecplan_selftest.cpp sweeps it on the CPU, under
// the address sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "tic_decode_plan.h"

namespace tic {

constexpr uint32_t kAdaptDecLanes = 256;     // lanes (ranges, or blocks) of a workgroup of the range and block grids
constexpr size_t kAdaptDecTabBytes = 13320;  // sizeof(AdaptDecTab) (tic_adaptive.h asserts it)
constexpr size_t kAdaptDecTabSlot = 13568;   // ... in the upload buffer: the next multiple of 256
// Rounds of the stitch a chunk runs at most: three with the passes behind them, then sixteen more (tic_adaptive_dec_gpu.hip, rounds protocol)
constexpr int kAdaptBatchRounds0 = 3, kAdaptBatchRoundsMore = 16, kAdaptBatchRounds = kAdaptBatchRounds0 + kAdaptBatchRoundsMore;

// Stream bits per lane of a stream's decode: two average blocks, 256 at least (a lane's walk is one dependent chain of look-ups: its length
// is the kernel's time), 4,096 at most.  (adaptive_dec_range_bits, tic_adaptive_dec_gpu.hip, is this function.)
inline int adaptive_dec_range_rule(size_t len, size_t payload_bit, size_t nblocks) {
    const size_t payload = len * 8 - payload_bit;
    const size_t r = 2 * payload / (nblocks ? nblocks : 1);
    return (int)(r < 256 ? 256 : (r > 4096 ? 4096 : r));
}
// (a stream of fewer than 2^32 - 8,192 bits: bit positions are 32-bit, and a walk may step past the end by a symbol)
inline uint32_t adaptive_dec_ranges_of(size_t len, size_t payload_bit, int range_bits) {
    const size_t payload = len * 8 - payload_bit;
    return (uint32_t)((payload + (size_t)range_bits - 1) / (size_t)range_bits);
}
// The streams whose bit positions the kernels can hold: the bound of adaptive_device_takes (tic_api.hip)
inline bool adaptive_dec_fits(size_t nblocks, size_t len, size_t payload_bit) {
    const size_t bits = len * 8;
    return nblocks != 0 && nblocks < (1ull << 31) && bits > payload_bit && bits + 8192 < (1ull << 32);
}

// What the kernels read of a frame.  word0, range0, blk0 and the workgroup numbers count inside the chunk.
struct AdaptDecFrame {
    uint32_t word0, nwords, last_mask, total_bits; // the stream's 32-bit words in the chunk's stream buffer, the bytes of the last one that are the stream's, 8 * len
    uint32_t payload_bit, range_bits;              // the first bit of block 0; stream bits per lane: the frame's own choice
    uint32_t nranges, range0;
    uint32_t blk0, nblocks;
    uint32_t rwg0, bwg0; // its first workgroup in the range grid (ceil(nranges / 256) of them) and in the block grid (ceil(nblocks / 256))
};
// What they report of a frame, and of the chunk: the exits every round launched moved (a frame's chain is known only when the last round
// launched moved none of its exits; the chunk has settled when that round moved none at all).  The chunk's entry lies in front of the frames'.
struct AdaptDecFrameStatus {
    uint32_t giveup, blocks; // kAdaptGiveup* bits (tic_adaptive.h); blocks on the chain up to the stream's end
    uint32_t changed[kAdaptBatchRounds];
    uint32_t pad_;
};
struct AdaptDecChunkStatus {
    uint32_t changed[kAdaptBatchRounds];
    uint32_t pad_[32 - kAdaptBatchRounds];
};

struct AdaptDecPlanIn {
    int h, w, quality;
    size_t len, payload_bit; // stream bytes, header and table included; the payload's first bit (AdaptTable::payload_bit)
    bool takes;              // the batch kernels take it (tic_api.hip adaptive_batch_takes); any other frame is in no chunk
};
struct AdaptDecPlanLimits {
    size_t stream_bytes, pix_bytes, coef_bytes, tab_bytes; // of a chunk's stream slots, pixel slots, coefficients (blocks * 128) and table slots
    int frames;
};
struct AdaptDecPlanFrame {
    int index; // the caller's index
    int h, w, quality;
    size_t len, nblk, pitch;
    AdaptDecFrame d;
    size_t pix_off; // in the chunk's pixel buffer
    size_t tab_off; // in the upload buffer's table piece
};
struct AdaptDecPlanChunk {
    int first, count; // frames [first, first + count) of AdaptDecPlan::frames
    size_t words, pix_bytes, blocks, tab_bytes;
    uint32_t ranges, range_wgs, block_wgs;
    size_t work_bytes; // six words per range, a word and an int per block: adaptive_dec_batch_work_bytes
};
struct AdaptDecPlan {
    std::vector<AdaptDecPlanFrame> frames; // the frames taken, in the caller's order
    std::vector<AdaptDecPlanChunk> chunks; // in that order too
};

inline size_t adaptive_dec_batch_work_bytes(size_t ranges, size_t blocks) { return (ranges * 6 + blocks * 2) * 4; }

inline AdaptDecPlanFrame adec_plan_frame(int index, const AdaptDecPlanIn &in) {
    AdaptDecPlanFrame f{};
    f.index = index, f.h = in.h, f.w = in.w, f.quality = in.quality, f.len = in.len;
    f.nblk = num_blocks(in.h, in.w);
    f.pitch = dec_pix_pitch(in.w);
    f.d.nwords = (uint32_t)((in.len + 3) / 4);
    f.d.last_mask = (in.len & 3) ? 0xffffffffu << (8u * (4u - (uint32_t)(in.len & 3))) : 0xffffffffu;
    f.d.total_bits = (uint32_t)(in.len * 8);
    f.d.payload_bit = (uint32_t)in.payload_bit;
    f.d.range_bits = (uint32_t)adaptive_dec_range_rule(in.len, in.payload_bit, f.nblk);
    f.d.nranges = adaptive_dec_ranges_of(in.len, in.payload_bit, (int)f.d.range_bits);
    f.d.nblocks = (uint32_t)f.nblk;
    return f;
}

// Frames [first, first + count) of p.frames become the next chunk: their places in it and its totals.
inline void adec_plan_close_chunk(AdaptDecPlan &p, int first, int count) {
    AdaptDecPlanChunk c{};
    c.first = first, c.count = count;
    for (int k = first; k < first + count; k++) {
        AdaptDecPlanFrame &f = p.frames[(size_t)k];
        f.d.word0 = (uint32_t)c.words, f.d.range0 = c.ranges, f.d.blk0 = (uint32_t)c.blocks, f.d.rwg0 = c.range_wgs, f.d.bwg0 = c.block_wgs;
        f.pix_off = c.pix_bytes, f.tab_off = c.tab_bytes;
        c.words += dec_stream_slot(f.len) / 4, c.blocks += f.nblk, c.pix_bytes += dec_pix_slot(f.pitch, f.h), c.tab_bytes += kAdaptDecTabSlot;
        c.ranges += f.d.nranges;
        c.range_wgs += (f.d.nranges + kAdaptDecLanes - 1) / kAdaptDecLanes;
        c.block_wgs += (f.d.nblocks + kAdaptDecLanes - 1) / kAdaptDecLanes;
    }
    c.work_bytes = adaptive_dec_batch_work_bytes(c.ranges, c.blocks);
    p.chunks.push_back(c);
}

// Chunks: the frames taken, in order, while the chunk's stream slots, pixel slots, coefficients, table slots and frame count stay inside the
// limits - a frame joins the chunk unless the chunk is non-empty and would pass one (a single frame larger than a limit is a chunk of its own).
inline AdaptDecPlan plan_adaptive_decode_batch(const AdaptDecPlanIn *in, int n, const AdaptDecPlanLimits &lim) {
    AdaptDecPlan p;
    p.frames.reserve((size_t)(n > 0 ? n : 0));
    int first = 0, count = 0;
    size_t in_bytes = 0, pix_bytes = 0, coef_bytes = 0, tab_bytes = 0;
    for (int i = 0; i < n; i++) {
        if (!in[i].takes) continue;
        const AdaptDecPlanFrame f = adec_plan_frame(i, in[i]);
        const size_t sb = dec_stream_slot(f.len), pb = dec_pix_slot(f.pitch, f.h), cb = f.nblk * 128;
        if (count > 0 && (in_bytes + sb > lim.stream_bytes || pix_bytes + pb > lim.pix_bytes || coef_bytes + cb > lim.coef_bytes ||
                          tab_bytes + kAdaptDecTabSlot > lim.tab_bytes || count >= lim.frames)) {
            adec_plan_close_chunk(p, first, count);
            first += count, count = 0, in_bytes = pix_bytes = coef_bytes = tab_bytes = 0;
        }
        p.frames.push_back(f);
        count++, in_bytes += sb, pix_bytes += pb, coef_bytes += cb, tab_bytes += kAdaptDecTabSlot;
    }
    if (count > 0) adec_plan_close_chunk(p, first, count);
    return p;
}

// The frame of every workgroup of the chunk's range grid (c.range_wgs entries) and block grid (c.block_wgs), as the kernels look it up
inline void adec_plan_fill_wg_tables(const AdaptDecPlanFrame *pf, int count, uint32_t *rwg_frame, uint32_t *bwg_frame) {
    for (int k = 0; k < count; k++) {
        const AdaptDecFrame &d = pf[k].d;
        for (uint32_t t = 0; t < (d.nranges + kAdaptDecLanes - 1) / kAdaptDecLanes; t++) rwg_frame[d.rwg0 + t] = (uint32_t)k;
        for (uint32_t t = 0; t < (d.nblocks + kAdaptDecLanes - 1) / kAdaptDecLanes; t++) bwg_frame[d.bwg0 + t] = (uint32_t)k;
    }
}

// The one buffer a chunk uploads: F descriptors, the frame of every workgroup of the range grid and of the block grid, the inverse
// transform's arguments (`idct_arg_bytes` each) and its workgroup table (`idct_wgs` entries of 8 bytes: frame, first tile), a table slot per
// frame, the streams - every piece at a multiple of 256 bytes.
struct AdaptDecUploadLayout {
    size_t o_frames, o_rwg, o_bwg, o_idct_args, o_idct_wgs, o_tabs, o_streams, up_bytes;
    static size_t up(size_t b) { return (b + 255) / 256 * 256; }
    AdaptDecUploadLayout(const AdaptDecPlanChunk &c, size_t idct_arg_bytes, size_t idct_wgs) {
        const size_t F = (size_t)c.count;
        o_frames = 0;
        o_rwg = up(o_frames + F * sizeof(AdaptDecFrame));
        o_bwg = up(o_rwg + (size_t)c.range_wgs * 4);
        o_idct_args = up(o_bwg + (size_t)c.block_wgs * 4);
        o_idct_wgs = up(o_idct_args + F * idct_arg_bytes);
        o_tabs = up(o_idct_wgs + idct_wgs * 8);
        o_streams = up(o_tabs + c.tab_bytes);
        up_bytes = o_streams + c.words * 4;
    }
};

// The chunk's device buffer behind the upload: status words (the chunk's, then a frame's each), the work arrays, the coefficients.
struct AdaptDecWorkLayout {
    size_t o_status, status_bytes, o_work, o_coef, bytes;
    explicit AdaptDecWorkLayout(const AdaptDecPlanChunk &c) {
        o_status = 0;
        status_bytes = sizeof(AdaptDecChunkStatus) + (size_t)c.count * sizeof(AdaptDecFrameStatus);
        o_work = AdaptDecUploadLayout::up(status_bytes);
        o_coef = AdaptDecUploadLayout::up(o_work + c.work_bytes);
        bytes = o_coef + c.blocks * 128;
    }
};

} // namespace tic
