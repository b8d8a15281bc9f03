// tic_decode_plan.h - the plan of tic_decompress_batch (tic_api.hip), free of HIP and of the context: which frames go into which chunk, where a
// frame's words, ranges, blocks and pixels lie inside its chunk, the chunk's totals, range and window, and the byte layout of the one buffer a
// chunk uploads.  All of it is a function of the frames' geometries and stream lengths and of three limits;
// tests/native/decplan_selftest.cpp sweeps it on the CPU, under the address sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "tic_entropy.h"
#include "tic_entropy_dec_gpu.h"

namespace tic {

// Row pitch of decoded pixels in a buffer of the library's own (a chunk's pixel buffer, the host-mapped buffer of a small tic_decompress):
// whole 8-byte row stores.
inline size_t dec_pix_pitch(int w) { return ((size_t)w + 7) / 8 * 8; }
// What a frame takes of a chunk's stream buffer (16-byte aligned, and 16 bytes the kernels may read behind it) and of its pixel buffer.
inline size_t dec_stream_slot(size_t len) { return (len + 15) / 16 * 16 + 16; }
inline size_t dec_pix_slot(size_t pitch, int h) { return (pitch * (size_t)h + 255) / 256 * 256; }

struct DecPlanIn {
    int h, w, quality;
    size_t len;  // stream bytes, header included
    bool takes;  // the batch kernels take it (tic_api.hip: blocks, no scaled_dct, device_decoder_takes); any other frame is in no chunk
};
struct DecPlanLimits {
    size_t stream_bytes, pix_bytes; // of a chunk's stream slots and pixel slots
    int frames;
};

// A frame of a chunk.  word0, range0, blk0 and pix_off count inside the chunk.
struct DecPlanFrame {
    int index; // the caller's index
    int h, w, quality;
    size_t len, nblk, pitch;
    uint32_t word0, nwords, last_mask, stream_bits; // the stream's 32-bit words in the chunk's stream buffer; the bytes of the last one that are the stream's
    uint32_t nranges, range0;                       // its ranges at the chunk's range_bits
    uint32_t blk0;
    size_t pix_off;
};
struct DecPlanChunk {
    int first, count; // frames [first, first + count) of DecPlan::frames
    size_t words, pix_bytes, blocks;
    size_t ranges288; // sum of dec_ranges_288(len): what the work buffer is provided from
    uint32_t ranges;  // sum of nranges: what it is carved up by
    int range_bits;   // the largest of the frames' choices (dec_range_rule)
    bool small_win;   // every stream has at most 240 bits per block on average
};
struct DecPlan {
    std::vector<DecPlanFrame> frames; // the frames taken, in the caller's order
    std::vector<DecPlanChunk> chunks; // in that order too
};

inline DecPlanFrame dec_plan_frame(int index, const DecPlanIn &in) {
    DecPlanFrame f{};
    f.index = index, f.h = in.h, f.w = in.w, f.quality = in.quality, f.len = in.len;
    f.nblk = num_blocks(in.h, in.w);
    f.pitch = dec_pix_pitch(in.w);
    f.nwords = (uint32_t)((in.len + 3) / 4);
    f.last_mask = (in.len & 3) ? 0xffffffffu << (8u * (4u - (uint32_t)(in.len & 3))) : 0xffffffffu;
    f.stream_bits = (uint32_t)(in.len * 8);
    return f;
}

// Frames [first, first + count) of p.frames become the next chunk: their places in it and its totals.
inline void dec_plan_close_chunk(DecPlan &p, int first, int count) {
    DecPlanChunk c{};
    c.first = first, c.count = count, c.small_win = true;
    for (int k = first; k < first + count; k++) {
        DecPlanFrame &f = p.frames[(size_t)k];
        f.word0 = (uint32_t)c.words, f.blk0 = (uint32_t)c.blocks, f.pix_off = c.pix_bytes;
        c.words += dec_stream_slot(f.len) / 4, c.blocks += f.nblk, c.pix_bytes += dec_pix_slot(f.pitch, f.h);
        c.ranges288 += dec_ranges_288(f.len);
        const int rb = dec_range_rule(f.len, f.nblk);
        c.range_bits = rb > c.range_bits ? rb : c.range_bits;
        c.small_win = c.small_win && f.len * 8 / f.nblk <= 240;
    }
    for (int k = first; k < first + count; k++) { // (the ranges: once the chunk's range is known)
        DecPlanFrame &f = p.frames[(size_t)k];
        f.nranges = (uint32_t)dec_ranges_of(f.len * 8, c.range_bits);
        f.range0 = c.ranges;
        c.ranges += f.nranges;
    }
    p.chunks.push_back(c);
}

// Chunks: the frames taken, in order, while the chunk's stream slots, pixel slots and frame count stay inside the limits - a frame joins the
// chunk unless the chunk is non-empty and would pass one (a single frame larger than a limit is a chunk of its own).
inline DecPlan plan_decode_batch(const DecPlanIn *in, int n, const DecPlanLimits &lim) {
    DecPlan p;
    p.frames.reserve((size_t)(n > 0 ? n : 0));
    int first = 0, count = 0;
    size_t in_bytes = 0, pix_bytes = 0;
    for (int i = 0; i < n; i++) {
        if (!in[i].takes) continue;
        const DecPlanFrame f = dec_plan_frame(i, in[i]);
        const size_t sb = dec_stream_slot(f.len), pb = dec_pix_slot(f.pitch, f.h);
        if (count > 0 && (in_bytes + sb > lim.stream_bytes || pix_bytes + pb > lim.pix_bytes || count >= lim.frames)) {
            dec_plan_close_chunk(p, first, count);
            first += count, count = 0, in_bytes = pix_bytes = 0;
        }
        p.frames.push_back(f);
        count++, in_bytes += sb, pix_bytes += pb;
    }
    if (count > 0) dec_plan_close_chunk(p, first, count);
    return p;
}

// The one buffer a chunk uploads: F descriptors, the frame of every wave of the measure grid, the frame of every workgroup of the fused grid,
// the streams - every piece at a multiple of 256 bytes.
struct DecUploadLayout {
    size_t o_frames, o_tiles, o_wgs, o_streams, up_bytes;
    static size_t up(size_t b) { return (b + 255) / 256 * 256; }
    DecUploadLayout(size_t F, size_t tiles, size_t wgs, size_t words) {
        o_frames = 0;
        o_tiles = up(o_frames + F * sizeof(DecFrame));
        o_wgs = up(o_tiles + tiles * 4);
        o_streams = up(o_wgs + wgs * 4);
        up_bytes = o_streams + words * 4;
    }
};

} // namespace tic
