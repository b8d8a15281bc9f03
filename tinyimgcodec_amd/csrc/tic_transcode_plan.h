// tic_transcode_plan.h - the plan of the batch transcoding calls (tic_entropy_decode_batch, tic_retable_adaptive_batch, tic_retable_default_batch;
// tic_api.hip), free of HIP and of the context.  It joins a READER's plan - tic_decode_plan.h for default-table streams, tic_adaptive_decode_plan.h
// for streams with an embedded table - with the WRITER's table of the other family (tic_adaptive_frames.h, tic_entropy_frames.h): a chunk's
// coefficients stay on the device between the two, frame k's rows from row blk0 of the chunk's buffer on, and the writer's record of a frame names
// that row explicitly (first_block == blk0).  A chunk holds at most kEntropyMaxFrames frames (a writer's table has one entry per lane of a wave),
// inside the reader's limits.  A frame the reader did not complete is SKIPPED: the adaptive writer's table keeps its record (its statistics are
// taken with the others' and never looked at) and marks it `skip`, the default writer's table has no record of it - either way a gap in the
// coefficient buffer, and nothing of that frame is ever encoded from it.  tests/native/transcode_plan_selftest.cpp sweeps all of it on the CPU,
// under the address sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "tic_adaptive_decode_plan.h"
#include "tic_adaptive_frames.h"
#include "tic_decode_plan.h"
#include "tic_entropy.h"
#include "tic_entropy_frames.h"

namespace tic {

// What the batch transcoders put into one chunk at most: stream slots, coefficients (blocks * 128), table slots of the adaptive reader, frames.
struct TranscodeLimits {
    size_t stream_bytes, coef_bytes, tab_bytes;
    int frames;
};
inline TranscodeLimits transcode_default_limits() { return TranscodeLimits{(size_t)96 << 20, (size_t)256 << 20, (size_t)16 << 20, kEntropyMaxFrames}; }
inline int transcode_chunk_frames(int frames) { return frames < 1 ? 1 : (frames > kEntropyMaxFrames ? kEntropyMaxFrames : frames); }

// A frame of a chunk as the writers see it, whichever reader decoded it.
struct TranscodeFrame {
    int index;          // the caller's index
    int h, w, quality;  // the header's fields
    size_t nblk, blk0;  // its rows in the chunk's coefficient buffer
    bool skip;          // the reader did not complete it: its rows hold anything
};

// The reader's plan for default-table (and scaled_dct) streams: plan_decode_batch's frames and chunks (dec_plan_frame, dec_plan_close_chunk), cut
// by the transcoders' limits - coefficient bytes where the pixel decoder counts pixel bytes.  The plan's pixel fields (pitch, pix_off, pix_bytes)
// are filled and unused.
inline DecPlan plan_transcode_default_reader(const DecPlanIn *in, int n, const TranscodeLimits &lim) {
    DecPlan p;
    p.frames.reserve((size_t)(n > 0 ? n : 0));
    const int max_frames = transcode_chunk_frames(lim.frames);
    int first = 0, count = 0;
    size_t in_bytes = 0, coef_bytes = 0;
    for (int i = 0; i < n; i++) {
        if (!in[i].takes) continue;
        const DecPlanFrame f = dec_plan_frame(i, in[i]);
        const size_t sb = dec_stream_slot(f.len), cb = f.nblk * 128;
        if (count > 0 && (in_bytes + sb > lim.stream_bytes || coef_bytes + cb > lim.coef_bytes || count >= max_frames)) {
            dec_plan_close_chunk(p, first, count);
            first += count, count = 0, in_bytes = coef_bytes = 0;
        }
        p.frames.push_back(f);
        count++, in_bytes += sb, coef_bytes += cb;
    }
    if (count > 0) dec_plan_close_chunk(p, first, count);
    return p;
}

// ... for streams with an embedded table: plan_adaptive_decode_batch with the frame count capped (no pixel limit: nothing is transformed).
inline AdaptDecPlan plan_transcode_adaptive_reader(const AdaptDecPlanIn *in, int n, const TranscodeLimits &lim) {
    const AdaptDecPlanLimits al = {lim.stream_bytes, ~(size_t)0, lim.coef_bytes, lim.tab_bytes, transcode_chunk_frames(lim.frames)};
    return plan_adaptive_decode_batch(in, n, al);
}

inline TranscodeFrame transcode_frame(const DecPlanFrame &f) { return TranscodeFrame{f.index, f.h, f.w, f.quality, f.nblk, (size_t)f.blk0, false}; }
inline TranscodeFrame transcode_frame(const AdaptDecPlanFrame &f) { return TranscodeFrame{f.index, f.h, f.w, f.quality, f.nblk, (size_t)f.d.blk0, false}; }

// The adaptive writer's table of a chunk: a record per frame, in chunk order, first_block = blk0 (the frames' rows lie back to back, so the table
// fill_adaptive_table makes has exactly these - checked, not assumed).  The statistics launch reads it as it is; `skip` is set for the packing
// launches by assign_adaptive_streams (total_bits == 0), which the caller gives every skipped frame.  *span: rows of the coefficient buffer the
// chunk covers (the bits-per-block array is indexed by row).  False where fill_adaptive_table refuses, or a frame's rows are not where the table says.
inline bool transcode_adaptive_table(AdaptFrameTable *t, const TranscodeFrame *f, int n, size_t *span, size_t *ngroups) {
    size_t nb[kEntropyMaxFrames];
    if (n < 1 || n > kEntropyMaxFrames) return false;
    for (int k = 0; k < n; k++) nb[k] = f[k].nblk;
    if (!fill_adaptive_table(t, n, nb, span, ngroups)) return false;
    for (int k = 0; k < n; k++) {
        if (t->rec[k].first_block != f[k].blk0) return false;
        t->rec[k].first_block = f[k].blk0; // (explicit: the reader's plan decides where a frame's rows lie)
    }
    return true;
}

// The default writer's table of a chunk: a record per frame that is NOT skipped, in chunk order, first_block = blk0 - a gap where a skipped frame
// lies.  entry[k]: frame k's record, -1 for a skipped frame; *count: records.  Stream areas back to back, compress_bound() rounded up to 16 each
// (*stream_bytes: their sum).  False where fill_entropy_table refuses (a frame of more than kEntropyMaxGroups groups) or no frame is left.
inline bool transcode_entropy_table(EntropyFrameTable *t, int mode, const TranscodeFrame *f, int n, int *entry, int *count, size_t *stream_bytes, size_t *nparts,
                                    size_t *ngroups, size_t *nplaces) {
    size_t nb[kEntropyMaxFrames], off[kEntropyMaxFrames], cap[kEntropyMaxFrames], blk0[kEntropyMaxFrames];
    int hs[kEntropyMaxFrames], ws[kEntropyMaxFrames], qs[kEntropyMaxFrames];
    if (n < 1 || n > kEntropyMaxFrames) return false;
    int m = 0;
    size_t bytes = 0;
    for (int k = 0; k < n; k++) {
        entry[k] = -1;
        if (f[k].skip) continue;
        const size_t bound = (compress_bound(f[k].h, f[k].w) + 15) / 16 * 16;
        nb[m] = f[k].nblk, off[m] = bytes, cap[m] = (bound - 16) / 4, blk0[m] = f[k].blk0;
        hs[m] = f[k].h, ws[m] = f[k].w, qs[m] = f[k].quality;
        bytes += bound;
        entry[k] = m++;
    }
    *count = m, *stream_bytes = bytes;
    if (m == 0 || !fill_entropy_table(t, mode, m, nb, off, cap, hs, ws, qs, nparts, ngroups, nplaces)) return false;
    for (int j = 0; j < m; j++) t->rec[j].first_block = blk0[j];
    return true;
}

} // namespace tic
