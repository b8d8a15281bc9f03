// tic_host_pipeline.h - the host-side pieces the batch entry points of tic_api.hip share, free of HIP and of the context: the queue between
// the pipeline's threads, the loop that spreads a chunk's frames over a few copy threads, and the three decisions about a caller's buffers
// that are functions of addresses and sizes alone.  tests/native/pipeline_selftest.cpp runs all of it on the CPU, under the thread and the
// address sanitizer.  The plan of a mixed batch (plan_mixed_batch: order, chunks, transform runs, the entropy stage's records) is here too;
// tests/native/batchplan_selftest.cpp sweeps it.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "tic_entropy.h"
#include "tic_entropy_frames.h"

namespace tic {

// A FIFO that can be closed.  pop() blocks while the queue is empty and open; it returns false once the queue is closed AND drained: what
// was pushed before close() is still delivered.  close() wakes every waiting consumer.
template <class T> class ClosableQueue {
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<T> q_;
    bool closed_ = false;

  public:
    void push(T v) {
        {
            std::lock_guard<std::mutex> l(mu_);
            q_.push_back(std::move(v));
        }
        cv_.notify_one();
    }
    void close() {
        {
            std::lock_guard<std::mutex> l(mu_);
            closed_ = true;
        }
        cv_.notify_all();
    }
    bool pop(T &v) {
        std::unique_lock<std::mutex> l(mu_);
        cv_.wait(l, [&] { return closed_ || !q_.empty(); });
        if (q_.empty()) return false;
        v = std::move(q_.front());
        q_.pop_front();
        return true;
    }
};

// fn(k) for k in [0, cnt) on T threads, thread t taking k = t, t + T, ...; on the calling thread when T <= 1.  Every thread started here
// calls bind() first (the caller's thread never does).
template <class Bind, class Fn> void run_strided(int cnt, int T, Bind bind, Fn fn) {
    if (T <= 1) {
        for (int k = 0; k < cnt; k++) fn(k);
        return;
    }
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++)
        th.emplace_back([=]() {
            bind();
            for (int k = t; k < cnt; k += T) fn(k);
        });
    for (auto &x : th) x.join();
}

// [p, p + bytes) widened to whole pages: what a registration of the range covers.
constexpr uintptr_t kPageBytes = 4096;
inline uintptr_t page_floor(uintptr_t a) { return a & ~(kPageBytes - 1); }
inline uintptr_t page_ceil(uintptr_t a) { return (a + kPageBytes - 1) & ~(kPageBytes - 1); }

// The density rule of the in-place registration: `cnt` frames of `frame_bytes` between lo and hi (lowest first byte, highest last byte + 1)
// are registered as one range only if the range, in pages, is mostly frames - at most a quarter more plus 1 MiB (arrays allocated one after
// the other lie 16 bytes to a few pages apart); a range over scattered frames would pin memory that is not theirs.
inline bool range_is_mostly_frames(uintptr_t lo, uintptr_t hi, size_t frame_bytes, size_t cnt) {
    const size_t span = page_ceil(hi) - page_floor(lo), frames = frame_bytes * cnt;
    return span <= frames + frames / 4 + ((size_t)1 << 20);
}

// Are the `cnt` buffers rows of ONE block of memory, fit for 8-byte stores of `row_bytes` (a multiple of 8) each?  Equal positive
// distance P between neighbours, P a multiple of 8, the first buffer 8-byte aligned, P and every capacity at least a row.  *pitch = P.
inline bool rows_of_one_block(uint8_t *const *outs, const size_t *caps, int cnt, size_t row_bytes, size_t *pitch) {
    if (cnt < 2 || outs[1] <= outs[0]) return false;
    const uint8_t *base = outs[0];
    const size_t P = (size_t)(outs[1] - outs[0]);
    if (P % 8 != 0 || (uintptr_t)base % 8 != 0 || P < row_bytes) return false;
    for (int k = 0; k < cnt; k++)
        if (outs[k] != base + (size_t)k * P || caps[k] < row_bytes) return false;
    *pitch = P;
    return true;
}

// A decoded frame as the device buffer holds it and as the caller wants it: `bytes` of pixels at offset `off` of the device buffer (frames
// start at multiples of 256 there), to go to `out`, where the caller gave away `cap` bytes.
struct ArenaFrame {
    const uint8_t *out;
    size_t off, bytes, cap;
};
// May ONE copy of the device buffer, from its start to the last frame's end, land at the first frame's address?  The frames must lie in the
// caller's memory at the device buffer's distances, and the copy - the padding between two frames included - may only cover bytes the
// caller gave away: a frame of a whole number of 256 bytes has no padding behind it, behind any other (but the last) `cap` must reach to
// the next frame.  at(k) gives frame k.
template <class At> bool frames_are_one_arena(size_t n, At at) {
    for (size_t k = 0; k < n; k++) {
        const ArenaFrame f = at(k);
        if (k > 0) {
            const ArenaFrame p = at(k - 1);
            if (f.out != p.out + (f.off - p.off)) return false;
        }
        if (k + 1 < n && f.bytes % 256 != 0 && f.cap < at(k + 1).off - f.off) return false;
    }
    return true;
}

// ---- the plan of a mixed batch (tic_compress_batch_v) ---------------------------------------------------------------------------------------
// Row pitch of staged frames: rows that are already a multiple of 8 bytes are staged back to back (one memcpy per
// frame when the caller's rows are contiguous too); other widths are padded so that 8-byte row loads stay aligned.
inline size_t batch_pitch(int w) { return (w % 8 == 0) ? (size_t)w : ((size_t)w + 255) / 256 * 256; }

constexpr size_t kMixedChunkBytes = (size_t)32 << 20; // staged pixels per chunk
constexpr int kMixedChunkFrames = kEntropyMaxFrames;  // frames per chunk: one launch of the entropy stage's descriptor form

// A frame of the pipeline, in plan order.  The offsets count inside the frame's chunk: pixels (staged at `pitch`), coefficients and stream areas
// of a chunk's frames lie back to back in the slot's buffers, in chunk order.
struct MixedFrame {
    int index;                  // the caller's index
    int h, w, quality;
    size_t nblk, pitch, img_bytes; // img_bytes = pitch * h, a multiple of 8
    size_t bound;               // bytes of the frame's stream area: compress_bound(h, w) (+ the plan's stream_extra) rounded up to 16
    size_t img_off, first_block, stream_off;
};
// A maximal run of neighbours the transform takes in ONE launch, as one tall frame: equal width and quality, every height a multiple of 8
// (frames staged back to back at one pitch, ending on a block row - merge_frames' condition without equal heights).  A frame whose height
// is no multiple of 8 is a run of its own.
struct MixedRun {
    int first, count;           // frames [first, first + count) of the plan's order
    int h_total;                // rows of the tall frame
};
struct MixedChunk {
    int first, count;           // frames [first, first + count) of the plan's order
    size_t img_bytes, nblk, stream_bytes; // totals
    std::vector<MixedRun> runs;
};
struct MixedPlan {
    std::vector<int> empty;     // caller's indices of frames without blocks: a header-only stream from the host
    std::vector<int> single;    // ... of frames the batch kernels do not take (more than kEntropyMaxGroups groups, or more pixels than a chunk holds): coded alone
    std::vector<MixedFrame> frames; // the rest, ordered by (quality, width, height), stable
    std::vector<MixedChunk> chunks;
    size_t max_img = 0, max_nblk = 0, max_stream = 0; // what a slot must hold: the largest chunk's totals
    int max_count = 0;
};

// chunk_frames: frames per chunk (1..kMixedChunkFrames; anything else: kMixedChunkFrames); chunk_bytes: staged pixels per chunk.  A frame of
// more than chunk_bytes goes to `single`.  stream_extra: bytes a stream may have beyond compress_bound() (1 for the scaled form's flush byte:
// where the bound is a multiple of 16 the rounding alone leaves no room for it).
inline MixedPlan plan_mixed_batch(const int *hs, const int *ws, const int *qs, int n, int chunk_frames, size_t chunk_bytes, size_t stream_extra = 0) {
    MixedPlan p;
    if (chunk_frames < 1 || chunk_frames > kMixedChunkFrames) chunk_frames = kMixedChunkFrames;
    const EntropyGeom g8 = entropy_geom(kEntropyEightLanes); // (the mode with more groups per block)
    for (int i = 0; i < n; i++) {
        MixedFrame f;
        f.index = i, f.h = hs[i], f.w = ws[i], f.quality = qs[i];
        f.nblk = num_blocks(f.h, f.w);
        if (f.nblk == 0) {
            p.empty.push_back(i);
            continue;
        }
        f.pitch = batch_pitch(f.w), f.img_bytes = f.pitch * (size_t)f.h;
        f.bound = (compress_bound(f.h, f.w) + stream_extra + 15) / 16 * 16;
        f.img_off = f.first_block = f.stream_off = 0;
        const size_t parts = (f.nblk + g8.part_blocks - 1) / g8.part_blocks, groups = (parts + g8.group_parts - 1) / g8.group_parts;
        if (groups > kEntropyMaxGroups || f.img_bytes > chunk_bytes) {
            p.single.push_back(i);
            continue;
        }
        p.frames.push_back(f);
    }
    std::stable_sort(p.frames.begin(), p.frames.end(), [](const MixedFrame &a, const MixedFrame &b) {
        if (a.quality != b.quality) return a.quality < b.quality;
        if (a.w != b.w) return a.w < b.w;
        return a.h < b.h;
    });
    const int m = (int)p.frames.size();
    for (int first = 0; first < m;) {
        MixedChunk c;
        c.first = first, c.count = 0, c.img_bytes = c.nblk = c.stream_bytes = 0;
        while (first + c.count < m && c.count < chunk_frames) {
            MixedFrame &f = p.frames[(size_t)(first + c.count)];
            if (c.count > 0 && c.img_bytes + f.img_bytes > chunk_bytes) break;
            f.img_off = c.img_bytes, f.first_block = c.nblk, f.stream_off = c.stream_bytes;
            c.img_bytes += f.img_bytes, c.nblk += f.nblk, c.stream_bytes += f.bound;
            c.count++;
        }
        for (int k = 0; k < c.count;) {
            const MixedFrame &a = p.frames[(size_t)(first + k)];
            MixedRun r = {first + k, 1, a.h};
            while (a.h % 8 == 0 && k + r.count < c.count) {
                const MixedFrame &b = p.frames[(size_t)(first + k + r.count)];
                if (b.w != a.w || b.quality != a.quality || b.h % 8 != 0) break;
                r.h_total += b.h;
                r.count++;
            }
            c.runs.push_back(r);
            k += r.count;
        }
        p.max_img = std::max(p.max_img, c.img_bytes), p.max_nblk = std::max(p.max_nblk, c.nblk);
        p.max_stream = std::max(p.max_stream, c.stream_bytes), p.max_count = std::max(p.max_count, c.count);
        first += c.count;
        p.chunks.push_back(std::move(c));
    }
    return p;
}

// The entropy stage's table of chunk `c` for a packing mode.  *nparts, *ngroups, *nplaces: the launch's totals.
inline bool mixed_chunk_table(const MixedPlan &p, const MixedChunk &c, int mode, EntropyFrameTable *t, size_t *nparts, size_t *ngroups, size_t *nplaces) {
    size_t nblk[kEntropyMaxFrames], off[kEntropyMaxFrames], cap[kEntropyMaxFrames];
    int hs[kEntropyMaxFrames], ws[kEntropyMaxFrames], qs[kEntropyMaxFrames];
    if (c.count < 1 || c.count > kEntropyMaxFrames) return false;
    for (int k = 0; k < c.count; k++) {
        const MixedFrame &f = p.frames[(size_t)(c.first + k)];
        nblk[k] = f.nblk, off[k] = f.stream_off, cap[k] = (f.bound - 16) / 4;
        hs[k] = f.h, ws[k] = f.w, qs[k] = f.quality;
    }
    return fill_entropy_table(t, mode, c.count, nblk, off, cap, hs, ws, qs, nparts, ngroups, nplaces);
}

} // namespace tic
