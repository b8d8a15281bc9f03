// batchplan_selftest - the plan of a mixed batch (tinyimgcodec_amd/csrc/tic_host_pipeline.h: plan_mixed_batch, mixed_chunk_table) on the CPU.
// tests/test_compress_batch_mixed_cpu.py builds it with the address and undefined-behaviour sanitizers (with tic_entropy.cpp for
// num_blocks / compress_bound) and runs it.
//   batchplan_selftest   -> "batchplan_selftest ok: <n> plans", exit 0; the first failed check is printed, exit 1
// For the frame list of the GPU test and for random lists, at several chunk limits and both packing modes, it checks that
//   - every caller's index appears exactly once: in `empty`, in `single`, or in exactly one chunk;
//   - the order is (quality, width, height), stable, and the chunks respect their frame and byte limits;
//   - pixels, coefficients and stream areas of a chunk tile their buffers without gap or overlap, every stream area holds
//     compress_bound(h, w) and starts on a multiple of 16;
//   - the runs tile the chunk, a run's frames share width and quality and have heights that are multiples of 8 (or the run is one frame),
//     its rows are the sum of its frames' rows, and no two neighbouring runs could have been one;
//   - the entropy stage's records tile the coefficient buffer and the packing and placing grids without gap or overlap, in both modes.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../tinyimgcodec_amd/csrc/tic_host_pipeline.h"

using namespace tic;

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            printf("batchplan_selftest FAILED: %s (line %d)\n", #cond, __LINE__);      \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

static int plans = 0;

static void check_plan(const std::vector<int> &hs, const std::vector<int> &ws, const std::vector<int> &qs, int chunk_frames, size_t chunk_bytes) {
    const int n = (int)hs.size();
    const MixedPlan p = plan_mixed_batch(hs.data(), ws.data(), qs.data(), n, chunk_frames, chunk_bytes);
    const int limit = (chunk_frames >= 1 && chunk_frames <= kMixedChunkFrames) ? chunk_frames : kMixedChunkFrames;
    std::vector<int> seen((size_t)n, 0);
    for (int i : p.empty) {
        CHECK(i >= 0 && i < n && num_blocks(hs[(size_t)i], ws[(size_t)i]) == 0);
        seen[(size_t)i]++;
    }
    for (int i : p.single) {
        CHECK(i >= 0 && i < n);
        const size_t nblk = num_blocks(hs[(size_t)i], ws[(size_t)i]);
        CHECK(nblk > 0 && (batch_pitch(ws[(size_t)i]) * (size_t)hs[(size_t)i] > chunk_bytes || (nblk + 127) / 128 > kEntropyMaxGroups));
        seen[(size_t)i]++;
    }
    for (size_t k = 0; k < p.frames.size(); k++) {
        const MixedFrame &f = p.frames[k];
        CHECK(f.index >= 0 && f.index < n && f.h == hs[(size_t)f.index] && f.w == ws[(size_t)f.index] && f.quality == qs[(size_t)f.index]);
        CHECK(f.nblk == num_blocks(f.h, f.w) && f.nblk > 0 && f.pitch >= (size_t)f.w && f.pitch % 8 == 0 && f.img_bytes == f.pitch * (size_t)f.h);
        CHECK(f.bound >= compress_bound(f.h, f.w) && f.bound % 16 == 0 && f.img_bytes <= chunk_bytes);
        if (k > 0) { // (quality, width, height), and the caller's order among equals
            const MixedFrame &a = p.frames[k - 1];
            CHECK(a.quality < f.quality || (a.quality == f.quality && (a.w < f.w || (a.w == f.w && (a.h < f.h || (a.h == f.h && a.index < f.index))))));
        }
    }
    size_t next = 0, max_img = 0, max_nblk = 0, max_stream = 0;
    int max_count = 0;
    for (size_t ci = 0; ci < p.chunks.size(); ci++) {
        const MixedChunk &c = p.chunks[ci];
        CHECK((size_t)c.first == next && c.count >= 1 && c.count <= limit);
        size_t img = 0, blk = 0, str = 0;
        for (int k = 0; k < c.count; k++) {
            const MixedFrame &f = p.frames[(size_t)(c.first + k)];
            CHECK(f.img_off == img && f.first_block == blk && f.stream_off == str && f.stream_off % 16 == 0 && f.img_off % 8 == 0);
            img += f.img_bytes, blk += f.nblk, str += f.bound;
            seen[(size_t)f.index]++;
        }
        CHECK(c.img_bytes == img && c.nblk == blk && c.stream_bytes == str);
        CHECK(c.count == 1 || img <= chunk_bytes);
        if (ci + 1 < p.chunks.size()) // the chunk was closed for a reason: full, or the next frame would not fit
            CHECK(c.count == limit || img + p.frames[(size_t)(c.first + c.count)].img_bytes > chunk_bytes);
        // runs
        int at = c.first;
        for (size_t r = 0; r < c.runs.size(); r++) {
            const MixedRun &run = c.runs[r];
            CHECK(run.first == at && run.count >= 1);
            const MixedFrame &a = p.frames[(size_t)run.first];
            int rows = 0;
            for (int k = 0; k < run.count; k++) {
                const MixedFrame &f = p.frames[(size_t)(run.first + k)];
                CHECK(f.w == a.w && f.quality == a.quality && (run.count == 1 || f.h % 8 == 0));
                CHECK(f.img_off == a.img_off + (size_t)rows * a.pitch && f.first_block == a.first_block + (size_t)(rows / 8) * ((size_t)(a.w + 7) / 8));
                rows += f.h;
            }
            CHECK(rows == run.h_total);
            at += run.count;
            if (r + 1 < c.runs.size()) { // maximal
                const MixedFrame &l = p.frames[(size_t)(at - 1)], &nx = p.frames[(size_t)at];
                CHECK(!(l.w == nx.w && l.quality == nx.quality && l.h % 8 == 0 && nx.h % 8 == 0));
            }
        }
        CHECK(at == c.first + c.count);
        // records, both modes
        for (int mode : {kEntropyLanePerBlock, kEntropyEightLanes}) {
            EntropyFrameTable t;
            size_t nparts = 0, ngroups = 0, nplaces = 0;
            CHECK(mixed_chunk_table(p, c, mode, &t, &nparts, &ngroups, &nplaces));
            const EntropyGeom g = entropy_geom(mode);
            size_t b = 0, pa = 0, gr = 0, pl = 0;
            for (int k = 0; k < kEntropyMaxFrames; k++) {
                if (k >= c.count) {
                    CHECK(t.first_group[k] == 0xffffffffu && t.first_place[k] == 0xffffffffu);
                    continue;
                }
                const MixedFrame &f = p.frames[(size_t)(c.first + k)];
                const EntropyFrameRec &r = t.rec[k];
                CHECK(r.first_block == b && r.nblocks == f.nblk && r.first_part == pa && r.first_group == gr && r.first_place == pl);
                CHECK(t.first_group[k] == gr && t.first_place[k] == pl);
                CHECK(r.out_off == f.stream_off && 16 + 4 * r.cap_words <= f.bound && 16 + 4 * r.cap_words + 4 > compress_bound(f.h, f.w) - 4);
                CHECK(r.h == f.h && r.w == f.w && r.quality == f.quality);
                const size_t parts = (f.nblk + g.part_blocks - 1) / g.part_blocks;
                CHECK(parts * g.part_blocks >= f.nblk && (parts - 1) * g.part_blocks < f.nblk);
                b += f.nblk, pa += parts, gr += (parts + g.group_parts - 1) / g.group_parts, pl += (parts + g.place_parts - 1) / g.place_parts;
                CHECK((parts + g.group_parts - 1) / g.group_parts <= kEntropyMaxGroups);
            }
            CHECK(b == c.nblk && pa == nparts && gr == ngroups && pl == nplaces);
        }
        max_img = std::max(max_img, img), max_nblk = std::max(max_nblk, blk), max_stream = std::max(max_stream, str), max_count = std::max(max_count, c.count);
        next += (size_t)c.count;
    }
    CHECK(next == p.frames.size());
    CHECK(p.max_img == max_img && p.max_nblk == max_nblk && p.max_stream == max_stream && p.max_count == max_count);
    for (int i = 0; i < n; i++) CHECK(seen[(size_t)i] == 1);
    plans++;
}

int main() {
    // the frame list of tests/test_compress_batch_mixed_gpu.py, in three orders
    const std::vector<int> H = {1, 8, 7, 15, 40, 64, 72, 128, 200, 512}, W = {1, 8, 9, 17, 52, 64, 40, 136, 264, 512};
    const std::vector<int> Q = {50, 5, 90, 10, 99, 50, 5, 90, 10, 99};
    for (int chunk : {0, 1, 3, 64, 65})
        for (size_t bytes : {(size_t)1, (size_t)4096, (size_t)100000, kMixedChunkBytes}) {
            check_plan(H, W, Q, chunk, bytes);
            check_plan(std::vector<int>(H.rbegin(), H.rend()), std::vector<int>(W.rbegin(), W.rend()), std::vector<int>(Q.rbegin(), Q.rend()), chunk, bytes);
        }
    {   // two runs that merge: 40 x 52 and 72 x 52 at one quality, 64 x 64 twice
        const MixedPlan p = plan_mixed_batch(std::vector<int>{40, 64, 72, 64, 7}.data(), std::vector<int>{52, 64, 52, 64, 52}.data(),
                                             std::vector<int>{50, 50, 50, 50, 50}.data(), 5, 0, kMixedChunkBytes);
        CHECK(p.chunks.size() == 1 && p.chunks[0].runs.size() == 3); // (7 x 52 alone, 40 + 72 rows of 52, 64 + 64 rows of 64)
        CHECK(p.chunks[0].runs[0].count == 1 && p.chunks[0].runs[1].h_total == 112 && p.chunks[0].runs[2].h_total == 128);
    }
    {   // the reference's benchmark loop: 49 images x 6 qualities -> 5 chunks of at most 64, at most chunks + 5 launches
        std::vector<int> h, w, q;
        for (int i = 0; i < 49; i++)
            for (int qq : {10, 25, 50, 75, 90, 95}) h.push_back(512), w.push_back(512), q.push_back(qq);
        const MixedPlan p = plan_mixed_batch(h.data(), w.data(), q.data(), 294, 0, kMixedChunkBytes);
        size_t runs = 0;
        for (const MixedChunk &c : p.chunks) runs += c.runs.size();
        CHECK(p.chunks.size() == 5 && runs <= p.chunks.size() + 5 && p.single.empty() && p.empty.empty());
        check_plan(h, w, q, 0, kMixedChunkBytes);
    }
    // frames without blocks, a frame beyond the byte budget, a frame beyond 8,192 groups (sizes only: nothing is allocated)
    check_plan({0, 16, 8, 1024, 8}, {16, 0, 8, 1024, 8}, {50, 50, 50, 50, 50}, 1, 524288);
    check_plan({8, 8200, 8}, {8, 8200, 8}, {50, 50, 50}, 0, (size_t)1 << 40);
    {
        const MixedPlan p = plan_mixed_batch(std::vector<int>{8, 8200, 0}.data(), std::vector<int>{8, 8200, 5}.data(), std::vector<int>{1, 2, 3}.data(), 3, 0, (size_t)1 << 40);
        CHECK(p.single.size() == 1 && p.single[0] == 1 && p.empty.size() == 1 && p.empty[0] == 2 && p.frames.size() == 1);
    }
    check_plan({}, {}, {}, 0, kMixedChunkBytes);
    // random lists
    std::mt19937 rng(20240607);
    for (int t = 0; t < 300; t++) {
        const int n = (int)(rng() % 200);
        std::vector<int> h((size_t)n), w((size_t)n), q((size_t)n);
        for (int i = 0; i < n; i++) {
            const unsigned kind = rng() % 8;
            h[(size_t)i] = kind == 0 ? (int)(rng() % 3) : kind < 4 ? (int)(8 * (1 + rng() % 40)) : (int)(1 + rng() % 700);
            w[(size_t)i] = kind == 1 ? 0 : kind < 5 ? (int)(8 * (1 + rng() % 6)) : (int)(1 + rng() % 700);
            q[(size_t)i] = (int)(1 + rng() % (t % 3 == 0 ? 3 : 99));
        }
        const int chunks[] = {0, 1, 2, 7, 64};
        const size_t bytes[] = {kMixedChunkBytes, (size_t)1 << 16, (size_t)1 << 12, (size_t)300000};
        check_plan(h, w, q, chunks[rng() % 5], bytes[rng() % 4]);
    }
    printf("batchplan_selftest ok: %d plans\n", plans);
    return 0;
}
