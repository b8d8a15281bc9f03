// adaptplan_selftest - the host plan of the adaptive batch encoder (tinyimgcodec_amd/csrc/tic_adaptive_frames.h: adaptive_chunk_table,
// assign_adaptive_streams, adaptive_slot_layout, on top of plan_mixed_batch) on the CPU.  tests/test_adaptive_batch_cpu.py builds it with
// the address and undefined-behaviour sanitizers (with tic_entropy.cpp for num_blocks / compress_bound) and runs it.
//   adaptplan_selftest   -> "adaptplan_selftest ok: <n> plans", exit 0; the first failed check is printed, exit 1
// For the fixture's frame list, the 294 frames of the benchmark loop and a few hundred random lists, at several chunk limits, it checks that
//   - every frame appears exactly once: alone behind the batch, or in exactly one chunk (none is empty here: the entry refuses those);
//   - a chunk's records tile its coefficients, and their workgroups tile the grid without gap or overlap;
//   - no workgroup spans two frames: a frame's workgroups are its blocks in 256s, rounded up, and every workgroup index finds - by the
//     kernels' rule: the last frame whose first workgroup is not behind it - the frame it belongs to, with its blocks inside that frame;
//   - entries behind the last frame are 0xffffffff;
//   - stream areas assigned from (random) exact lengths sit at multiples of 16, hold their stream's words, do not overlap and sum to the
//     reported total; an unpacked frame is marked and takes no room;
//   - the statistics, table and header records and the per-block and per-workgroup arrays tile a slot's buffer in order, every piece
//     holding what its count needs, and a larger chunk never carves less (the slots are sized for the largest).
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../tinyimgcodec_amd/csrc/tic_adaptive_frames.h"

using namespace tic;

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            printf("adaptplan_selftest FAILED: %s (line %d)\n", #cond, __LINE__);      \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

static int plans = 0;
static std::mt19937_64 rng(20261019);

// The kernels' find_frame: the number of entries <= idx, minus one.
static int find_frame(const uint32_t *first, uint32_t idx) {
    int c = 0;
    for (int l = 0; l < kEntropyMaxFrames; l++) c += first[l] <= idx;
    return c - 1;
}

static void check_layout(size_t count, size_t nblk, size_t ngroups) {
    const AdaptSlotLayout l = adaptive_slot_layout(count, nblk, ngroups);
    const size_t at[] = {l.stats, l.err, l.rb_frames, l.frames, l.tabs, l.heads, l.upload_end, l.gsum, l.end};
    const size_t need[] = {count * sizeof(AdaptStats), 4, sizeof(EntropyFrameTable), sizeof(AdaptFrameTable), count * sizeof(HuffWide),
                           count * kAdaptHeadStride, nblk * 4, ngroups * 8};
    CHECK(l.stats == 0 && l.bbits == l.upload_end);
    for (int i = 0; i < 8; i++) CHECK(at[i] % 256 == 0 && at[i] + need[i] <= at[i + 1]);
    const AdaptSlotLayout m = adaptive_slot_layout(count + 1, nblk + 7, ngroups + 1);
    CHECK(m.upload_end >= l.upload_end && m.end >= l.end);
}

static void check_plan(const std::vector<int> &hs, const std::vector<int> &ws, const std::vector<int> &qs, int chunk_frames, size_t chunk_bytes) {
    const int n = (int)hs.size();
    const MixedPlan p = plan_mixed_batch(hs.data(), ws.data(), qs.data(), n, chunk_frames, chunk_bytes);
    std::vector<int> seen((size_t)n, 0);
    CHECK(p.empty.empty());
    for (int i : p.single) seen[(size_t)i]++;
    size_t max_groups = 0;
    for (const MixedChunk &c : p.chunks) {
        AdaptFrameTable t;
        size_t nblk = 0, ngroups = 0;
        CHECK(adaptive_chunk_table(p, c, &t, &nblk, &ngroups));
        CHECK(nblk == c.nblk);
        size_t blk = 0, grp = 0;
        for (int k = 0; k < kEntropyMaxFrames; k++) {
            const AdaptFrameRec &r = t.rec[k];
            if (k >= c.count) {
                CHECK(t.first_group[k] == 0xffffffffu && r.nblocks == 0);
                continue;
            }
            const MixedFrame &f = p.frames[(size_t)(c.first + k)];
            seen[(size_t)f.index]++;
            CHECK(r.first_block == blk && r.first_block == f.first_block && r.nblocks == f.nblk && r.nblocks >= 1);
            CHECK(r.first_group == grp && t.first_group[k] == grp && r.ngroups == (r.nblocks + kAdaptGroupBlocks - 1) / kAdaptGroupBlocks && r.ngroups >= 1);
            CHECK(r.out_off == 0 && r.out_words == 0 && r.base_bits == 0 && r.skip == 0);
            blk += r.nblocks, grp += r.ngroups;
        }
        CHECK(blk == nblk && grp == ngroups);
        CHECK(ngroups <= p.max_nblk / kAdaptGroupBlocks + (size_t)p.max_count); // (what ensure_adapt_slots sizes the slots for)
        max_groups = std::max(max_groups, ngroups);
        // every workgroup finds its frame, and its blocks lie inside it
        std::vector<int> owner(nblk, -1);
        for (size_t g = 0; g < ngroups; g++) {
            const int f = find_frame(t.first_group, (uint32_t)g);
            CHECK(f >= 0 && f < c.count);
            const AdaptFrameRec &r = t.rec[f];
            CHECK(g >= r.first_group && g < (size_t)r.first_group + r.ngroups);
            const size_t b0 = (g - r.first_group) * kAdaptGroupBlocks;
            CHECK(b0 < r.nblocks);
            for (size_t b = b0; b < std::min<size_t>(b0 + kAdaptGroupBlocks, r.nblocks); b++) {
                CHECK(owner[r.first_block + b] == -1);
                owner[r.first_block + b] = f;
            }
        }
        for (size_t b = 0; b < nblk; b++) CHECK(owner[b] >= 0);
        // stream areas from exact lengths (here: random ones; a few frames unpacked)
        unsigned long long total[kEntropyMaxFrames];
        uint32_t base[kEntropyMaxFrames];
        for (int k = 0; k < c.count; k++) {
            base[k] = 128 + 32 + (uint32_t)(rng() % 20000);
            total[k] = rng() % 7 == 0 ? 0ull : base[k] + rng() % (t.rec[k].nblocks * 520 * 8);
        }
        size_t stream_bytes = 0, off = 0;
        assign_adaptive_streams(&t, c.count, total, base, &stream_bytes);
        for (int k = 0; k < c.count; k++) {
            const AdaptFrameRec &r = t.rec[k];
            CHECK(r.out_off % 16 == 0 && r.out_off == off);
            CHECK(r.skip == (total[k] == 0) && r.out_words * 32 >= total[k] && r.out_words * 32 < total[k] + 32);
            CHECK(r.skip ? r.out_words == 0 : r.base_bits == base[k]);
            off += (r.out_words * 4 + 15) / 16 * 16;
            CHECK(r.first_block == p.frames[(size_t)(c.first + k)].first_block && t.first_group[k] == r.first_group); // (the layout part is kept)
        }
        CHECK(off == stream_bytes);
        check_layout((size_t)c.count, nblk, ngroups);
    }
    for (int i = 0; i < n; i++) CHECK(seen[(size_t)i] == 1);
    if (!p.chunks.empty()) check_layout((size_t)p.max_count, p.max_nblk, max_groups);
    plans++;
}

int main() {
    const int limits[] = {0, 1, 2, 3, 7, 64};
    const size_t bytes[] = {kMixedChunkBytes, (size_t)1 << 20, 40000, 4096};
    { // the fixture's frames
        const std::vector<int> hs = {1, 8, 8, 13, 8, 8, 8, 7, 32, 64, 64}, ws = {1, 8, 8, 21, 2040, 2048, 2056, 4100, 32, 64, 64},
                               qs = {50, 50, 50, 75, 50, 90, 5, 20, 50, 50, 97};
        for (int l : limits)
            for (size_t b : bytes) check_plan(hs, ws, qs, l, b);
    }
    { // the benchmark loop: 49 images of 512 x 512 at six qualities
        std::vector<int> hs, ws, qs;
        for (int i = 0; i < 49; i++)
            for (int q : {90, 80, 50, 20, 10, 5}) hs.push_back(512), ws.push_back(512), qs.push_back(q);
        for (int l : {0, 3, 64})
            for (size_t b : {kMixedChunkBytes, (size_t)4 << 20, (size_t)300000}) check_plan(hs, ws, qs, l, b);
    }
    for (int it = 0; it < 300; it++) {
        const int n = 1 + (int)(rng() % 90);
        std::vector<int> hs, ws, qs;
        for (int i = 0; i < n; i++) {
            const bool wide = rng() % 8 == 0;
            hs.push_back(1 + (int)(rng() % (wide ? 16 : 200)));
            ws.push_back(1 + (int)(rng() % (wide ? 5000 : 300)));
            qs.push_back(1 + (int)(rng() % 99));
        }
        check_plan(hs, ws, qs, limits[rng() % 6], bytes[rng() % 4]);
    }
    { // the table refuses what it cannot hold
        AdaptFrameTable t;
        size_t nb[kEntropyMaxFrames + 1], a, b;
        for (size_t &x : nb) x = 1;
        CHECK(!fill_adaptive_table(&t, 0, nb, &a, &b) && !fill_adaptive_table(&t, kEntropyMaxFrames + 1, nb, &a, &b));
        CHECK(fill_adaptive_table(&t, kEntropyMaxFrames, nb, &a, &b) && a == (size_t)kEntropyMaxFrames && b == (size_t)kEntropyMaxFrames);
        nb[3] = 0;
        CHECK(!fill_adaptive_table(&t, 5, nb, &a, &b));
    }
    printf("adaptplan_selftest ok: %d plans\n", plans);
    return 0;
}
