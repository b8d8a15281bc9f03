// decplan_selftest - the plan of tic_decompress_batch (tinyimgcodec_amd/csrc/tic_decode_plan.h: the functions the library itself calls) on
// the CPU: seeded batches of 0 .. 1,100 frames of mixed geometries and stream lengths, under the production limits and under small ones, every
// plan checked against definitions written out naively here.  Host only: no HIP header, no device.  Built with tic_entropy.cpp (num_blocks).
//
//   decplan_selftest               the header's cut                                         -> "decplan_selftest ok", exit 0
//   decplan_selftest --break-cut   a wrong cut: the limits tested AFTER the frame joined    -> counts its counterexamples, exit 1
//
// The second form is what shows that the sweep can fail.
#define TIC_DEC_WORKSPACE_ONLY
#include "../../tinyimgcodec_amd/csrc/tic_decode_plan.h"

#include <stdio.h>
#include <string.h>

#include <vector>

using namespace tic;

namespace {

struct Rng { // xorshift64*: the same cases on every run
    unsigned long long s;
    unsigned long long next() {
        s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
        return s * 2685821657736338717ull;
    }
    size_t in(size_t lo, size_t hi) { return lo + (size_t)(next() % (unsigned long long)(hi - lo + 1)); } // [lo, hi]
};

// ---- the definitions, naively
size_t naive_pitch(int w) { return (size_t)(w % 8 == 0 ? w : (w + 7) / 8 * 8); }
size_t naive_nblk(int h, int w) { return h <= 0 || w <= 0 ? 0 : (size_t)((h + 7) / 8) * (size_t)((w + 7) / 8); }
size_t naive_sb(size_t len) { return (len + 15) / 16 * 16 + 16; }
size_t naive_pb(const DecPlanIn &f) { return (naive_pitch(f.w) * (size_t)f.h + 255) / 256 * 256; }

// The wrong cut of --break-cut: a frame joins first, and the chunk ends when it HAS passed a limit.
DecPlan broken_plan(const DecPlanIn *in, int n, const DecPlanLimits &lim) {
    DecPlan p;
    int first = 0, count = 0;
    size_t in_bytes = 0, pix_bytes = 0;
    for (int i = 0; i < n; i++) {
        if (!in[i].takes) continue;
        p.frames.push_back(dec_plan_frame(i, in[i]));
        count++, in_bytes += naive_sb(in[i].len), pix_bytes += naive_pb(in[i]);
        if (in_bytes > lim.stream_bytes || pix_bytes > lim.pix_bytes || count >= lim.frames) {
            dec_plan_close_chunk(p, first, count);
            first += count, count = 0, in_bytes = pix_bytes = 0;
        }
    }
    if (count > 0) dec_plan_close_chunk(p, first, count);
    return p;
}

struct Tally {
    unsigned long long plans = 0, chunks = 0, frames = 0, bad = 0;
    int shown = 0;
    int n = 0; // the batch under test
    DecPlanLimits lim{};
    void fail(const char *what, size_t chunk, size_t frame) {
        if (bad++ == 0 || shown < 8) {
            printf("  counterexample: %s (batch of %d, limits %zu / %zu / %d, chunk %zu, frame %zu)\n", what, n, lim.stream_bytes, lim.pix_bytes, lim.frames, chunk, frame);
            shown++;
        }
    }
};
#define CHECK(cond, what, ci, k) \
    do {                         \
        if (!(cond)) t.fail(what, ci, k); \
    } while (0)

void check_plan(Tally &t, const DecPlanIn *in, int n, const DecPlanLimits &lim, const DecPlan &p, Rng &rng) {
    t.plans++, t.n = n, t.lim = lim;
    // 1. coverage and order: the plan's frames are the frames taken, each once, ascending; the chunks tile them in order
    std::vector<int> taken;
    for (int i = 0; i < n; i++)
        if (in[i].takes) taken.push_back(i);
    CHECK(p.frames.size() == taken.size(), "as many frames as are taken", 0, 0);
    if (p.frames.size() != taken.size()) return;
    for (size_t k = 0; k < taken.size(); k++) CHECK(p.frames[k].index == taken[k], "frames in the caller's order, none twice, none untaken", 0, k);
    size_t next = 0;
    for (size_t ci = 0; ci < p.chunks.size(); ci++) {
        CHECK((size_t)p.chunks[ci].first == next && p.chunks[ci].count >= 1, "chunks follow each other, none empty", ci, next);
        if ((size_t)p.chunks[ci].first != next || p.chunks[ci].count < 1) return;
        next += (size_t)p.chunks[ci].count;
    }
    CHECK(next == p.frames.size(), "the chunks hold every frame", p.chunks.size(), next);
    if (next != p.frames.size()) return;
    for (size_t ci = 0; ci < p.chunks.size(); ci++) {
        const DecPlanChunk &c = p.chunks[ci];
        const DecPlanFrame *pf = &p.frames[(size_t)c.first];
        const size_t F = (size_t)c.count;
        t.chunks++, t.frames += F;
        // 2. the limits: passed only by a single frame; the next frame would pass one
        size_t sb = 0, pb = 0;
        for (size_t k = 0; k < F; k++) sb += naive_sb(in[pf[k].index].len), pb += naive_pb(in[pf[k].index]);
        CHECK(c.count <= lim.frames, "no more frames than the limit", ci, F);
        CHECK(F == 1 || (sb <= lim.stream_bytes && pb <= lim.pix_bytes), "only a single frame passes a byte limit", ci, F);
        if (ci + 1 < p.chunks.size()) {
            const DecPlanIn &nx = in[pf[F].index];
            CHECK(sb + naive_sb(nx.len) > lim.stream_bytes || pb + naive_pb(nx) > lim.pix_bytes || c.count >= lim.frames, "the next frame would pass a limit", ci, F);
        }
        // 3. alignment and overlap of the stream and pixel regions; 4. the chunk's values
        size_t words = 0, pix = 0, blocks = 0, r288 = 0, ranges = 0;
        int range_bits = 0;
        bool small_win = true;
        for (size_t k = 0; k < F; k++) {
            const DecPlanIn &f = in[pf[k].index];
            const int rb = dec_range_rule(f.len, naive_nblk(f.h, f.w));
            range_bits = rb > range_bits ? rb : range_bits;
            small_win = small_win && f.len * 8 / naive_nblk(f.h, f.w) <= 240;
        }
        CHECK(c.range_bits == range_bits && dec_range_ok(c.range_bits), "range_bits is the largest of the frames' rules, and legal", ci, 0);
        CHECK(c.small_win == small_win, "small_win", ci, 0);
        for (size_t k = 0; k < F; k++) {
            const DecPlanFrame &g = pf[k];
            const DecPlanIn &f = in[g.index];
            CHECK(g.h == f.h && g.w == f.w && g.quality == f.quality && g.len == f.len, "the frame's own figures", ci, k);
            CHECK(g.nblk == naive_nblk(f.h, f.w) && g.nblk > 0 && g.pitch == naive_pitch(f.w) && g.pitch % 8 == 0 && g.pitch >= (size_t)f.w, "nblk and pitch", ci, k);
            CHECK((size_t)g.word0 * 4 % 16 == 0 && g.word0 == words, "word0: 16-byte aligned, behind the stream in front", ci, k);
            CHECK((size_t)g.nwords * 4 >= f.len && (size_t)g.nwords * 4 < f.len + 4 && g.stream_bits == f.len * 8, "nwords and stream_bits", ci, k);
            CHECK(g.last_mask == (f.len % 4 == 0 ? 0xffffffffu : f.len % 4 == 1 ? 0xff000000u : f.len % 4 == 2 ? 0xffff0000u : 0xffffff00u), "last_mask", ci, k);
            CHECK(g.pix_off % 256 == 0 && g.pix_off == pix, "pix_off: 256-byte aligned, behind the frame in front", ci, k);
            CHECK(g.blk0 == blocks && g.range0 == ranges && g.nranges == dec_ranges_of(8 * f.len, range_bits), "blk0, range0, nranges", ci, k);
            words += naive_sb(f.len) / 4, pix += naive_pb(f), blocks += g.nblk, ranges += dec_ranges_of(8 * f.len, range_bits);
            r288 += f.len * 8 / 288 + 2;
            CHECK((size_t)g.word0 * 4 + f.len + 16 <= words * 4 && g.pix_off + g.pitch * (size_t)g.h <= pix, "a region ends in front of its neighbour", ci, k);
        }
        CHECK(c.words == words && c.pix_bytes == pix && c.blocks == blocks && c.ranges == ranges && c.ranges288 == r288, "the chunk's totals", ci, F);
        CHECK(words * 4 == sb && pix == pb && words * 4 < (1ull << 32), "the last region ends at the totals", ci, F);
        // 5. the work buffer: what is provided from the plan's figures covers what the launcher carves at the plan's range
        CHECK(dec_work_provision_bytes(F, c.ranges288, c.blocks) >= dec_work_carve_bytes(F, ranges, c.blocks, c.range_bits), "the work buffer's provision covers the carve-up", ci, F);
        // 6. the upload buffer: tiles and workgroups are the launchers' figures (any number here)
        const size_t tiles = rng.in(1, 2 * ranges + 1), wgs = rng.in(1, blocks);
        const DecUploadLayout up(F, tiles, wgs, c.words);
        CHECK(up.o_frames == 0 && up.o_frames < up.o_tiles && up.o_tiles < up.o_wgs && up.o_wgs < up.o_streams && up.o_streams < up.up_bytes, "upload offsets ascend", ci, F);
        CHECK((up.o_tiles | up.o_wgs | up.o_streams) % 256 == 0, "upload offsets are 256-byte aligned", ci, F);
        CHECK(up.o_frames + F * sizeof(DecFrame) <= up.o_tiles && up.o_tiles + tiles * 4 <= up.o_wgs && up.o_wgs + wgs * 4 <= up.o_streams &&
                  up.o_streams + c.words * 4 == up.up_bytes, "every upload piece fits in front of the next", ci, F);
        CHECK(up.up_bytes <= F * sizeof(DecFrame) + tiles * 4 + wgs * 4 + c.words * 4 + 3 * 255, "no more padding than the alignment asks for", ci, F);
    }
}

// ---- what a batch can be: geometries with widths that are no multiple of 8, frames too short for the device decoder, empty frames, frames
// the decoder refuses for reasons of its own; lengths from the decoder's floor (16 + 1,024 bytes) to a few MB
std::vector<DecPlanIn> make_batch(Rng &rng, int n, int kind) {
    static const int kSide[] = {256, 260, 264, 272, 320, 512, 517, 520, 203, 1000, 1080, 1920, 2048, 2051};
    static const int kSmall[] = {256, 260, 264, 259, 320, 257};
    std::vector<DecPlanIn> in((size_t)n);
    for (DecPlanIn &f : in) {
        if (kind == 0) f.h = kSmall[rng.in(0, 5)], f.w = kSmall[rng.in(0, 5)];
        else f.h = kSide[rng.in(0, 13)], f.w = kSide[rng.in(0, 13)];
        f.quality = (int)rng.in(1, 100);
        const size_t top = (size_t)1 << (kind == 0 ? rng.in(11, 13) : kind == 1 ? rng.in(11, 22) : rng.in(18, 22));
        f.len = rng.in(top / 2 < 1040 ? 1040 : top / 2, top);
        const size_t roll = rng.in(0, 19);
        if (roll == 0) f.h = 0, f.w = 8, f.len = 16;                  // empty
        else if (roll == 1) f.h = f.w = 64, f.len = rng.in(16, 4000); // too short
        else if (roll == 2) f.len = rng.in(16, 1039);                 // too few stream bits
        const size_t nb = naive_nblk(f.h, f.w);
        f.takes = nb >= 1024 && f.len >= 1040 && roll != 3; // (roll 3: a frame the decoder does not take for another reason - a scaled_dct stream, a hook)
    }
    return in;
}

int hand_derived() {
    // Two 512 x 512 streams of 30,000 and 4,071 bytes, then a 203 x 517 one of 100,001 bytes, production limits: one chunk.
    //   512 x 512: 64 x 64 = 4,096 blocks, pitch 512, 262,144 bytes of pixels (a whole number of 256)
    //   203 x 517: 26 x 65 = 1,690 blocks, pitch 520, 520 x 203 = 105,560 bytes -> 413 x 256 = 105,728
    //   A 30,000 bytes: slot 30,000 + 16 = 30,016 bytes = 7,504 words; 7,500 words, all of the last one; 240,000 bits; rule: 2 x 240,000 / 4,096 = 117 bits ->
    //       4 words -> 5 -> the floor, 9 words = 288; 240,000 / 288 = 833 (+ 2) = 835 ranges of 288
    //   B 4,071 bytes: slot 4,080 + 16 = 4,096 bytes = 1,024 words; 1,018 words, 3 bytes of the last one (mask ffffff00); 32,568 bits (not below 7 x 4,096);
    //       rule: 15 bits -> 1 word -> 288; 32,568 / 288 = 113 (+ 2) = 115
    //   C 100,001 bytes: slot 100,016 + 16 = 100,032 bytes = 25,008 words; 25,001 words, 1 byte of the last one (mask ff000000); 800,008 bits;
    //       rule: 2 x 800,008 / 1,690 = 946 bits -> (946 + 31) / 32 = 30 words -> 31 = 992 bits; 800,008 / 288 = 2,777 (+ 2) = 2,779
    //   the chunk: range 992; ranges (bits - 128 + 991) / 992 = 242, 33, 807 (from 0, 242, 275: 1,082); C has 473 bits per block: the large window;
    //       words from 0, 7,504, 8,528: 33,536; blocks from 0, 4,096, 8,192: 9,882; pixels from 0, 262,144, 524,288: 630,016; 3,729 ranges of 288
    const DecPlanIn in[3] = {{512, 512, 50, 30000, true}, {512, 512, 5, 4071, true}, {203, 517, 90, 100001, true}};
    const DecPlan p = plan_decode_batch(in, 3, {(size_t)96 << 20, (size_t)288 << 20, 1024});
    bool ok = p.chunks.size() == 1 && p.frames.size() == 3;
    if (ok) {
        const DecPlanChunk &c = p.chunks[0];
        const DecPlanFrame &a = p.frames[0], &b = p.frames[1], &d = p.frames[2];
        ok = c.first == 0 && c.count == 3 && c.words == 33536 && c.pix_bytes == 630016 && c.blocks == 9882 && c.ranges288 == 3729 && c.ranges == 1082 && c.range_bits == 992 && !c.small_win;
        ok = ok && a.index == 0 && a.nblk == 4096 && a.pitch == 512 && a.word0 == 0 && a.nwords == 7500 && a.last_mask == 0xffffffffu && a.stream_bits == 240000 && a.nranges == 242 &&
             a.range0 == 0 && a.blk0 == 0 && a.pix_off == 0;
        ok = ok && b.index == 1 && b.nblk == 4096 && b.pitch == 512 && b.word0 == 7504 && b.nwords == 1018 && b.last_mask == 0xffffff00u && b.stream_bits == 32568 && b.nranges == 33 &&
             b.range0 == 242 && b.blk0 == 4096 && b.pix_off == 262144;
        ok = ok && d.index == 2 && d.nblk == 1690 && d.pitch == 520 && d.word0 == 8528 && d.nwords == 25001 && d.last_mask == 0xff000000u && d.stream_bits == 800008 && d.nranges == 807 &&
             d.range0 == 275 && d.blk0 == 8192 && d.pix_off == 524288;
    }
    // Two frames per chunk: A and B at their own range, 288 bits - (bits - 128 + 287) / 288 = 833 and 113 ranges, the small window - and C alone, from 0.
    const DecPlan q = plan_decode_batch(in, 3, {(size_t)96 << 20, (size_t)288 << 20, 2});
    ok = ok && q.chunks.size() == 2 && q.chunks[0].count == 2 && q.chunks[0].range_bits == 288 && q.chunks[0].small_win && q.chunks[0].ranges == 946 && q.frames[0].nranges == 833 &&
         q.frames[1].nranges == 113 && q.frames[1].range0 == 833 && q.chunks[0].words == 8528 && q.chunks[0].pix_bytes == 524288 && q.chunks[1].first == 2 && q.chunks[1].count == 1 &&
         q.chunks[1].range_bits == 992 && q.frames[2].word0 == 0 && q.frames[2].range0 == 0 && q.frames[2].blk0 == 0 && q.frames[2].pix_off == 0 && q.chunks[1].words == 25008 &&
         q.chunks[1].pix_bytes == 105728 && q.chunks[1].ranges == 807 && q.chunks[1].ranges288 == 2779;
    // The upload buffer of the first plan's chunk with 20 waves and 40 workgroups: descriptors at 0, 3 of them, then 80 and 160 bytes, each piece rounded up to 256
    const DecUploadLayout up(3, 20, 40, 33536);
    const size_t o_tiles = (3 * sizeof(DecFrame) + 255) / 256 * 256;
    ok = ok && up.o_frames == 0 && up.o_tiles == o_tiles && up.o_wgs == o_tiles + 256 && up.o_streams == o_tiles + 512 && up.up_bytes == o_tiles + 512 + 134144;
    if (!ok) printf("decplan_selftest FAILED: the hand-derived case\n");
    return ok ? 0 : 2;
}

} // namespace

int main(int argc, char **argv) {
    const bool break_cut = argc > 1 && strcmp(argv[1], "--break-cut") == 0;
    if (hand_derived()) return 2;
    // the production limits; then frames 1, 3 and 7, stream limits of a few KB, pixel limits below one frame (256 x 256 = 65,536 bytes)
    static const DecPlanLimits kLimits[] = {{(size_t)96 << 20, (size_t)288 << 20, 1024}, {(size_t)96 << 20, (size_t)288 << 20, 1}, {(size_t)96 << 20, (size_t)288 << 20, 3},
                                            {5000, (size_t)288 << 20, 7},                {(size_t)96 << 20, 30000, 1024},        {20000, 400000, 3},
                                            {(size_t)1 << 20, (size_t)4 << 20, 7}};
    Tally t;
    Rng rng{0x9E3779B97F4A7C15ull};
    for (int n = 0; n <= 1100; n++) {
        const std::vector<DecPlanIn> in = make_batch(rng, n, n % 3);
        for (const DecPlanLimits &lim : kLimits) {
            const DecPlan p = break_cut ? broken_plan(in.data(), n, lim) : plan_decode_batch(in.data(), n, lim);
            check_plan(t, in.data(), n, lim, p, rng);
        }
    }
    printf("decplan sweep: %llu plans, %llu chunks, %llu frames, %llu counterexamples\n", t.plans, t.chunks, t.frames, t.bad);
    if (t.bad) {
        printf("decplan_selftest FAILED (%s cut): %llu counterexamples\n", break_cut ? "broken" : "header's", t.bad);
        return 1;
    }
    printf("decplan_selftest ok\n");
    return 0;
}
