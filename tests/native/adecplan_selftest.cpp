// adecplan_selftest - the plan of tic_decompress_batch_adaptive (tinyimgcodec_amd/csrc/tic_adaptive_decode_plan.h: the functions the library
// itself calls) on the CPU: seeded batches of 0 .. 300 frames of random geometries, stream lengths and payload starts against random limits, every
// plan checked against definitions written out naively here.  Host only: no HIP header, no device.  Built with tic_entropy.cpp (num_blocks).
//
//   adecplan_selftest               the header's cut                                         -> "adecplan_selftest ok", exit 0
//   adecplan_selftest --break-cut   a wrong cut: the limits tested AFTER the frame joined    -> counts its counterexamples, exit 1
//
// The second form is what shows that the sweep can fail.
#define TIC_DEC_WORKSPACE_ONLY
#include "../../tinyimgcodec_amd/csrc/tic_adaptive_decode_plan.h"

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
size_t naive_pb(const AdaptDecPlanIn &f) { return (naive_pitch(f.w) * (size_t)f.h + 255) / 256 * 256; }
size_t naive_cb(const AdaptDecPlanIn &f) { return naive_nblk(f.h, f.w) * 128; }
size_t naive_range(const AdaptDecPlanIn &f) {
    const size_t r = 2 * (f.len * 8 - f.payload_bit) / naive_nblk(f.h, f.w);
    return r < 256 ? 256 : r > 4096 ? 4096 : r;
}
size_t naive_ranges(const AdaptDecPlanIn &f) {
    size_t n = 0;
    for (size_t bit = f.payload_bit; bit < f.len * 8; bit += naive_range(f)) n++;
    return n;
}
size_t wgs_of(size_t lanes) { return (lanes + 255) / 256; }

bool passes(const AdaptDecPlanLimits &lim, size_t sb, size_t pb, size_t cb, size_t tb) {
    return sb > lim.stream_bytes || pb > lim.pix_bytes || cb > lim.coef_bytes || tb > lim.tab_bytes;
}

// The wrong cut of --break-cut: a frame joins first, and the chunk ends when it HAS passed a limit.
AdaptDecPlan broken_plan(const AdaptDecPlanIn *in, int n, const AdaptDecPlanLimits &lim) {
    AdaptDecPlan p;
    int first = 0, count = 0;
    size_t sb = 0, pb = 0, cb = 0, tb = 0;
    for (int i = 0; i < n; i++) {
        if (!in[i].takes) continue;
        p.frames.push_back(adec_plan_frame(i, in[i]));
        count++, sb += naive_sb(in[i].len), pb += naive_pb(in[i]), cb += naive_cb(in[i]), tb += kAdaptDecTabSlot;
        if (passes(lim, sb, pb, cb, tb) || count >= lim.frames) {
            adec_plan_close_chunk(p, first, count);
            first += count, count = 0, sb = pb = cb = tb = 0;
        }
    }
    if (count > 0) adec_plan_close_chunk(p, first, count);
    return p;
}

struct Tally {
    unsigned long long plans = 0, chunks = 0, frames = 0, bad = 0;
    int shown = 0;
    int n = 0; // the batch under test
    AdaptDecPlanLimits lim{};
    void fail(const char *what, size_t chunk, size_t frame) {
        if (bad++ == 0 || shown < 8) {
            printf("  counterexample: %s (batch of %d, limits %zu / %zu / %zu / %zu / %d, chunk %zu, frame %zu)\n", what, n, lim.stream_bytes, lim.pix_bytes,
                   lim.coef_bytes, lim.tab_bytes, lim.frames, chunk, frame);
            shown++;
        }
    }
};
#define CHECK(cond, what, ci, k) \
    do {                         \
        if (!(cond)) t.fail(what, ci, k); \
    } while (0)

struct Piece {
    size_t at, bytes;
};
bool disjoint_ascending(const std::vector<Piece> &p, size_t end) {
    for (size_t i = 0; i < p.size(); i++) {
        if (p[i].at % 256 != 0) return false;
        if (p[i].at + p[i].bytes > (i + 1 < p.size() ? p[i + 1].at : end)) return false;
    }
    return true;
}

void check_plan(Tally &t, const AdaptDecPlanIn *in, int n, const AdaptDecPlanLimits &lim, const AdaptDecPlan &p, Rng &rng) {
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
        const AdaptDecPlanChunk &c = p.chunks[ci];
        const AdaptDecPlanFrame *pf = &p.frames[(size_t)c.first];
        const size_t F = (size_t)c.count;
        t.chunks++, t.frames += F;
        // 2. the limits: passed only by a single frame; the next frame would pass one
        size_t sb = 0, pb = 0, cb = 0, tb = 0;
        for (size_t k = 0; k < F; k++) sb += naive_sb(in[pf[k].index].len), pb += naive_pb(in[pf[k].index]), cb += naive_cb(in[pf[k].index]), tb += kAdaptDecTabSlot;
        CHECK(c.count <= lim.frames, "no more frames than the limit", ci, F);
        CHECK(F == 1 || !passes(lim, sb, pb, cb, tb), "only a single frame passes a byte limit", ci, F);
        if (ci + 1 < p.chunks.size()) {
            const AdaptDecPlanIn &nx = in[pf[F].index];
            CHECK(passes(lim, sb + naive_sb(nx.len), pb + naive_pb(nx), cb + naive_cb(nx), tb + kAdaptDecTabSlot) || c.count >= lim.frames, "the next frame would pass a limit", ci, F);
        }
        // 3. every frame's places: aligned, behind the frame in front (so no two frames' words, ranges, blocks, workgroups, pixel or table slots
        //    overlap), ending in front of the next; 4. the totals are the sums
        size_t words = 0, pix = 0, blocks = 0, ranges = 0, rwgs = 0, bwgs = 0, tabs = 0;
        for (size_t k = 0; k < F; k++) {
            const AdaptDecPlanFrame &g = pf[k];
            const AdaptDecPlanIn &f = in[g.index];
            const AdaptDecFrame &d = g.d;
            CHECK(g.h == f.h && g.w == f.w && g.quality == f.quality && g.len == f.len && d.payload_bit == f.payload_bit, "the frame's own figures", ci, k);
            CHECK(g.nblk == naive_nblk(f.h, f.w) && g.nblk > 0 && d.nblocks == g.nblk && g.pitch == naive_pitch(f.w) && g.pitch % 8 == 0 && g.pitch >= (size_t)f.w, "nblk and pitch", ci, k);
            CHECK((size_t)d.word0 * 4 % 16 == 0 && d.word0 == words, "word0: 16-byte aligned, behind the stream in front", ci, k);
            CHECK((size_t)d.nwords * 4 >= f.len && (size_t)d.nwords * 4 < f.len + 4 && d.total_bits == f.len * 8, "nwords and total_bits", ci, k);
            CHECK(d.last_mask == (f.len % 4 == 0 ? 0xffffffffu : f.len % 4 == 1 ? 0xff000000u : f.len % 4 == 2 ? 0xffff0000u : 0xffffff00u), "last_mask", ci, k);
            CHECK(d.range_bits == naive_range(f) && d.range_bits >= 256 && d.range_bits <= 4096, "the frame's own range", ci, k);
            CHECK(d.nranges == naive_ranges(f) && d.nranges >= 1, "nranges: the ranges that start in front of the stream's end", ci, k);
            CHECK(d.payload_bit + (unsigned long long)(d.nranges - 1) * d.range_bits < d.total_bits, "the last range starts inside the stream", ci, k);
            CHECK(d.range0 == ranges && d.blk0 == blocks && d.rwg0 == rwgs && d.bwg0 == bwgs, "range0, blk0 and the first workgroups: behind the frame in front", ci, k);
            CHECK(g.pix_off % 256 == 0 && g.pix_off == pix, "pix_off: 256-byte aligned, behind the frame in front", ci, k);
            CHECK(g.tab_off % 256 == 0 && g.tab_off == tabs && kAdaptDecTabSlot >= kAdaptDecTabBytes, "tab_off: 256-byte aligned, behind the table in front", ci, k);
            words += naive_sb(f.len) / 4, pix += naive_pb(f), blocks += g.nblk, ranges += d.nranges, rwgs += wgs_of(d.nranges), bwgs += wgs_of(g.nblk), tabs += kAdaptDecTabSlot;
            CHECK((size_t)d.word0 * 4 + f.len + 16 <= words * 4 && g.pix_off + g.pitch * (size_t)g.h <= pix, "a region ends in front of its neighbour", ci, k);
        }
        CHECK(c.words == words && c.pix_bytes == pix && c.blocks == blocks && c.ranges == ranges && c.range_wgs == rwgs && c.block_wgs == bwgs && c.tab_bytes == tabs,
              "the chunk's totals", ci, F);
        CHECK(words * 4 == sb && pix == pb && blocks * 128 == cb && tabs == tb && words * 4 < (1ull << 32), "the last region ends at the totals", ci, F);
        CHECK(c.work_bytes == (6 * ranges + 2 * blocks) * 4, "the work buffer: six words per range, two per block", ci, F);
        // 5. every workgroup -> frame entry points at the frame that owns the workgroup, and every lane of it is a range (block) of that frame or none
        //    (the tables as the library fills them; a sentinel shows an entry nobody wrote, the guard word one written behind the grid)
        std::vector<uint32_t> rwg_frame(rwgs + 1, 0xffffffffu), bwg_frame(bwgs + 1, 0xffffffffu);
        if (c.range_wgs == rwgs && c.block_wgs == bwgs) adec_plan_fill_wg_tables(pf, c.count, rwg_frame.data(), bwg_frame.data());
        CHECK(rwg_frame[rwgs] == 0xffffffffu && bwg_frame[bwgs] == 0xffffffffu, "nothing is written behind the workgroup tables", ci, F);
        rwg_frame.pop_back(), bwg_frame.pop_back();
        for (size_t g = 0; g < rwg_frame.size() && g < rwgs; g++) {
            CHECK(rwg_frame[g] < F, "every range workgroup has a frame", ci, g);
            if (rwg_frame[g] >= F) continue;
            const AdaptDecFrame &d = pf[rwg_frame[g]].d;
            CHECK(g >= d.rwg0 && (g - d.rwg0) * 256 < d.nranges, "a range workgroup's frame owns it", ci, g);
        }
        for (size_t g = 0; g < bwg_frame.size() && g < bwgs; g++) {
            CHECK(bwg_frame[g] < F, "every block workgroup has a frame", ci, g);
            if (bwg_frame[g] >= F) continue;
            const AdaptDecFrame &d = pf[bwg_frame[g]].d;
            CHECK(g >= d.bwg0 && (g - d.bwg0) * 256 < d.nblocks, "a block workgroup's frame owns it", ci, g);
        }
        // 6. the upload buffer (the inverse transform's figures are the library's: any number here) and the device buffer behind it
        const size_t arg_bytes = 8 * rng.in(1, 20), iwgs = rng.in(1, 4 * blocks);
        const AdaptDecUploadLayout up(c, arg_bytes, iwgs);
        CHECK(up.o_frames == 0 && disjoint_ascending({{up.o_frames, F * sizeof(AdaptDecFrame)}, {up.o_rwg, rwgs * 4}, {up.o_bwg, bwgs * 4}, {up.o_idct_args, F * arg_bytes},
                                                      {up.o_idct_wgs, iwgs * 8}, {up.o_tabs, tabs}, {up.o_streams, words * 4}}, up.up_bytes),
              "the upload pieces: 256-byte aligned, in order, none overlapping", ci, F);
        CHECK(up.o_streams + words * 4 == up.up_bytes && up.up_bytes <= F * (sizeof(AdaptDecFrame) + arg_bytes) + (rwgs + bwgs) * 4 + iwgs * 8 + tabs + words * 4 + 6 * 255,
              "no more padding than the alignment asks for", ci, F);
        const AdaptDecWorkLayout wl(c);
        CHECK(wl.status_bytes == sizeof(AdaptDecChunkStatus) + F * sizeof(AdaptDecFrameStatus) &&
                  disjoint_ascending({{wl.o_status, wl.status_bytes}, {wl.o_work, c.work_bytes}, {wl.o_coef, blocks * 128}}, wl.bytes) && wl.o_coef + blocks * 128 == wl.bytes,
              "the device buffer's pieces", ci, F);
    }
}

// ---- what a batch can be: sides from 1 to 2051, no multiples of 8 among them, lengths from a table and a few payload bytes to a few MB, payload
// starts from the smallest table (two counts and two entries each) to the largest; frames the kernels do not take
std::vector<AdaptDecPlanIn> make_batch(Rng &rng, int n, int kind) {
    static const int kSide[] = {1, 7, 8, 9, 13, 21, 64, 96, 203, 256, 260, 512, 517, 1000, 1080, 1920, 2040, 2048, 2051};
    std::vector<AdaptDecPlanIn> in((size_t)n);
    for (AdaptDecPlanIn &f : in) {
        const size_t top = kind == 0 ? 9 : 18;
        f.h = kSide[rng.in(0, top)], f.w = kSide[rng.in(0, top)];
        f.quality = (int)rng.in(1, 99);
        f.payload_bit = 128 + rng.in(2 * 16 + 4 * 9, 8 * 2610);
        const size_t body = (size_t)1 << (kind == 0 ? rng.in(0, 13) : kind == 1 ? rng.in(0, 22) : rng.in(16, 22));
        f.len = f.payload_bit / 8 + 1 + rng.in(body / 2, body);
        const size_t roll = rng.in(0, 19);
        if (roll == 0) f.h = 0, f.w = 8, f.len = 16, f.payload_bit = 0; // empty
        f.takes = roll > 2 && adaptive_dec_fits(naive_nblk(f.h, f.w), f.len, f.payload_bit); // (rolls 1, 2: a flat frame, a table that does not parse, a hook)
    }
    return in;
}

AdaptDecPlanLimits make_limits(Rng &rng, int round) {
    if (round == 0) return {(size_t)96 << 20, (size_t)288 << 20, (size_t)256 << 20, (size_t)16 << 20, 1024}; // the library's
    AdaptDecPlanLimits lim;
    lim.stream_bytes = (size_t)1 << rng.in(10, 27), lim.pix_bytes = (size_t)1 << rng.in(10, 29), lim.coef_bytes = (size_t)1 << rng.in(10, 29);
    lim.tab_bytes = kAdaptDecTabSlot * rng.in(1, 400) - rng.in(0, 1);
    lim.frames = (int)rng.in(1, round % 2 ? 8 : 1024);
    return lim;
}

int hand_derived() {
    // A 64 x 96 stream of 2,649 bytes whose payload starts at bit 1,500, a 13 x 21 one of 201 bytes from bit 700, an 8 x 2,040 one of 30,001 bytes from bit 2,000; the library's limits.
    //   A: 8 x 12 = 96 blocks; 21,192 bits, payload 19,692: 2 x 19,692 / 96 = 410 bits per lane; (19,692 + 409) / 410 = 49 ranges; 2,649 = 4 x 662 + 1: 663 words,
    //      mask ff000000; slot 2,656 + 16 = 2,672 bytes = 668 words; pitch 96, 6,144 bytes of pixels (a whole number of 256)
    //   B: 2 x 3 = 6 blocks; 1,608 bits, payload 908: 302 bits per lane; 4 ranges (3 x 302 = 906 < 908); 51 words, mask ff000000; slot 208 + 16 = 224 bytes = 56 words;
    //      pitch 24, 312 bytes -> 512
    //   C: 255 blocks; 240,008 bits, payload 238,008: 1,866 bits per lane; (238,008 + 1,865) / 1,866 = 128 ranges; 7,501 words, mask ff000000; slot 30,016 + 16 = 7,508 words;
    //      pitch 2,040, 16,320 bytes -> 16,384
    const AdaptDecPlanIn in[3] = {{64, 96, 50, 2649, 1500, true}, {13, 21, 75, 201, 700, true}, {8, 2040, 50, 30001, 2000, true}};
    //   the chunk: words from 0, 668, 724: 8,232; ranges from 0, 49, 53: 181; blocks from 0, 96, 102: 357; a workgroup of either grid each; pixels from 0, 6,144, 6,656:
    //      23,040; tables from 0, 13,568, 27,136: 40,704; work (6 x 181 + 2 x 357) x 4 = 7,200 bytes
    const AdaptDecPlanLimits lib = {(size_t)96 << 20, (size_t)288 << 20, (size_t)256 << 20, (size_t)16 << 20, 1024};
    const AdaptDecPlan p = plan_adaptive_decode_batch(in, 3, lib);
    bool ok = p.chunks.size() == 1 && p.frames.size() == 3;
    if (ok) {
        const AdaptDecPlanChunk &c = p.chunks[0];
        const AdaptDecPlanFrame &a = p.frames[0], &b = p.frames[1], &d = p.frames[2];
        ok = c.first == 0 && c.count == 3 && c.words == 8232 && c.pix_bytes == 23040 && c.blocks == 357 && c.ranges == 181 && c.range_wgs == 3 && c.block_wgs == 3 &&
             c.tab_bytes == 40704 && c.work_bytes == 7200;
        ok = ok && a.index == 0 && a.nblk == 96 && a.pitch == 96 && a.d.word0 == 0 && a.d.nwords == 663 && a.d.last_mask == 0xff000000u && a.d.total_bits == 21192 &&
             a.d.payload_bit == 1500 && a.d.range_bits == 410 && a.d.nranges == 49 && a.d.range0 == 0 && a.d.blk0 == 0 && a.d.rwg0 == 0 && a.d.bwg0 == 0 && a.pix_off == 0 && a.tab_off == 0;
        ok = ok && b.index == 1 && b.nblk == 6 && b.pitch == 24 && b.d.word0 == 668 && b.d.nwords == 51 && b.d.last_mask == 0xff000000u && b.d.total_bits == 1608 &&
             b.d.range_bits == 302 && b.d.nranges == 4 && b.d.range0 == 49 && b.d.blk0 == 96 && b.d.rwg0 == 1 && b.d.bwg0 == 1 && b.pix_off == 6144 && b.tab_off == 13568;
        ok = ok && d.index == 2 && d.nblk == 255 && d.pitch == 2040 && d.d.word0 == 724 && d.d.nwords == 7501 && d.d.total_bits == 240008 && d.d.range_bits == 1866 &&
             d.d.nranges == 128 && d.d.range0 == 53 && d.d.blk0 == 102 && d.d.rwg0 == 2 && d.d.bwg0 == 2 && d.pix_off == 6656 && d.tab_off == 27136;
    }
    // Two table slots per chunk: A and B, then C alone, from 0
    AdaptDecPlanLimits two = lib;
    two.tab_bytes = 2 * kAdaptDecTabSlot;
    const AdaptDecPlan q = plan_adaptive_decode_batch(in, 3, two);
    ok = ok && q.chunks.size() == 2 && q.chunks[0].count == 2 && q.chunks[0].words == 724 && q.chunks[0].ranges == 53 && q.chunks[1].first == 2 && q.chunks[1].count == 1 &&
         q.frames[2].d.word0 == 0 && q.frames[2].d.range0 == 0 && q.frames[2].d.blk0 == 0 && q.frames[2].d.rwg0 == 0 && q.frames[2].pix_off == 0 && q.frames[2].tab_off == 0 &&
         q.chunks[1].words == 7508 && q.chunks[1].pix_bytes == 16384;
    if (!ok) printf("adecplan_selftest FAILED: the hand-derived case\n");
    return ok ? 0 : 2;
}

} // namespace

int main(int argc, char **argv) {
    const bool break_cut = argc > 1 && strcmp(argv[1], "--break-cut") == 0;
    if (hand_derived()) return 2;
    Tally t;
    Rng rng{0x9E3779B97F4A7C15ull};
    for (int n = 0; n <= 300; n++) {
        const std::vector<AdaptDecPlanIn> in = make_batch(rng, n, n % 3);
        for (int round = 0; round < 6; round++) {
            const AdaptDecPlanLimits lim = make_limits(rng, round);
            const AdaptDecPlan p = break_cut ? broken_plan(in.data(), n, lim) : plan_adaptive_decode_batch(in.data(), n, lim);
            check_plan(t, in.data(), n, lim, p, rng);
        }
    }
    printf("adecplan sweep: %llu plans, %llu chunks, %llu frames, %llu counterexamples\n", t.plans, t.chunks, t.frames, t.bad);
    if (t.bad) {
        printf("adecplan_selftest FAILED (%s cut): %llu counterexamples\n", break_cut ? "broken" : "header's", t.bad);
        return 1;
    }
    printf("adecplan_selftest ok\n");
    return 0;
}
