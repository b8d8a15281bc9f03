// transcode_plan_selftest - the plan of the batch transcoders (tinyimgcodec_amd/csrc/tic_transcode_plan.h: the functions the library itself calls)
// on the CPU: both readers' plans inside the transcoders' limits and both writers' tables, with gaps, against definitions written out naively
// here.  Host only: no HIP header, no device.  Built with tic_entropy.cpp (num_blocks, compress_bound), under the address sanitizer.
//
//   transcode_plan_selftest              the header's functions                              -> "transcode_plan_selftest ok", exit 0
//   transcode_plan_selftest --break-gap  a default writer's table that closes the gaps       -> counts its counterexamples, exit 1
//
// The second form is what shows that the sweep can fail.
#define TIC_DEC_WORKSPACE_ONLY
#include "../../tinyimgcodec_amd/csrc/tic_transcode_plan.h"

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

size_t naive_nblk(int h, int w) { return h <= 0 || w <= 0 ? 0 : (size_t)((h + 7) / 8) * (size_t)((w + 7) / 8); }
size_t naive_sb(size_t len) { return (len + 15) / 16 * 16 + 16; }

long g_checks = 0, g_bad = 0;
bool g_break_gap = false;
#define CHECK(c)                                                                    \
    do {                                                                            \
        g_checks++;                                                                 \
        if (!(c)) {                                                                 \
            if (g_bad++ < 10) fprintf(stderr, "line %d: %s\n", __LINE__, #c);       \
        }                                                                           \
    } while (0)

// frame geometries with the block counts the issue names: around 255 / 256 / 257 and 1,024 / 1,025, and frames without blocks
void geometry(Rng &r, int *h, int *w) {
    static const int kBlocks[] = {0, 1, 2, 63, 64, 65, 254, 255, 256, 257, 258, 511, 512, 513, 1023, 1024, 1025, 1089, 2145};
    const int nb = kBlocks[r.in(0, sizeof kBlocks / sizeof kBlocks[0] - 1)];
    if (nb == 0) {
        *h = r.in(0, 1) ? 0 : 16, *w = *h ? 0 : 16;
        return;
    }
    // nb = rows x cols with a pixel size that is not a multiple of 8 now and then
    int rows = 1;
    for (int d = 2; d * d <= nb; d++)
        if (nb % d == 0 && r.in(0, 2) == 0) rows = d;
    *h = rows * 8 - (int)r.in(0, 7), *w = nb / rows * 8 - (int)r.in(0, 7);
}

// ---- the chunk cut both readers' plans share, naively: frames taken, in order; a frame joins unless the chunk is non-empty and would pass a limit
struct NaiveChunk {
    std::vector<int> idx;
};
std::vector<NaiveChunk> naive_cut(const std::vector<size_t> &len, const std::vector<size_t> &nblk, const std::vector<char> &takes, const TranscodeLimits &lim, bool tabs) {
    std::vector<NaiveChunk> out;
    const int maxf = lim.frames < 1 ? 1 : (lim.frames > 64 ? 64 : lim.frames);
    NaiveChunk cur;
    size_t sb = 0, cb = 0, tb = 0;
    for (size_t i = 0; i < len.size(); i++) {
        if (!takes[i]) continue;
        const size_t s = naive_sb(len[i]), c = nblk[i] * 128, t = tabs ? kAdaptDecTabSlot : 0;
        if (!cur.idx.empty() && (sb + s > lim.stream_bytes || cb + c > lim.coef_bytes || tb + t > lim.tab_bytes || (int)cur.idx.size() >= maxf)) {
            out.push_back(cur);
            cur = NaiveChunk(), sb = cb = tb = 0;
        }
        cur.idx.push_back((int)i), sb += s, cb += c, tb += t;
    }
    if (!cur.idx.empty()) out.push_back(cur);
    return out;
}

// the default writer's table with the gaps closed: what --break-gap puts in the header's place
bool broken_entropy_table(EntropyFrameTable *t, int mode, const TranscodeFrame *f, int n, int *entry, int *count, size_t *stream_bytes, size_t *nparts, size_t *ngroups,
                          size_t *nplaces) {
    if (!transcode_entropy_table(t, mode, f, n, entry, count, stream_bytes, nparts, ngroups, nplaces)) return false;
    size_t blk = 0;
    for (int j = 0; j < *count; j++) t->rec[j].first_block = blk, blk += t->rec[j].nblocks;
    return true;
}

void check_writer_tables(Rng &r, const TranscodeFrame *tf_in, int n, size_t chunk_blocks) {
    TranscodeFrame tf[kEntropyMaxFrames];
    size_t at = 0;
    for (int k = 0; k < n; k++) {
        tf[k] = tf_in[k];
        CHECK(tf[k].blk0 == at && tf[k].nblk >= 1); // the readers' plans lay the rows back to back, in chunk order
        at += tf[k].nblk;
    }
    CHECK(at == chunk_blocks);
    // ---- the adaptive writer: every frame has a record at its own rows, whatever is skipped later
    {
        AdaptFrameTable t;
        size_t span = 0, ngroups = 0, grp = 0;
        CHECK(transcode_adaptive_table(&t, tf, n, &span, &ngroups));
        CHECK(span == chunk_blocks);
        for (int k = 0; k < kEntropyMaxFrames; k++) {
            if (k >= n) {
                CHECK(t.first_group[k] == 0xffffffffu);
                continue;
            }
            const AdaptFrameRec &rec = t.rec[k];
            CHECK(rec.first_block == tf[k].blk0 && rec.nblocks == tf[k].nblk && rec.first_group == grp && t.first_group[k] == grp);
            CHECK(rec.ngroups == (tf[k].nblk + 255) / 256);
            CHECK(rec.first_block + rec.nblocks <= span);
            grp += rec.ngroups;
        }
        CHECK(grp == ngroups);
        // a frame whose rows are not where the table would put them is refused
        if (n >= 2) {
            TranscodeFrame moved[kEntropyMaxFrames];
            memcpy(moved, tf, sizeof(TranscodeFrame) * (size_t)n);
            moved[n - 1].blk0 += 1;
            CHECK(!transcode_adaptive_table(&t, moved, n, &span, &ngroups));
        }
        // skipped frames: no stream area, no words
        unsigned long long total_bits[kEntropyMaxFrames];
        uint32_t base_bits[kEntropyMaxFrames];
        for (int k = 0; k < n; k++) {
            tf[k].skip = r.in(0, 3) == 0;
            total_bits[k] = tf[k].skip ? 0ull : 200ull + r.in(0, 100000), base_bits[k] = 160;
        }
        size_t bytes = 0, off = 0;
        assign_adaptive_streams(&t, n, total_bits, base_bits, &bytes);
        for (int k = 0; k < n; k++) {
            CHECK((t.rec[k].skip != 0) == tf[k].skip && t.rec[k].out_off == off && t.rec[k].first_block == tf[k].blk0);
            CHECK(tf[k].skip ? t.rec[k].out_words == 0 : t.rec[k].out_words == (total_bits[k] + 31) / 32);
            off += ((size_t)t.rec[k].out_words * 4 + 15) / 16 * 16;
        }
        CHECK(off == bytes);
    }
    // ---- the default writer: records of the frames that are not skipped, each at its own rows
    for (int mode = 0; mode < 2; mode++) {
        EntropyFrameTable t;
        int entry[kEntropyMaxFrames], count = -1;
        size_t bytes = 0, nparts = 0, ngroups = 0, nplaces = 0;
        const bool ok = (g_break_gap ? broken_entropy_table : transcode_entropy_table)(&t, mode, tf, n, entry, &count, &bytes, &nparts, &ngroups, &nplaces);
        int live = 0;
        for (int k = 0; k < n; k++) live += !tf[k].skip;
        const EntropyGeom g = entropy_geom(mode);
        bool too_large = false;
        for (int k = 0; k < n; k++) {
            const size_t parts = (tf[k].nblk + g.part_blocks - 1) / g.part_blocks;
            too_large = too_large || (!tf[k].skip && (parts + g.group_parts - 1) / g.group_parts > kEntropyMaxGroups);
        }
        CHECK(ok == (live > 0 && !too_large));
        CHECK(count == live);
        if (!ok) continue;
        size_t off = 0, part = 0, grp = 0, plc = 0;
        int j = 0;
        for (int k = 0; k < n; k++) {
            if (tf[k].skip) {
                CHECK(entry[k] == -1);
                continue;
            }
            CHECK(entry[k] == j);
            const EntropyFrameRec &rec = t.rec[j];
            const size_t bound = (16 + tf[k].nblk * 208 + 8 + 15) / 16 * 16; // compress_bound, rounded up
            CHECK(rec.first_block == tf[k].blk0 && rec.nblocks == tf[k].nblk); // never another frame's rows: a skipped frame leaves a gap
            CHECK(rec.out_off == off && rec.cap_words == (bound - 16) / 4 && rec.out_off % 16 == 0);
            CHECK(rec.h == tf[k].h && rec.w == tf[k].w && rec.quality == tf[k].quality);
            CHECK(rec.first_part == part && rec.first_group == grp && rec.first_place == plc && t.first_group[j] == grp && t.first_place[j] == plc);
            const size_t parts = (tf[k].nblk + g.part_blocks - 1) / g.part_blocks;
            part += parts, grp += (parts + g.group_parts - 1) / g.group_parts, plc += (parts + g.place_parts - 1) / g.place_parts;
            off += bound;
            j++;
        }
        CHECK(off == bytes && part == nparts && grp == ngroups && plc == nplaces);
        for (int k = j; k < kEntropyMaxFrames; k++) CHECK(t.first_group[k] == 0xffffffffu && t.first_place[k] == 0xffffffffu);
    }
}

void sweep_case(Rng &r, int n, int limit_kind) {
    std::vector<DecPlanIn> din((size_t)n);
    std::vector<AdaptDecPlanIn> ain((size_t)n);
    std::vector<size_t> len((size_t)n), nblk((size_t)n);
    std::vector<char> takes((size_t)n);
    for (int i = 0; i < n; i++) {
        int h, w;
        geometry(r, &h, &w);
        nblk[(size_t)i] = naive_nblk(h, w);
        CHECK(num_blocks(h, w) == nblk[(size_t)i]);
        len[(size_t)i] = 16 + 400 + r.in(0, 40) * nblk[(size_t)i] + r.in(0, 3);
        takes[(size_t)i] = nblk[(size_t)i] != 0 && r.in(0, 4) != 0; // frames without blocks and frames not taken are in no chunk
        const int q = (int)r.in(1, 99);
        din[(size_t)i] = DecPlanIn{h, w, q, len[(size_t)i], takes[(size_t)i] != 0};
        ain[(size_t)i] = AdaptDecPlanIn{h, w, q, len[(size_t)i], 128 + r.in(40, 2000), takes[(size_t)i] != 0};
    }
    TranscodeLimits lim = transcode_default_limits();
    CHECK(lim.frames == kEntropyMaxFrames);
    if (limit_kind == 1) lim.frames = 1;                         // chunks of one, by count
    if (limit_kind == 2) lim.stream_bytes = 1;                   // ... by stream bytes
    if (limit_kind == 3) lim.coef_bytes = 1;                     // ... by coefficients
    if (limit_kind == 4) lim.frames = (int)r.in(2, 7);           // small chunks
    if (limit_kind == 5) lim.frames = 1000;                      // more than a writer's table holds: capped
    if (limit_kind == 6) lim.coef_bytes = 128 * r.in(256, 4096); // a cut in the middle
    // ---- the default-table reader
    {
        const DecPlan p = plan_transcode_default_reader(din.data(), n, lim);
        const std::vector<NaiveChunk> want = naive_cut(len, nblk, takes, lim, false);
        CHECK(p.chunks.size() == want.size());
        size_t at = 0;
        for (size_t c = 0; c < p.chunks.size() && c < want.size(); c++) {
            const DecPlanChunk &ch = p.chunks[c];
            CHECK(ch.count == (int)want[c].idx.size() && ch.first == (int)at && ch.count >= 1 && ch.count <= kEntropyMaxFrames);
            if (limit_kind >= 1 && limit_kind <= 3) CHECK(ch.count == 1);
            TranscodeFrame tf[kEntropyMaxFrames];
            size_t words = 0;
            for (int k = 0; k < ch.count && k < (int)want[c].idx.size(); k++) {
                const DecPlanFrame &f = p.frames[at + (size_t)k];
                CHECK(f.index == want[c].idx[(size_t)k] && f.nblk == nblk[(size_t)f.index] && f.len == len[(size_t)f.index]);
                CHECK(f.word0 == words);
                words += naive_sb(f.len) / 4;
                tf[k] = transcode_frame(f);
                CHECK(tf[k].index == f.index && tf[k].h == f.h && tf[k].w == f.w && tf[k].quality == f.quality && !tf[k].skip);
            }
            CHECK(ch.words == words);
            check_writer_tables(r, tf, ch.count, ch.blocks);
            at += (size_t)ch.count;
        }
        CHECK(at == p.frames.size());
    }
    // ---- the reader of streams with an embedded table
    {
        const AdaptDecPlan p = plan_transcode_adaptive_reader(ain.data(), n, lim);
        const std::vector<NaiveChunk> want = naive_cut(len, nblk, takes, lim, true);
        CHECK(p.chunks.size() == want.size());
        size_t at = 0;
        for (size_t c = 0; c < p.chunks.size() && c < want.size(); c++) {
            const AdaptDecPlanChunk &ch = p.chunks[c];
            CHECK(ch.count == (int)want[c].idx.size() && ch.first == (int)at && ch.count >= 1 && ch.count <= kEntropyMaxFrames);
            TranscodeFrame tf[kEntropyMaxFrames];
            for (int k = 0; k < ch.count && k < (int)want[c].idx.size(); k++) {
                const AdaptDecPlanFrame &f = p.frames[at + (size_t)k];
                CHECK(f.index == want[c].idx[(size_t)k] && f.nblk == nblk[(size_t)f.index]);
                tf[k] = transcode_frame(f);
                CHECK(tf[k].blk0 == f.d.blk0 && tf[k].nblk == f.d.nblocks);
            }
            check_writer_tables(r, tf, ch.count, ch.blocks);
            at += (size_t)ch.count;
        }
        CHECK(at == p.frames.size());
    }
}

} // namespace

int main(int argc, char **argv) {
    g_break_gap = argc > 1 && strcmp(argv[1], "--break-gap") == 0;
    Rng r{0x9e3779b97f4a7c15ull};
    int cases = 0;
    for (int n = 0; n <= 130; n++)
        for (int kind = 0; kind <= 6; kind++) {
            sweep_case(r, n, kind);
            cases++;
        }
    CHECK(transcode_chunk_frames(0) == 1 && transcode_chunk_frames(-5) == 1 && transcode_chunk_frames(64) == 64 && transcode_chunk_frames(65) == 64);
    if (g_bad) {
        printf("transcode_plan_selftest FAILED: %ld of %ld checks in %d cases\n", g_bad, g_checks, cases);
        return 1;
    }
    printf("transcode_plan_selftest ok %d cases, %ld checks\n", cases, g_checks);
    return 0;
}
