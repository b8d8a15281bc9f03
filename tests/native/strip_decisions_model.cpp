// strip_decisions_model.cpp - a host model of what dctq_strip_kernel DECIDES (not of what it computes): which strips have a rational tie,
// which blocks trip their guard band, what each wave's batch of eight makes of them.  It predicts the four numbers of
// tic_last_rare_path_stats and the plan tic_last_strip_launch reports, so that tests/test_strip_decisions_gpu.py can hold the device to
// them - the third link of DESIGN.md section 3: the device's accept test IS the accept test guard_selftest.cpp proves harmless.
//
// Arithmetic: tic_math.h (dct8_aan<float>, build_consts, kMagic), as guard_selftest.cpp takes it; device code is built -ffp-contract=off,
// so every float32 result below is the device's, bit for bit.  Pass 1, the level shift (-1024 on output 0), pass 2 and the quantiser's two
// fused multiply-adds, in the order asked for: columns first with mulN / thrR, rows first with mulT / thrG.
// Decisions: written from DESIGN.md 5.1 and the kernel's header comment.
//   - the lane of pass 2 holds a frequency row u (columns first) or a frequency column v (rows first) and three accept thresholds for
//     the groups {1,2,3} | {5,6,7} | {0,4} of the other index; a group trips when a member's distance |t - rint(t)| exceeds its threshold;
//   - a strip has a RATIONAL TIE when the {0,4} group trips in lane 0 or 4 of any of its blocks               -> stats[1], per strip;
//   - a block has an IRRATIONAL TRIP when any other (lane, group) trips;
//   - a wave carries a batch of 8 blocks over its whole walk.  A strip with tripped blocks joins the batch with them   -> stats[0], per block
//     unless they do not fit what is left of the batch, or all eight blocks tripped: then the whole strip is marked for the exact redo
//                                                                                                                      -> stats[2], per strip
//     (a strip that did not fit takes no room: a later, smaller one may still join);
//   - stats[3] is the largest final batch of any wave.
// The walk of every (workgroup, wave) is strip_plan() / strip_cursor() / strip_step() of tic_strip_plan.h, as strip_plan_selftest.cpp walks
// them.  Only strips of the fast rectangle count; a frame without one predicts zeros and no launch.
//
// --mutant NAME evaluates a deliberately WRONG accept test (what a device defect would look like); the tests require every mutant to
// predict other counts than the true model on a case the GPU runs:
//   swap_groups  thresholds of {1,2,3} and {5,6,7} exchanged        lane_xor1   lane u takes the thresholds of lane u ^ 1
//   other_table  thrG columns first, thrR rows first                rat_thr_all the {0,4} threshold for every group
//
// Modes:
//   run     (default)  --h --w --stride [--nframes --frame-stride] --quality Q --order 0|1 --max-wgs --sched --chunk --split a,b,.. --cus --resident
//                      (--raw FILE | --seed N) [--mutant NAME] [--strips]   -> one JSON object: stats, plan, counts, (tripping strips)
//   classes            --blocks FILE --quality Q --order 0|1     -> per block: 24 x [delta, beta, tripped], class = 3 * lane + group
//   search             --quality Q --order 0|1 --seed N --tries K -> per class one "just tripped in this class only" and one "just accepted
//                      with this class its only near approach" block, found by seeded random search
// Build: g++ -O2 -std=c++17 -ffp-contract=off (tests/test_strip_decisions_cpu.py; a second build with -fsanitize=address,undefined).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../tinyimgcodec_amd/csrc/tic_math.h"
#include "../../tinyimgcodec_amd/csrc/tic_strip_plan.h"

using namespace tic;

enum Mutant { kTrue = 0, kSwapGroups, kLaneXor1, kOtherTable, kRatThrAll };

static int group_of(int k) { return (k == 0 || k == 4) ? 2 : (k < 4 ? 0 : 1); }

// The distances of a block's 64 coefficients as the fast path forms them: dist[lane][k], lane = u and k = v columns first, lane = v and k = u
// rows first.
static void block_distances(const uint8_t *px, long stride, bool cols, const DctqConsts &C, float dist[8][8]) {
    float y[8][8], e[8];
    for (int a = 0; a < 8; a++) { // pass 1: down pixel column a (columns first) | along pixel row a (rows first)
        float d[8];
        for (int k = 0; k < 8; k++) d[k] = (float)(cols ? px[k * stride + a] : px[a * stride + k]);
        dct8_aan(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]);
        d[0] -= 1024.0f;
        for (int k = 0; k < 8; k++) y[k][a] = d[k]; // y[frequency of pass 1][pixel index of pass 2]
    }
    for (int lane = 0; lane < 8; lane++) { // pass 2
        // columns first: lane u transforms y[u][c] over c -> v;  rows first: lane v transforms y[v][r] over r -> u
        for (int k = 0; k < 8; k++) e[k] = y[lane][k];
        dct8_aan(e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7]);
        const float *mul = (cols ? C.mulN : C.mulT) + lane * 8;
        for (int k = 0; k < 8; k++) {
            const float s = fmaf(e[k], mul[k], kMagic);
            const float nr = kMagic - s;
            dist[lane][k] = fabsf(fmaf(e[k], mul[k], nr));
        }
    }
}

static float threshold(const DctqConsts &C, bool cols, int lane, int grp, Mutant m) {
    if (m == kSwapGroups && grp < 2) grp ^= 1;
    if (m == kLaneXor1) lane ^= 1;
    if (m == kRatThrAll) grp = 2;
    const bool table_r = (m == kOtherTable) ? !cols : cols;
    return (table_r ? C.thrR : C.thrG)[4 * lane + grp];
}

struct BlockFacts {
    bool tie;  // the {0,4} group of lane 0 or 4 trips
    bool trip; // any other (lane, group) trips
};
static BlockFacts block_facts(const uint8_t *px, long stride, bool cols, const DctqConsts &C, Mutant m, double delta[24] = nullptr, bool tripped[24] = nullptr) {
    float dist[8][8];
    block_distances(px, stride, cols, C, dist);
    BlockFacts f = {false, false};
    for (int lane = 0; lane < 8; lane++) {
        float mx[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < 8; k++) {
            const int g = group_of(k);
            if (dist[lane][k] > mx[g]) mx[g] = dist[lane][k];
        }
        for (int g = 0; g < 3; g++) {
            const bool t = mx[g] > threshold(C, cols, lane, g, m);
            if (delta) delta[3 * lane + g] = 0.5 - (double)mx[g];
            if (tripped) tripped[3 * lane + g] = t;
            if (!t) continue;
            if (g == 2 && (lane == 0 || lane == 4)) f.tie = true;
            else f.trip = true;
        }
    }
    return f;
}

static uint64_t rng_state;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static bool read_file(const char *path, std::vector<uint8_t> &buf) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t tmp[65536];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
    fclose(f);
    return true;
}

static int fail(const char *msg) {
    fprintf(stderr, "strip_decisions_model: %s\n", msg);
    return 2;
}

static int mode_classes(const char *path, const DctqConsts &C, bool cols) {
    std::vector<uint8_t> buf;
    if (!read_file(path, buf) || buf.size() % 64 != 0) return fail("cannot read the blocks (64 bytes each)");
    printf("{\"beta\": [");
    for (int c = 0; c < 24; c++) printf("%s%.17g", c ? ", " : "", 0.5 - (double)threshold(C, cols, c / 3, c % 3, kTrue));
    printf("], \"blocks\": [");
    for (size_t b = 0; b < buf.size() / 64; b++) {
        double delta[24];
        bool tr[24];
        const BlockFacts f = block_facts(buf.data() + 64 * b, 8, cols, C, kTrue, delta, tr);
        printf("%s{\"tie\": %d, \"trip\": %d, \"delta\": [", b ? ", " : "", (int)f.tie, (int)f.trip);
        for (int c = 0; c < 24; c++) printf("%s%.17g", c ? ", " : "", delta[c]);
        printf("], \"tripped\": [");
        for (int c = 0; c < 24; c++) printf("%s%d", c ? ", " : "", (int)tr[c]);
        printf("]}");
    }
    printf("]}\n");
    return 0;
}

// Seeded random search: noise blocks of several amplitudes around several means.  Per class the first block that trips in this class
// alone (every other class at least two bands from its tie), and the first that trips nowhere, comes within [beta, 2 beta) of the tie in
// this class and stays two bands away in every other.
static int mode_search(const DctqConsts &C, bool cols, uint64_t seed, long tries) {
    rng_state = seed * 0x9E3779B97F4A7C15ull + 0x2545F4914F6CDD1Dull;
    double beta[24];
    for (int c = 0; c < 24; c++) beta[c] = 0.5 - (double)threshold(C, cols, c / 3, c % 3, kTrue);
    std::vector<uint8_t> found_t(24 * 64), found_a(24 * 64);
    bool have_t[24] = {false}, have_a[24] = {false};
    int left = 48;
    for (long n = 0; n < tries && left > 0; n++) {
        uint8_t px[64];
        const uint32_t shape = rnd();
        const int amp = 1 + (int)(shape & 0xffu), mean = (int)((shape >> 8) & 0xffu), mode = (int)((shape >> 16) & 3u);
        for (int k = 0; k < 64; k++) {
            int v = mode == 0 ? (int)(rnd() & 0xffu) : mean + (int)(rnd() % (uint32_t)amp) - amp / 2;
            px[k] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
        double delta[24];
        bool tr[24];
        block_facts(px, 8, cols, C, kTrue, delta, tr);
        int ntr = 0, nnear = 0, which_t = -1, which_n = -1; // tripped classes; classes closer than two bands
        for (int c = 0; c < 24; c++) {
            if (tr[c]) ntr++, which_t = c;
            if (delta[c] < 2.0 * beta[c]) nnear++, which_n = c;
        }
        if (ntr == 1 && nnear == 1 && delta[which_t] < beta[which_t] && !have_t[which_t]) {
            have_t[which_t] = true, left--;
            memcpy(&found_t[64 * which_t], px, 64);
        } else if (ntr == 0 && nnear == 1 && delta[which_n] >= beta[which_n] && !have_a[which_n]) {
            have_a[which_n] = true, left--;
            memcpy(&found_a[64 * which_n], px, 64);
        }
    }
    printf("{\"tripped\": [");
    for (int c = 0, first = 1; c < 24; c++) {
        if (!have_t[c]) continue;
        printf("%s{\"class\": %d, \"px\": [", first ? "" : ", ", c);
        for (int k = 0; k < 64; k++) printf("%s%d", k ? "," : "", found_t[64 * c + k]);
        printf("]}");
        first = 0;
    }
    printf("], \"accepted\": [");
    for (int c = 0, first = 1; c < 24; c++) {
        if (!have_a[c]) continue;
        printf("%s{\"class\": %d, \"px\": [", first ? "" : ", ", c);
        for (int k = 0; k < 64; k++) printf("%s%d", k ? "," : "", found_a[64 * c + k]);
        printf("]}");
        first = 0;
    }
    printf("]}\n");
    return 0;
}

int main(int argc, char **argv) {
    std::string mode = "run", raw, blocks, mutant = "none", split = "15,13,10,7,5,3";
    long h = 0, w = 0, stride = 0, nframes = 1, frame_stride = 0, order = 1, tries = 2000000;
    long max_wgs = 0, sched = 1, chunk = 8, cus = 256, resident = 1536;
    double quality = 50.0;
    uint64_t seed = 0;
    bool have_seed = false, list_strips = false;
    int a = 1;
    if (a < argc && argv[a][0] != '-') mode = argv[a++];
    for (; a < argc; a++) {
        const std::string k = argv[a];
        if (k == "--strips") { list_strips = true; continue; }
        if (a + 1 >= argc) return fail("missing value");
        const char *v = argv[++a];
        if (k == "--h") h = atol(v);
        else if (k == "--w") w = atol(v);
        else if (k == "--stride") stride = atol(v);
        else if (k == "--nframes") nframes = atol(v);
        else if (k == "--frame-stride") frame_stride = atol(v);
        else if (k == "--quality") quality = atof(v);
        else if (k == "--order") order = atol(v);
        else if (k == "--max-wgs") max_wgs = atol(v);
        else if (k == "--sched") sched = atol(v);
        else if (k == "--chunk") chunk = atol(v);
        else if (k == "--split") split = v;
        else if (k == "--cus") cus = atol(v);
        else if (k == "--resident") resident = atol(v);
        else if (k == "--raw") raw = v;
        else if (k == "--blocks") blocks = v;
        else if (k == "--seed") seed = strtoull(v, nullptr, 10), have_seed = true;
        else if (k == "--tries") tries = atol(v);
        else if (k == "--mutant") mutant = v;
        else return fail("unknown option");
    }
    static DctqConsts C;
    if (!build_consts(quality, &C)) return fail("quality outside 1..99");
    if (order != 0 && order != 1) return fail("--order 0 (rows first) or 1 (columns first)");
    const bool cols = order == 1;
    Mutant m;
    if (mutant == "none") m = kTrue;
    else if (mutant == "swap_groups") m = kSwapGroups;
    else if (mutant == "lane_xor1") m = kLaneXor1;
    else if (mutant == "other_table") m = kOtherTable;
    else if (mutant == "rat_thr_all") m = kRatThrAll;
    else return fail("unknown mutant");
    if (mode == "classes") return mode_classes(blocks.c_str(), C, cols);
    if (mode == "search") return mode_search(C, cols, seed, tries);
    if (mode != "run") return fail("unknown mode");

    if (h <= 0 || w <= 0 || stride < w || nframes < 1 || h > (1 << 20) || w > (1 << 20) || nframes > 65535) return fail("bad geometry");
    if (frame_stride == 0) frame_stride = h * stride;
    if (frame_stride < h * stride) return fail("frame stride smaller than a frame");
    const size_t total = (size_t)frame_stride * (size_t)(nframes - 1) + (size_t)h * (size_t)stride;
    std::vector<uint8_t> img;
    if (!raw.empty()) {
        if (!read_file(raw.c_str(), img)) return fail("cannot read the frame");
        if (img.size() < total - (size_t)(stride - w)) return fail("frame file too short");
        img.resize(total, 0);
    } else if (have_seed) {
        rng_state = seed * 0x9E3779B97F4A7C15ull + 0x2545F4914F6CDD1Dull;
        img.resize(total);
        for (size_t k = 0; k < total; k++) img[k] = (uint8_t)(rnd() & 0xffu);
    } else
        return fail("--raw FILE or --seed N");

    StripTune tune{};
    tune.cus = (int)cus, tune.resident = (int)resident, tune.max_wgs = (int)max_wgs, tune.sched = (int)sched, tune.chunk = (int)chunk;
    {
        const char *sp = split.c_str();
        for (int k = 0; k < 8 && sp && *sp; k++) {
            tune.split[k] = atoi(sp);
            sp = strchr(sp, ',');
            if (sp) sp++;
        }
    }
    // (the launcher's test of the frame: 8-byte aligned rows and frames; the device buffer itself is aligned)
    const int aligned8 = (stride % 8 == 0) && (nframes == 1 || frame_stride % 8 == 0);
    const StripFrame fr = {(int)h, (int)w, stride, (int)((w + 7) / 8), aligned8, (int)nframes};
    const StripPlan pl = strip_plan(fr, tune);
    unsigned long long stats[4] = {0, 0, 0, 0};
    long n_tie_blocks = 0, n_trip_blocks = 0, n_trip_strips = 0, n_blocks = 0;
    std::string strips_json;
    if (pl.launch) {
        const uint32_t nfast = pl.hd.nfast;
        std::vector<uint8_t> tie(nfast), mask(nfast);
        std::vector<uint8_t> seen(nfast);
        for (long z = 0; z < nframes; z++) {
            const uint8_t *plane = img.data() + (size_t)z * (size_t)frame_stride;
            for (uint32_t t = 0; t < nfast; t++) {
                const uint32_t ty = t / (uint32_t)pl.fast_tx, tx = t % (uint32_t)pl.fast_tx;
                uint8_t tb = 0, mb = 0;
                for (int b = 0; b < 8; b++) {
                    const BlockFacts f = block_facts(plane + (size_t)ty * 8 * (size_t)stride + (size_t)tx * 64 + (size_t)b * 8, stride, cols, C, m);
                    if (f.tie) tb = 1, n_tie_blocks++;
                    if (f.trip) mb |= (uint8_t)(1u << b), n_trip_blocks++;
                    n_blocks++;
                }
                tie[t] = tb, mask[t] = mb;
                if (mb) n_trip_strips++;
                if (list_strips && (tb || mb)) {
                    char line[96];
                    snprintf(line, sizeof line, "%s[%ld, %u, %d, %u]", strips_json.empty() ? "" : ", ", z, t, (int)tb, (unsigned)mb);
                    strips_json += line;
                }
            }
            std::fill(seen.begin(), seen.end(), 0);
            const StripHead &hd = pl.hd;
            const uint32_t in_wrap32 = strip_in_wrap(hd);
            for (uint32_t by = 0; by < pl.grid_y; by++)
                for (uint32_t bx = 0; bx < pl.grid_x; bx++)
                    for (uint32_t wave = 0; wave < (uint32_t)kStripWavesPerWG; wave++) {
                        const StripCursor cur = strip_cursor(hd, pl.wm, bx, by, wave);
                        if (cur.n_my > kStripMaxPerWave) return fail("a wave walks more than 64 strips");
                        uint32_t txp = cur.txp, in_off = cur.in_off, oblk = strip_oblk(cur.ty, cur.txp, pl.wm);
                        int nE = 0;
                        for (int k = 0; k < cur.n_my; k++) {
                            // the strip the cursor stands on, from its pixel offset (the plan's own walk, not t_first + k * tstep)
                            const uint32_t ty = in_off / (8u * hd.stride), tx = (in_off % (8u * hd.stride)) / 64u;
                            if (tx != txp || tx >= hd.fast_tx) return fail("the walk left the fast rectangle");
                            const uint32_t t = ty * hd.fast_tx + tx;
                            if (t >= nfast || seen[t]) return fail("a strip outside the rectangle, or walked twice");
                            seen[t] = 1;
                            if (tie[t]) stats[1]++;
                            if (mask[t]) {
                                const int nnew = __builtin_popcount(mask[t]);
                                if (nE + nnew <= 8 && mask[t] != 0xff) nE += nnew, stats[0] += (unsigned long long)nnew;
                                else stats[2]++;
                            }
                            strip_step(txp, in_off, oblk, hd.step_tx, hd.fast_tx, hd.in_step32, in_wrap32, pl.wm);
                        }
                        if ((unsigned long long)nE > stats[3]) stats[3] = (unsigned long long)nE;
                    }
            for (uint32_t t = 0; t < nfast; t++)
                if (!seen[t]) return fail("a strip nobody walked");
        }
    }
    // the plan in the terms of tic_last_strip_launch: order (0 none, 1 rows first, 2 columns first), kind, teams, grid x, y, tstep, fast x, y
    printf("{\"stats\": [%llu, %llu, %llu, %llu], \"plan\": [%d, %d, %d, %d, %d, %d, %d, %d], \"multi_round\": %d, ", stats[0], stats[1], stats[2], stats[3],
           pl.launch ? (cols ? 2 : 1) : 0, pl.launch ? (int)(pl.hd.misc & 0xffu) : 0, pl.launch ? pl.team_count : 0, pl.launch ? (int)pl.grid_x : 0,
           pl.launch ? (int)pl.grid_y : 0, pl.launch ? pl.tstep : 0, pl.fast_tx, pl.fast_ty, (int)pl.multi_round);
    printf("\"blocks\": %ld, \"tie_blocks\": %ld, \"trip_blocks\": %ld, \"trip_strips\": %ld, \"fast_strips\": %ld", n_blocks, n_tie_blocks, n_trip_blocks, n_trip_strips,
           pl.launch ? (long)pl.hd.nfast * nframes : 0L);
    if (list_strips) printf(", \"strips\": [%s]", strips_json.c_str());
    printf("}\n");
    return 0;
}
