// strip_plan_selftest.cpp - the strip kernel's schedule (csrc/tic_strip_plan.h) walked on the CPU: for each frame and schedule, strip_plan(), then
// strip_cursor() for every (workgroup, wave) of the grid, then the walk itself with the kernel's own step and wrap rule (strip_step, and its halves
// strip_step_in / strip_step_blk for the first two steps, as in the kernel).  Asserted: every strip of the fast rectangle is visited exactly once; every pixel offset lies inside the frame and is the
// offset of the strip the walk believes it is at; every block index is that strip's; no wave exceeds 64 strips; a wave without strips sits on
// strip 0; the cursor agrees with the general (dividing) form of the schedule written out below from the DctqArgs terms of the plan.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined strip_plan_selftest.cpp && ./a.out            -> "strip_plan_selftest ok"
//   ./a.out broken   (one strip taken off the rectangle the kernel is told about)                   -> "strip_plan_selftest FAILED", exit 1
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../tinyimgcodec_amd/csrc/tic_strip_plan.h"

using namespace tic;

static int g_fail = 0;
static bool g_broken = false;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            if (g_fail < 20) { printf("  FAIL %s: ", name); printf(__VA_ARGS__); printf("\n"); } \
            g_fail++;                                        \
        }                                                    \
    } while (0)

static StripTune tune_default() {
    StripTune t{};
    t.cus = 256, t.resident = 256 * 6, t.max_wgs = 0, t.sched = 1, t.chunk = 8;
    const int sp[8] = {15, 13, 10, 7, 5, 3, 0, 0};
    for (int k = 0; k < 8; k++) t.split[k] = sp[k];
    return t;
}

// The schedule's general form (what the kernel computed before the plan existed), from the plan's DctqArgs terms: first strip and count.
static void reference_cursor(const StripPlan &p, uint32_t bx, uint32_t by, uint32_t wave, uint32_t &tf, int &n) {
    const uint32_t nfast = (uint32_t)p.fast_tx * (uint32_t)p.fast_ty;
    uint32_t t_lim;
    if (p.team_count > 0) {
        tf = ((uint32_t)p.split[by] * (uint32_t)p.team_count + bx) * 4u + wave;
        t_lim = tf + (uint32_t)(p.split[by + 1] - p.split[by]) * (uint32_t)p.tstep;
    } else if (p.round_wgs > 0) {
        const uint32_t rho = bx / (uint32_t)p.round_wgs, wl = bx % (uint32_t)p.round_wgs;
        const uint32_t base = rho * (uint32_t)p.round_wgs * (uint32_t)p.wg_span;
        tf = base + wl * 4u + wave;
        t_lim = base + (uint32_t)p.round_wgs * (uint32_t)p.wg_span;
    } else {
        tf = bx * (uint32_t)p.wg_stride + wave;
        t_lim = bx * (uint32_t)p.wg_stride + (uint32_t)p.wg_span;
    }
    const uint32_t t_end = t_lim < nfast ? t_lim : nfast;
    n = tf < t_end ? (int)((t_end - tf + (uint32_t)p.tstep - 1u) / (uint32_t)p.tstep) : 0;
    if (n == 0) tf = 0;
}

struct Seen {
    bool launched;
    uint32_t kind;
    int team, fast_tx, fast_ty;
    uint32_t gx, gy;
    int max_n;
};

static Seen run_case(const char *name, int w, int h, long stride, int aligned8, int nframes, long gap, const StripTune &tune) {
    StripFrame f{h, w, stride, (w + 7) / 8, aligned8, nframes};
    StripPlan p = strip_plan(f, tune);
    Seen s{p.launch, p.hd.misc & 0xffu, p.team_count, p.fast_tx, p.fast_ty, p.grid_x, p.grid_y, 0};
    const long frame_bytes = (long)h * stride;
    const long frame_stride_in = frame_bytes + gap;
    if (!p.launch) {
        CHECK(p.fast_tx == 0 && p.fast_ty == 0, "no launch, but a fast rectangle %d x %d", p.fast_tx, p.fast_ty);
        printf("  %-34s no fast rectangle\n", name);
        return s;
    }
    CHECK(p.fast_tx == w / 64 && p.fast_ty == h / 8, "rectangle %d x %d", p.fast_tx, p.fast_ty);
    const uint32_t nfast = (uint32_t)p.fast_tx * (uint32_t)p.fast_ty;
    StripHead hd = p.hd;
    if (g_broken) hd.nfast -= 1;
    const StripWarm &wm = p.wm;
    const uint32_t in_wrap32 = strip_in_wrap(hd);
    CHECK(in_wrap32 == p.in_wrap32, "in_wrap32");
    for (int z = 0; z < (nframes > 0 ? nframes : 1); z++) {
        std::vector<unsigned char> visits(nfast, 0);
        const long frame0 = (long)z * frame_stride_in; // the frame's first byte, from the batch's
        for (uint32_t by = 0; by < p.grid_y; by++)
            for (uint32_t bx = 0; bx < p.grid_x; bx++)
                for (uint32_t wave = 0; wave < (uint32_t)kStripWavesPerWG; wave++) {
                    const StripCursor c = strip_cursor(hd, wm, bx, by, wave);
                    uint32_t tf_ref;
                    int n_ref;
                    reference_cursor(p, bx, by, wave, tf_ref, n_ref);
                    if (!g_broken) CHECK(c.t_first == tf_ref && c.n_my == n_ref, "wg (%u,%u) wave %u: cursor %u x %d, general form %u x %d", bx, by, wave, c.t_first, c.n_my, tf_ref, n_ref);
                    CHECK(c.n_my >= 0 && c.n_my <= kStripMaxPerWave, "wg (%u,%u) wave %u walks %d strips", bx, by, wave, c.n_my);
                    if (c.n_my > s.max_n) s.max_n = c.n_my;
                    if (c.n_my == 0) CHECK(c.t_first == 0 && c.in_off == 0 && c.txp == 0 && c.ty == 0, "idle wave not on strip 0");
                    uint32_t txp = c.txp, in_off = c.in_off, oblk = strip_oblk(c.ty, c.txp, wm);
                    for (int k = 0; k < c.n_my; k++) {
                        const unsigned long long t = (unsigned long long)c.t_first + (unsigned long long)k * hd.tstep;
                        if (t >= nfast) {
                            CHECK(false, "wg (%u,%u) wave %u step %d: strip %llu outside the rectangle", bx, by, wave, k, t);
                            break;
                        }
                        const uint32_t ty = (uint32_t)(t / (uint32_t)p.fast_tx), tx = (uint32_t)(t % (uint32_t)p.fast_tx);
                        const long off = (long)ty * 8 * stride + (long)tx * 64;
                        CHECK(txp == tx && (long)in_off == off, "wg (%u,%u) wave %u step %d: column %u offset %u, strip %llu is column %u offset %ld", bx, by, wave, k, txp, in_off, t, tx, off);
                        CHECK(oblk == ty * (uint32_t)f.bw + tx * 8u, "wg (%u,%u) wave %u step %d: block %u", bx, by, wave, k, oblk);
                        // the strip's last byte: pixel row 7, byte 63 - inside the frame's pixels, hence inside [frame0, frame0 + frame_bytes)
                        const long last = frame0 + (long)in_off + 7 * stride + 63;
                        CHECK(last < frame0 + (long)(h - 1) * stride + w && last < frame0 + frame_bytes, "wg (%u,%u) wave %u step %d: reads byte %ld of a frame of %ld", bx, by, wave, k, last - frame0, frame_bytes);
                        visits[(size_t)t]++;
                        if (k < 2) // as the kernel: its first two loads step in two halves (the block index follows behind the loads)
                            strip_step_blk(oblk, strip_step_in(txp, in_off, hd.step_tx, hd.fast_tx, hd.in_step32, in_wrap32), wm);
                        else
                            strip_step(txp, in_off, oblk, hd.step_tx, hd.fast_tx, hd.in_step32, in_wrap32, wm);
                    }
                }
        uint32_t missed = 0, twice = 0;
        for (uint32_t t = 0; t < nfast; t++) missed += visits[t] == 0, twice += visits[t] > 1;
        CHECK(missed == 0 && twice == 0, "frame %d: %u strips missed, %u visited more than once (of %u)", z, missed, twice, nfast);
    }
    static const char *kinds[3] = {"rows", "chunk", "round"};
    printf("  %-34s %6u strips, grid %u x %u x %d, %s%s, tstep %u, at most %d strips per wave\n", name, nfast, p.grid_x, p.grid_y, nframes, kinds[s.kind],
           p.team_count > 0 ? " (team)" : "", hd.tstep, s.max_n);
    return s;
}

int main(int argc, char **argv) {
    g_broken = argc > 1 && !strcmp(argv[1], "broken");
    const StripTune dflt = tune_default();
    const char *name = "";
    Seen s;
    printf("strip_plan_selftest%s\n", g_broken ? " (broken: the kernel is told of one strip fewer)" : "");
    name = "64x8";
    s = run_case(name, 64, 8, 64, 1, 1, 0, dflt); // one strip: 1 workgroup, three of its waves idle
    CHECK(s.launched && s.gx == 1 && s.max_n == 1, "one strip expected");
    name = "72x16";
    s = run_case(name, 72, 16, 72, 1, 1, 0, dflt); // 9 blocks per row: one strip per block row, the ninth block is the exact kernel's
    name = "72x16 rows not 8-aligned";
    s = run_case(name, 72, 16, 75, 0, 1, 0, dflt); // no fast rectangle
    CHECK(!s.launched, "an unaligned frame has no fast rectangle");
    name = "4096x8";
    s = run_case(name, 4096, 8, 4096, 1, 1, 0, dflt); // one strip row
    name = "1920x1080";
    s = run_case(name, 1920, 1080, 1920, 1, 1, 0, dflt); // 30 strips per row: the cursor wraps inside a walk
    name = "64x4096 (one strip per row)";
    s = run_case(name, 64, 4096, 64, 1, 1, 0, dflt); // magic 0
    name = "4096x4096";
    s = run_case(name, 4096, 4096, 4096, 1, 1, 0, dflt);
    CHECK(s.team == 256 && s.gy == 6 && s.kind == kStripRows, "4096^2 takes the team schedule");
    name = "4160x4096 pitch 4224";
    s = run_case(name, 4160, 4096, 4224, 1, 1, 0, dflt); // tstep no multiple of fast_tx, rows longer than the pixels
    // the smallest frame 2048 wide that takes the team schedule at 256 CUs x 6 under the plan's own rule, one block row fewer, one more
    {
        int h_team = 0;
        for (int h = 8; h <= 4096 && !h_team; h += 8) {
            StripFrame f{h, 2048, 2048, 256, 1, 1};
            if (strip_plan(f, dflt).team_count > 0) h_team = h;
        }
        printf("  smallest 2048-wide frame on the team schedule: 2048x%d\n", h_team);
        name = "team threshold";
        CHECK(h_team > 8, "no team frame found");
        std::string n0 = "2048x" + std::to_string(h_team - 8), n1 = "2048x" + std::to_string(h_team), n2 = "2048x" + std::to_string(h_team + 8);
        name = n0.c_str();
        s = run_case(name, 2048, h_team - 8, 2048, 1, 1, 0, dflt);
        CHECK(s.team == 0, "below the threshold");
        name = n1.c_str();
        s = run_case(name, 2048, h_team, 2048, 1, 1, 0, dflt);
        CHECK(s.team == 256, "at the threshold");
        name = n2.c_str();
        s = run_case(name, 2048, h_team + 8, 2048, 1, 1, 0, dflt);
        CHECK(s.team == 256, "above the threshold");
    }
    name = "3 x 1024x512, 4 KiB between frames";
    s = run_case(name, 1024, 512, 1024, 1, 3, 4096, dflt);
    for (int sched = 0; sched < 3; sched++) {
        StripTune t = dflt;
        t.max_wgs = 64, t.sched = sched;
        std::string n = "512x512, 64 workgroups, sched " + std::to_string(sched);
        name = n.c_str();
        s = run_case(name, 512, 512, 512, 1, 1, 0, t);
        CHECK(s.gx * s.gy == 64, "grid of %u x %u", s.gx, s.gy);
        n = "4096x4096, 64 workgroups, sched " + std::to_string(sched); // larger than such a chip: each schedule in its own form
        name = n.c_str();
        s = run_case(name, 4096, 4096, 4096, 1, 1, 0, t);
        CHECK(s.kind == (uint32_t)(sched == 0 ? kStripRows : (sched == 1 ? kStripChunk : kStripRound)), "schedule kind %u", s.kind);
        n = "1920x1080, 64 workgroups, sched " + std::to_string(sched);
        name = n.c_str();
        s = run_case(name, 1920, 1080, 1920, 1, 1, 0, t);
    }
    {
        StripTune t = dflt;
        t.max_wgs = 2048; // eight rounds: the ninth row boundary travels in `misc`
        name = "4096x4096, 2048 workgroups";
        s = run_case(name, 4096, 4096, 4096, 1, 1, 0, t);
        CHECK(s.team == 256 && s.gy == 8, "eight rounds expected");
        t = dflt, t.split[0] = 0;
        name = "4096x4096, no team";
        s = run_case(name, 4096, 4096, 4096, 1, 1, 0, t);
        CHECK(s.team == 0 && s.kind == kStripRows, "strided expected");
    }
    name = "16384x16384";
    s = run_case(name, 16384, 16384, 16384, 1, 1, 0, dflt);
    CHECK(s.kind == kStripChunk && s.max_n == 8, "16384^2 takes the chunked schedule");
    name = "256 x 1920x1080";
    s = run_case(name, 1920, 1080, 1920, 1, 256, 0, dflt);
    if (g_fail) {
        printf("strip_plan_selftest FAILED: %d checks\n", g_fail);
        return 1;
    }
    printf("strip_plan_selftest ok\n");
    return 0;
}
