// tic_strip_plan.h - the schedule of the strip kernel (dctq_strip_kernel, tic_kernels.hip), free of HIP: which workgroups and waves walk which
// strips of a frame's fast rectangle.  Two halves that must agree and therefore live in one file:
//   strip_plan()   (host)          : the launcher's schedule arithmetic - grid, schedule kind, the words the kernel gets
//   strip_cursor() (host + device) : what the kernel's prologue makes of those words - a wave's first strip, its count, its first offsets
//   strip_step()   (host + device) : the walk's step and wrap rule (the kernel's pixel-load macros call it, and its two halves)
// tests/native/strip_plan_selftest.cpp walks every (workgroup, wave) of a set of frames on the CPU with these very functions, under the
// address and undefined-behaviour sanitizers: every strip once, every offset inside the frame, no wave beyond 64 strips.
//
// A strip is 8 horizontally adjacent blocks (64 x 8 pixels); the fast rectangle is [0, fast_ty) x [0, fast_tx) strips, numbered row by row;
// a workgroup has 4 waves.  Three kinds of schedule:
//   rows  : a 2-D grid, x = workgroup of a round, y = round.  The rectangle is cut into rows of tstep = 4 * grid.x strips; round r takes rows
//           [split byte r, split byte r + 1), wave (x, wave) strip 4 * x + wave of each.  The team schedule (grids that are resident at once:
//           later rounds start later and get fewer rows) and the strided schedule (one round that takes every row) are both this form.  The
//           strip count needs no division: only the last row of the rectangle can be partial.
//   chunk : workgroup x streams strips [4 * S * x, 4 * S * (x + 1)), its waves interleaved (tstep = 4): the count is a shift.
//   round : rounds of round_wgs workgroups walking a dense range together (a test-hook schedule: keeps the general form, one division).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TIC_PLAN_HD __host__ __device__ __forceinline__
#else
#define TIC_PLAN_HD inline
#endif

namespace tic {

constexpr int kStripWavesPerWG = 4;      // (== kWavesPerWG, tic_kernels.hip asserts it)
constexpr int kStripMaxPerWave = 64;     // one bit per strip of a wave's walk in the kernel's exact-redo mask
constexpr int kStripResidentPerWave = 16; // a grid is "larger than the chip" when its waves would walk more strips than this
enum : uint32_t { kStripRows = 0, kStripChunk = 1, kStripRound = 2 };

// The schedule words every wave's start needs before its first pixel load.  With the image pointer and the constants pointer they are the
// kernel's leading arguments, 14 dwords in all: what kernel-argument preload can deliver in user SGPRs at wave launch.
struct StripHead {
    unsigned long long split; // rows: byte r = first row of round r, r = 0..7 (byte 8: misc)
    uint32_t stride;          // bytes between pixel rows (frames of the strip kernel are < 4 GiB)
    uint32_t misc;            // bits 0..7 schedule kind | 8..15 split byte 8 | 16..23 chunk: strips per wave S
    uint32_t tstep;           // strips a wave advances by
    uint32_t nfast;           // fast_ty * fast_tx
    uint32_t fast_tx;
    uint32_t magic_fast_tx;   // floor(2^32 / fast_tx) + 1, 0 for fast_tx = 1: mulhi(n, magic) = n / fast_tx while n * fast_tx < 2^32
    uint32_t in_step32;       // advancing by tstep strips adds this to the pixel offset ...
    uint32_t step_tx;         // ... and tstep % fast_tx to the strip column
};
// What the start needs behind the first loads, and the loop's other invariants: one 64-byte line of the kernel arguments.
struct alignas(64) StripWarm {
    int16_t *out;
    long frame_stride_in, frame_stride_out;          // batch of equally sized frames: grid plane z = frame
    uint32_t oblk_step, oblk_wrap;                   // block index: per step, and added when the strip column wraps
    uint32_t bw;                                     // blocks per block row
    uint32_t round_wgs, round_span, magic_round_wgs; // round schedule only
};
static_assert(sizeof(StripWarm) == 64, "one cache line");

struct StripCursor {
    uint32_t t_first; // first strip of the walk (0 for a wave without strips: it loads, and discards, strip 0)
    uint32_t txp;     // its column
    uint32_t ty;      // its row
    uint32_t in_off;  // byte offset of its first pixel
    int n_my;         // strips in the walk
};

TIC_PLAN_HD uint32_t strip_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((unsigned long long)a * b) >> 32); }
TIC_PLAN_HD uint32_t strip_in_wrap(const StripHead &h) { return 8u * h.stride - 64u * h.fast_tx; } // added to the pixel offset on a wrap

// (workgroup (bx, by), wave) -> the wave's cursor.  In the rows and chunk schedules it depends on the head alone (the kernel issues its first
// pixel loads before anything of `w` has arrived); the index of the first block, strip_oblk, needs w.bw.
TIC_PLAN_HD StripCursor strip_cursor(const StripHead &h, const StripWarm &w, uint32_t bx, uint32_t by, uint32_t wave) {
    const uint32_t kind = h.misc & 0xffu;
    uint32_t tf;
    int n;
    if (kind == kStripRows) {
        const uint32_t row0 = (uint32_t)(h.split >> (8u * (by & 7u))) & 0xffu;
        const uint32_t row1 = by < 7u ? (uint32_t)(h.split >> (8u * by + 8u)) & 0xffu : (h.misc >> 8) & 0xffu;
        const uint32_t rows = row1 - row0;
        tf = row0 * h.tstep + bx * (uint32_t)kStripWavesPerWG + wave;
        // all rows but the rectangle's last are complete: the walk loses at most its last strip (rows = 0: `last` wraps, n = -1 -> 0)
        const uint32_t last = tf + (rows - 1u) * h.tstep;
        n = (int)rows - (last >= h.nfast ? 1 : 0);
        n = n < 0 ? 0 : n;
    } else if (kind == kStripChunk) {
        const uint32_t span = ((h.misc >> 16) & 0xffu) * (uint32_t)kStripWavesPerWG;
        const uint32_t base = bx * span;
        const uint32_t lim = base + span < h.nfast ? base + span : h.nfast;
        tf = base + wave;
        n = tf < lim ? (int)((lim - tf + (uint32_t)kStripWavesPerWG - 1u) / (uint32_t)kStripWavesPerWG) : 0;
    } else {
        const uint32_t rho = w.magic_round_wgs ? strip_mulhi(bx, w.magic_round_wgs) : bx;
        const uint32_t wl = bx - rho * w.round_wgs;
        const uint32_t base = rho * w.round_wgs * w.round_span;
        const uint32_t lim = base + w.round_wgs * w.round_span < h.nfast ? base + w.round_wgs * w.round_span : h.nfast;
        tf = base + wl * (uint32_t)kStripWavesPerWG + wave;
        n = tf < lim ? (int)((lim - tf + h.tstep - 1u) / h.tstep) : 0;
    }
    StripCursor c;
    c.n_my = n;
    c.t_first = n == 0 ? 0u : tf;
    const uint32_t ty = h.magic_fast_tx ? strip_mulhi(c.t_first, h.magic_fast_tx) : c.t_first; // (magic 0: one strip per row)
    c.txp = c.t_first - ty * h.fast_tx;
    c.ty = ty;
    c.in_off = ty * (8u * h.stride) + c.txp * 64u;
    return c;
}
TIC_PLAN_HD uint32_t strip_oblk(uint32_t ty, uint32_t txp, const StripWarm &w) { return ty * w.bw + txp * 8u; }

// The walk's step: tstep strips on, the wrap terms when the column passes fast_tx (at most once: step_tx < fast_tx).  In two halves, the
// pixel offset (returns whether the column wrapped) and the block index: the kernel's first two loads take the first half alone.
TIC_PLAN_HD bool strip_step_in(uint32_t &txp, uint32_t &in_off, uint32_t step_tx, uint32_t fast_tx, uint32_t in_step32, uint32_t in_wrap32) {
    txp += step_tx, in_off += in_step32;
    const bool wrap = txp >= fast_tx;
    if (__builtin_expect(wrap, 0)) txp -= fast_tx, in_off += in_wrap32;
    return wrap;
}
TIC_PLAN_HD void strip_step_blk(uint32_t &oblk, bool wrap, const StripWarm &w) { oblk += w.oblk_step + (wrap ? w.oblk_wrap : 0u); }
// Both halves at once: the step of the kernel's loop.
TIC_PLAN_HD void strip_step(uint32_t &txp, uint32_t &in_off, uint32_t &oblk, uint32_t step_tx, uint32_t fast_tx, uint32_t in_step32, uint32_t in_wrap32,
                            const StripWarm &w) {
    txp += step_tx, in_off += in_step32, oblk += w.oblk_step;
    if (__builtin_expect(txp >= fast_tx, 0)) txp -= fast_tx, in_off += in_wrap32, oblk += w.oblk_wrap;
}

// ---- host: the plan ----
struct StripFrame {
    int h, w;
    long stride; // bytes between rows
    int bw;      // blocks per row = ceil(w / 8)
    int aligned8; // image pointer and stride are multiples of 8
    int nframes; // >= 1
};
struct StripTune {
    int cus, resident; // compute units; workgroups the chip holds at once (cus * resident workgroups per CU)
    int max_wgs;       // persistent grid size (0: `resident`)
    int sched;         // grids larger than the chip: 0 strided, 1 chunked, 2 round-interleaved
    int chunk;         // strips per wave of schedules 1 and 2
    int split[8];      // per-round row weights of the team schedule (split[0] <= 0 disables it)
};
struct StripPlan {
    bool launch;      // the strip kernel runs (else the exact kernel takes the whole frame)
    bool multi_round; // more workgroups than the chip holds at once
    int fast_tx, fast_ty; // the fast rectangle (0 x 0 when !launch)
    uint32_t grid_x, grid_y;
    StripHead hd;
    StripWarm wm;     // the schedule's fields of it (out and the frame strides are the launcher's)
    // the same schedule in the terms of DctqArgs (diagnostics, the kernel's rare paths)
    int nwaves, wg_stride, tstep, wg_span, round_wgs, team_count, step_ty, step_tx;
    int split[9];
    uint32_t in_wrap32;
};

inline uint32_t strip_magic(long d) { return d <= 1 ? 0u : (uint32_t)((1ull << 32) / (unsigned long long)d + 1ull); } // 0: divisor 1

inline StripPlan strip_plan(const StripFrame &f, const StripTune &tune) {
    StripPlan p{};
    const int W = kStripWavesPerWG, max_strips = kStripMaxPerWave;
    const int nf = f.nframes > 0 ? f.nframes : 1;
    p.fast_tx = (f.aligned8 && (long)f.h * f.stride < (1L << 32)) ? f.w / 64 : 0; // 32-bit pixel offsets in the walk
    p.fast_ty = f.h / 8;
    const int nfast = p.fast_tx * p.fast_ty;
    if (nfast <= 0) {
        p.fast_tx = p.fast_ty = 0;
        return p;
    }
    // persistent waves, each looping over its strips; one mask bit per strip of a wave's walk: at most 64 strips per wave.
    // persistent grid = exactly the workgroups the chip holds at once: a larger grid runs in two uneven rounds, a smaller one leaves wave
    // slots empty
    int wgs = (nfast + W - 1) / W;
    const int cap_env = tune.max_wgs > 0 ? tune.max_wgs : tune.resident;
    int cap = cap_env / nf; // a batch shares the chip's wave slots between its frames
    if (cap < 64) cap = 64;
    if (wgs > cap) wgs = cap;
    const int min_wgs = (nfast + W * max_strips - 1) / (W * max_strips);
    if (wgs < min_wgs) wgs = min_wgs; // strips per wave are bounded (exact-redo mask)
    p.nwaves = wgs * W;
    p.wg_stride = W;
    p.tstep = p.nwaves;
    p.wg_span = nfast;
    uint32_t kind = kStripRows;
    const int S = tune.chunk < 1 ? 1 : (tune.chunk > max_strips ? max_strips : tune.chunk);
    const int min_wgs16 = (nfast + W * kStripResidentPerWave - 1) / (W * kStripResidentPerWave);
    p.multi_round = (long)min_wgs16 * nf > (long)cap_env;
    if (tune.sched == 1 && p.multi_round) { // each workgroup streams a contiguous chunk of 4*S strips
        kind = kStripChunk;
        p.wg_stride = p.wg_span = W * S;
        p.tstep = W;
        wgs = (nfast + p.wg_stride - 1) / p.wg_stride;
        p.nwaves = wgs * W;
    } else if (tune.sched == 2 && p.multi_round && nf == 1) { // rounds of `resident` workgroups walking a dense range together
        kind = kStripRound;
        p.round_wgs = cap_env;
        p.wg_span = W * S;
        p.tstep = p.round_wgs * W;
        wgs = (nfast + p.wg_span - 1) / p.wg_span; // the last round may hold workgroups with nothing to do
        wgs = (wgs + p.round_wgs - 1) / p.round_wgs * p.round_wgs;
        p.nwaves = wgs * W;
    }
    p.grid_x = (uint32_t)wgs, p.grid_y = 1;
    int R = 1; // rounds of the rows form
    if (kind == kStripRows) {
        p.split[0] = 0;
        p.split[1] = (nfast + p.tstep - 1) / p.tstep; // strided: one round, every row (<= 64: min_wgs)
    }
    if (!p.multi_round && nf == 1 && tune.split[0] > 0 && wgs == cap_env && tune.cus > 0 && wgs % tune.cus == 0 && wgs / tune.cus <= 8) {
        // the whole grid is resident: teams of wgs/cus workgroups (in practice the workgroups of one CU, dispatched one round after the
        // other), rows split by the per-round weights - later rounds start later and get fewer rows, so that all waves end together
        const int Rt = wgs / tune.cus;
        const int tstep = tune.cus * W;
        const int rows_total = (nfast + tstep - 1) / tstep;
        int split[9] = {0};
        bool ok = rows_total <= 255; // the kernel takes the row boundaries as bytes
        double wsum = 0, acc = 0;
        for (int r = 0; r < Rt; r++) wsum += tune.split[r] > 0 ? tune.split[r] : 1;
        for (int r = 0; r < Rt; r++) {
            acc += tune.split[r] > 0 ? tune.split[r] : 1;
            split[r + 1] = r + 1 == Rt ? rows_total : (int)(rows_total * acc / wsum + 0.5);
        }
        for (int r = 0; r < Rt; r++)
            if (split[r + 1] - split[r] > max_strips) ok = false; // strips per wave are bounded: fall back to one round
        if (ok) {
            p.team_count = tune.cus;
            p.tstep = tstep;
            R = Rt;
            for (int r = 0; r <= Rt; r++) p.split[r] = split[r];
            p.grid_x = (uint32_t)tune.cus, p.grid_y = (uint32_t)Rt;
        }
    }
    p.step_ty = p.tstep / p.fast_tx;
    p.step_tx = p.tstep % p.fast_tx;
    // exactness of the magic divisions: n * d < 2^32 for every dividend n the prologue can form (and no 32-bit strip index wraps); frames
    // beyond that (more than ~10^5 pixels wide and millions of strips) go through the exact kernel as a whole
    const unsigned long long dmax = (unsigned long long)(p.round_wgs > 0 ? p.round_wgs : p.tstep);
    if ((unsigned long long)nfast * (unsigned long long)p.fast_tx >= (1ull << 32) || ((unsigned long long)nfast + dmax) * dmax >= (1ull << 32)) {
        p.fast_tx = p.fast_ty = 0;
        return p;
    }
    p.launch = true;
    StripHead &h = p.hd;
    h.split = 0;
    h.misc = kind | ((uint32_t)(kind == kStripChunk ? S : 0) << 16);
    if (kind == kStripRows)
        for (int k = 0; k <= R; k++) {
            if (k < 8) h.split |= (unsigned long long)(p.split[k] & 0xff) << (8 * k);
            else h.misc |= (uint32_t)(p.split[k] & 0xff) << 8;
        }
    h.stride = (uint32_t)f.stride;
    h.tstep = (uint32_t)p.tstep;
    h.nfast = (uint32_t)nfast;
    h.fast_tx = (uint32_t)p.fast_tx;
    h.magic_fast_tx = strip_magic(p.fast_tx);
    h.in_step32 = (uint32_t)((long)p.step_ty * 8 * f.stride + (long)p.step_tx * 64);
    h.step_tx = (uint32_t)p.step_tx;
    p.in_wrap32 = strip_in_wrap(h);
    p.wm.oblk_step = (uint32_t)((long)p.step_ty * f.bw + (long)p.step_tx * 8);
    p.wm.oblk_wrap = (uint32_t)((long)f.bw - (long)p.fast_tx * 8);
    p.wm.bw = (uint32_t)f.bw;
    p.wm.round_wgs = (uint32_t)p.round_wgs;
    p.wm.round_span = (uint32_t)(kind == kStripRound ? p.wg_span : 0);
    p.wm.magic_round_wgs = kind == kStripRound ? strip_magic(p.round_wgs) : 0u;
    return p;
}
} // namespace tic
