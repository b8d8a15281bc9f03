// tic_scaled_frames.h - the per-frame records of the integer transform's descriptor form (fdctq_scaled_kernel_v, tic_scaled.hip), free of
// HIP: the batch entry points of tic_api.hip fill them, the kernel reads them, tests/native/scaledplan_selftest.cpp walks them on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace tic {

constexpr int kScaledMaxFrames = 64; // records per launch: one table entry per lane of a wave (= kEntropyMaxFrames)

// One frame of a launch: h x w pixels (multiples of 8) at img_base + img_off, rows `pitch` bytes apart, transformed at setting qf into blocks
// [first_block, first_block + (h / 8) * bw) of the launch's output.  A frame is walked in strips of 8 horizontally adjacent blocks, row of
// blocks by row of blocks; first_strip: the strips of the records in front of it (a prefix sum - a row's last strip may be short, so it is no
// function of first_block).  Two records may name the same pixels with different settings and different output blocks.
struct ScaledFrameRec {
    unsigned long long img_off;     // bytes from the table's img_base to the frame's first pixel
    long long pitch;                // bytes between pixel rows
    unsigned long long first_block; // in the launch's output, 64 coefficients each
    uint32_t bw;                    // blocks per row = w / 8
    uint32_t tiles_x;               // strips per row of blocks = ceil(bw / 8)
    uint32_t first_strip;           // prefix sum over the launch
    uint32_t nstrips;               // (h / 8) * tiles_x
    int32_t qf;                     // 0 best, 1 high, 2 med, 3 low
    uint32_t aligned8;              // address and pitch are multiples of 8: one 8-byte load per lane
    uint32_t pad[4];
};
static_assert(sizeof(ScaledFrameRec) == 64, "a record is 64 bytes");

// The table a launch reads.  A wave finds a strip's record by ONE load per lane and a ballot: lane l compares first_strip[l] with the strip's
// index; entries behind the last record are 0xffffffff.
struct ScaledFrameTable {
    uint32_t first_strip[kScaledMaxFrames];
    ScaledFrameRec rec[kScaledMaxFrames];
    unsigned long long img_base, out_base; // device addresses: pixels, int16 [blocks][64] zig-zag
};

// Fills `t` for n frames (1 <= n <= kScaledMaxFrames, every one with blocks): frame k of hs[k] x ws[k] pixels at img_base + img_off[k] with
// rows pitch[k] bytes apart, setting qfs[k], output from block first_block[k] on.  *total_strips: the launch's strips.  Returns false when n,
// a size or a setting is out of range or the strips do not fit 31 bits.
inline bool fill_scaled_table(ScaledFrameTable *t, int n, unsigned long long img_base, unsigned long long out_base, const unsigned long long *img_off,
                              const long long *pitch, const int *hs, const int *ws, const int *qfs, const unsigned long long *first_block,
                              uint32_t *total_strips) {
    if (n < 1 || n > kScaledMaxFrames) return false;
    for (int k = 0; k < kScaledMaxFrames; k++) {
        t->first_strip[k] = 0xffffffffu;
        t->rec[k] = ScaledFrameRec();
    }
    t->img_base = img_base, t->out_base = out_base;
    unsigned long long strip = 0;
    for (int k = 0; k < n; k++) {
        if (hs[k] < 8 || ws[k] < 8 || (hs[k] & 7) != 0 || (ws[k] & 7) != 0 || qfs[k] < 0 || qfs[k] > 3) return false;
        ScaledFrameRec &r = t->rec[k];
        r.img_off = img_off[k], r.pitch = pitch[k], r.first_block = first_block[k];
        r.bw = (uint32_t)ws[k] / 8u, r.tiles_x = (r.bw + 7u) / 8u;
        const unsigned long long strips = (unsigned long long)(hs[k] / 8) * r.tiles_x;
        if (strip + strips > 0x7fffffffull) return false;
        r.first_strip = (uint32_t)strip, r.nstrips = (uint32_t)strips;
        r.qf = qfs[k];
        r.aligned8 = (((img_base + img_off[k]) | (unsigned long long)pitch[k]) & 7ull) == 0ull;
        t->first_strip[k] = (uint32_t)strip;
        strip += strips;
    }
    *total_strips = (uint32_t)strip;
    return true;
}

// The record of strip g as the kernel's ballot finds it: the last one whose first_strip is <= g.
inline int scaled_record_of_strip(const ScaledFrameTable &t, uint32_t g) {
    int f = -1;
    for (int l = 0; l < kScaledMaxFrames; l++) f += t.first_strip[l] <= g;
    return f;
}

} // namespace tic
