// tic_entropy_frames.h - the per-frame records of the device entropy stage's descriptor form (entropy_gpu_fused_v), free of HIP: the host
// plan of a mixed batch (tic_host_pipeline.h) fills them, the kernels of tic_entropy_gpu.hip read them.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace tic {

enum { kEntropyLanePerBlock = 0, kEntropyEightLanes = 1 };

// How a packing mode cuts a frame: blocks per partition (a wave), partitions per packing workgroup (= per group sum), partitions per
// placing workgroup.  (tic_entropy_gpu.hip asserts that its kernels' constants are these.)
struct EntropyGeom {
    unsigned part_blocks, group_parts, place_parts;
};
inline EntropyGeom entropy_geom(int mode) { return mode == kEntropyLanePerBlock ? EntropyGeom{64u, 4u, 8u} : EntropyGeom{8u, 16u, 32u}; }
constexpr size_t kEntropyMaxGroups = 8192; // groups per frame up to which the placing kernel sums the group sums directly (32-bit sums)

constexpr int kEntropyMaxFrames = 64; // frames per launch of the descriptor form: one table entry per lane of a wave

// One frame of a launch.  first_part / first_group / first_place: the partitions, packing workgroups and placing workgroups of the frames
// in front of it (prefix sums: a frame's partitions are rounded up, so they are not functions of first_block).
struct EntropyFrameRec {
    unsigned long long first_block; // in d_zz, 64 coefficients each
    unsigned long long nblocks;
    unsigned long long out_off;     // byte offset of the frame's stream (16-byte header + payload) in d_out, a multiple of 16
    unsigned long long cap_words;   // payload words the stream area holds
    uint32_t first_part, first_group, first_place;
    int32_t h, w, quality;          // the header's fields
    uint32_t pad[2];
};
static_assert(sizeof(EntropyFrameRec) == 64, "a record is 64 bytes");

// The table a launch reads.  A workgroup finds its frame by ONE load per lane and a ballot: lane l compares first_group[l] (packing grid)
// or first_place[l] (placing grid) with the workgroup's index; entries behind the last frame are 0xffffffff.
struct EntropyFrameTable {
    uint32_t first_group[kEntropyMaxFrames];
    uint32_t first_place[kEntropyMaxFrames];
    EntropyFrameRec rec[kEntropyMaxFrames];
};

// Fills `t` for frames of nblocks[k] blocks (k < n <= kEntropyMaxFrames, every one >= 1), coefficients back to back, the stream of frame k at
// out_off[k] with cap_words[k] payload words.  Returns false when a frame has more than kEntropyMaxGroups groups or n is out of range.
// *nparts, *ngroups, *nplaces: the launch's totals.
inline bool fill_entropy_table(EntropyFrameTable *t, int mode, int n, const size_t *nblocks, const size_t *out_off, const size_t *cap_words,
                               const int *hs, const int *ws, const int *qs, size_t *nparts, size_t *ngroups, size_t *nplaces) {
    if (n < 1 || n > kEntropyMaxFrames) return false;
    const EntropyGeom g = entropy_geom(mode);
    size_t blk = 0, part = 0, grp = 0, plc = 0;
    for (int k = 0; k < kEntropyMaxFrames; k++) {
        t->first_group[k] = t->first_place[k] = 0xffffffffu;
        t->rec[k] = EntropyFrameRec();
    }
    for (int k = 0; k < n; k++) {
        if (nblocks[k] == 0) return false;
        const size_t parts = (nblocks[k] + g.part_blocks - 1) / g.part_blocks;
        const size_t groups = (parts + g.group_parts - 1) / g.group_parts, places = (parts + g.place_parts - 1) / g.place_parts;
        if (groups > kEntropyMaxGroups || part + parts > 0x7fffffffu) return false;
        EntropyFrameRec &r = t->rec[k];
        r.first_block = blk, r.nblocks = nblocks[k], r.out_off = out_off[k], r.cap_words = cap_words[k];
        r.first_part = (uint32_t)part, r.first_group = (uint32_t)grp, r.first_place = (uint32_t)plc;
        r.h = hs[k], r.w = ws[k], r.quality = qs[k];
        t->first_group[k] = (uint32_t)grp, t->first_place[k] = (uint32_t)plc;
        blk += nblocks[k], part += parts, grp += groups, plc += places;
    }
    *nparts = part, *ngroups = grp, *nplaces = plc;
    return true;
}

} // namespace tic
