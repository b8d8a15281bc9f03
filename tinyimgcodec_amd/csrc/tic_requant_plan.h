// tic_requant_plan.h - the host plan of requantisation, free of HIP and of the context: the table the store kernel's descriptor form reads
// (requant_kernel_v, tic_requant_gpu.hip), the chunk arithmetic of a wave's walk, which both kernels share, and the measuring kernel's grid.  tests/native/requant_plan_selftest.cpp compiles it alone and sweeps it under the address
// and undefined-behaviour sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "tic_rate_plan.h"

#if defined(__HIPCC__)
#define TIC_RQ_HD __host__ __device__ inline
#else
#define TIC_RQ_HD inline
#endif

namespace tic {

// ---- the walk both kernels and the self-test share --------------------------------------------------------------------------------------
// A workgroup is kRequantWaves waves; a wave takes CHUNKS of 8 consecutive blocks and keeps kRequantUnroll of them in flight per round.  The
// waves that share a span of blocks (a job's, or a frame's) stride over its chunks: wave `first_chunk` of `nwaves` takes, in the round that
// starts at `base` (first_chunk, first_chunk + nwaves * kRequantUnroll, ...), the chunks base + u * nwaves, u = 0 .. kRequantUnroll - 1.
constexpr int kRequantWaves = 4, kRequantUnroll = 4;
static_assert(kSizeGroupChunks == (size_t)(kRequantWaves * kRequantUnroll), "a workgroup's round is what the job table counts groups by");
struct RequantWalk {
    unsigned long long nblocks, nchunks, first_chunk, nwaves;
};
// The walk of wave `wave` of workgroup `group` among the `ngroups` workgroups of a span of nblocks blocks.
TIC_RQ_HD RequantWalk requant_walk(unsigned long long nblocks, unsigned long long group, unsigned long long ngroups, int wave) {
    return RequantWalk{nblocks, (nblocks + 7ull) / 8ull, group * kRequantWaves + (unsigned long long)wave, ngroups * kRequantWaves};
}
TIC_RQ_HD unsigned long long requant_round_stride(const RequantWalk &w) { return w.nwaves * kRequantUnroll; }
// The block of the span that `lane` (8 lanes per block) holds in chunk u of the round at `base`; false: none (behind the span's end).
TIC_RQ_HD bool requant_lane_block(const RequantWalk &w, unsigned long long base, int u, int lane, unsigned long long *chunk, unsigned long long *blk) {
    *chunk = base + (unsigned long long)u * w.nwaves;
    *blk = *chunk * 8ull + (unsigned long long)(lane >> 3);
    return *chunk < w.nchunks && *blk < w.nblocks;
}

// A JOB is a run of source blocks requantised from one quality to another.  A launch takes up to kSizeMaxProbes of them (one table entry per
// lane of a wave, found as the size kernel finds its probe); a job's workgroups are the size kernel's (size_probe_groups: one per 16 chunks of
// 8 blocks, at most kSizeMaxGroups, beyond that the waves stride).  Jobs may share their source (one frame at many target qualities); their
// destinations must not overlap each other.  A destination may be its own source (each lane stores the 16 bytes it loaded).
struct RequantJobRec {
    unsigned long long src_block; // first source block in the launch's source coefficients, 64 each
    unsigned long long dst_block; // first destination block in the launch's destination
    unsigned long long nblocks;
    uint32_t first_group, ngroups; // its workgroups: [first_group, first_group + ngroups) of the grid
    uint32_t q_from, q_to;         // 1..99: indices into the context's constants (DctqConsts::div)
    uint32_t flag;                 // the range flag it raises
    uint32_t pad;
};
static_assert(sizeof(RequantJobRec) == 48, "a record is 48 bytes");
struct RequantJobTable {
    uint32_t first_group[kSizeMaxProbes]; // 0xffffffff behind the last job
    RequantJobRec rec[kSizeMaxProbes];
};

// What one launch owns in the context's table buffers, pinned and on the device: its table and the range flags of its jobs.  One copy brings
// table and zeroed flags up, one brings the flags back.
struct RequantLaunch {
    RequantJobTable tab;
    uint32_t flags[kSizeMaxProbes];
};

struct RequantJobIn {
    size_t src_block, dst_block, nblocks;
    int q_from, q_to;
    uint32_t flag;
};

// Fills `t` for n jobs (1..kSizeMaxProbes) of at least one block each and qualities inside 1..99.  *ngroups: the launch's grid.  src_cap /
// dst_cap: the blocks the launch's source and destination hold - a job that reaches past either is refused, as are two destinations that
// overlap.  (Whether source and destination are the same memory is the caller's: then a job's destination must be its own source and no
// other job may read it.)  False: the table is not usable.
inline bool fill_requant_job_table(RequantJobTable *t, int n, const RequantJobIn *in, size_t src_cap, size_t dst_cap, size_t *ngroups) {
    if (n < 1 || n > kSizeMaxProbes) return false;
    for (int k = 0; k < kSizeMaxProbes; k++) {
        t->first_group[k] = 0xffffffffu;
        t->rec[k] = RequantJobRec();
    }
    size_t grp = 0;
    for (int k = 0; k < n; k++) {
        const RequantJobIn &j = in[k];
        if (j.nblocks == 0 || j.q_from < 1 || j.q_from > 99 || j.q_to < 1 || j.q_to > 99 || j.flag >= (uint32_t)kSizeMaxProbes) return false;
        if (j.src_block > src_cap || j.nblocks > src_cap - j.src_block) return false;
        if (j.dst_block > dst_cap || j.nblocks > dst_cap - j.dst_block) return false;
        for (int i = 0; i < k; i++) // (64 jobs at most: the quadratic check is 2,016 comparisons)
            if (j.dst_block < in[i].dst_block + in[i].nblocks && in[i].dst_block < j.dst_block + j.nblocks) return false;
        const size_t groups = size_probe_groups(j.nblocks);
        RequantJobRec &r = t->rec[k];
        r.src_block = j.src_block, r.dst_block = j.dst_block, r.nblocks = j.nblocks;
        r.first_group = (uint32_t)grp, r.ngroups = (uint32_t)groups;
        r.q_from = (uint32_t)j.q_from, r.q_to = (uint32_t)j.q_to, r.flag = j.flag;
        t->first_group[k] = (uint32_t)grp;
        grp += groups;
    }
    *ngroups = grp;
    return true;
}

// The measuring kernel's grid for a frame of n blocks at nq qualities: size_probe_groups(n) workgroups walk the frame; where those are too
// few to fill the device, `split` of them share each round of chunks and divide the qualities among themselves (every split-th one) - the
// frame is then read `split` times, out of the cache.  kRequantFillGroups: four workgroups per CU of a 256-CU device.
constexpr size_t kRequantFillGroups = 1024;
inline size_t requant_size_split(size_t n, size_t nq) {
    const size_t g = size_probe_groups(n);
    size_t split = g >= kRequantFillGroups ? 1 : (kRequantFillGroups + g - 1) / g;
    if (split > nq) split = nq;
    return split < 1 ? 1 : split;
}

} // namespace tic
