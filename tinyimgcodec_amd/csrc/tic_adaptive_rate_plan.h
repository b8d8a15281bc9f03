// tic_adaptive_rate_plan.h - the host plan of the adaptive statistics probe kernel (adaptive_stats_probe_kernel_v,
// tic_adaptive_stats_gpu.hip), free of HIP and of the context.  The kernel finds its probes through the size kernel's table
// (fill_size_probe_table, tic_rate_plan.h: unchanged); what it adds is a cap on a probe's workgroups below the plan's own.
// tests/native/adaptive_size_selftest.cpp compiles it alone and sweeps it under the address and undefined-behaviour sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "tic_rate_plan.h"

namespace tic {

// A workgroup counts its symbols in 32-bit words of LDS: at most 66 per block (a DC, 63 AC entries with no ZRL among them or fewer with
// some, an EOB), so a workgroup may walk this many blocks at most.
constexpr size_t kAdaptProbeGroupBlocks = (size_t)1 << 25;

// Caps every probe of a filled table at max_groups workgroups (0: the table stays as fill_size_probe_table left it) and renumbers the
// grid: probes keep their order, blocks and results; a capped probe's waves stride further.  *ngroups: the launch's grid.  False (the
// table is then unusable) when max_groups is negative or a workgroup of a probe would walk more than kAdaptProbeGroupBlocks blocks.
inline bool cap_probe_groups(SizeProbeTable *t, int n, int max_groups, size_t *ngroups) {
    if (n < 1 || n > kSizeMaxProbes || max_groups < 0) return false;
    size_t grp = 0;
    for (int k = 0; k < n; k++) {
        SizeProbeRec &r = t->rec[k];
        size_t g = r.ngroups;
        if (max_groups && g > (size_t)max_groups) g = (size_t)max_groups;
        if (g == 0 || (r.nblocks + g - 1) / g > kAdaptProbeGroupBlocks) return false;
        r.first_group = (uint32_t)grp, r.ngroups = (uint32_t)g;
        t->first_group[k] = (uint32_t)grp;
        grp += g;
    }
    *ngroups = grp;
    return true;
}

} // namespace tic
