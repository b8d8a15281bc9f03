// tic_adaptive_stats_gpu.h - the adaptive statistics of up to kSizeMaxProbes probes in one launch (see tic_adaptive_stats_gpu.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "tic_adaptive_frames.h"
#include "tic_adaptive_rate_plan.h"

namespace tic {

// Empty statistics in d_stats[0 .. count): what the probe kernel adds into.
hipError_t adaptive_stats_probe_reset(AdaptStats *d_stats, int count, hipStream_t stream);

// ONE launch for the probes of a SizeProbeTable (fill_size_probe_table, then cap_probe_groups): coefficients back to back from d_zz (int16
// [blocks][64] zig-zag, absolute DC; the DPCM restarts at every probe), probe k's statistics ADDED into d_stats[rec.result] - reset on the
// same stream before.  ngroups: the table's total.  d_probes is read by the kernel: device memory, complete on `stream` before the
// launch.  Reads the coefficients once, writes nothing else.
hipError_t adaptive_stats_probe_v(const int16_t *d_zz, const SizeProbeTable *d_probes, size_t ngroups, AdaptStats *d_stats, hipStream_t stream);

} // namespace tic
