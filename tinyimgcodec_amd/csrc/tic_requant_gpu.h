// tic_requant_gpu.h - requantisation of stored coefficients on the device (see tic_requant_gpu.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "tic_math.h"
#include "tic_requant_plan.h"
#include "tic_size_gpu.h"

namespace tic {

// d_src / d_dst: int16 [.][64], zig-zag, absolute DC, 16-byte aligned - what the reader writes and the packers read.  ONE launch runs the
// jobs of a RequantJobTable (tic_requant_plan.h: fill_requant_job_table, which also bounds every job inside the two buffers); ngroups: the
// table's total.  d_consts: the context's constants, [100], index = quality.  d_jobs is read by the kernel: device memory, complete on
// `stream` before the launch.  The kernel ORs 1 into d_flags[rec.flag] where a result of the job leaves int16 (the element stored there
// is then unspecified); the caller zeroes the flags on the same stream first.
hipError_t requant_gpu_v(const int16_t *d_src, int16_t *d_dst, const RequantJobTable *d_jobs, size_t ngroups, const DctqConsts *d_consts,
                         uint32_t *d_flags, hipStream_t stream);

// The measuring instance: ONE launch reads the nblocks >= 1 blocks at d_src and adds, for each of the nq target qualities of `qs`
// (1..kSizeMaxProbes of them), the SizeResult of the frame requantised from qs.q_from to qs.q_to[i] into d_res[i] - the size kernel's run /
// size walk (tic_size_walk.h, the same SizeTabDev) applied to the values as they are produced; no requantised coefficient is written.
// nocode is set where a value has no Huffman code AND where one leaves int16 (either way the writer gives no stream).  The caller zeroes
// the results on the same stream first.  A workgroup's qualities: `split` workgroups share a round of chunks, each taking every split-th
// quality (requant_size_split: 1 for frames that fill the device by themselves, so that the frame is read once).
struct RequantQualities {
    int nq, q_from;
    uint8_t q_to[kSizeMaxProbes];
};
hipError_t requant_size_gpu_v(const int16_t *d_src, size_t nblocks, const RequantQualities &qs, const DctqConsts *d_consts, const SizeTabDev *d_tab,
                              SizeResult *d_res, hipStream_t stream);

} // namespace tic
