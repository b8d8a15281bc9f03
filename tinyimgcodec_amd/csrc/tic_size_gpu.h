// tic_size_gpu.h - the size of a default-table stream from its coefficients, on the device (see tic_size_gpu.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "tic_rate_plan.h"

namespace tic {

// Code lengths as the size kernel looks them up: len[run * kSizeTabSizes + size] = bits a non-zero AC entry of size category `size`
// adds behind a run of `run` zeros (run 0..62: the ZRLs of run >> 4, the (run & 15, size) code, the size bits); row 63 holds the DC
// categories (code + category bits) plus the EOB every block ends with.  Size 0 adds nothing (an AC zero); a size without a code
// (AC above 10, DC above 11) is kSizeNoCode, which lands above the 16 bits a lane's sum of eight entries can reach.
constexpr int kSizeTabRuns = 64, kSizeTabSizes = 17, kSizeDcRow = 63;
constexpr uint32_t kSizeNoCode = 1u << 16;
struct SizeTabDev {
    uint32_t len[kSizeTabRuns * kSizeTabSizes];
};
void build_size_tab(SizeTabDev *t);

// Per frame: payload bits of the stream (before the rounding up to a byte), and whether a coefficient has no Huffman code - the
// condition under which the packing kernels of tic_entropy_gpu.hip raise error 1.
struct SizeResult {
    unsigned long long bits;
    uint32_t nocode, pad;
};

// d_zz: int16 [nframes][blocks_per_frame][64], zig-zag, absolute DC - what the packing kernels read.  The kernel ADDS into
// d_res[0 .. nframes): the caller zeroes them on the same stream first (one memset serves any number of launches into different
// entries).  Reads the coefficients once, writes nothing else.
hipError_t stream_size_gpu(const int16_t *d_zz, size_t blocks_per_frame, int nframes, const SizeTabDev *d_tab, SizeResult *d_res,
                           hipStream_t stream);

// The descriptor form: ONE launch sums the probes of a SizeProbeTable (tic_rate_plan.h: fill_size_probe_table) - up to kSizeMaxProbes,
// each a frame's coefficients at one quality with its own block count, back to back from d_zz - into d_res[rec.result].  ngroups: the
// table's total.  d_probes is read by the kernel: device memory, complete on `stream` before the launch.  The caller zeroes the results.
hipError_t stream_size_gpu_v(const int16_t *d_zz, const SizeProbeTable *d_probes, size_t ngroups, const SizeTabDev *d_tab, SizeResult *d_res,
                             hipStream_t stream);

} // namespace tic
