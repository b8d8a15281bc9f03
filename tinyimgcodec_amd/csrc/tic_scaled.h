// tic_scaled.h - launch interface of the integer ("scaled DCT") forward transform (tic_scaled.hip): the transform stage of the
// reference's standalone C encoder (c/img.c: IMG_fdct + IMG_quantize), uint8 pixels -> the zz16 layout of tic_kernels.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tic_scaled_frames.h"

namespace tic {

constexpr uint32_t kFlagScaled = 1u << 30; // header flag word of a scaled-DCT stream (img.c:185, codec.py:127-128)

struct ScaledArgs {
    const uint8_t *img; // device, uint8 [h][stride], h and w multiples of 8
    int16_t *out;       // device, int16 [N][64] zig-zag, absolute DC
    long stride;        // bytes between rows
    int bw;             // blocks per row = w / 8
    int tiles_x;        // 8-block strips per block row = ceil(bw / 8)
    int ntiles;         // strips per frame = (h / 8) * tiles_x
    int qf;             // 0 best, 1 high, 2 med, 3 low
    int aligned8;       // img, stride and frame stride are multiples of 8 -> one 8-byte load per lane
    int nframes;        // grid row per frame
    long frame_stride_in, frame_stride_out; // bytes between frames
};

// ev_start / ev_stop (both or neither): bound to the kernel's own dispatch packet, as launch_dctq's.
hipError_t launch_fdctq_scaled(const ScaledArgs &a, hipStream_t stream, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);

// The descriptor form: the `total_strips` strips of the frames d_table names (fill_scaled_table, tic_scaled_frames.h; complete on the device
// before `stream` reaches the launch) in ONE launch, whatever their sizes and settings.  The grid is sized as above, kMaxGroups workgroups
// at most; the test-hooks build lowers it to TIC_SCALED_V_GROUPS (tic_hooks.h).
hipError_t launch_fdctq_scaled_v(const ScaledFrameTable *d_table, uint32_t total_strips, hipStream_t stream, hipEvent_t ev_start = nullptr,
                                 hipEvent_t ev_stop = nullptr);

} // namespace tic
