// tic_size_walk.h - the bits of one lane's eight zig-zag entries in a default-table stream: what the size kernel (tic_size_gpu.hip) sums over a
// frame, and what the requantiser's measuring kernel (tic_requant_gpu.hip) sums over the values it produces.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tic_size_gpu.h"

namespace tic {

// Size category of a coefficient: its bit length, 0 for 0.  The exponent of the float is exact for |v| <= 65535.
__device__ __forceinline__ int size_category(int v) {
    int e;
    (void)frexpf((float)v, &e);
    return e;
}

template <int N>
__device__ __forceinline__ int dpp_row_shr(int v) {
    return __builtin_amdgcn_update_dpp(0, v, 0x110 + N, 0xf, 0xf, false);
}

// The bits of one lane's eight entries (k = lane & 7: entries 8k .. 8k + 7 of its block); prev_dc: the DC of the block before (used by
// k == 0), 0 for the frame's first block.  Bits below bit 16, entries without a code counted above it.
__device__ __forceinline__ uint32_t lane_bits(const uint4 v, int k, int prev_dc, const uint32_t *tab) {
    int c[8];
    c[0] = (int)(int16_t)(v.x & 0xffff); c[1] = (int)v.x >> 16; c[2] = (int)(int16_t)(v.y & 0xffff); c[3] = (int)v.y >> 16;
    c[4] = (int)(int16_t)(v.z & 0xffff); c[5] = (int)v.z >> 16; c[6] = (int)(int16_t)(v.w & 0xffff); c[7] = (int)v.w >> 16;
    // zero run that ends with this lane's last entry (tz) and whether the lane holds nothing else (az); the DC position is no AC zero
    int nz_mask = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) nz_mask |= (c[j] != 0 && !(k == 0 && j == 0)) ? (1 << j) : 0;
    int az = nz_mask == 0;
    int tz = az ? (k == 0 ? 7 : 8) : (__clz(nz_mask) - 24);
    // carry-through scan over the 8 lanes of the block (a lane only uses lanes of its own block: k >= D)
#define TIC_CARRY_STEP(D)                                          \
    {                                                              \
        const int pa = dpp_row_shr<D>(az), pt = dpp_row_shr<D>(tz); \
        if (k >= D) {                                              \
            tz = az ? pt + tz : tz;                                \
            az = az & pa;                                          \
        }                                                          \
    }
    TIC_CARRY_STEP(1)
    TIC_CARRY_STEP(2)
    TIC_CARRY_STEP(4)
#undef TIC_CARRY_STEP
    int run = dpp_row_shr<1>(tz); // the zero run in front of this lane's first entry (at most 55)
    if (k == 0) {
        run = kSizeDcRow;    // the DC difference takes the table's DC row ...
        c[0] = c[0] - prev_dc;
    }
    uint32_t acc = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        acc += tab[run * kSizeTabSizes + size_category(c[j])];
        run = c[j] != 0 ? 0 : run + 1;
        if (j == 0 && k == 0) run = 0; // ... and the AC run starts behind it
    }
    return acc;
}

} // namespace tic
