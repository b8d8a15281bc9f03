// tic_scaled_math.h - arithmetic of the reference's integer encoder (c/img.c), shared by the device kernel (tic_scaled.hip) and the
// host self-test (tests/native/scaled_selftest.cpp): 32-bit integers only, no floating point anywhere.
//
//   fdct8_scaled : one 8-point pass of IMG_fdct (img.c:55-88 rows, 91-124 columns - the same butterflies): the AAN forward DCT with
//                  the 8-bit constants 181, 98, 139, 334 and arithmetic >> 8.  The AAN scale factors stay in the outputs (hence
//                  "scaled"); the decoder divides them out (codec.py:59-62).  Every output is truncated to int16 by the caller.
//   quant_scaled : IMG_quantize (img.c:194-205): sign(d) * (((QUANT >> 1) + |d|) * (65536 / (QUANT << qf)) >> 16).
//   scaled_tab   : per natural index u*8+v one word: reciprocal (bits 0..15, at most 6,553) | QUANT >> 1 (bits 16..22) | scan
//                  position (bits 24..29).
// Ranges: pixels are int8 after the level shift, a row pass gives at most 8 * 128 = 1,024 in output 0 and 1,282 elsewhere (exhaustive over the
// 256 rows of extreme pixels), a column pass 12,871 at (1, 1) - the largest a greedy search over 0 / 255 blocks finds, not a proven
// maximum (tests/scaled_blocks.py; tests/test_scaled_blocks_cpu.py holds both to these figures).  A pass gains a factor of about 10 (128 ->
// 1,282), which keeps a column pass near 13,000 whatever the search misses: no int16 truncation changes a value, and every product
// below stays under 2^31 (12,871 * 334; (60 + 12,871) * 6,553).
#pragma once
#include <stdint.h>

#include "tic_tables.h"

#if defined(__HIPCC__)
#define TIC_HD __host__ __device__ __forceinline__
#else
#define TIC_HD inline
#endif

namespace tic {

TIC_HD void fdct8_scaled(int &s0, int &s1, int &s2, int &s3, int &s4, int &s5, int &s6, int &s7) {
    const int t0 = s0 + s7, t7 = s0 - s7, t1 = s1 + s6, t6 = s1 - s6;
    const int t2 = s2 + s5, t5 = s2 - s5, t3 = s3 + s4, t4 = s3 - s4;
    // even part
    const int e10 = t0 + t3, e13 = t0 - t3, e11 = t1 + t2, e12 = t1 - t2;
    const int z1 = ((e12 + e13) * 181) >> 8;
    s0 = e10 + e11;
    s4 = e10 - e11;
    s2 = e13 + z1;
    s6 = e13 - z1;
    // odd part
    const int o10 = t4 + t5, o11 = t5 + t6, o12 = t6 + t7;
    const int z5 = (o10 - o12) * 98;
    const int z2 = (z5 + o10 * 139) >> 8;
    const int z4 = (z5 + o12 * 334) >> 8;
    const int z3 = (o11 * 181) >> 8;
    const int z11 = t7 + z3, z13 = t7 - z3;
    s5 = z13 + z2;
    s3 = z13 - z2;
    s1 = z11 + z4;
    s7 = z11 - z4;
}

TIC_HD int quant_scaled(int d, uint32_t tab) {
    const uint32_t a = (uint32_t)(d < 0 ? -d : d);
    const int q = (int)(((((tab >> 16) & 0x7fu) + a) * (tab & 0xffffu)) >> 16);
    return (int)(int16_t)(d < 0 ? -q : q);
}

constexpr uint32_t scaled_tab_entry(int qf, int nat) {
    int pos = 0;
    for (int k = 0; k < 64; k++)
        if (kZigzag[k] == nat) pos = k;
    return (uint32_t)(65536 / (kQTable[nat] << qf)) | ((uint32_t)(kQTable[nat] >> 1) << 16) | ((uint32_t)pos << 24);
}

struct ScaledTab {
    uint32_t w[4][64];
};
constexpr ScaledTab make_scaled_tab() {
    ScaledTab t{};
    for (int qf = 0; qf < 4; qf++)
        for (int i = 0; i < 64; i++) t.w[qf][i] = scaled_tab_entry(qf, i);
    return t;
}

// One block on the host, natural (row-major) pixels in, zig-zag coefficients out: IMG_encodeBlock up to the entropy coder.
inline void fdctq_scaled_block_host(const uint8_t px[64], int qf, int16_t zz[64]) {
    constexpr ScaledTab T = make_scaled_tab();
    int d[64];
    for (int r = 0; r < 8; r++) {
        int s[8];
        for (int c = 0; c < 8; c++) s[c] = (int)(int8_t)(px[r * 8 + c] ^ 0x80);
        fdct8_scaled(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]);
        for (int c = 0; c < 8; c++) d[r * 8 + c] = (int)(int16_t)s[c];
    }
    for (int c = 0; c < 8; c++) {
        int s[8];
        for (int r = 0; r < 8; r++) s[r] = d[r * 8 + c];
        fdct8_scaled(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]);
        for (int u = 0; u < 8; u++) {
            const uint32_t t = T.w[qf][u * 8 + c];
            zz[(t >> 24) & 63u] = (int16_t)quant_scaled((int)(int16_t)s[u], t);
        }
    }
}

} // namespace tic
