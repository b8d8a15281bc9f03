// Host build of the integer encoder's arithmetic (tinyimgcodec_amd/csrc/tic_scaled_math.h - the very functions the gfx950 kernel is
// made of) for tests/test_scaled_encode_cpu.py: blocks in, zz16 coefficients out, compared there with the reference's.
//   scaled_selftest <in> <out>     in: int32 nblocks, int32 setting, nblocks * 64 pixels (row-major per block); out: nblocks * 64 int16
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../tinyimgcodec_amd/csrc/tic_scaled_math.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t head[2];
    if (fread(head, 4, 2, in) != 2 || head[0] < 0 || head[1] < 0 || head[1] > 3) return 2;
    std::vector<uint8_t> px((size_t)head[0] * 64);
    if (!px.empty() && fread(px.data(), 1, px.size(), in) != px.size()) return 2;
    fclose(in);
    std::vector<int16_t> zz((size_t)head[0] * 64);
    for (int32_t b = 0; b < head[0]; b++) tic::fdctq_scaled_block_host(px.data() + (size_t)b * 64, head[1], zz.data() + (size_t)b * 64);
    // the table: reciprocals of img.c:164-180 in 16 bits, every scan position exactly once
    constexpr tic::ScaledTab T = tic::make_scaled_tab();
    for (int qf = 0; qf < 4; qf++) {
        unsigned long long seen = 0;
        for (int i = 0; i < 64; i++) {
            const uint32_t t = T.w[qf][i];
            if ((t & 0xffffu) != (uint32_t)(65536 / (tic::kQTable[i] << qf)) || ((t >> 16) & 0x7fu) != (uint32_t)(tic::kQTable[i] >> 1)) return 3;
            seen |= 1ull << ((t >> 24) & 63u);
        }
        if (seen != ~0ull) return 3;
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out || (!zz.empty() && fwrite(zz.data(), 2, zz.size(), out) != zz.size())) return 2;
    fclose(out);
    puts("scaled_selftest ok");
    return 0;
}
