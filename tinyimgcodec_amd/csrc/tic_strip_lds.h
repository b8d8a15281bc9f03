// tic_strip_lds.h - LDS layout constants of the strip kernel's loop that are chosen by a bank model, kept apart from the kernel so
// that the model can read them: tests/test_strip_lds_layout_cpu.py parses the initialiser lists below and replays every LDS access
// of the layout against the lane groups and bank rules of the LDS.  Plain constants, host and device.
#pragma once

namespace tic {

// Dword transpose between the two passes, columns-first instantiation: eight lane-linear planes of 64 dwords, one per pass-1
// output u.  Value (u, c) of block b sits at dword 4 * kTPlaneQ[u] + 8 * b + c of the wave's buffer: the writer lane 8*b + c stores
// to plane u at its own lane index (ds_write_addtid_b32: no address register), the reader lane 8*b + u finds its eight dwords as 32
// contiguous bytes (two ds_read_b128).  Plane offsets in 16-byte units; their residues mod 16 (0, 1, 8, 9, 0, 1, 8, 9) put the
// sixteen lanes of every ds_read_b128 lane group on 64 distinct banks.
constexpr int kTPlaneQ[8] = {0, 17, 40, 57, 80, 97, 120, 137};
constexpr int kTPlaneStepQ = 40; // kTPlaneQ[u] = kTPlaneStepQ * (u >> 1) + kTPlaneOddQ * (u & 1): what a lane computes
constexpr int kTPlaneOddQ = 17;
constexpr int kTPlaneWaveBytes = 2448; // the last plane ends here: (137 + 16) * 16

constexpr bool strip_tplanes_ok() {
    for (int u = 0; u < 8; u++)
        if (kTPlaneQ[u] != kTPlaneStepQ * (u >> 1) + kTPlaneOddQ * (u & 1) || (kTPlaneQ[u] + 16) * 16 > kTPlaneWaveBytes) return false;
    return kTPlaneQ[0] == 0;
}
static_assert(strip_tplanes_ok(), "plane table, lane formula and buffer size must agree");

// Zig-zag staging, columns-first instantiation: the lane 8*b + u packs its eight quantised values (u, v) into four dwords - plane p
// takes v = kZPairLo[p] in the low half and v = kZPairHi[p] in the high half - and stores dword p at its own lane index in plane p
// (ds_write_addtid_b32 again): value (u, v) of block b is the halfword at byte 4 * kZPlaneDw[p] + 4 * (8*b + u) + 2 * half.  The lane
// that stores chunk k of block b (scan positions 8k .. 8k+7) gathers them with eight ds_read_u16.  Pairing and plane residues mod 32
// (0, 0, 7, 7) are a best result of an exhaustive search (105 pairings x 32^3 residues) under the bank model: 8 conflict cycles per
// strip remain (4 per half wave), no layout of this family is free of them.
constexpr int kZPlaneDw[4] = {0, 64, 135, 199};
constexpr int kZPairLo[4] = {0, 1, 2, 4};
constexpr int kZPairHi[4] = {5, 3, 7, 6};
constexpr int kZPlaneWaveBytes = 1052; // (199 + 64) * 4
constexpr int kZGatherConflictCycles = 8; // per strip, both half waves: what the bank model finds for the constants above

// byte offset of value (u, v) of block 0 in the staging (block b: + 32 * b)
constexpr int strip_zstage_byte(int u, int v) {
    for (int p = 0; p < 4; p++) {
        if (kZPairLo[p] == v) return 4 * kZPlaneDw[p] + 4 * u;
        if (kZPairHi[p] == v) return 4 * kZPlaneDw[p] + 4 * u + 2;
    }
    return -1;
}
static_assert(strip_zstage_byte(7, 6) == 4 * 199 + 28 + 2 && strip_zstage_byte(0, 0) == 0, "every v has its plane and half");

} // namespace tic
