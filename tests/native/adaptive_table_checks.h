// adaptive_table_checks.h - what the host self-tests of the per-image-table decoder (adaptive_host_selftest.cpp,
// damaged_adaptive_selftest.cpp) ask of a parsed table and of the look-up table built from it.  -> nullptr, or what is wrong.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../tinyimgcodec_amd/csrc/tic_adaptive.h"

using tic::AdaptDecTab;
using tic::AdaptTable;
using tic::kAdaptDecK;

// a parsed table is a prefix code inside the parser's limits
static const char *table_fault(const AdaptTable &t, size_t len) {
    if (t.ndc < 1 || t.ndc > 16 || t.nac < 1 || t.nac > 256) return "entry counts out of range";
    if (t.payload_bit < 128 + 32 || t.payload_bit > len * 8) return "payload_bit outside the stream";
    for (int k = 0; k < 2; k++) {
        const int n = k ? t.nac : t.ndc;
        int len_of[256];
        unsigned long long left[256]; // the codewords left-aligned in 64 bits
        for (int i = 0; i < n; i++) {
            const int li = k ? t.ac_len[i] : t.dc_len[i], si = k ? (t.ac_sym[i] & 15) : t.dc_sym[i];
            const unsigned long long ci = k ? t.ac_code[i] : t.dc_code[i];
            if (li + si > tic::kAdaptMaxSymbolBits || (!k && (li > 15 || si > 15))) return "a symbol longer than the limit";
            if (li < 64 && (ci >> li) != 0) return "a codeword with bits above its length";
            if (li == 0 && n > 1) return "a codeword of length zero beside others";
            len_of[i] = li;
            left[i] = li ? ci << (64 - li) : 0ull;
        }
        for (int i = 0; i < n; i++) // every pair: the shorter codeword is no prefix of the longer (equal ones included)
            for (int j = i + 1; j < n; j++) {
                const int m = len_of[i] < len_of[j] ? len_of[i] : len_of[j];
                if (m > 0 && ((left[i] ^ left[j]) >> (64 - m)) == 0) return "a codeword is a prefix of another";
            }
    }
    return nullptr;
}

// A built look-up table names only entries of the parsed table.  The table is a prefix code (table_fault), so the windows of two short
// codes do not overlap: when every short entry's windows hold that entry and no other window is filled, every filled window names an
// entry; likewise the long list, strictly ascending, with one place for every long entry and no more.
static const char *lut_fault(const AdaptTable &t, const AdaptDecTab &d) {
    for (int k = 0; k < 2; k++) {
        const int n = k ? t.nac : t.ndc;
        size_t longs = 0, windows = 0, filled = 0;
        if (d.nlong[k] > 256) return "a long list of more than 256 codes";
        for (uint32_t i = 0; i < d.nlong[k]; i++) {
            const int len = d.long_ls[k][i] >> 8;
            if (len <= kAdaptDecK || len > 64) return "a long entry with a short length";
            if (len < 64 && (d.long_code[k][i] << len) != 0) return "a long code that is not left-aligned";
            if (i && d.long_code[k][i - 1] >= d.long_code[k][i]) return "the long list does not ascend";
        }
        for (int i = 0; i < n; i++) {
            const int len = k ? t.ac_len[i] : t.dc_len[i];
            const unsigned long long code = k ? t.ac_code[i] : t.dc_code[i];
            const uint16_t ls = (uint16_t)((len << 8) | (k ? t.ac_sym[i] : t.dc_sym[i]));
            if (len <= kAdaptDecK) {
                const unsigned first = (unsigned)(code << (kAdaptDecK - len)), count = 1u << (kAdaptDecK - len);
                for (unsigned j = 0; j < count; j++)
                    if (d.prim[k][first + j] != ls) return "a short entry's window does not hold it";
                windows += count;
            } else {
                const unsigned long long want = code << (64 - len);
                const unsigned long long *at = std::lower_bound(d.long_code[k], d.long_code[k] + d.nlong[k], want);
                if (at == d.long_code[k] + d.nlong[k] || *at != want || d.long_ls[k][at - d.long_code[k]] != ls) return "a long entry is not in the long list";
                longs++;
            }
        }
        for (unsigned w = 0; w < (1u << kAdaptDecK); w++) filled += d.prim[k][w] != 0;
        if (filled != windows) return "a primary entry that is no entry of the table";
        if (d.nlong[k] != longs) return "a long entry that is no entry of the table";
    }
    return nullptr;
}
