// tic_adaptive.h - per-image Huffman tables (compress(..., auto_generate_huffman_table=True) of the reference, codec.py:133-164,
// huffman.py:101-194): host table builder and decoder (tic_adaptive.cpp), device statistics and packing (tic_adaptive_gpu.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace tic {

// Symbol bins of the adaptive tables: AC (run << 4) | size at 0..255, DC size category c at kAdaptDcBin + c.
constexpr int kAdaptDcBin = 256, kAdaptBins = 272;
// Longest symbol (code + value bits) the packing kernel and the decoder take.
constexpr int kAdaptMaxSymbolBits = 64;
// Serialized table bits at most: 2 x 16 count bits, 16 DC entries of 8 + 15 bits, 256 AC entries of 16 + 64 bits.
constexpr size_t kAdaptMaxTableBytes = (32 + 16 * 23 + 256 * 80 + 7) / 8;

// What the statistics kernel leaves per frame: symbol counts and first-occurrence keys (DC: block index; AC: block * 64 + ordinal of
// the symbol in the block's run-length list, huffman.py:12-33), and an error word (1: a DC category or AC size above 15, which the
// reference's write_huffman_table cannot store, codec.py:73-84).
struct AdaptStats {
    unsigned long long count[kAdaptBins];
    unsigned long long first[kAdaptBins]; // ~0: the symbol does not occur
    unsigned int err;
};

// The table as the packing kernels use it: codeword (right-aligned, up to 64 bits) and its length per bin.
struct HuffWide {
    unsigned long long code[kAdaptBins];
    unsigned int len[kAdaptBins];
};

// HuffmanTree.__init__ / value_to_bitstring_table (huffman.py:137-194) of DC and AC from counts and first-occurrence keys, and
// write_huffman_table (codec.py:73-84) into `table` (MSB first, zero-padded): TIC_OK, TIC_E_RANGE (a symbol longer than
// kAdaptMaxSymbolBits, or no symbol at all), TIC_E_SPACE (table_cap).
int huffman_table_build(const unsigned long long *dc_count, const unsigned long long *dc_first, const unsigned long long *ac_count,
                        const unsigned long long *ac_first, unsigned long long *dc_code, uint8_t *dc_len, unsigned long long *ac_code,
                        uint8_t *ac_len, uint8_t *table, size_t table_cap, size_t *table_bits);

// decompress()'s Huffman + run-length part (codec.py:167-189, huffman.py:36-38,66-98) for a stream with an embedded table, read
// as written (flag 1 << 31 most significant bit first): zz = int16 [N][64] zig-zag with the DC integrated.  Strict: TIC_E_STREAM for
// a malformed table (not a prefix code, a code the stream then meets without a symbol, counts out of range), a truncated stream,
// a block of more than 63 AC entries or a DC outside int16.
int adaptive_decode(const uint8_t *data, size_t len, int h, int w, int16_t *zz, const char **why);

// Device part (tic_adaptive_gpu.hip).  d_stats: statistics of the n blocks of d_zz (zero the counts and the error, set the
// first keys to ~0 before).  The packing: d_out (32-bit words, zeroed, the header and table bits already in place) receives the
// payload from bit `base_bits`; nothing at or past word `out_words` is written (*d_err = 1 instead).  d_work:
// adaptive_work_bytes(n).
size_t adaptive_work_bytes(size_t nblocks);
hipError_t adaptive_stats(const int16_t *d_zz, size_t nblocks, AdaptStats *d_stats, hipStream_t stream);
hipError_t adaptive_pack(const int16_t *d_zz, size_t nblocks, const HuffWide *d_tab, void *d_work, uint32_t *d_out,
                         unsigned long long base_bits, unsigned long long out_words, unsigned int *d_err, hipStream_t stream);

} // namespace tic
