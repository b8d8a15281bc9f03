// tic_adaptive.h - per-image Huffman tables (compress(..., auto_generate_huffman_table=True) of the reference, codec.py:133-164,
// huffman.py:101-194): host table builder, table parser and decoder (tic_adaptive.cpp), device statistics and packing
// (tic_adaptive_gpu.hip), device decoder (tic_adaptive_dec_gpu.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "tic_adaptive_decode_plan.h"
#include "tic_adaptive_frames.h"

namespace tic {

// (symbol bins, AdaptStats, HuffWide and the records of the descriptor form: tic_adaptive_frames.h, free of HIP)

// HuffmanTree.__init__ / value_to_bitstring_table (huffman.py:137-194) of DC and AC from counts and first-occurrence keys, and
// write_huffman_table (codec.py:73-84) into `table` (MSB first, zero-padded): TIC_OK, TIC_E_RANGE (a symbol longer than
// kAdaptMaxSymbolBits, or no symbol at all), TIC_E_SPACE (table_cap).
int huffman_table_build(const unsigned long long *dc_count, const unsigned long long *dc_first, const unsigned long long *ac_count,
                        const unsigned long long *ac_first, unsigned long long *dc_code, uint8_t *dc_len, unsigned long long *ac_code,
                        uint8_t *ac_len, uint8_t *table, size_t table_cap, size_t *table_bits);

// The length of an adaptive stream is a function of the symbol statistics alone: the table comes from counts and first-occurrence keys,
// the payload is counts x (code length + value bits).  adaptive_stream_bits: header (128), table and payload bits of a stream whose
// table huffman_table_build made (dc_len / ac_len) from these counts - the ONE expression every encoder and every size entry takes its
// length from.  adaptive_stream_size: the table build and that sum, *bytes = the bits rounded up to a byte (bitbuffer.py:17-18); TIC_E_ARG
// and TIC_E_RANGE exactly where huffman_table_build returns them.
unsigned long long adaptive_stream_bits(const unsigned long long *dc_count, const unsigned long long *ac_count, const uint8_t *dc_len,
                                        const uint8_t *ac_len, size_t table_bits);
int adaptive_stream_size(const unsigned long long *dc_count, const unsigned long long *dc_first, const unsigned long long *ac_count,
                         const unsigned long long *ac_first, size_t *bytes);
// The statistics adaptive_stats_kernel leaves for the n blocks of zz (int16 [n][64] zig-zag, absolute DC), walked on the host with
// block_symbols' definition (tic_adaptive_gpu.hip): DPCM against the block before (the first against 0), run lengths, a ZRL per 16 zeros,
// an EOB behind every block, trailing zeros silent.  st->err = 1 for a DC category or AC size above 15 (counted in bin size & 15, as the
// kernel does).
void adaptive_host_stats(const int16_t *zz, size_t n, AdaptStats *st);
// The adaptive twin of entropy_size: adaptive_host_stats, then adaptive_stream_size.  A frame without blocks TIC_E_ARG (no symbol to build
// a table from), a category or size above 15 TIC_E_RANGE.
int entropy_size_adaptive(const int16_t *zz, int h, int w, size_t *bytes);

// decompress()'s Huffman + run-length part (codec.py:167-189, huffman.py:36-38,66-98) for a stream with an embedded table, read
// as written (flag 1 << 31 most significant bit first): zz = int16 [N][64] zig-zag with the DC integrated.  Strict: TIC_E_STREAM for
// a malformed table (not a prefix code, a code the stream then meets without a symbol, counts out of range), a truncated stream,
// a block of more than 63 AC entries or a DC outside int16.
int adaptive_decode(const uint8_t *data, size_t len, int h, int w, int16_t *zz, const char **why);

// The embedded table of such a stream as read_huffman_table (codec.py:87-99) reads it, entries in stream order: symbol (DC: size
// category; AC: (run << 4) | size), code length and codeword (right-aligned), and the payload's first bit (128 + table bits, not
// byte-aligned).
struct AdaptTable {
    int ndc, nac;
    uint8_t dc_sym[16], dc_len[16], ac_sym[256], ac_len[256];
    unsigned long long dc_code[16], ac_code[256];
    size_t payload_bit;
};
// The one table parser of both decoders, with adaptive_decode's strict checks (and its messages): the flag of the header, counts in
// range, a prefix code, code + value bits <= kAdaptMaxSymbolBits.  `len` bytes of `data` are readable: the whole stream, or its first
// 16 + kAdaptMaxTableBytes bytes (no table reaches further).
int adaptive_parse_table(const uint8_t *data, size_t len, AdaptTable *t, const char **why);

// Look-up tables of the device decoder (tic_adaptive_dec_gpu.hip), DC at [0] and AC at [1]: a primary table indexed by the next
// kAdaptDecK stream bits - (length << 8) | symbol for codes of at most kAdaptDecK bits, 0 (an escape) where the window starts a longer
// code or no code - and the longer codes left-aligned in 64 bits in ascending order with (length << 8) | symbol beside them: a lane
// takes the last one not above its window and confirms the prefix.  13.3 KB: the kernels stage it in LDS.
constexpr int kAdaptDecK = 11;
struct AdaptDecTab {
    uint16_t prim[2][1 << kAdaptDecK];
    unsigned long long long_code[2][256];
    uint16_t long_ls[2][256];
    uint32_t nlong[2];
};
// False when a code has length zero (the one-symbol tree of a flat frame: its symbols take no bits, so there is nothing to
// synchronise on): such a stream is the host decoder's.
bool adaptive_dec_tab_build(const AdaptTable &t, AdaptDecTab *out);
bool adaptive_dec_tab_buildable(const AdaptTable &t); // whether it would succeed, without building (the batch's take rule)

// Device decoder (tic_adaptive_dec_gpu.hip): the payload of `len` stream bytes at d_stream (4-byte aligned; the bytes of its last word
// behind `len` are masked) from bit `payload_bit` -> d_zz = int16 [nblocks][64] zig-zag with the DC integrated.  d_work:
// adaptive_dec_work_bytes(len, payload_bit, nblocks, range_bits) bytes.  Nothing is synchronised: the caller reads *d_status behind the
// stream.  Rounds [round0, round0 + nrounds) of the stitch are launched (round0 = 0 starts a decode and zeroes the status) and, with
// `finish`, the passes behind them: block positions, decode and the DC sum (nrounds may be 0 then).  What the passes leave counts only
// when the last round launched before them moved no exit.
constexpr int kAdaptDecMaxRounds = 512;
struct AdaptDecStatus {
    uint32_t giveup;                      // kAdaptGiveup* bits
    uint32_t blocks;                      // blocks on the chain up to the stream's end
    uint32_t changed[kAdaptDecMaxRounds]; // exits round r moved: the chain is known only when the last round launched moved none
};
constexpr uint32_t kAdaptGiveupNoSync = 4,    // (set by the caller) no fixed point within kAdaptDecMaxRounds rounds
                   kAdaptGiveupIncident = 8,  // a window without a code or a block of more than 63 AC entries on the chain before block N
                   kAdaptGiveupShort = 16,    // the chain reaches the stream's end before block N
                   kAdaptGiveupDc = 32;       // a running DC outside int16
int adaptive_dec_range_bits(size_t len, size_t payload_bit, size_t nblocks);
size_t adaptive_dec_work_bytes(size_t len, size_t payload_bit, size_t nblocks, int range_bits);
hipError_t adaptive_decode_gpu(const void *d_stream, size_t len, size_t payload_bit, size_t nblocks, int range_bits, const AdaptDecTab *d_tab,
                               void *d_work, AdaptDecStatus *d_status, int16_t *d_zz, int round0, int nrounds, bool finish, hipStream_t stream);

// Descriptor form: the frames of a chunk (tic_adaptive_decode_plan.h) in one launch per kernel.  All pointers are device memory: `frames`
// the chunk's descriptors, rwg_frame / bwg_frame the frame of every workgroup of the range and block grids, `tabs` an AdaptDecTab per
// frame kAdaptDecTabSlot bytes apart, `words` the chunk's stream buffer, `work` adaptive_dec_batch_work_bytes(ranges, blocks) bytes, `cs`
// the chunk's status with the frames' (`fs`) right behind it, `zz` int16 [blocks][64].  Rounds and `finish` as adaptive_decode_gpu, at
// most kAdaptBatchRounds rounds; what the passes leave for a frame counts only when the last round launched moved none of ITS exits.
struct AdaptDecBatch {
    const AdaptDecFrame *frames;
    const uint32_t *rwg_frame, *bwg_frame;
    const char *tabs;
    const uint32_t *words;
    void *work;
    AdaptDecChunkStatus *cs;
    AdaptDecFrameStatus *fs;
    int16_t *zz;
    uint32_t nframes, ranges, blocks, range_wgs, block_wgs;
};
hipError_t adaptive_decode_gpu_batch(const AdaptDecBatch &a, int round0, int nrounds, bool finish, hipStream_t stream);

// Device part of the encoder (tic_adaptive_gpu.hip).  d_stats: statistics of the n blocks of d_zz (zero the counts and the error, set the
// first keys to ~0 before).  The packing: d_out (32-bit words, zeroed, the header and table bits already in place) receives the
// payload from bit `base_bits`; nothing at or past word `out_words` is written (*d_err = 1 instead).  d_work:
// adaptive_work_bytes(n).
size_t adaptive_work_bytes(size_t nblocks);
hipError_t adaptive_stats(const int16_t *d_zz, size_t nblocks, AdaptStats *d_stats, hipStream_t stream);
hipError_t adaptive_pack(const int16_t *d_zz, size_t nblocks, const HuffWide *d_tab, void *d_work, uint32_t *d_out,
                         unsigned long long base_bits, unsigned long long out_words, unsigned int *d_err, hipStream_t stream);

// Descriptor form: ONE launch per kernel for the `count` frames of a chunk (at most kEntropyMaxFrames), coefficients back to back in d_zz,
// `ngroups` workgroups in all (fill_adaptive_table).  d_stats: an AdaptStats per frame; the statistics launch resets them itself.  The
// packing: frame k uses d_tabs[k], its record's base_bits, out_words and area at d_streams + out_off - zeroed by the caller; its header and
// table, d_heads + k * kAdaptHeadStride, are copied in here (whole words up to base_bits).  Frames marked `skip` are left alone.
// d_bbits: a word per block of the chunk, d_gsum: 8 bytes per workgroup.  *d_err = 1 where a frame would write at or past its out_words.
hipError_t adaptive_stats_v(const int16_t *d_zz, const AdaptFrameTable *d_frames, int count, size_t ngroups, AdaptStats *d_stats,
                            hipStream_t stream);
hipError_t adaptive_pack_v(const int16_t *d_zz, const AdaptFrameTable *d_frames, int count, size_t ngroups, const HuffWide *d_tabs,
                           const uint8_t *d_heads, uint32_t *d_bbits, unsigned long long *d_gsum, void *d_streams, unsigned int *d_err,
                           hipStream_t stream);

} // namespace tic
