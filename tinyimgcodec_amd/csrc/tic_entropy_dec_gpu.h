// tic_entropy_dec_gpu.h - Huffman + run-length decode of a long stream on the device (see tic_entropy_dec_gpu.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
// TIC_DEC_WORKSPACE_ONLY: the workspace arithmetic and the plain structs below, without the launchers - for a host compiler without the HIP
// headers (tests/native/decws_selftest.cpp, decplan_selftest.cpp)
#ifndef TIC_DEC_WORKSPACE_ONLY
#include <hip/hip_runtime.h>
#define TIC_DEC_HD __host__ __device__
#else
#define TIC_DEC_HD
#endif

namespace tic {

// ---- the device decoder's ranges and its work buffer.  A range is the stream bits one lane walks: an odd number of 32-bit words.
constexpr int kDecRangeMin = 288, kDecRangeMax = 2016;
TIC_DEC_HD constexpr uint32_t dec_cap_of(uint32_t range) { return range / 6u + 2u; } // block starts a range can hold (a block has at least 6 bits: 2-bit DC code + EOB)
inline bool dec_range_ok(int range_bits) { return range_bits >= kDecRangeMin && range_bits <= kDecRangeMax && range_bits % 64 == 32; }
// The rule for it: `mult` average blocks, at least `floor_words` 32-bit words - 33 for nearly flat content, below 7 stream bits per block -,
// as an odd number of words up to 63 (why: tic_api.hip decode_range_bits).  stream_bytes with the header, as everywhere here.
inline int dec_range_rule(size_t stream_bytes, size_t nblocks, size_t mult = 2, size_t floor_words = 9) {
    if (floor_words == 9 && stream_bytes * 8 < 7 * nblocks) floor_words = 33;
    size_t k = (mult * (stream_bytes * 8) / nblocks + 31) / 32;
    k |= 1;
    return (int)(k < floor_words ? floor_words : (k > 63 ? 63 : k)) * 32;
}
inline size_t dec_ranges_of(size_t stream_bits, int range_bits) { return (stream_bits - 128 + (size_t)range_bits - 1) / (size_t)range_bits; } // (behind the 16-byte header)

// The carve-up of the work buffer, the only one: both launchers take their pieces through it, in this order, every piece rounded up to
// 256 B - an 8-byte total per frame, two traces of dec_cap_of(range_bits) 2-byte entries per range, a 4-byte position per block.
// `end` is what a launch uses.
struct DecWorkCarve {
    size_t totals, starts, hand, bpos, end;
    static size_t up(size_t b) { return (b + 255) / 256 * 256; }
    DecWorkCarve(size_t nframes, size_t total_ranges, size_t total_blocks, int range_bits) {
        const size_t trace = total_ranges * dec_cap_of((uint32_t)range_bits) * 2;
        totals = 0;
        starts = totals + up(nframes * 8);
        hand = starts + up(trace);
        bpos = hand + up(trace);
        end = bpos + up(total_blocks * 4);
    }
};
inline size_t dec_work_carve_bytes(size_t nframes, size_t total_ranges, size_t total_blocks, int range_bits) {
    return DecWorkCarve(nframes, total_ranges, total_blocks, range_bits).end;
}

// What is provided for it, before the range is known (a chunk's range is its frames' largest; the single-frame call may come back with
// kDecRangeMax, a hook may name any): the carve-up at the SHORTEST range with b / 288 + 2 ranges for a frame of b stream bits
// (`total_ranges_288`: their sum), plus one range of the LONGEST kind per frame and trace.  A bound for every legal range R, because a
// frame's trace entries are
//     ceil((b - 128) / R) * dec_cap_of(R) <= ((b - 129) / R + 1) * (R / 6 + 2) = (b - 129) / 6 + 2 (b - 129) / R + R / 6 + 2
//                                         <  (b / 288 + 1) * 50 + dec_cap_of(kDecRangeMax)           [R >= 288: 2 / R <= 1 / 144; R / 6 + 2 <= 338]
//                                         <  (floor(b / 288) + 2) * dec_cap_of(288) + dec_cap_of(kDecRangeMax),
// the 2 x 2 bytes per entry of the added ranges are added outside the rounding (up(a + b) <= up(a) + b + 255: 2 x 256 B more), and the
// other two pieces are the launch's own.  tests/native/decws_selftest.cpp sweeps it.
inline size_t dec_work_provision_bytes(size_t nframes, size_t total_ranges_288, size_t total_blocks) {
    return dec_work_carve_bytes(nframes, total_ranges_288, total_blocks, kDecRangeMin) + nframes * ((size_t)dec_cap_of(kDecRangeMax) * 2 * 2) + 2 * 256;
}
inline size_t dec_ranges_288(size_t stream_bytes) { return stream_bytes * 8 / kDecRangeMin + 2; } // a frame's share of total_ranges_288

// The host decoder's look-up tables (tic_entropy.cpp EncTables::Dec): the next 11 / 16 stream bits -> (code length << 8) | symbol,
// 0 when no codeword (of at most 11 bits, for the short tables) is a prefix of them.
struct DecLutsDev {
    uint16_t dc11[2048];
    uint16_t ac11[2048];
    uint16_t ac16[65536];
    // the measure walk's tables: one look-up consumes a CHAIN of symbols (it needs block ends, not values): entry = (bits consumed << 3)
    // | (table of the next step: 0 mdc, 1 mac, 2 mlong) << 1 | (the chain ended with EOB); a window without a codeword has an entry too (tic_entropy.cpp chain_entry).  mdc: the next 11 stream bits with the DC category next;
    // mac: the next 12 bits inside the AC symbols; mlong: the AC codewords of 12..16 bits (index: the next 16 bits - 0xff40), one symbol.
    uint8_t mdc[2048];
    uint8_t mac[4096];
    uint8_t mlong[256];
    // the fused kernel's table: one look-up of the next 11 stream bits gives up to TWO AC symbols with their values' places
    // (tic_entropy.cpp dec_pair_luts_fill), then the long codewords one by one, then a zero entry (the slot of an index out of range)
    uint32_t ac2[2048];
    uint32_t long32[192 + 4];
};

// DecStatus::giveup bit: the integrated DC of a block does not fit int16.  np.cumsum keeps the running DC as int32 (codec.py:53) and
// the reference transforms what it holds; the fused kernel's LDS image and the int16 layout hold the saturated value, so the whole
// stream goes to the host route, whose inverse stage takes the true DC from an int32 side array (tic_entropy.h DcWide).
constexpr int kDecGiveupWideDc = 512;

struct DecStatus {
    int giveup;                 // != 0: something unusual on the true chain - the caller decodes the whole stream on the host
    int dc_out;                 // running DC behind the last block produced here
    unsigned long long m;       // blocks produced: the pixels of blocks [0, m) have been written
    unsigned long long pos_out; // first stream bit behind block m - 1
    uint32_t head[4];           // the stream's first 16 bytes as the kernels saw them (a caller that launched on a GUESS of the header compares)
};
// A run behind which nothing is left to do: the kernels saw the header the caller decoded for, flagged nothing and produced every block.
inline bool dec_status_complete(const DecStatus &st, const void *head16, size_t nblocks) {
    return memcmp(st.head, head16, 16) == 0 && st.giveup == 0 && st.m == (unsigned long long)nblocks;
}

// Where the pixels go and how the coefficients become pixels (the inverse stage of decode(), codec.py:46-70): the arguments of
// idct_kernel, minus the coefficient array - the fused kernel never writes one.
struct DecIdctArgs {
    uint8_t *out;      // device, uint8 [h][stride]
    int h, w;
    long stride;
    int bw;            // blocks per row
    int aligned8;      // out and stride are multiples of 8: whole 8-byte row stores
    const struct DctqConsts *consts; // constants of the stream's quality (quality 50 on the scaled_dct branch)
    int scaled;        // decode()'s scaled_dct branch (codec.py:59-62)
    double pow2;       // 2 ** (quality field of the stream) on that branch
    uint32_t head[4];  // the 16-byte header h, w, stride and the constants above were derived from: a workgroup of the fused kernel whose
                       // stream starts with other bytes writes NO pixel (a launch on a guessed header must not touch memory outside the
                       // real image - a caller decoding into a window of a larger surface keeps its neighbours)
};

// One stream of a batch (entropy_decode_idct_gpu_batch): where its words, ranges, tiles, blocks and workgroups sit in the batch's arrays.
// The stream starts at word `word0` of the batch's stream buffer (every stream 4-byte aligned there); the same margin-free run as
// entropy_decode_idct_gpu with margin_bits = 0 (fast_end = stream_bits).
struct DecFrame {
    uint32_t word0, nwords, last_mask;  // the stream's words
    uint32_t fast_end, stream_bits;
    uint32_t nranges, range0;           // its ranges; index of its first range among the batch's (traces: range0 * cap entries in)
    uint32_t tile0, ntiles;             // its waves in the measure kernel's grid
    uint32_t blk0, nblocks;             // its blocks; index of its first block among the batch's (positions)
    uint32_t wg0, nwgs;                 // its workgroups in the fused kernel's grid
    uint32_t pad_;
    DecIdctArgs idct;                   // where its pixels go, its geometry, constants and header
};

#ifndef TIC_DEC_WORKSPACE_ONLY

size_t entropy_decode_gpu_work_bytes(size_t stream_bytes, size_t nblocks);
// d_stream_words: the whole stream (header included) in device memory, 4-byte aligned; the 4-byte word that holds its last byte is
// read whole (the bytes behind the stream's end are masked off), nothing behind that word is touched.  range_bits: stream bits per lane, a value entropy_decode_gpu_range_ok() accepts - an odd
// number of 32-bit words from 288 to 2,016 bits (shorter = shorter chains = faster, but every range must
// hold a block start of the true chain: giveup has bit 4 set when one did not - try a longer range).  d_work: zeroed when it was allocated;
// `epoch`: a number never used before on this workspace (the single-launch scans recognise this call's words by it), != 0.
// margin_bits: 2048 = blocks that start in the stream's last 2,048 bits are left to the caller (the host decoder's rule: whatever the
// stream holds, no block of the chain reaches its end); 0 = the chain runs to the end, m = all blocks of a whole stream, and giveup bit 256
// says that a block reached behind the end (a cut stream: call again with 2048).
// flat_grid: launches of up to this many workgroups add up all sums in front of a workgroup; larger ones use inclusive sums (wave_lookback).
// Writes the PIXELS of blocks [0, m) through `idct`; *d_status (zeroed by the caller) says how many that is and where the stream
// and the running DC stand behind them.  Asynchronous on `stream`; *d_status is complete when the stream has drained.
size_t entropy_decode_gpu_desc_words(size_t stream_bytes, size_t nblocks);
bool entropy_decode_gpu_range_ok(int range_bits);
hipError_t entropy_decode_idct_gpu(const void *d_stream_words, size_t stream_bytes, size_t nblocks, const DecLutsDev *d_luts, void *d_work,
                                   size_t work_bytes, unsigned long long *d_desc, size_t desc_words, uint32_t epoch, const DecIdctArgs &idct,
                                   DecStatus *d_status, int range_bits, int margin_bits, hipStream_t stream, int flat_grid = 4096);

// The same two launches with a COEFFICIENT sink: the unchanged measure / stitch kernel, then the fused kernel's phase 1, which stores blocks [0, m) as
// rows of the zz16 layout - int16 [nblocks][64], zig-zag order, absolute DC (saturated to int16: giveup bit kDecGiveupWideDc says that it was) -
// at d_coef (16-byte aligned) instead of transforming them.  head16: the stream's own 16 header bytes (coefficients are stored only under them).
// Work buffer, look-back words, epoch, range, margin and status as above.
hipError_t entropy_decode_coef_gpu(const void *d_stream_words, size_t stream_bytes, size_t nblocks, const DecLutsDev *d_luts, void *d_work,
                                   size_t work_bytes, unsigned long long *d_desc, size_t desc_words, uint32_t epoch, const uint8_t head16[16], int16_t *d_coef,
                                   DecStatus *d_status, int range_bits, int margin_bits, hipStream_t stream, int flat_grid = 4096);

// The batch form: `nframes` whole streams in two launches.  d_frames / d_tile_frame / d_wg_frame: device copies of the descriptors, the frame of
// every wave of the measure grid and of every workgroup of the fused grid; d_status: nframes entries, zeroed by the caller; the sums'
// look-back words and the epoch as above; small_win: every stream has at most 240 bits per block on average.  A frame whose status comes back
// with giveup != 0 or m != its block count is the caller's to decode again on its own.
uint32_t entropy_decode_batch_tiles(uint32_t nranges, int range_bits);
uint32_t entropy_decode_batch_wgs(size_t nblocks);
hipError_t entropy_decode_idct_gpu_batch(const void *d_words_all, const DecFrame *d_frames, const uint32_t *d_tile_frame, const uint32_t *d_wg_frame, uint32_t nframes,
                                         uint32_t total_tiles, uint32_t total_wgs, uint32_t total_ranges, size_t total_blocks, bool small_win, const DecLutsDev *d_luts, void *d_work,
                                         size_t work_bytes, unsigned long long *d_desc, size_t desc_words, uint32_t epoch, DecStatus *d_status, int range_bits, hipStream_t stream,
                                         int flat_grid = 4096);

// ... with the coefficient sink: frame f's blocks as rows of the zz16 layout from row blk0 of d_coef on (16-byte aligned, the chunk's total_blocks rows),
// absolute DC, the DC sum starting over with every frame; DecFrame::idct carries the frame's 16 header bytes (idct.head) and nothing else.  A frame
// whose status is not complete (dec_status_complete) may have left any of its OWN rows unwritten or half-written; no other frame's rows are touched.
hipError_t entropy_decode_coef_gpu_batch(const void *d_words_all, const DecFrame *d_frames, const uint32_t *d_tile_frame, const uint32_t *d_wg_frame, uint32_t nframes,
                                         uint32_t total_tiles, uint32_t total_wgs, uint32_t total_ranges, size_t total_blocks, bool small_win, const DecLutsDev *d_luts, void *d_work,
                                         size_t work_bytes, unsigned long long *d_desc, size_t desc_words, uint32_t epoch, DecStatus *d_status, int range_bits, int16_t *d_coef,
                                         hipStream_t stream, int flat_grid = 4096);

#endif // TIC_DEC_WORKSPACE_ONLY

} // namespace tic
