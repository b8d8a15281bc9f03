// tic_entropy.h - host entropy stage (see tic_entropy.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace tic {
size_t num_blocks(int h, int w);
size_t compress_bound(int h, int w);
void write_header(uint8_t *out, int h, int w, int quality);
int entropy_encode(const int16_t *zz, int h, int w, int quality, uint8_t *out, size_t cap, size_t *out_len);
// compress()'s writer on encode()'s own arrays: dc int32 [N] the DC DIFFERENCES (first block raw), ac int32 [N][63].  The running DC is
// never formed: TIC_E_RANGE only where a difference (|d| >= 2048) or an AC value (|v| >= 1024) has no code.
int entropy_encode_dpcm(const int32_t *dc, const int32_t *ac, int h, int w, int quality, uint8_t *out, size_t cap, size_t *out_len);
// The length of the stream entropy_encode would write (any quality: the header's fields do not change it), from a walk of its own that
// only sums code lengths; TIC_E_RANGE exactly where entropy_encode returns it.
int entropy_size(const int16_t *zz, int h, int w, size_t *bytes);
// The same for a stream of the reference's integer encoder (c/img.c): quality field = setting 0..3, flag 1 << 30, one flush byte more
// (BB_flushBits); h and w multiples of 8.
void write_header_scaled(uint8_t *out, int h, int w, int qf);
int entropy_encode_scaled(const int16_t *zz, int h, int w, int qf, uint8_t *out, size_t cap, size_t *out_len);
int parse_header(const uint8_t *data, size_t len, int *h, int *w, int *quality, uint32_t *flag);
// A block whose integrated DC does not fit the int16 layout.  np.cumsum keeps the running DC as int32 (codec.py:53) and the reference
// transforms whatever it holds: differences of +-2047 take it out of int16 within 17 blocks.  zz then holds the saturated value and
// the list the true one, by frame-wide block index in ascending order; idct_kernel's wide-DC form reads it from an int32 side array.
// (A running DC beyond int32 is out of scope: np.cumsum wraps there.)
struct DcWide {
    size_t block;
    int32_t dc;
};
// Huffman + run-length decode into int16 [N][64] zig-zag with the DC already integrated (np.cumsum).  wide (may be null): cleared,
// then the blocks whose DC left int16; empty for every stream an encoder of ours writes.
int entropy_decode(const uint8_t *data, size_t len, int h, int w, int16_t *zz, std::vector<DcWide> *wide = nullptr);
// What the device decoder (tic_entropy_dec_gpu.hip) leaves to the host: blocks [first_block, N) from read position pos_bits with
// running DC running_dc, into zz_tail (N - first_block blocks); and the decoder's look-up tables for the device.
// wide as above (block indices count from the frame's first block, not from first_block).
int entropy_decode_tail(const uint8_t *data, size_t len, int h, int w, size_t first_block, size_t pos_bits, int running_dc, int16_t *zz_tail,
                        std::vector<DcWide> *wide = nullptr);
void dec_luts_fill(uint16_t *dc11, uint16_t *ac11, uint16_t *ac16);
// the device decoder's chain tables (DecLutsDev::mdc / mac / mlong, tic_entropy_dec_gpu.h)
void dec_chain_luts_fill(uint8_t *mdc /*[2048]*/, uint8_t *mac /*[4096]*/, uint8_t *mlong /*[256]*/);
void dec_pair_luts_fill(uint32_t *ac2 /*[2048]*/, uint32_t *long32 /*[192]*/);
} // namespace tic
