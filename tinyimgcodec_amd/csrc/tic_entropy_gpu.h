// tic_entropy_gpu.h - device-side entropy stage (see tic_entropy_gpu.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "tic_entropy_frames.h"

namespace tic {

// Huffman tables as the kernels use them: the codeword already shifted left by the size category (the value bits are
// ORed in below it) and the symbol's total length.  Index (run << 4) | size for AC, size for DC; bits == 0: no code.
struct HuffDev {
    uint32_t ac_sym[256], ac_bits[256];
    uint32_t dc_sym[16], dc_bits[16];
    // the same in one word per symbol (lane-per-block packing kernel): (total bits << 27) | (codeword << size); 0: no code
    uint32_t ac_pack[256], dc_pack[16];
};
void build_huff_dev(HuffDev *t);

// The device entropy stage (tic_entropy_gpu.hip): pack -> (tile sums) -> place.  d_work: entropy_fused_work_bytes() bytes,
// never initialised by the caller.  Frame f's stream (16-byte header + payload) starts at d_out + f * out_frame_stride and
// may hold cap_words payload words (the stream area need not be zeroed; nothing past it is written); d_lens[f] (may be
// null) receives its length in bytes.  d_status (may be null, may be host-mapped; single-frame calls) receives {payload bits
// of frame 0, error}.  *d_err: 1 = a coefficient without a Huffman code, 2 = a stream does not fit; it must be zero on
// entry, and the placing kernel zeroes *d_err_next, the flag of the next call (two flags used in turn need no memset
// between calls).
// mode: kEntropyLanePerBlock - the packing kernel with a lane per block (a wave = 64 blocks, up to 512 bits per block);
//       *d_err = 4 when a block needs more: the caller runs the stage again with kEntropyEightLanes, the packing kernel with
//       8 lanes per block, which has no such limit (any block the format allows).  Both feed the same placing kernel.
// (kEntropyLanePerBlock, kEntropyEightLanes: tic_entropy_frames.h)
size_t entropy_fused_work_bytes(size_t nblocks_total);
hipError_t entropy_gpu_fused(const int16_t *d_zz, size_t blocks_per_frame, int nframes, const HuffDev *d_tab, void *d_work,
                             size_t work_bytes, void *d_out, size_t out_frame_stride, size_t cap_words, int h, int w, int quality,
                             unsigned long long *d_lens, unsigned long long *d_status, int *d_err, int *d_err_next, int mode,
                             hipStream_t stream, hipStream_t place_stream = nullptr, hipEvent_t pack_done = nullptr, uint32_t flag = 0);
// place_stream (with pack_done, an event of the caller's): the placing kernel - the stage's only writer of d_out, d_lens, d_status and
// *d_err_next - is queued on place_stream behind the packing on `stream`; the packing of the NEXT frame may then run on `stream` beside it.
// flag: the header's fourth word.  0 = a default-table stream (payload zero-padded to a byte, codec.py:102-114).  1 << 30 = a stream of the
// reference's integer encoder (img.c:183-192): `quality` is its setting 0..3 and the payload ends as BB_flushBits ends it (img.h:36-40) -
// floor(bits / 8) whole bytes and ONE more byte with the pending bits, a zero byte when there are none; lengths and the fit test count it.

// The stage in descriptor form: frames of any sizes and qualities in ONE pack and ONE place launch.  h_frames / d_frames: the same table
// (tic_entropy_frames.h) on the host - the launcher takes the grid sizes from it - and on the device, complete before `stream` reaches the
// launches; nframes 1..kEntropyMaxFrames, every frame with at least one block and at most 8,192 groups (no tile-sum level here: the caller
// codes larger frames alone), the records laid out for `mode` (fill_entropy_table).  Frame f's stream starts at d_out + rec[f].out_off and may
// hold rec[f].cap_words payload words; d_lens[f] receives its length.  *d_err / *d_err_next and the workspace as above: d_work of
// entropy_fused_work_bytes_v(total blocks, nframes) bytes.
size_t entropy_fused_work_bytes_v(size_t nblocks_total, size_t nframes);
hipError_t entropy_gpu_fused_v(const int16_t *d_zz, const EntropyFrameTable *h_frames, const EntropyFrameTable *d_frames, int nframes,
                               const HuffDev *d_tab, void *d_work, size_t work_bytes, void *d_out, unsigned long long *d_lens, int *d_err,
                               int *d_err_next, int mode, hipStream_t stream, uint32_t flag = 0);
// flag: as above, for every frame of the launch (1 << 30: rec[f].quality is the setting 0..3 and cap_words counts the flush byte's word).

} // namespace tic
