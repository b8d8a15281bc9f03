// tic_api.hip - the C-ABI of libtinyimgcodec_hip.so (include/tinyimgcodec_hip.h): context, device buffers,
// launches of the transform kernels on the context's own HIP stream, the stream-overlapped batch pipeline, and
// the glue to the host entropy stage.  No CPU fallback exists for the transform stage.
#include <hip/hip_runtime.h>
#include <chrono>

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/tinyimgcodec_hip.h"
#include "../../include/tinyimgcodec_hip_adaptive_rate.h"
#include "../../include/tinyimgcodec_hip_requantize.h"
#include "../../include/tinyimgcodec_hip_transcode.h"
#include "../../include/tinyimgcodec_hip_transcode_batch.h"
#include "../../include/tinyimgcodec_hip_wide.h"
#include "tic_adaptive.h"
#include "tic_adaptive_stats_gpu.h"
#include "tic_decode_plan.h"
#include "tic_entropy.h"
#include "tic_entropy_dec_gpu.h"
#include "tic_entropy_gpu.h"
#include "tic_hooks.h"
#include "tic_host_pipeline.h"
#include "tic_kernels.h"
#include "tic_math.h"
#include "tic_rd_plan.h"
#include "tic_requant_gpu.h"
#include "tic_scaled.h"
#include "tic_size_gpu.h"
#include "tic_transcode_plan.h"

using namespace tic;

namespace {
constexpr int kAsyncSlots = 64; // tickets of the asynchronous calls that may be open at once per context
constexpr int kDecSlots = 4;    // ... of the asynchronous decodes (each holds a workspace: tens of MB for a 4096^2 stream)
// Phase times of the batch pipeline (tic_last_batch_phases): a handful of steady_clock reads per chunk, summed per context.
// 0 staging copies into pinned memory (pageable input) or registration of the caller's frames, 1 enqueueing (H2D, kernels, lengths),
// 2 waiting for a chunk, 3 stream read-back, 4 hand-out into the caller's buffers, 5 waiting for a free slot.
// (phases 0, 1, 5 belong to the submitting thread, 2 and 3 to the reading thread, 4 to the hand-out thread)
struct BatchTrace {
    double t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    static std::chrono::steady_clock::time_point &t0() {
        static thread_local std::chrono::steady_clock::time_point v;
        return v;
    }
    void start() { t0() = std::chrono::steady_clock::now(); }
    void stop(int k) { t[k] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0()).count(); }
};
#define BT_START() ctx->bt.start()
#define BT_STOP(K) ctx->bt.stop(K)

constexpr size_t kDecTailEnd = 512, kDecTailCoef = 64 * 1024; // device decoder: bytes of stream end prefetched, bytes of tail coefficients (pinned)
constexpr int kChunk = 16;
// ... of small frames more: a chunk of sixteen 512 x 512 frames is 4 MB - its copies and launches cost as much as its work (the reference's
// benchmark set, 49 such frames, took four chunks: 20,000 frames/s); up to 64 frames while a chunk's pixels stay within 32 MB
static inline int chunk_frames(int n, size_t img_bytes) {
    size_t c = img_bytes ? (32u << 20) / img_bytes : (size_t)kChunk;
    c = c < (size_t)kChunk ? (size_t)kChunk : (c > 64 ? 64 : c);
    if (const char *e = test_hook("TIC_BATCH_CHUNK")) c = atoi(e) >= 1 && atoi(e) <= 64 ? (size_t)atoi(e) : c; // (tests: several chunks of small frames)
    return n < (int)c ? n : (int)c;
}
// What a context keeps between calls.  Hooks build only: every buffer a context owns is recorded when it is
// allocated and dropped when it is freed, as SCRATCH - any content is legal when a public call begins - or STATE - it carries an
// invariant from one call to the next.  TIC_POISON and tic_test_poison fill the scratch ones; nothing ever fills a state buffer
// (a buffer that a kernel spin-waits on, the decoder's look-back words, is state by that rule alone).
enum BufKind { kBufDev, kBufPinned, kBufMapped };
enum BufClass { kBufScratch, kBufState };
struct BufRec {
    void *p;
    size_t bytes;
    int kind, cls;
    const char *name;
};
#ifdef TIC_TEST_HOOKS
std::atomic<int> g_live_buffers{0}; // owned buffers allocated in this process (tic_test_live_buffers)
#endif
// A buffer a context owns: the pointer, its capacity in bytes, and its entry in the registry above - name and class, given once, where
// the field is declared.  It converts to its pointer, so that it reads as one wherever it is used; it frees its memory when it is
// released or destroyed, and nothing else does.  Not copied; a move leaves the source null.
template <class T, BufKind K> struct Buf {
    T *p = nullptr;
    T *d = nullptr; // host-mapped memory only: the kernels' address of it (coherent: the host reads it behind a polled or drained stream)
    size_t cap = 0;
    const char *const name;
    const BufClass cls;
    Buf(const char *registry_name, BufClass c = kBufScratch) : name(registry_name), cls(c) {}
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p(o.p), d(o.d), cap(o.cap), name(o.name), cls(o.cls) { o.p = o.d = nullptr, o.cap = 0; }
    ~Buf() { (void)free_mem(); }
    operator T *() const { return p; }
    template <class U> explicit operator U *() const { return (U *)p; } // (a cast of the buffer is a cast of its pointer)
    // When `need` bytes exceed the capacity, the buffer is freed and one of `alloc` bytes (0: `need`) takes its place.  Nothing may be
    // in flight on the old buffer.  A failed allocation leaves it null with capacity 0.
    int grow(tic_ctx *ctx, size_t need, size_t alloc = 0);
    void release(tic_ctx *ctx);

private:
    hipError_t alloc_mem(size_t bytes) {
        hipError_t e = K == kBufDev ? hipMalloc((void **)&p, bytes)
                                    : hipHostMalloc((void **)&p, bytes, K == kBufPinned ? hipHostMallocDefault : hipHostMallocMapped | hipHostMallocCoherent);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
#ifdef TIC_TEST_HOOKS
        g_live_buffers++;
#endif
        if (K == kBufMapped && (e = hipHostGetDevicePointer((void **)&d, p, 0)) != hipSuccess) {
            (void)free_mem(); // (null again, as after any failed allocation)
            return e;
        }
        cap = bytes;
        return hipSuccess;
    }
    hipError_t free_mem() { // the one place a context's memory is freed
        if (!p) return hipSuccess;
#ifdef TIC_TEST_HOOKS
        g_live_buffers--;
#endif
        void *const q = p;
        p = d = nullptr, cap = 0;
        return K == kBufDev ? hipFree(q) : hipHostFree(q);
    }
};
template <class T> using DevBuf = Buf<T, kBufDev>;
template <class T> using PinBuf = Buf<T, kBufPinned>;
template <class T> using MappedBuf = Buf<T, kBufMapped>;

struct Slot {
    PinBuf<uint8_t> pin_in{"bslot.pin_in"};
    PinBuf<int16_t> pin_out{"bslot.pin_out"};
    DevBuf<void> d_img{"bslot.d_img"};
    DevBuf<void> d_coef{"bslot.d_coef"};
    hipEvent_t done = nullptr;
    hipEvent_t rb_done = nullptr; // the chunk's streams have arrived in pin_out (recorded behind the read-back copy)
    // device entropy stage of the chunk
    DevBuf<void> d_work{"bslot.d_work"}; // workspace of the fused entropy pass
    int parity = 0;                      // which of the two descriptor arrays / error flags the next call uses
    DevBuf<unsigned long long> d_lens{"bslot.d_lens"}; // stream length per frame (device / pinned host)
    PinBuf<unsigned long long> h_lens{"bslot.h_lens"};
    DevBuf<int> d_err{"bslot.d_err", kBufState}; // two flags used in turn: zero when allocated, the chunk's last kernel clears the next one
    PinBuf<int> h_err{"bslot.h_err"};
    DevBuf<void> d_streams{"bslot.d_streams"}; // finished streams, one compress_bound() apart
    // mixed batches (tic_compress_batch_v): the entropy stage's table of the chunk - filled in pinned memory, uploaded in stream order -
    // and, for the read-back, where each stream lands in pin_out (pinned: the shader reads it where it lies)
    PinBuf<EntropyFrameTable> h_frames{"bslot.h_frames"};
    DevBuf<EntropyFrameTable> d_frames{"bslot.d_frames"};
    PinBuf<unsigned long long> h_rb_off{"bslot.h_rb_off"};
    // scaled batches (tic_compress_batch_scaled_v): the table of the chunk's ONE transform launch, pinned and on the device
    PinBuf<ScaledFrameTable> h_sframes{"bslot.h_sframes"};
    DevBuf<ScaledFrameTable> d_sframes{"bslot.d_sframes"};
    // adaptive batches (tic_compress_batch_adaptive_v): the chunk's statistics, tables, headers and bit counts, carved by adaptive_slot_layout
    // (tic_adaptive_frames.h), and the pinned mirror of their host-visible part.  Stream lengths are known only behind the statistics, so a
    // chunk may find d_streams or pin_out short and grow THIS slot's
    DevBuf<char> d_adapt{"bslot.d_adapt"};
    PinBuf<char> h_adapt{"bslot.h_adapt"};
    int first = 0, count = 0; // frames [first, first+count) are in flight in this slot
    int pending = 0;          // pieces of the chunk's work not yet finished (SlotGate); 0 = the slot is free
    size_t rb_row = 0;        // row pitch of the streams read back into pin_out (0: they went straight to the caller)
    void release(tic_ctx *ctx); // frees everything the slot owns
};
static const char *const kDecWsNames[3] = {"dec_ws.work", "dec_ws.desc", "dec_ws.status"};
static const char *const kDecSlotWsNames[3] = {"dec_slot.work", "dec_slot.desc", "dec_slot.status"};
static const char *const kDecBatchWsNames[3] = {"dbat.work", "dbat.desc", "dbat.status"};
// Workspace of the device Huffman decoder (tic_entropy_dec_gpu.hip), one per user: the single-frame calls, every asynchronous decode slot
// and the batch.  Nothing of an earlier run may be in flight when it grows or a run begins.
struct DecWorkspace {
    const char *const *names; // registry names of work, desc and status: one set per user of a workspace
    DevBuf<void> work{names[0]};
    DevBuf<unsigned long long> desc{names[1], kBufState}; // look-back words of the decoder's scans: an array of their own, zero or stamped
    size_t desc_words = 0;                                // with a past epoch (state: wave_lookback spins on these words)
    uint32_t epoch = 0;                 // runs on these words (the single-launch scans tell their words by it)
    MappedBuf<DecStatus> h_status{names[2]}; // host-mapped, one entry per frame of a run
    // at least `work_need` bytes of work buffer (`work_alloc` when it grows), `desc_need` look-back words (max(8192, 2 x desc_need) when they
    // grow: zeroed, epoch 0) and `status` status entries (`status_alloc`)
    int grow(tic_ctx *ctx, size_t work_need, size_t work_alloc, size_t desc_need, size_t status, size_t status_alloc);
    int begin(tic_ctx *ctx, hipStream_t stream, size_t status); // a run of `status` frames on `stream`
    void release(tic_ctx *ctx);
    explicit DecWorkspace(const char *const *registry_names = kDecWsNames) : names(registry_names) {}
};
} // namespace

struct tic_ctx {
    // Every entry point that takes a context holds this lock for its whole duration: a context shared between host threads is
    // safe (calls serialise); threads that want to overlap use one context each (the Python mirror's default context is
    // per thread).  Recursive because the host-buffer entry points call the device-buffer ones.
    std::recursive_mutex mu;
    int device = -1;
    hipStream_t stream = nullptr;     // all single-frame work
    hipStream_t bstream[2] = {nullptr, nullptr}; // batch pipeline streams
    hipStream_t rstream = nullptr;               // read-back of finished streams: never queued behind a later chunk's work
    // The buffers below are Buf fields: each owns its memory, knows its capacity (.cap) and carries its registry name and class.
    PinBuf<int16_t> h_zz{"h_zz"};                // pinned landing buffer of the host Huffman decoder (tic_decompress)
    DevBuf<DctqConsts> d_consts{"d_consts", kBufState}; // [100], index = quality; slot 0 = the custom (non-integral) quality of tic_set_custom_quality
    double custom_quality = 0.0;      // what slot 0 holds (0: nothing yet)
    DevBuf<unsigned long long> d_fallback{"d_fallback", kBufState};
    StripLaunchInfo last_strip{}; // what the last tic_dctq_dev / tic_dctq_dev_frames launch decided (tic_last_strip_launch)
    bool stats = false; // count guard-band fallbacks with a global atomic (diagnostic; serialises at ~12 ns per wave)
    hipEvent_t ev0 = nullptr, ev1 = nullptr; // the interval of the timed entry points (timed_launches)
    // scratch for the host-buffer entry points
    DevBuf<void> d_img{"d_img"};
    DevBuf<void> d_coef{"d_coef"};
    std::vector<int16_t> h_coef;
    // device entropy stage workspace
    DevBuf<HuffDev> d_huff{"d_huff", kBufState};
    DevBuf<unsigned long long> d_total_bits{"d_total_bits", kBufState}; // status block of the device entropy stage: payload bits [2], error flags [2] (used in turn)
    int *d_err = nullptr;                                               // ... the error flags: a view of d_total_bits
    MappedBuf<unsigned long long> h_stat{"h_stat", kBufState}; // host-mapped status block of the device entropy stage (bits, error); behind
    unsigned long long *d_stat = nullptr;                      // its first 64 bytes: the {bits, error} pairs of the asynchronous calls' tickets
                                                               // (d_stat: the kernels' view of h_stat)
    // asynchronous device-resident calls (tic_compress_dev_async): ticket t lives in slot t % kAsyncSlots
    struct AsyncSlot { long long ticket = -1; size_t cap = 0; int early_rc = TIC_OK; hipEvent_t done = nullptr; bool empty_image = false; };
    AsyncSlot async_slots[kAsyncSlots];
    long long async_next = 0;
    // ... their transform and packing kernels run on two LANES in turn (streams of their own, a coefficient buffer, an entropy workspace and
    // a pair of error flags each), the placing kernels - the only writers of the callers' buffers - on the context's stream in ticket order:
    // frame t + 1 is transformed and packed beside the packing and placing of frame t (tic_compress_dev_async)
    struct AsyncLane {
        hipStream_t stream = nullptr;
        static constexpr const char *kWorkName = "lane.d_work";
        DevBuf<void> d_coef{"lane.d_coef"};
        DevBuf<void> d_work[2] = {{kWorkName}, {kWorkName}}; // two entropy workspaces of one size used in turn: the lane packs its next frame
                                                             // while the placing kernel of the frame before still reads the other one
        DevBuf<int> d_err{"lane.d_err", kBufState}; // [4], used in turn (a placing kernel zeroes the flag of the lane's frame three ahead: no packing in flight uses it)
        unsigned long long frames = 0;        // frames this lane has taken
        hipEvent_t packed = nullptr, placed[2] = {nullptr, nullptr}; // the lane's last packing has run / the frame that used workspace k has been placed (on ctx->stream)
        bool placed_valid[2] = {false, false};
        unsigned long long order_seen = 0; // the burst (lane_epoch) whose starting point this lane's stream already waits for
    };
    AsyncLane lanes[2];
    hipEvent_t lane_order = nullptr; // a burst's lanes start behind what the context's stream held when the burst began
    int async_open = 0;              // tickets open
    unsigned long long lane_epoch = 0;
    DevBuf<void> d_ent_work{"d_ent_work"};      // workspace of the device entropy stage (tile sums, bit counts, staging slots)
    int ent_parity = 0;
    // Which packing kernel the device entropy stage starts with: the lane-per-block kernel up to this quality, the 8-lane kernel
    // above it.  -1 (the default): always the 8-lane kernel - round 3 built the lane-per-block kernel and measured it no faster
    // (4096^2 noise: pack 26 us either way, place 13.5 against 8.5 us; Lenna tiled: 21 + 7 against 24 + 8.5 us; DESIGN.md
    // section 5.4), so it stays selectable (tic_set_entropy_lane_kernel) and tested, not default.  With it on, a frame in which a block needs more
    // than 512 bits (noise at quality >= ~85) makes it raise error 4: the stage is run again with the 8-lane kernel and the limit
    // drops below that quality for the rest of the context's life.
    int ent_lane_max_quality = -1;
    DevBuf<void> d_stream_buf{"d_stream_buf"};
    DevBuf<int32_t> d_dc32{"d_dc32"};            // int32 DC of every block of a frame whose running DC left int16 (decode_on_host; idct_kernel's wide-DC form)
    // device Huffman decoder (tic_decompress of long streams): tables, workspace, status
    DevBuf<DecLutsDev> d_dec_luts{"d_dec_luts", kBufState};
    DecWorkspace dec_ws;
    PinBuf<uint8_t> h_dec_tail{"h_dec_tail"};                   // pinned: kDecTailEnd bytes of stream end + kDecTailCoef bytes of tail coefficients
    int last_decode_path = 0;                                  // 0 none, 1 device decoder, 2 host decoder (tic_last_decode_path)
    // asynchronous device-resident decodes (tic_decompress_dev_async): ticket t lives in slot t % kDecSlots; every slot has its own HIP
    // stream, workspace, look-back words and status words, so that the frames of a burst overlap (the measure kernel is one wave per
    // SIMD waiting for table entries, the fused kernel issues float64 arithmetic: they share a CU well)
    struct DecSlot {
        long long ticket = -1;
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        DecWorkspace ws{kDecSlotWsNames};
        bool launched = false;   // false: the call ran synchronously (no guess to launch on): rc / h / w are its outcome
        int rc = TIC_OK, h = 0, w = 0;
        uint8_t head[16] = {0};  // the header the launch guessed
        size_t n = 0;
        const void *d_stream = nullptr; // the call, for the synchronous second try
        size_t len = 0;
        void *d_out = nullptr;
        ptrdiff_t out_stride = 0;
        size_t out_cap = 0;
    };
    DecSlot dec_slots[kDecSlots];
    long long dec_async_next = 0;
    hipEvent_t dec_order = nullptr; // a slot's stream starts behind everything queued on the context's stream so far
    // Small frames to HOST memory (tic_compress): the placing kernel writes the finished stream straight into this host-mapped pinned buffer
    // and the host copies it out with memcpy - no device-to-host DMA copy, whose submission and completion cost more than the transfer of a
    // 30 - 80 KB stream: compress() of a 512 x 512 image 54 us instead of 62 (profiles/r05_decoder.txt).  (The same for the PIXELS of a small
    // decompress(): measured, no gain - 262 KB written across PCIe by the kernel and copied again by the host cost what the DMA copy does.)
    MappedBuf<uint8_t> h_small{"h_small"}; // (h_small.d: the placing kernel's address of it)
    uint8_t dec_head[16] = {0};                                  // header of the last stream tic_decompress_dev decoded on the device: the next call's guess
    bool dec_head_valid = false;
    int dec_head_streak = 0;   // device decodes in a row (before the last one) whose header was dec_head: a guess is made from 1 on, i.e. after two equal headers
    bool dec_guess_on = true;  // tic_set_decode_guess
    int last_decode_guess = 0;                                  // tic_decompress_dev: 1 the last call's guess of the header held, -1 it did not (decoded again), 0 no guess
    int last_decode_range = 0, last_decode_tries = 0;          // stream bits per lane of the device decoder's last run, and how many runs the last long stream took
    int last_decode_giveup = 0;                                // why the device decoder handed the last long stream to the host (DecStatus::giveup bits)
    // batched decode (tic_decompress_batch): one pinned + one device buffer for a chunk's descriptors and streams, a device and a pinned
    // buffer for its pixels, workspace, look-back words and per-frame status words - kept across calls
    struct DecBatch {
        PinBuf<uint8_t> h_in{"dbat.h_in"};
        DevBuf<uint8_t> d_in{"dbat.d_in"};
        DevBuf<uint8_t> d_pix{"dbat.d_pix"};
        PinBuf<uint8_t> h_pix{"dbat.h_pix"};
        DecWorkspace ws{kDecBatchWsNames};
    } dbat;
    int last_dbatch_frames = 0, last_dbatch_fallback = 0, last_dbatch_chunks = 0, last_dbatch_direct = 0;
    int last_dbatch_range = 0;                                 // tic_last_decompress_batch_work: the last chunk handed to the batch launcher -
    size_t last_dbatch_work_used = 0, last_dbatch_work_held = 0; // its range, the bytes of work buffer it carves, the bytes the context held
    // batch pipeline buffers, kept across calls (pinned allocations are expensive)
    std::vector<Slot> bslots;
    // what every slot holds at least: bytes of staged pixels, of coefficients, of the pinned landing buffer, of stream areas, of entropy
    // workspace, and frames per chunk
    struct SlotNeed {
        size_t img = 0, coef = 0, pin_out = 0, streams = 0, work = 0;
        int frames = 0;
        bool covers(const SlotNeed &o) const {
            return img >= o.img && coef >= o.coef && pin_out >= o.pin_out && streams >= o.streams && work >= o.work && frames >= o.frames;
        }
    } bslot_cap;
    int last_vbatch_frames = 0, last_vbatch_single = 0, last_vbatch_chunks = 0, last_vbatch_launches = 0; // tic_last_compress_batch_v
    int last_abatch_frames = 0, last_abatch_single = 0, last_abatch_chunks = 0;                           // tic_last_compress_batch_adaptive
    // host side of the batch pipeline: the device's NUMA node and the CPUs of that node this process may run on
    int numa_node = -1;
    bool numa_bind = true;      // the pipeline's own threads (staging, read-back, hand-out) bind themselves to those CPUs
    cpu_set_t numa_cpus;
    int numa_ncpus = 0;
    // how the last batch call took its input: frames copied to the device from where the caller holds them (pinned or registered
    // memory) / frames staged through the pipeline's pinned slots (pageable memory)
    int last_batch_direct_frames = 0, last_batch_staged_frames = 0;
    int last_batch_zero_copy = 0; // streams of the last batch the read-back kernel stored straight into the caller's buffers
    mutable BatchTrace bt; // phase times of the last batch call
    // Pageable frames of a batch call are pinned in place for the duration of the call where that is one cheap registration
    // (auto_register_frames) instead of being copied into the pinned slots by CPU threads
    bool auto_register = true;
    std::vector<void *> autoregs;      // ranges this call registered (unregistered before it returns)
    int last_batch_autoreg_frames = 0;
    int stage_threads = 0; // host threads that stage pageable frames (0: min(8, cores / 2)); tic_set_stage_threads
    char pci[32] = {0};
    std::string err;
    char arch[128] = {0};
    std::vector<BufRec> bufs; // hooks build: every buffer the context owns (buf_add, buf_drop)
    // per-image Huffman tables (tic_compress_adaptive): statistics, the frame's table and an error word in one allocation, the packing
    // workspace and the stream, kept across calls
    DevBuf<AdaptStats> d_adapt_stats{"d_adapt_stats"};
    HuffWide *d_adapt_tab = nullptr; // views of d_adapt_stats: the table and the error word behind the statistics
    uint32_t *d_adapt_err = nullptr;
    DevBuf<void> d_adapt_work{"d_adapt_work"};
    DevBuf<uint32_t> d_adapt_out{"d_adapt_out"};
    // ... and their device decoder (tic_decompress_adaptive): look-up tables and status words in one allocation, the workspace
    AdaptDecTab adec_tab; // the host copy, built per call
    DevBuf<AdaptDecTab> d_adec_tab{"d_adec_tab"};
    AdaptDecStatus *d_adec_status = nullptr; // a view of d_adec_tab: the status words behind the tables
    DevBuf<void> d_adec_work{"d_adec_work"};
    // ... and its batch form (tic_decompress_batch_adaptive): a chunk's status words, work arrays and coefficients in one device buffer
    // (AdaptDecWorkLayout), the pinned landing buffer of the status words; upload and pixel buffers are the batched decode's (dbat)
    struct AdaptDecBatchBuf {
        DevBuf<char> d_work{"adbat.d_work"};
        PinBuf<char> h_status{"adbat.h_status"};
    } adbat;
    int last_adbatch_frames = 0, last_adbatch_single = 0, last_adbatch_chunks = 0, last_adbatch_direct = 0; // tic_last_decompress_batch_adaptive (_direct)
    int last_tbatch_frames = 0, last_tbatch_single = 0, last_tbatch_chunks = 0;                             // tic_last_transcode_batch
    // rate control (tic_stream_sizes_dev, tic_compress_to_size_dev): the size kernel's table, a result per probe on the device and its
    // pinned landing buffer, and what the last search did
    DevBuf<SizeTabDev> d_size_tab{"d_size_tab", kBufState};
    DevBuf<SizeResult> d_rate{"d_rate"};
    PinBuf<SizeResult> h_rate{"h_rate"};
    int last_rate_probes = 0, last_rate_waits = 0;
    // ... their batch forms (tic_stream_sizes_v, tic_compress_batch_to_size): the pinned buffer a chunk's pixels are staged in (the chunk
    // itself and its probes' coefficients live in d_img / d_coef), the probe tables of one submission, and what the last call did
    PinBuf<uint8_t> h_rate_pix{"h_rate_pix"};
    PinBuf<SizeProbeTable> h_rate_tabs{"h_rate_tabs"};
    DevBuf<SizeProbeTable> d_rate_tabs{"d_rate_tabs"};
    int last_rbatch_frames = 0, last_rbatch_single = 0, last_rbatch_chunks = 0, last_rbatch_probes = 0, last_rbatch_waits = 0, last_rbatch_launches = 0;
    // ... and of rate-distortion control (tic_rd_points_v, tic_compress_batch_to_psnr, tic_distortion_v_dev): the tables of the measuring
    // kernel's descriptor form, one per launch
    PinBuf<SseProbeTable> h_rd_tabs{"h_rd_tabs"};
    DevBuf<SseProbeTable> d_rd_tabs{"d_rd_tabs"};
    int last_rbatch_sse_launches = 0;
    // the integer encoder's batch forms (tic_compress_batch_scaled_v, tic_dctq_scaled_v_dev, tic_rd_points_scaled_v): the tables of the
    // transform's descriptor form outside the batch slots, one per launch, and what the last calls did
    PinBuf<ScaledFrameTable> h_scaled_tabs{"h_scaled_tabs"};
    DevBuf<ScaledFrameTable> d_scaled_tabs{"d_scaled_tabs"};
    int last_sbatch_frames = 0, last_sbatch_single = 0, last_sbatch_chunks = 0, last_sbatch_launches = 0; // tic_last_compress_batch_scaled
    int last_srd_frames = 0, last_srd_single = 0, last_srd_chunks = 0, last_srd_launches = 0, last_srd_size_launches = 0,
        last_srd_sse_launches = 0; // tic_last_rd_scaled_batch
    // rate control of the adaptive family (tic_adaptive_sizes, tic_compress_adaptive_to_size, tic_adaptive_sizes_v): the statistics of a
    // submission's probes on the device and their pinned landing buffer, the frame tables of adaptive_stats_v_kernel where that kernel is
    // asked for (the probe kernel's tables are h_rate_tabs / d_rate_tabs), and what the last call did.  All grow on demand.
    DevBuf<AdaptStats> d_arate_stats{"d_arate_stats"};
    PinBuf<AdaptStats> h_arate_stats{"h_arate_stats"};
    PinBuf<AdaptFrameTable> h_arate_frames{"h_arate_frames"};
    DevBuf<AdaptFrameTable> d_arate_frames{"d_arate_frames"};
    int last_arate_probes = 0, last_arate_waits = 0, last_arate_launches = 0;
    // requantisation (tinyimgcodec_hip_requantize.h): the store launches' tables and range flags, the workspace tic_requant_kernels_timed
    // stores into (the calls themselves requantise in place in d_coef, where the reader left the rows), and what the last call did.
    DevBuf<int16_t> d_requant{"d_requant"};
    PinBuf<RequantLaunch> h_requant_tabs{"h_requant_tabs"};
    DevBuf<RequantLaunch> d_requant_tabs{"d_requant_tabs"};
    int last_rq_route = 0, last_rq_measure = 0, last_rq_store = 0, last_rq_rounds = 0;
};

// NUMA node of a device (its PCI function's numa_node in sysfs) and the CPUs of that node within this process's affinity mask.
static void find_numa(tic_ctx *ctx) {
    CPU_ZERO(&ctx->numa_cpus);
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof bus, ctx->device) != hipSuccess) return;
    for (char *p = bus; *p; p++) *p = (char)tolower(*p);
    char path[256];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE *f = fopen(path, "r");
    if (!f) return;
    int node = -1;
    const int ok = fscanf(f, "%d", &node);
    fclose(f);
    if (ok != 1 || node < 0) return;
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    f = fopen(path, "r");
    if (!f) return;
    char list[4096] = {0};
    const size_t n = fread(list, 1, sizeof list - 1, f);
    fclose(f);
    list[n] = 0;
    cpu_set_t mine;
    CPU_ZERO(&mine);
    if (sched_getaffinity(0, sizeof mine, &mine) != 0) return;
    // "0-63,128-191": walked with a local cursor (strtol) - contexts are created concurrently, strtok's state is process-global
    for (const char *p = list; *p;) {
        while (*p && (*p < '0' || *p > '9')) p++;
        if (!*p) break;
        char *end = nullptr;
        long a = strtol(p, &end, 10), b = a;
        p = end;
        if (*p == '-') {
            b = strtol(p + 1, &end, 10);
            p = end;
        }
        for (long c = a; c <= b && c < CPU_SETSIZE; c++)
            if (CPU_ISSET(c, &mine)) { CPU_SET(c, &ctx->numa_cpus); ctx->numa_ncpus++; }
    }
    ctx->numa_node = node;
}
// Called at the start of every thread the pipeline creates (never on the caller's thread).
static void bind_pipeline_thread(const tic_ctx *ctx) {
    // only when the node offers room for the pipeline's threads (8 stagers + reader + hand-out + consumers): a process mask that
    // leaves one or two CPUs of the device's node would put all of them on those
    if (ctx->numa_bind && ctx->numa_node >= 0 && ctx->numa_ncpus >= 8) (void)sched_setaffinity(0, sizeof ctx->numa_cpus, &ctx->numa_cpus);
}

static thread_local std::string g_create_err;

static int set_err(tic_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx)
        ctx->err = buf;
    else
        g_create_err = buf;
    return code;
}

// A batch call's failure in frame i: the message the failing step left, behind "frame i: ".
static int frame_err(tic_ctx *ctx, int code, int i) {
    const std::string why = ctx->err;
    return set_err(ctx, code, "frame %d: %s", i, why.c_str());
}

#define HIPCHK(ctx, call)                                                                                    \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return set_err(ctx, TIC_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__,  \
                           __LINE__);                                                                        \
    } while (0)

#define TIC_LOCK(ctx)                                      \
    std::unique_lock<std::recursive_mutex> ctx_lock_;      \
    if (ctx) ctx_lock_ = std::unique_lock<std::recursive_mutex>((ctx)->mu)

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The registry of the hooks build (BufRec above; folds away in the shipped library, where test_hooks_enabled() is a constant).
// buf_fill: one byte value into a whole buffer, device memory by hipMemset - waited for, the context's streams do not wait for the
// null stream by themselves - and pinned or host-mapped memory by the host.
static hipError_t buf_fill(const BufRec &r, int byte) {
    if (r.kind != kBufDev) {
        memset(r.p, byte, r.bytes);
        return hipSuccess;
    }
    const hipError_t e = hipMemset(r.p, byte, r.bytes);
    return e != hipSuccess ? e : hipStreamSynchronize(nullptr);
}
// A buffer the context now owns.  Under TIC_POISON=<byte> a scratch buffer is filled with the byte at once, before anything the
// allocation site clears itself.
static hipError_t buf_add(tic_ctx *ctx, void *p, size_t bytes, int kind, int cls, const char *name) {
    if (!test_hooks_enabled() || !ctx || !p) return hipSuccess;
    const BufRec r = {p, bytes, kind, cls, name};
    ctx->bufs.push_back(r);
    const char *e = test_hook("TIC_POISON");
    return e && cls == kBufScratch ? buf_fill(r, (int)(strtol(e, nullptr, 0) & 255)) : hipSuccess;
}
// ... and one it is about to free
static void buf_drop(tic_ctx *ctx, const void *p) {
    if (!test_hooks_enabled() || !ctx || !p) return;
    for (size_t i = 0; i < ctx->bufs.size(); i++)
        if (ctx->bufs[i].p == p) {
            ctx->bufs.erase(ctx->bufs.begin() + (ptrdiff_t)i);
            return;
        }
}

// Buf::grow and Buf::release: the only callers of buf_add and buf_drop (tic_test_poison reads the registry they keep).
template <class T, BufKind K> int Buf<T, K>::grow(tic_ctx *ctx, size_t need, size_t alloc) {
    if (need <= cap) return TIC_OK;
    buf_drop(ctx, p);
    HIPCHK(ctx, free_mem());
    alloc = alloc ? alloc : need;
    if (const hipError_t e = alloc_mem(alloc); e != hipSuccess) // (HIPCHK's text; the buffer's name and size stand for the call's arguments)
        return set_err(ctx, TIC_E_HIP, "%s(%s, %zu) failed: %s (%s:%d)", K == kBufDev ? "hipMalloc" : K == kBufPinned ? "hipHostMalloc" : "hipHostMalloc+GetDevicePointer",
                       name, alloc, hipGetErrorString(e), __FILE__, __LINE__);
    HIPCHK(ctx, buf_add(ctx, p, alloc, K, cls, name));
    return TIC_OK;
}
template <class T, BufKind K> void Buf<T, K>::release(tic_ctx *ctx) {
    buf_drop(ctx, p);
    (void)free_mem();
}

int DecWorkspace::grow(tic_ctx *ctx, size_t work_need, size_t work_alloc, size_t desc_need, size_t status, size_t status_alloc) {
    int rc = work.grow(ctx, work_need, work_alloc);
    if (rc) return rc;
    if (desc_need > desc_words) {
        desc_words = 0; // (counted only once the new words are zero)
        rc = desc.grow(ctx, desc_need * 8, (desc_need < 8192 ? 8192 : 2 * desc_need) * 8);
        if (rc) return rc;
        HIPCHK(ctx, hipMemset(desc, 0, desc.cap));
        desc_words = desc.cap / 8;
        epoch = 0;
    }
    return h_status.grow(ctx, status * sizeof(DecStatus), status_alloc * sizeof(DecStatus));
}

int DecWorkspace::begin(tic_ctx *ctx, hipStream_t stream, size_t status) {
    if (const char *e = test_hook("TIC_DEC_EPOCH")) { // (tests: the wrap below within a few calls; forwards only - no word carries a later epoch)
        const unsigned long v = strtoul(e, nullptr, 0);
        if (v > epoch && v < (1ul << 22)) epoch = (uint32_t)v;
    }
    if (++epoch >= (1u << 22)) { // (the scans carry 24 bits of 2 x epoch: start over on clean words long before a value could recur)
        HIPCHK(ctx, hipMemsetAsync(desc, 0, desc_words * 8, stream));
        epoch = 1;
    }
    memset(h_status, 0, status * sizeof(DecStatus)); // (host-mapped; nothing of an earlier run is in flight)
    if (test_hooks_enabled()) set_err(ctx, TIC_OK, "decoder run on %s: epoch %u", names[0], epoch); // (hooks build: where a test can read it, tic_last_error)
    return TIC_OK;
}

void DecWorkspace::release(tic_ctx *ctx) {
    work.release(ctx), desc.release(ctx), h_status.release(ctx);
    desc_words = 0, epoch = 0;
}

// (every Buf member of Slot is named here: one left out would still be freed with the slot, but its registry record would stay behind
// and tic_test_poison would fill freed memory - tests/test_context_state_cpu.py holds this list, and DecWorkspace's, against the fields)
void Slot::release(tic_ctx *ctx) {
    pin_in.release(ctx), pin_out.release(ctx), d_img.release(ctx), d_coef.release(ctx), d_work.release(ctx), d_lens.release(ctx), h_lens.release(ctx);
    d_err.release(ctx), h_err.release(ctx), d_streams.release(ctx), h_frames.release(ctx), d_frames.release(ctx), h_rb_off.release(ctx);
    h_sframes.release(ctx), d_sframes.release(ctx), d_adapt.release(ctx), h_adapt.release(ctx);
    for (hipEvent_t e : {done, rb_done})
        if (e) (void)hipEventDestroy(e);
    done = rb_done = nullptr;
    parity = first = count = pending = 0, rb_row = 0;
}

extern "C" {

const char *tic_version(void) { return "tinyimgcodec_amd 0.1.0 (gfx950)"; }
int tic_build_has_test_hooks(void) { return tic::test_hooks_enabled() ? 1 : 0; }

int tic_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *tic_last_error(const tic_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }
// (internal, for tic_comm.hip)
__attribute__((visibility("hidden"))) int tic_ctx_device(const tic_ctx *ctx) { return ctx ? ctx->device : -1; }
__attribute__((visibility("hidden"))) void *tic_ctx_stream(const tic_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }
const char *tic_device_arch(const tic_ctx *ctx) { return ctx ? ctx->arch : ""; }

size_t tic_num_blocks(int h, int w) { return num_blocks(h, w); }
size_t tic_compress_bound(int h, int w) { return compress_bound(h, w); }

// Drains and destroys every stream, destroys the events, and deletes the context: its buffers free themselves (Buf), behind the last
// synchronisation.  Supported with tickets open.
void tic_destroy(tic_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    std::vector<hipStream_t> streams = {ctx->rstream, ctx->bstream[0], ctx->bstream[1]};
    for (const auto &ln : ctx->lanes) streams.push_back(ln.stream);
    for (const auto &sl : ctx->dec_slots) streams.push_back(sl.stream);
    for (hipStream_t s : streams)
        if (s) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
        }
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    std::vector<hipEvent_t> events = {ctx->ev0, ctx->ev1, ctx->lane_order, ctx->dec_order};
    for (const auto &sl : ctx->bslots) events.insert(events.end(), {sl.done, sl.rb_done});
    for (const auto &sl : ctx->async_slots) events.push_back(sl.done);
    for (const auto &ln : ctx->lanes) events.insert(events.end(), {ln.packed, ln.placed[0], ln.placed[1]});
    for (const auto &sl : ctx->dec_slots) events.push_back(sl.done);
    for (hipEvent_t e : events)
        if (e) (void)hipEventDestroy(e);
    delete ctx;
}

static int create_impl(tic_ctx *ctx, int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return set_err(nullptr, TIC_E_NODEVICE, "no HIP device available (%s): the transform stage has no CPU fallback",
                       e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return set_err(nullptr, TIC_E_ARG, "device %d out of range (0..%d)", device, n - 1);
    ctx->device = device;
    hipDeviceProp_t prop;
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipGetDeviceProperties(&prop, device)) != hipSuccess)
        return set_err(nullptr, TIC_E_HIP, "cannot open device %d: %s", device, hipGetErrorString(e));
    snprintf(ctx->arch, sizeof ctx->arch, "%s", prop.gcnArchName);
    if (hipDeviceGetPCIBusId(ctx->pci, sizeof ctx->pci, device) != hipSuccess) {
        (void)hipGetLastError();
        ctx->pci[0] = 0;
    }
    find_numa(ctx);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_err(nullptr, TIC_E_NODEVICE, "device %d is %s; this library contains gfx950 (MI355X) code only", device,
                       prop.gcnArchName);
#define CK(call)                                                                                          \
    if ((e = (call)) != hipSuccess)                                                                       \
        return set_err(nullptr, TIC_E_HIP, "%s failed: %s", #call, hipGetErrorString(e));
    CK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    CK(hipStreamCreateWithFlags(&ctx->bstream[0], hipStreamNonBlocking));
    CK(hipStreamCreateWithFlags(&ctx->bstream[1], hipStreamNonBlocking));
    CK(hipStreamCreateWithFlags(&ctx->rstream, hipStreamNonBlocking));
    CK(hipEventCreate(&ctx->ev0));
    CK(hipEventCreate(&ctx->ev1));
    std::vector<DctqConsts> all(100);
    memset(all.data(), 0, all.size() * sizeof(DctqConsts));
    for (int q = 1; q <= 99; q++) build_consts(q, &all[q]);
    // (a buffer that does not come leaves its message in the context, which is about to go: handed on to tic_last_error(NULL))
#define GROW(buf, bytes) \
    if ((buf).grow(ctx, bytes) != TIC_OK) return set_err(nullptr, TIC_E_HIP, "%s", ctx->err.c_str());
    GROW(ctx->d_consts, all.size() * sizeof(DctqConsts));
    CK(hipMemcpy(ctx->d_consts, all.data(), all.size() * sizeof(DctqConsts), hipMemcpyHostToDevice));
    {
        HuffDev hd;
        build_huff_dev(&hd);
        GROW(ctx->d_huff, sizeof(HuffDev));
        CK(hipMemcpy(ctx->d_huff, &hd, sizeof(HuffDev), hipMemcpyHostToDevice));
        // one 32-byte status block: payload bits [2] of the device entropy stage, then its error flags [2]
        GROW(ctx->d_total_bits, 32);
        CK(hipMemset(ctx->d_total_bits, 0, 32));
        ctx->d_err = reinterpret_cast<int *>(ctx->d_total_bits + 2);
        // the stage's last kernel writes {payload bits, error} straight into pinned host memory: no copy behind it
        GROW(ctx->h_stat, 64 + kAsyncSlots * 16);
        memset(ctx->h_stat, 0, 64 + kAsyncSlots * 16);
        ctx->d_stat = ctx->h_stat.d;
    }
    GROW(ctx->d_fallback, 4 * sizeof(unsigned long long));
    CK(hipMemset(ctx->d_fallback, 0, 4 * sizeof(unsigned long long)));
#undef GROW
#undef CK
    return TIC_OK;
}

tic_ctx *tic_create(int device) {
    tic_ctx *ctx = new tic_ctx();
    if (create_impl(ctx, device) != TIC_OK) {
        if (ctx->device >= 0) tic_destroy(ctx); else delete ctx;
        return nullptr;
    }
    return ctx;
}

// ---- device memory helpers ---------------------------------------------------------------------------
int tic_dev_alloc(tic_ctx *ctx, size_t bytes, void **dptr) {
    TIC_LOCK(ctx);
    if (!ctx || !dptr) return TIC_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMalloc(dptr, bytes ? bytes : 1));
    return TIC_OK;
}
int tic_dev_free(tic_ctx *ctx, void *dptr) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipFree(dptr));
    return TIC_OK;
}
int tic_host_alloc_pinned(tic_ctx *ctx, size_t bytes, void **hptr) {
    TIC_LOCK(ctx);
    if (!ctx || !hptr) return TIC_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipHostMalloc(hptr, bytes ? bytes : 1, hipHostMallocDefault));
    return TIC_OK;
}
int tic_host_free_pinned(tic_ctx *ctx, void *hptr) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipHostFree(hptr));
    return TIC_OK;
}
// Pins memory the caller already holds (hipHostRegister): the batch entry points then copy such frames to the device from where
// they lie instead of staging them through their own pinned slots.
int tic_host_register(tic_ctx *ctx, void *hptr, size_t bytes) {
    TIC_LOCK(ctx);
    if (!ctx || !hptr || bytes == 0) return TIC_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipHostRegister(hptr, bytes, hipHostRegisterDefault));
    return TIC_OK;
}
int tic_host_unregister(tic_ctx *ctx, void *hptr) {
    TIC_LOCK(ctx);
    if (!ctx || !hptr) return TIC_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipHostUnregister(hptr));
    return TIC_OK;
}
// NUMA placement of the batch pipeline's host side.  *node = NUMA node of the context's device (-1 unknown), *ncpus = CPUs of that
// node this process may run on.  The pipeline's own threads bind to them unless binding is switched off (enable = 0); the pinned
// staging slots come from hipHostMalloc, which places them on the device's node by itself.
int tic_numa_info(tic_ctx *ctx, int *node, int *ncpus) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (node) *node = ctx->numa_node;
    if (ncpus) *ncpus = ctx->numa_ncpus;
    return TIC_OK;
}
int tic_set_stage_threads(tic_ctx *ctx, int threads) {
    TIC_LOCK(ctx);
    if (!ctx || threads < 0) return TIC_E_ARG;
    ctx->stage_threads = threads > 8 ? 8 : threads;
    return TIC_OK;
}
int tic_get_stage_threads(tic_ctx *ctx) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (ctx->stage_threads > 0) return ctx->stage_threads;
    const unsigned hw = std::thread::hardware_concurrency();
    const int T = (int)(hw ? hw / 2 : 4);
    return T < 1 ? 1 : (T > 8 ? 8 : T);
}
const char *tic_pci_bus_id(const tic_ctx *ctx) { return ctx ? ctx->pci : ""; }

int tic_set_numa_binding(tic_ctx *ctx, int enable) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    ctx->numa_bind = enable != 0;
    return TIC_OK;
}
// How the last tic_compress_batch / tic_dctq_batch call took its frames: copied from the caller's pinned or registered memory /
// staged through the pipeline's slots.
int tic_last_batch_input_path(tic_ctx *ctx, int *direct_frames, int *staged_frames) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (direct_frames) *direct_frames = ctx->last_batch_direct_frames;
    if (staged_frames) *staged_frames = ctx->last_batch_staged_frames;
    return TIC_OK;
}
// Pageable frames of a batch are pinned in place for the duration of the call where one registration covers them
// (auto_register_frames); enable = 0 stages them through the pipeline's pinned slots as rounds 1-3 did.
int tic_set_auto_register(tic_ctx *ctx, int enable) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    ctx->auto_register = enable != 0;
    return TIC_OK;
}
int tic_last_batch_auto_registered(tic_ctx *ctx, int *frames) {
    TIC_LOCK(ctx);
    if (!ctx || !frames) return TIC_E_ARG;
    *frames = ctx->last_batch_autoreg_frames;
    return TIC_OK;
}
int tic_last_batch_zero_copy(tic_ctx *ctx, int *streams) {
    TIC_LOCK(ctx);
    if (!ctx || !streams) return TIC_E_ARG;
    *streams = ctx->last_batch_zero_copy;
    return TIC_OK;
}
int tic_last_batch_phases(tic_ctx *ctx, double *ms8) {
    TIC_LOCK(ctx);
    if (!ctx || !ms8) return TIC_E_ARG;
    for (int k = 0; k < 8; k++) ms8[k] = ctx->bt.t[k] * 1e3;
    return TIC_OK;
}

int tic_memcpy_h2d(tic_ctx *ctx, void *dst, const void *src, size_t bytes) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TIC_OK;
}
int tic_memcpy_d2h(tic_ctx *ctx, void *dst, const void *src, size_t bytes) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TIC_OK;
}
int tic_memset_dev(tic_ctx *ctx, void *dst, int value, size_t bytes) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemsetAsync(dst, value, bytes, ctx->stream));
    return TIC_OK;
}
int tic_sync(tic_ctx *ctx) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (auto &sl : ctx->dec_slots) // (asynchronous decodes run on streams of their own)
        if (sl.stream) HIPCHK(ctx, hipStreamSynchronize(sl.stream));
    return TIC_OK;
}

// Test hook (hooks build only; the shipped library returns TIC_E_ARG and touches nothing): fills every scratch buffer of the context's
// registry with `byte`, behind everything its streams hold.  TIC_E_BUSY while a compress or decompress ticket is open - a frame in
// flight owns its buffers.  State buffers are never touched.
int tic_test_poison(tic_ctx *ctx, int byte) {
    TIC_LOCK(ctx);
    if (!test_hooks_enabled() || !ctx || byte < 0 || byte > 255) return TIC_E_ARG;
    if (ctx->async_open > 0) return TIC_E_BUSY;
    for (const auto &sl : ctx->dec_slots)
        if (sl.ticket >= 0) return TIC_E_BUSY;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (hipStream_t s : {ctx->stream, ctx->bstream[0], ctx->bstream[1], ctx->rstream, ctx->lanes[0].stream, ctx->lanes[1].stream})
        if (s) HIPCHK(ctx, hipStreamSynchronize(s));
    for (auto &sl : ctx->dec_slots)
        if (sl.stream) HIPCHK(ctx, hipStreamSynchronize(sl.stream));
    size_t filled = 0, bytes = 0, kept = 0;
    for (const BufRec &r : ctx->bufs) {
        if (r.cls != kBufScratch) {
            kept++;
            continue;
        }
        HIPCHK(ctx, buf_fill(r, byte));
        filled++, bytes += r.bytes;
    }
    // (what it did, where a test can read it: tic_last_error)
    set_err(ctx, TIC_OK, "tic_test_poison: %zu scratch buffers and %zu bytes filled with 0x%02x, %zu state buffers kept", filled, bytes, byte, kept);
    return TIC_OK;
}
// Test hook (hooks build only; the shipped library returns -1 and has no counter): the buffers the contexts of this process own now.
int tic_test_live_buffers(void) {
#ifdef TIC_TEST_HOOKS
    return g_live_buffers.load();
#else
    return -1;
#endif
}

// ---- transform stage -----------------------------------------------------------------------------------
// Waits for the context's stream.  A blocking hipStreamSynchronize wakes the thread some microseconds after the last kernel
// retired - a sixth of a 60 us device-resident compress - so short waits poll the stream first and only long ones block.
static hipError_t wait_stream(tic_ctx *ctx) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(ctx->stream);
        if (q != hipErrorNotReady) return q;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(250)) break;
    }
    return hipStreamSynchronize(ctx->stream);
}

static int check_geometry(tic_ctx *ctx, int h, int w, ptrdiff_t stride, int quality) {
    if (!ctx) return TIC_E_ARG;
    if (h < 0 || w < 0) return set_err(ctx, TIC_E_ARG, "negative image size %dx%d", h, w);
    if ((quality < 1 || quality > 99) && !(quality == TIC_QUALITY_CUSTOM && ctx->custom_quality != 0.0))
        return set_err(ctx, TIC_E_QUALITY, "quality %d outside 1..99 (the reference fails for 0, 100 and negatives)",
                       quality);
    if (h > 0 && w > 0 && stride < (ptrdiff_t)w) return set_err(ctx, TIC_E_ARG, "row stride %td < width %d", stride, w);
    return TIC_OK;
}

// ... for the entry points that write a stream: its header holds the quality as an integer (codec.py:102-114), the custom slot has none
static int check_stream_geometry(tic_ctx *ctx, int h, int w, ptrdiff_t stride, int quality) {
    if (ctx && quality == TIC_QUALITY_CUSTOM) return set_err(ctx, TIC_E_QUALITY, "a stream needs an integer quality 1..99 in its header");
    return check_geometry(ctx, h, w, stride, quality);
}

static DctqArgs make_args(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t stride, int quality, void *d_out) {
    DctqArgs a;
    a.img = (const uint8_t *)d_image;
    a.h = h;
    a.w = w;
    a.stride = (long)stride;
    a.bw = (w + 7) / 8;
    a.tiles_x = (a.bw + 7) / 8;
    a.ntiles = (h > 0 && w > 0) ? ((h + 7) / 8) * a.tiles_x : 0;
    a.aligned8 = ((((uintptr_t)d_image) | (uintptr_t)stride) & 7) == 0;
    a.consts = ctx->d_consts + quality;
    a.out = (int16_t *)d_out;
    a.fallback_count = ctx->stats ? ctx->d_fallback.p : nullptr;
    a.nframes = 1;
    a.frame_stride_in = 0;
    a.frame_stride_out = 0;
    a.dbg = nullptr;
    return a;
}

// Frames that follow each other without a gap and end on a block row ARE one tall frame for the transform stage (the DC is not
// differenced there): one persistent grid walks the whole batch in chunks, as for a 16384^2 frame, instead of a grid plane per
// frame with its own ramp and tail (256 x 1080p: 0.63-0.67 of the roofline per plane, see DESIGN.md section 5.5 for the merged form).
static void merge_frames(DctqArgs &a) {
    if (a.nframes <= 1 || (a.h & 7) != 0) return;
    const long long nblk = (long long)(a.h / 8) * a.bw;
    if (a.frame_stride_in != (long)a.h * a.stride || a.frame_stride_out != (long)(nblk * 128)) return;
    if ((unsigned long long)a.frame_stride_in * (unsigned long long)a.nframes >= (1ull << 32)) return; // the strip walk uses 32-bit offsets
    if ((long long)a.h * a.nframes > 0x7fffffffll / 8 || nblk * a.nframes > 0x7fffffffll) return;
    a.h *= a.nframes;
    a.ntiles = ((a.h + 7) / 8) * a.tiles_x;
    a.nframes = 1;
    a.frame_stride_in = 0;
    a.frame_stride_out = 0;
}

int tic_dctq_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, int quality, void *d_coeffs_zz,
                 int variant) {
    TIC_LOCK(ctx);
    int rc = check_geometry(ctx, h, w, row_stride, quality);
    if (rc) return rc;
    if (h == 0 || w == 0) return TIC_OK;
    if (!d_image || !d_coeffs_zz) return set_err(ctx, TIC_E_ARG, "null device pointer");
    const int v = dctq_kernel_id(variant);
    if (v < 0) return set_err(ctx, TIC_E_ARG, "unknown kernel variant %d", variant);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DctqArgs a = make_args(ctx, d_image, h, w, row_stride, quality, d_coeffs_zz);
    HIPCHK(ctx, launch_dctq(a, v, ctx->stream, nullptr, nullptr, &ctx->last_strip));
    return TIC_OK;
}

// Multi-frame form of a launch (DctqArgs and ScaledArgs alike): frame f's pixels lie f * frame_stride bytes behind the first frame's, its
// coefficients f * coeff_frame_stride bytes behind the first frame's.
extern "C++" { // (a template inside the C-ABI block)
template <class Args>
static int set_frames(tic_ctx *ctx, Args &a, int nframes, int h, int w, ptrdiff_t row_stride, ptrdiff_t frame_stride, ptrdiff_t coeff_frame_stride) {
    if (nframes > 65535) return set_err(ctx, TIC_E_ARG, "at most 65535 frames per launch");
    if (frame_stride < (ptrdiff_t)h * row_stride || coeff_frame_stride < (ptrdiff_t)(num_blocks(h, w) * 128))
        return set_err(ctx, TIC_E_ARG, "frame strides smaller than one frame");
    a.aligned8 = a.aligned8 && ((frame_stride & 7) == 0);
    a.nframes = nframes;
    a.frame_stride_in = (long)frame_stride;
    a.frame_stride_out = (long)coeff_frame_stride;
    return TIC_OK;
}
}

int tic_dctq_dev_frames(tic_ctx *ctx, const void *d_images, int nframes, int h, int w, ptrdiff_t row_stride,
                        ptrdiff_t frame_stride, int quality, void *d_coeffs_zz, ptrdiff_t coeff_frame_stride, int variant) {
    TIC_LOCK(ctx);
    int rc = check_geometry(ctx, h, w, row_stride, quality);
    if (rc) return rc;
    if (nframes < 0) return set_err(ctx, TIC_E_ARG, "negative frame count");
    if (h == 0 || w == 0 || nframes == 0) return TIC_OK;
    if (!d_images || !d_coeffs_zz) return set_err(ctx, TIC_E_ARG, "null device pointer");
    DctqArgs a = make_args(ctx, d_images, h, w, row_stride, quality, d_coeffs_zz);
    rc = set_frames(ctx, a, nframes, h, w, row_stride, frame_stride, coeff_frame_stride);
    if (rc) return rc;
    merge_frames(a);
    const int v = dctq_kernel_id(variant);
    if (v < 0) return set_err(ctx, TIC_E_ARG, "unknown kernel variant %d", variant);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, launch_dctq(a, v, ctx->stream, nullptr, nullptr, &ctx->last_strip));
    return TIC_OK;
}

// The timed entry points' submission: `warm` untimed launches, an event, `iters` timed launches, an event - ONE submission, nothing
// between the warm-up and the first event that the host waits for.  The first event is therefore stamped when the last warm-up launch
// retires, with the timed launches already in the queue behind it; recorded on an IDLE stream (warm = 0 after a synchronisation) it is
// stamped at once and the interval opens with whatever the host needs to get the first launch to the device - 28 us on the driver's box
// in round 5, 1.4 us per step at K = 20 (profiles/r06_driver_flags.txt).  *ms_total = the time between the two events.
// launch(i, ev_start, ev_stop) queues launch i of its phase (warm-up or timed) on the context's stream and returns a hipError_t.
// per_launch_ms: NULL, or room for 2 * iters floats.  Then every timed launch is handed a start and a stop event for its OWN dispatch
// packet (hipExtLaunchKernelGGL: the packet's time stamps, no marker packet between the launches - an event recorded behind every
// launch costs 3 us per launch) and per_launch_ms[2 i] = duration of launch i, per_launch_ms[2 i + 1] = the time between the start
// of the first timed launch and the end of launch i.  These events live for this call alone - created before the warm-up, destroyed
// on every way out - so a launch that does not bind them (the exact kernel, a banded frame) leaves them never recorded and the call
// reports TIC_E_ARG, whatever an earlier call on the context measured.
extern "C++" {
template <class Launch>
static int timed_launches(tic_ctx *ctx, int warm, int iters, float *ms_total, float *per_launch_ms, Launch launch) {
    struct Events {
        std::vector<hipEvent_t> v;
        ~Events() {
            for (hipEvent_t e : v)
                if (e) (void)hipEventDestroy(e);
        }
    } ev;
    ev.v.assign(per_launch_ms ? 2 * (size_t)iters : 0, nullptr);
    for (hipEvent_t &e : ev.v) HIPCHK(ctx, hipEventCreate(&e));
    for (int i = 0; i < warm; i++) HIPCHK(ctx, launch(i, nullptr, nullptr));
    HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    for (int i = 0; i < iters; i++) HIPCHK(ctx, launch(i, per_launch_ms ? ev.v[2 * i] : nullptr, per_launch_ms ? ev.v[2 * i + 1] : nullptr));
    HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
    HIPCHK(ctx, hipEventElapsedTime(ms_total, ctx->ev0, ctx->ev1));
    for (int i = 0; per_launch_ms && i < iters; i++)
        if (hipEventElapsedTime(per_launch_ms + 2 * i, ev.v[2 * i], ev.v[2 * i + 1]) != hipSuccess ||
            hipEventElapsedTime(per_launch_ms + 2 * i + 1, ev.v[0], ev.v[2 * i + 1]) != hipSuccess) {
            (void)hipGetLastError();
            return set_err(ctx, TIC_E_ARG, "per-launch times need a frame that takes the strip kernel in one launch");
        }
    return TIC_OK;
}
}

int tic_dctq_dev_timed(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, int quality,
                       void *d_coeffs_zz, int variant, int iters, float *ms_total) {
    TIC_LOCK(ctx);
    int rc = check_geometry(ctx, h, w, row_stride, quality);
    if (rc) return rc;
    if (!ms_total || iters < 1 || !d_image || !d_coeffs_zz) return set_err(ctx, TIC_E_ARG, "bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const DctqArgs a = make_args(ctx, d_image, h, w, row_stride, quality, d_coeffs_zz);
    const int v = dctq_kernel_id(variant);
    if (v < 0) return set_err(ctx, TIC_E_ARG, "unknown kernel variant %d", variant);
    return timed_launches(ctx, 0, iters, ms_total, nullptr, [&](int, hipEvent_t e0, hipEvent_t e1) { return launch_dctq(a, v, ctx->stream, e0, e1); });
}

// The benchmark's form of the timed entry: warm-up launches in front of the interval and, on request, per-launch times (timed_launches).
int tic_dctq_dev_timed_warm(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, int quality, void *d_coeffs_zz,
                            int variant, int warm, int iters, float *ms_total, float *per_launch_ms) {
    TIC_LOCK(ctx);
    int rc = check_geometry(ctx, h, w, row_stride, quality);
    if (rc) return rc;
    if (!ms_total || iters < 1 || warm < 0 || !d_image || !d_coeffs_zz) return set_err(ctx, TIC_E_ARG, "bad argument");
    if (per_launch_ms && iters > 32768) return set_err(ctx, TIC_E_ARG, "per-launch times for at most 32768 launches");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const DctqArgs a = make_args(ctx, d_image, h, w, row_stride, quality, d_coeffs_zz);
    const int v = dctq_kernel_id(variant);
    if (v < 0) return set_err(ctx, TIC_E_ARG, "unknown kernel variant %d", variant);
    return timed_launches(ctx, warm, iters, ms_total, per_launch_ms,
                          [&](int, hipEvent_t e0, hipEvent_t e1) { return launch_dctq(a, v, ctx->stream, e0, e1); });
}

// Batch form of the timed entry: `iters` back-to-back launches of the batched transform (nframes frames per launch).
int tic_dctq_dev_frames_timed(tic_ctx *ctx, const void *d_images, int nframes, int h, int w, ptrdiff_t row_stride,
                              ptrdiff_t frame_stride, int quality, void *d_coeffs_zz, ptrdiff_t coeff_frame_stride, int variant,
                              int iters, float *ms_total) {
    TIC_LOCK(ctx);
    int rc = check_geometry(ctx, h, w, row_stride, quality);
    if (rc) return rc;
    if (!ms_total || iters < 1 || nframes < 1 || nframes > 65535 || !d_images || !d_coeffs_zz) return set_err(ctx, TIC_E_ARG, "bad argument");
    const int v = dctq_kernel_id(variant);
    if (v < 0) return set_err(ctx, TIC_E_ARG, "unknown kernel variant %d", variant);
    DctqArgs a = make_args(ctx, d_images, h, w, row_stride, quality, d_coeffs_zz);
    rc = set_frames(ctx, a, nframes, h, w, row_stride, frame_stride, coeff_frame_stride);
    if (rc) return rc;
    merge_frames(a);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return timed_launches(ctx, 0, iters, ms_total, nullptr, [&](int, hipEvent_t e0, hipEvent_t e1) { return launch_dctq(a, v, ctx->stream, e0, e1); });
}

// Cold-cache form of the timed entry: launch i works on pair i % npairs of (image, coefficient buffer).  With enough
// distinct pairs (their total size well beyond the 256 MiB Infinity Cache) every launch reads and writes lines that have
// left the cache since their last use: the number is an HBM number, not an on-die one.
int tic_dctq_dev_timed_rotating(tic_ctx *ctx, const void *const *d_images, void *const *d_coeffs_zz, int npairs, int h, int w,
                                ptrdiff_t row_stride, int quality, int variant, int iters, float *ms_total) {
    TIC_LOCK(ctx);
    int rc = check_geometry(ctx, h, w, row_stride, quality);
    if (rc) return rc;
    if (!ms_total || iters < 1 || npairs < 1 || !d_images || !d_coeffs_zz) return set_err(ctx, TIC_E_ARG, "bad argument");
    const int v = dctq_kernel_id(variant);
    if (v < 0) return set_err(ctx, TIC_E_ARG, "unknown kernel variant %d", variant);
    for (int k = 0; k < npairs; k++)
        if (!d_images[k] || !d_coeffs_zz[k]) return set_err(ctx, TIC_E_ARG, "null device pointer in pair %d", k);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return timed_launches(ctx, 0, iters, ms_total, nullptr, [&](int i, hipEvent_t e0, hipEvent_t e1) {
        return launch_dctq(make_args(ctx, d_images[i % npairs], h, w, row_stride, quality, d_coeffs_zz[i % npairs]), v, ctx->stream, e0, e1);
    });
}

// Device entropy stage: pack with a lane per block (max_quality >= 1: for qualities up to it, with the automatic fall-back to the
// 8-lane kernel described at ent_lane_max_quality) or always with 8 lanes per block (max_quality < 1, the default).
int tic_set_entropy_lane_kernel(tic_ctx *ctx, int max_quality) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    ctx->ent_lane_max_quality = max_quality < 1 ? -1 : (max_quality > 99 ? 99 : max_quality);
    return TIC_OK;
}

// Non-integral qualities.  The reference's encode() / decode() compute with whatever number they are given (utils.py:50-53:
// factor = 5000 / q or 200 - 2 q, divisor = Q * factor / 100); the device keeps one constant block per INTEGER quality.  This
// installs the block of any number in [1, 99] in the context's spare slot; the transform and inverse entry points (tic_dctq,
// tic_encode, tic_encode_wide, tic_dctq_dev, tic_idctq) then take quality = TIC_QUALITY_CUSTOM to mean it.  (compress() packs the
// quality into the header as an integer - struct.error for a float in the reference - so the stream entry points have no use for it.)
int tic_set_custom_quality(tic_ctx *ctx, double quality) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    std::unique_ptr<DctqConsts> c(new DctqConsts());
    if (!build_consts(quality, c.get())) return set_err(ctx, TIC_E_QUALITY, "quality %g outside 1..99", quality);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); // (nothing in flight reads the slot: every entry point that uses it ends drained)
    HIPCHK(ctx, hipMemcpy(ctx->d_consts, c.get(), sizeof(DctqConsts), hipMemcpyHostToDevice));
    ctx->custom_quality = quality;
    return TIC_OK;
}

int tic_set_stats(tic_ctx *ctx, int enable) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    ctx->stats = enable != 0;
    return TIC_OK;
}

int tic_last_rare_path_stats(tic_ctx *ctx, unsigned long long stats[4]) {
    TIC_LOCK(ctx);
    if (!ctx || !stats) return TIC_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(stats, ctx->d_fallback, 4 * sizeof *stats, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_fallback, 0, 4 * sizeof *stats, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TIC_OK;
}

// What the launcher decided for the last transform launch through tic_dctq_dev / tic_dctq_dev_frames on this context (no other entry point
// updates it; the report of a call that returned before its launch is the call's before).  Host bookkeeping: no device work, no wait.
int tic_last_strip_launch(tic_ctx *ctx, int info[8]) {
    TIC_LOCK(ctx);
    if (!ctx || !info) return TIC_E_ARG;
    const StripLaunchInfo &s = ctx->last_strip;
    info[0] = s.order, info[1] = s.kind, info[2] = s.team_count, info[3] = s.grid_x;
    info[4] = s.grid_y, info[5] = s.tstep, info[6] = s.fast_tx, info[7] = s.fast_ty;
    return TIC_OK;
}

int tic_last_fallback_blocks(tic_ctx *ctx, unsigned long long *count) {
    if (!ctx || !count) return TIC_E_ARG;
    unsigned long long st[4];
    const int rc = tic_last_rare_path_stats(ctx, st);
    if (rc == TIC_OK) *count = st[0];
    return rc;
}

constexpr size_t kDecHostPixBytes = 1u << 20; // tic_decompress: images of at most this many bytes leave through tic_ctx::h_small as well
constexpr size_t kSmallHostBytes = 2u << 20; // tic_compress: frames whose stream bound is at most this go through tic_ctx::h_small
static int ensure_small(tic_ctx *ctx, size_t bytes) { return ctx->h_small.grow(ctx, bytes); }

static int ensure_scratch(tic_ctx *ctx, size_t img_bytes, size_t coef_bytes) {
    const int rc = ctx->d_img.grow(ctx, img_bytes);
    return rc ? rc : ctx->d_coef.grow(ctx, coef_bytes);
}

// Every host-image entry point brings its frame to the device here: the n blocks' uint8 pixels into the context's scratch image, rows
// padded to *pitch (a multiple of 256 bytes), queued on the context's stream; the coefficient workspace is provisioned beside it (with
// the 16 bytes of slack that the stream entry points provision for it).
static int upload_image(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, size_t n, size_t *pitch) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    *pitch = align_up((size_t)w, 256);
    const int rc = ensure_scratch(ctx, *pitch * (size_t)h, n * 128 + 16);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy2DAsync(ctx->d_img, *pitch, image, (size_t)row_stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice, ctx->stream));
    return TIC_OK;
}

int tic_dctq(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, int quality, int16_t *coeffs_zz) {
    TIC_LOCK(ctx);
    int rc = check_geometry(ctx, h, w, row_stride, quality);
    if (rc) return rc;
    const size_t n = num_blocks(h, w);
    if (n == 0) return TIC_OK;
    if (!image || !coeffs_zz) return set_err(ctx, TIC_E_ARG, "null host pointer");
    size_t pitch = 0;
    rc = upload_image(ctx, image, h, w, row_stride, n, &pitch);
    if (rc) return rc;
    DctqArgs a = make_args(ctx, ctx->d_img, h, w, (ptrdiff_t)pitch, quality, ctx->d_coef);
    HIPCHK(ctx, launch_dctq(a, 2, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(coeffs_zz, ctx->d_coef, n * 128, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TIC_OK;
}

int tic_encode(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, int quality, int32_t *dc,
               int32_t *ac) {
    TIC_LOCK(ctx);
    int rc = check_geometry(ctx, h, w, row_stride, quality);
    if (rc) return rc;
    const size_t n = num_blocks(h, w);
    if (n == 0) return TIC_OK;
    if (!dc || !ac) return set_err(ctx, TIC_E_ARG, "null output pointer");
    ctx->h_coef.resize(n * 64);
    rc = tic_dctq(ctx, image, h, w, row_stride, quality, ctx->h_coef.data());
    if (rc) return rc;
    int prev = 0;
    for (size_t b = 0; b < n; b++) { // codec.py:34-36
        const int16_t *c = ctx->h_coef.data() + b * 64;
        dc[b] = b ? c[0] - prev : c[0];
        prev = c[0];
        for (int k = 1; k < 64; k++) ac[b * 63 + (k - 1)] = c[k];
    }
    return TIC_OK;
}

// encode() for integer images outside 0..255 (codec.py:29 casts with astype(int32) and transforms whatever it finds):
// int32 pixels, float64 exact order on the device, int32 dc (DPCM applied) / ac as the reference returns them.
int tic_encode_wide(tic_ctx *ctx, const int32_t *image, int h, int w, ptrdiff_t row_stride_elems, int quality, int32_t *dc,
                    int32_t *ac) {
    TIC_LOCK(ctx);
    int rc = check_geometry(ctx, h, w, row_stride_elems, quality);
    if (rc) return rc;
    const size_t n = num_blocks(h, w);
    if (n == 0) return TIC_OK;
    if (!image || !dc || !ac) return set_err(ctx, TIC_E_ARG, "null pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rc = ensure_scratch(ctx, (size_t)h * (size_t)w * 4, n * 256);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy2DAsync(ctx->d_img, (size_t)w * 4, image, (size_t)row_stride_elems * 4, (size_t)w * 4, (size_t)h,
                                 hipMemcpyHostToDevice, ctx->stream));
    WideArgs a;
    a.img = (const int32_t *)ctx->d_img;
    a.out = (int32_t *)ctx->d_coef;
    a.h = h;
    a.w = w;
    a.stride = w;
    a.bw = (w + 7) / 8;
    a.tiles_x = (a.bw + 7) / 8;
    a.ntiles = ((h + 7) / 8) * a.tiles_x;
    a.consts = ctx->d_consts + quality;
    HIPCHK(ctx, launch_dctq_wide(a, ctx->stream));
    std::vector<int32_t> zz(n * 64);
    HIPCHK(ctx, hipMemcpyAsync(zz.data(), ctx->d_coef, n * 256, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    int32_t prev = 0;
    for (size_t b = 0; b < n; b++) { // codec.py:34-36 (np.diff wraps in int32 like the reference's arrays)
        const int32_t *c = zz.data() + b * 64;
        dc[b] = b ? (int32_t)((uint32_t)c[0] - (uint32_t)prev) : c[0];
        prev = c[0];
        for (int k = 1; k < 64; k++) ac[b * 63 + (k - 1)] = c[k];
    }
    return TIC_OK;
}

// ---- entropy stage / whole codec -------------------------------------------------------------------------
int tic_entropy_encode(const int16_t *coeffs_zz, int h, int w, int quality, uint8_t *out, size_t cap, size_t *out_len) {
    return entropy_encode(coeffs_zz, h, w, quality, out, cap, out_len);
}

int tic_entropy_size(const int16_t *coeffs_zz, int h, int w, size_t *bytes) { return entropy_size(coeffs_zz, h, w, bytes); }
// (include/tinyimgcodec_hip_wide.h) compress() of a wide image: the writer on tic_encode_wide's own int32 differences
int tic_entropy_encode_dpcm(const int32_t *dc, const int32_t *ac, int h, int w, int quality, uint8_t *out, size_t cap, size_t *out_len) {
    return entropy_encode_dpcm(dc, ac, h, w, quality, out, cap, out_len);
}

int tic_parse_header(const uint8_t *data, size_t len, int *h, int *w, int *quality, uint32_t *flag) {
    return parse_header(data, len, h, w, quality, flag);
}

// ---- device entropy stage: what its entry points share ------------------------------------------------------------------------------
// A stream's destination in device memory: room for a header (and the scaled form's flush byte), 16-byte aligned for the placing kernel.
static int check_dev_out(tic_ctx *ctx, const void *d_out, size_t cap, size_t min_cap) {
    if (!d_out || cap < min_cap) return set_err(ctx, TIC_E_SPACE, "output buffer too small");
    if (((uintptr_t)d_out & 15u) != 0) return set_err(ctx, TIC_E_ARG, "device output buffer must be 16-byte aligned");
    return TIC_OK;
}

// The stream of an image without blocks, queued on the context's stream: 16 bytes of header (codec.py:151) and, for a scaled-DCT stream,
// the byte BB_flushBits writes with nothing pending (17 bytes).
static int put_header_only(tic_ctx *ctx, void *d_out, int h, int w, int quality, bool scaled) {
    uint8_t hdr[17] = {0};
    if (scaled)
        write_header_scaled(hdr, h, w, quality);
    else
        write_header(hdr, h, w, quality);
    HIPCHK(ctx, hipMemcpyAsync(d_out, hdr, scaled ? 17 : 16, hipMemcpyHostToDevice, ctx->stream));
    return TIC_OK;
}

// Pack and place on the context's own workspace and stream: the n blocks at d_zz -> the stream at d_out, which holds `cap` bytes; the
// placing kernel writes the header and puts {payload bits, error} into the host-mapped status block; nothing is written past the
// caller's buffer.  The context's two error flags are used in turn (tic_entropy_gpu.h).
static hipError_t pack_and_place(tic_ctx *ctx, const void *d_zz, size_t n, int h, int w, int quality, void *d_out, size_t cap, int mode,
                                 uint32_t flag) {
    const int par = ctx->ent_parity;
    ctx->ent_parity ^= 1;
    const size_t cap_words = ((cap - 16) / 16) * 4; // whole 16-byte units behind the header
    return entropy_gpu_fused((const int16_t *)d_zz, n, 1, ctx->d_huff, ctx->d_ent_work, ctx->d_ent_work.cap, d_out, 0, cap_words, h, w, quality,
                             nullptr, ctx->d_stat, ctx->d_err + par, ctx->d_err + (par ^ 1), mode, ctx->stream, nullptr, nullptr, flag);
}

// What a placing kernel left in a {payload bits, error} pair of the host-mapped status block (read behind the kernel's completion), and
// what that means for a caller whose buffer holds `cap` bytes: TIC_OK and the stream's length, TIC_E_RANGE, or TIC_E_SPACE.
struct StreamStatus {
    unsigned long long bits;
    int err;
};
static StreamStatus read_status(const unsigned long long *h_pair) {
    const volatile unsigned long long *p = h_pair;
    return {p[0], (int)(p[1] & 0xffffffffull)};
}
static int stream_result(tic_ctx *ctx, StreamStatus st, size_t cap, bool scaled, size_t *out_len) {
    if (st.err == 1) return set_err(ctx, TIC_E_RANGE, "coefficient without a Huffman code (reference raises KeyError)");
    const size_t payload = scaled ? (size_t)(st.bits / 8) + 1 : (size_t)((st.bits + 7) / 8); // (scaled: BB_flushBits' byte)
    if (st.err == 2 || 16 + payload > cap)
        return set_err(ctx, TIC_E_SPACE, "output buffer too small (%zu bytes needed)", 16 + (size_t)((payload + 3) / 4) * 4);
    *out_len = 16 + payload;
    return TIC_OK;
}

// Device entropy stage: coefficients in HBM -> finished stream in HBM, three launches (pack: one walk over the symbols, tile sums,
// place), no host round trip and no copy.  Synchronous: the call returns the stream's length.
// scaled: the stream of the reference's integer encoder (tic_entropy_gpu.h: flag 1 << 30, setting 0..3 in the quality field, flush byte).
static int entropy_encode_dev_impl(tic_ctx *ctx, const void *d_coeffs_zz, int h, int w, int quality, void *d_out, size_t cap,
                                   size_t *out_len, bool scaled) {
    TIC_LOCK(ctx);
    if (!ctx || !out_len) return TIC_E_ARG;
    if (h < 0 || w < 0) return set_err(ctx, TIC_E_ARG, "negative image size");
    if (scaled) {
        if (quality < 0 || quality > 3) return set_err(ctx, TIC_E_QUALITY, "scaled-DCT setting %d outside 0..3", quality);
    } else if (quality < 1 || quality > 99)
        return set_err(ctx, TIC_E_QUALITY, "quality %d outside 1..99", quality);
    int rc = check_dev_out(ctx, d_out, cap, scaled ? 17 : 16);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = num_blocks(h, w);
    if (n == 0) {
        rc = put_header_only(ctx, d_out, h, w, quality, scaled);
        if (rc) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        *out_len = scaled ? 17 : 16;
        return TIC_OK;
    }
    if (!d_coeffs_zz) return set_err(ctx, TIC_E_ARG, "null coefficient pointer");
    rc = ctx->d_ent_work.grow(ctx, entropy_fused_work_bytes(n));
    if (rc) return rc;
    StreamStatus st = {0, 0};
    for (int attempt = 0; attempt < 2; attempt++) {
        // (a scaled-DCT stream always takes the 8-lane kernel, which has no limit per block: the lane kernel's limit is learnt per quality)
        const int mode = (attempt == 0 && !scaled && quality <= ctx->ent_lane_max_quality) ? kEntropyLanePerBlock : kEntropyEightLanes;
        HIPCHK(ctx, pack_and_place(ctx, d_coeffs_zz, n, h, w, quality, d_out, cap, mode, scaled ? kFlagScaled : 0u));
        HIPCHK(ctx, wait_stream(ctx));
        st = read_status(ctx->h_stat);
        if (st.err != 4 || mode == kEntropyEightLanes) break;
        ctx->ent_lane_max_quality = quality - 1; // a block of this frame needs more than a lane string holds: 8-lane kernel from here on
    }
    return stream_result(ctx, st, cap, scaled, out_len);
}

int tic_entropy_encode_dev(tic_ctx *ctx, const void *d_coeffs_zz, int h, int w, int quality, void *d_out, size_t cap,
                           size_t *out_len) {
    return entropy_encode_dev_impl(ctx, d_coeffs_zz, h, w, quality, d_out, cap, out_len, false);
}

// compress() with every stage on the device: transform kernels + device entropy stage; image and stream in HBM.
int tic_compress_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, int quality, void *d_out,
                     size_t cap, size_t *out_len) {
    TIC_LOCK(ctx);
    int rc = check_stream_geometry(ctx, h, w, row_stride, quality);
    if (rc) return rc;
    const size_t n = num_blocks(h, w);
    rc = ensure_scratch(ctx, 0, n * 128 + 16);
    if (rc) return rc;
    rc = tic_dctq_dev(ctx, d_image, h, w, row_stride, quality, ctx->d_coef, TIC_KERNEL_HYBRID);
    if (rc) return rc;
    return tic_entropy_encode_dev(ctx, ctx->d_coef, h, w, quality, d_out, cap, out_len);
}

// A lane's stream, events and error words (once), and its buffers for frames of n blocks.
static int ensure_lane(tic_ctx *ctx, tic_ctx::AsyncLane &ln, size_t n) {
    if (!ln.stream) {
        HIPCHK(ctx, hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
        HIPCHK(ctx, hipEventCreateWithFlags(&ln.packed, hipEventDisableTiming));
        HIPCHK(ctx, hipEventCreateWithFlags(&ln.placed[0], hipEventDisableTiming));
        HIPCHK(ctx, hipEventCreateWithFlags(&ln.placed[1], hipEventDisableTiming));
        const int rc = ln.d_err.grow(ctx, 4 * sizeof(int));
        if (rc) return rc;
        HIPCHK(ctx, hipMemset(ln.d_err, 0, 4 * sizeof(int)));
    }
    if (!ctx->lane_order) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->lane_order, hipEventDisableTiming));
    const size_t coef_bytes = n * 128 + 16, wb = entropy_fused_work_bytes(n);
    if (coef_bytes <= ln.d_coef.cap && wb <= ln.d_work[0].cap && wb <= ln.d_work[1].cap) return TIC_OK;
    // (grows only between bursts of one geometry: frames in flight still use the old buffers)
    HIPCHK(ctx, hipStreamSynchronize(ln.stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    int rc = ln.d_coef.grow(ctx, coef_bytes);
    for (int k = 0; k < 2 && rc == TIC_OK; k++) rc = ln.d_work[k].grow(ctx, wb);
    return rc;
}

// Asynchronous form of tic_compress_dev: the frame's launches (transform, pack, tile sums, place) are queued and the call returns; a
// caller that compresses resident frames back to back pays the submission ramp and the completion wake-up once per burst instead of once
// per frame.  Round 6: ONE context, TWO lanes.  Transform and packing of ticket t run on lane t & 1 - a stream, a coefficient buffer, an
// entropy workspace and a pair of error flags of its own - and only the placing kernel, the stage's single writer of the caller's buffer and
// of the ticket's status pair, is queued on the context's stream, behind the lane's packing and in ticket order.  The transform of frame
// t + 1 (bound by HBM) and its packing thus run beside the packing (bound by vector issue) and placing of frame t: what round 5 reached
// only from two contexts and two host threads (39 against 48 us per 4096^2 frame).  Ordering: a lane starts behind everything the context's
// stream held when the burst's first ticket was issued (every synchronous entry point returns with that stream drained, so nothing else can
// be in front of a later ticket); a lane's next frame waits for the placing of its previous one (it reuses the workspace that kernel
// reads); whatever is queued on the context's stream afterwards runs behind the placing kernels, hence behind every kernel of the tickets.
// The placing kernel leaves {payload bits, error} in the ticket's pair of the host-mapped status block; tic_async_result reads it once the
// ticket's event has fired.  Until then the caller leaves the frame's input and output alone.
int tic_compress_dev_async(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, int quality, void *d_out, size_t cap,
                           long long *ticket) {
    TIC_LOCK(ctx);
    if (!ctx || !ticket) return TIC_E_ARG;
    int rc = check_stream_geometry(ctx, h, w, row_stride, quality);
    if (rc) return rc;
    rc = check_dev_out(ctx, d_out, cap, 16);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long long t = ctx->async_next;
    tic_ctx::AsyncSlot &sl = ctx->async_slots[t % kAsyncSlots];
    if (sl.ticket >= 0) return set_err(ctx, TIC_E_ARG, "%d asynchronous calls are open: collect results (tic_async_result) first", kAsyncSlots);
    if (!sl.done) HIPCHK(ctx, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    volatile unsigned long long *hs = ctx->h_stat + 8 + 2 * (t % kAsyncSlots);
    unsigned long long *ds = ctx->d_stat + 8 + 2 * (t % kAsyncSlots);
    const size_t n = num_blocks(h, w);
    sl.cap = cap;
    sl.empty_image = n == 0;
    if (n == 0) {
        rc = put_header_only(ctx, d_out, h, w, quality, false);
        if (rc) return rc;
    } else {
        if (!d_image) return set_err(ctx, TIC_E_ARG, "null image pointer");
        tic_ctx::AsyncLane &ln = ctx->lanes[t & 1];
        rc = ensure_lane(ctx, ln, n);
        if (rc) return rc;
        hs[0] = 0;
        hs[1] = 0;
        if (ctx->async_open == 0) { // a burst begins: its lanes start behind whatever the context's stream holds now
            HIPCHK(ctx, hipEventRecord(ctx->lane_order, ctx->stream));
            ctx->lane_epoch++;
        }
        if (ln.order_seen != ctx->lane_epoch) {
            HIPCHK(ctx, hipStreamWaitEvent(ln.stream, ctx->lane_order, 0));
            ln.order_seen = ctx->lane_epoch;
        }
        const int wk = (int)(ln.frames & 1), ek = (int)(ln.frames & 3);
        if (ln.placed_valid[wk]) HIPCHK(ctx, hipStreamWaitEvent(ln.stream, ln.placed[wk], 0)); // the frame that used this workspace two lane-frames ago has been placed
        DctqArgs a = make_args(ctx, d_image, h, w, row_stride, quality, ln.d_coef);
        HIPCHK(ctx, launch_dctq(a, dctq_kernel_id(TIC_KERNEL_HYBRID), ln.stream));
        const size_t cap_words = ((cap - 16) / 16) * 4;
        // (the 8-lane packing kernel: it takes any block the format allows, so no second run can be needed)
        HIPCHK(ctx, entropy_gpu_fused((const int16_t *)ln.d_coef, n, 1, ctx->d_huff, ln.d_work[wk], ln.d_work[wk].cap, d_out, 0, cap_words, h, w, quality, nullptr, ds,
                                      ln.d_err + ek, ln.d_err + ((ek + 3) & 3), kEntropyEightLanes, ln.stream, ctx->stream, ln.packed));
        HIPCHK(ctx, hipEventRecord(ln.placed[wk], ctx->stream));
        ln.placed_valid[wk] = true;
        ln.frames++;
    }
    HIPCHK(ctx, hipEventRecord(sl.done, ctx->stream));
    sl.ticket = t;
    ctx->async_open++;
    ctx->async_next = t + 1;
    *ticket = t;
    return TIC_OK;
}

// Result of an asynchronous call: TIC_OK and the stream's length, or that frame's error (TIC_E_RANGE: a coefficient without a Huffman
// code, TIC_E_SPACE: the stream did not fit).  wait == 0: returns TIC_E_BUSY while the frame is still in flight.  A ticket is closed
// by the call that returns anything but TIC_E_BUSY.
int tic_async_result(tic_ctx *ctx, long long ticket, int wait, size_t *out_len) {
    TIC_LOCK(ctx);
    if (!ctx || !out_len || ticket < 0) return TIC_E_ARG;
    tic_ctx::AsyncSlot &sl = ctx->async_slots[ticket % kAsyncSlots];
    if (sl.ticket != ticket) return set_err(ctx, TIC_E_ARG, "ticket %lld is not open", ticket);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    {   // (any return other than TIC_E_BUSY closes the ticket - a failing event call included: the slot must not stay open for good)
        const hipError_t q = wait ? hipEventSynchronize(sl.done) : hipEventQuery(sl.done);
        if (!wait && q == hipErrorNotReady) return TIC_E_BUSY;
        if (q != hipSuccess) { sl.ticket = -1; ctx->async_open--; }
        HIPCHK(ctx, q);
    }
    sl.ticket = -1;
    ctx->async_open--;
    if (sl.empty_image) {
        *out_len = 16;
        return TIC_OK;
    }
    return stream_result(ctx, read_status(ctx->h_stat + 8 + 2 * (ticket % kAsyncSlots)), sl.cap, false, out_len);
}

int tic_compress(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, int quality, uint8_t *out,
                 size_t cap, size_t *out_len) {
    TIC_LOCK(ctx);
    int rc = check_stream_geometry(ctx, h, w, row_stride, quality);
    if (rc) return rc;
    if (!out || !out_len) return set_err(ctx, TIC_E_ARG, "null output pointer");
    const size_t n = num_blocks(h, w);
    if (n == 0) return entropy_encode(nullptr, h, w, quality, out, cap, out_len);
    if (!image) return set_err(ctx, TIC_E_ARG, "null image pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // image -> HBM, transform stage, entropy stage, all on the device; only the finished stream returns
    const size_t need = compress_bound(h, w);
    const bool small = need <= kSmallHostBytes && !test_hook("TIC_NO_SMALL_PATH"); // the placing kernel writes the stream into host memory itself
    rc = small ? ensure_small(ctx, kSmallHostBytes) : ctx->d_stream_buf.grow(ctx, need);
    if (rc) return rc;
    size_t pitch = 0, len = 0;
    rc = upload_image(ctx, image, h, w, row_stride, n, &pitch);
    if (rc) return rc;
    rc = tic_compress_dev(ctx, ctx->d_img, h, w, (ptrdiff_t)pitch, quality, small ? (void *)ctx->h_small.d : ctx->d_stream_buf,
                          small ? ctx->h_small.cap : ctx->d_stream_buf.cap, &len);
    if (rc) return rc;
    if (len > cap) return set_err(ctx, TIC_E_SPACE, "output buffer too small (%zu bytes needed, %zu given)", len, cap);
    if (small) {
        memcpy(out, ctx->h_small, len); // (tic_compress_dev returned behind a drained stream: the kernel's stores have arrived)
    } else {
        HIPCHK(ctx, hipMemcpyAsync(out, ctx->d_stream_buf, len, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    *out_len = len;
    return TIC_OK;
}

// ---- rate control: the size of a stream without the stream, and the best quality within a byte budget -----------------------------
// (No counterpart in the reference, whose only way to a size is len(compress(image, q)), codec.py:133-164; its benchmark is a table of
// such sizes, tests/benchmark.py.)  A PROBE of quality q is the transform into the context's coefficient workspace followed by the
// size kernel (tic_size_gpu.hip) adding into the probe's SizeResult: two launches, nothing staged, nothing placed, no stream byte
// written.  Any number of probes are queued back to back on the context's stream - they share the workspace, the stream orders them -
// and come back in ONE copy.
static int ensure_rate(tic_ctx *ctx, size_t nres) {
    if (!ctx->d_size_tab) {
        SizeTabDev t;
        build_size_tab(&t);
        const int rc = ctx->d_size_tab.grow(ctx, sizeof t);
        if (rc) return rc;
        const hipError_t e = hipMemcpy(ctx->d_size_tab, &t, sizeof t, hipMemcpyHostToDevice);
        if (e != hipSuccess) ctx->d_size_tab.release(ctx); // (never a table half written: the next call builds it again)
        HIPCHK(ctx, e);
    }
    // (a DistortionResult per probe as well, behind the nres SizeResults: dist_of)
    const size_t need = nres * (sizeof(SizeResult) + sizeof(DistortionResult)), alloc = align_up(need, 4096);
    const int rc = ctx->d_rate.grow(ctx, need, alloc);
    return rc ? rc : ctx->h_rate.grow(ctx, need, alloc);
}

// The distortion results of a submission of nq probes lie behind its nq size results, in the device buffer and in its landing buffer alike:
// one memset clears both, one copy brings both back.
static inline DistortionResult *dist_of(SizeResult *rate, int nq) { return reinterpret_cast<DistortionResult *>(rate + nq); }

// Launch arguments of the measuring kernel: coefficients as idct_kernel takes them (quality / scaled_exp as StreamHead), the original frame.
static void measure_args(const tic_ctx *ctx, const void *d_coeffs, const void *d_image, int h, int w, ptrdiff_t stride, int quality, int scaled_exp,
                         DistortionResult *d_res, IdctArgs *a, SseArgs *m) {
    a->coeffs = (const int16_t *)d_coeffs;
    a->out = nullptr;
    a->h = h;
    a->w = w;
    a->stride = 0;
    a->bw = (w + 7) / 8;
    a->tiles_x = (a->bw + 7) / 8;
    a->ntiles = (h > 0 && w > 0) ? ((h + 7) / 8) * a->tiles_x : 0;
    a->aligned8 = 0;
    a->consts = ctx->d_consts + (scaled_exp >= 0 ? 50 : quality); // codec.py:62: quality = 50 on the scaled branch
    a->scaled = scaled_exp >= 0;
    a->pow2 = scaled_exp >= 0 ? ldexp(1.0, scaled_exp) : 1.0;
    m->img = (const uint8_t *)d_image;
    m->stride = (long)stride;
    m->aligned8 = ((((uintptr_t)d_image) | (uintptr_t)stride) & 7) == 0;
    m->res = d_res;
}

// Queues the probes of q[0 .. nq) and the copy of their results into ctx->h_rate; the caller waits for the stream.
// distortion: every probe also runs the measuring kernel on its coefficients against the frame (a rate-distortion probe: three launches);
// its sums come back in the same copy (dist_of(ctx->h_rate, nq)).
static int queue_probes(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, size_t n, const int *q, int nq, bool distortion = false) {
    const size_t res_bytes = (size_t)nq * (sizeof(SizeResult) + (distortion ? sizeof(DistortionResult) : 0));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_rate, 0, res_bytes, ctx->stream));
    for (int i = 0; i < nq; i++) {
        DctqArgs a = make_args(ctx, d_image, h, w, row_stride, q[i], ctx->d_coef);
        HIPCHK(ctx, launch_dctq(a, dctq_kernel_id(TIC_KERNEL_AUTO), ctx->stream));
        HIPCHK(ctx, stream_size_gpu((const int16_t *)ctx->d_coef, n, 1, ctx->d_size_tab, ctx->d_rate + i, ctx->stream));
        if (distortion) {
            IdctArgs ia;
            SseArgs m;
            measure_args(ctx, ctx->d_coef, d_image, h, w, row_stride, q[i], -1, dist_of(ctx->d_rate, nq) + i, &ia, &m);
            HIPCHK(ctx, launch_idct_sse(ia, m, ctx->stream));
        }
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_rate, ctx->d_rate, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    return TIC_OK;
}

// Stream length of a probe: 16-byte header + the payload rounded up to a byte (bitbuffer.py:17-18); -1: a coefficient without a code.
static inline long long probe_size(const SizeResult &r) { return r.nocode ? -1ll : (long long)(16ull + ((r.bits + 7ull) >> 3)); }

int tic_entropy_size_dev(tic_ctx *ctx, const void *d_coeffs_zz, int h, int w, size_t *bytes) {
    TIC_LOCK(ctx);
    if (!ctx || !bytes) return TIC_E_ARG;
    if (h < 0 || w < 0) return set_err(ctx, TIC_E_ARG, "negative image size");
    const size_t n = num_blocks(h, w);
    if (n == 0) {
        *bytes = 16;
        return TIC_OK;
    }
    if (!d_coeffs_zz) return set_err(ctx, TIC_E_ARG, "null coefficient pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = ensure_rate(ctx, 1);
    if (rc) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->d_rate, 0, sizeof(SizeResult), ctx->stream));
    HIPCHK(ctx, stream_size_gpu((const int16_t *)d_coeffs_zz, n, 1, ctx->d_size_tab, ctx->d_rate, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_rate, ctx->d_rate, sizeof(SizeResult), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, wait_stream(ctx));
    const long long s = probe_size(ctx->h_rate[0]);
    if (s < 0) return set_err(ctx, TIC_E_RANGE, "coefficient without a Huffman code (reference raises KeyError)");
    *bytes = (size_t)s;
    return TIC_OK;
}

// Times `iters` back-to-back launches of the size kernel on resident coefficients, behind `warm` untimed ones (timed_launches).
int tic_entropy_size_dev_timed(tic_ctx *ctx, const void *d_coeffs_zz, int h, int w, int warm, int iters, float *ms_total) {
    TIC_LOCK(ctx);
    if (!ctx || !ms_total || warm < 0 || iters <= 0) return TIC_E_ARG;
    if (h < 0 || w < 0) return set_err(ctx, TIC_E_ARG, "negative image size");
    const size_t n = num_blocks(h, w);
    if (n && !d_coeffs_zz) return set_err(ctx, TIC_E_ARG, "null coefficient pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = ensure_rate(ctx, 1);
    if (rc) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->d_rate, 0, sizeof(SizeResult), ctx->stream));
    return timed_launches(ctx, warm, iters, ms_total, nullptr, [&](int, hipEvent_t, hipEvent_t) {
        return stream_size_gpu((const int16_t *)d_coeffs_zz, n, 1, ctx->d_size_tab, ctx->d_rate, ctx->stream);
    });
}

static int check_size_args(tic_ctx *ctx, int h, int w, ptrdiff_t row_stride, const int *qualities, int nq, long long *sizes) {
    if (!ctx) return TIC_E_ARG;
    if (nq < 0 || (nq > 0 && (!qualities || !sizes))) return set_err(ctx, TIC_E_ARG, "bad quality list");
    for (int i = 0; i < nq; i++) {
        const int rc = check_stream_geometry(ctx, h, w, row_stride, qualities[i]);
        if (rc) return rc;
    }
    return TIC_OK;
}

int tic_stream_sizes_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, const int *qualities, int nq,
                         long long *sizes) {
    TIC_LOCK(ctx);
    int rc = check_size_args(ctx, h, w, row_stride, qualities, nq, sizes); // (a bad quality fails here: nothing has been queued)
    if (rc || nq == 0) return rc;
    const size_t n = num_blocks(h, w);
    if (n == 0) { // header only (codec.py:151)
        for (int i = 0; i < nq; i++) sizes[i] = 16;
        return TIC_OK;
    }
    if (!d_image) return set_err(ctx, TIC_E_ARG, "null image pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rc = ensure_scratch(ctx, 0, n * 128 + 16);
    if (rc) return rc;
    rc = ensure_rate(ctx, (size_t)nq);
    if (rc) return rc;
    rc = queue_probes(ctx, d_image, h, w, row_stride, n, qualities, nq);
    if (rc) return rc;
    HIPCHK(ctx, wait_stream(ctx));
    for (int i = 0; i < nq; i++) sizes[i] = probe_size(ctx->h_rate[i]);
    return TIC_OK;
}

int tic_stream_sizes(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, const int *qualities, int nq, long long *sizes) {
    TIC_LOCK(ctx);
    int rc = check_size_args(ctx, h, w, row_stride, qualities, nq, sizes);
    if (rc || nq == 0) return rc;
    const size_t n = num_blocks(h, w);
    if (n == 0) return tic_stream_sizes_dev(ctx, nullptr, h, w, row_stride, qualities, nq, sizes);
    if (!image) return set_err(ctx, TIC_E_ARG, "null image pointer");
    size_t pitch = 0;
    rc = upload_image(ctx, image, h, w, row_stride, n, &pitch);
    if (rc) return rc;
    return tic_stream_sizes_dev(ctx, ctx->d_img, h, w, (ptrdiff_t)pitch, qualities, nq, sizes);
}

// The search.  Its contract is the bisection of the header (tic_compress_to_size_dev); what is free is WHEN a quality is probed.  The
// bisection and its look-ahead are RateSearch's (tic_rate_plan.h, which the batch form drives for a chunk of frames at once): a round is
// one queue of the candidates it names, one wait, and its replay.  A wait costs about what a probe of a 4096^2 frame does (some 15 us), a
// probe of a small frame a fraction of that: deep look-ahead for small frames, none for frames beyond 4096^2 (single_frame_depth).

// The last step of a search (by size or by distortion) that ended at quality q, whose probe said `len` bytes: transform, pack and place
// into the context's own buffer, then exactly its bytes into the caller's - the length is known from the probe, so the copy is queued
// behind the placing kernel and the whole stream costs one wait.
static int chosen_stream(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, size_t n, int q, size_t len, void *out,
                         bool out_on_host, size_t cap, size_t *out_len, int *quality) {
    if (len > cap) {
        *out_len = len;
        return set_err(ctx, TIC_E_SPACE, "output buffer too small (%zu bytes needed, %zu given)", len, cap);
    }
    int rc = ctx->d_stream_buf.grow(ctx, compress_bound(h, w));
    if (rc) return rc;
    rc = ctx->d_ent_work.grow(ctx, entropy_fused_work_bytes(n));
    if (rc) return rc;
    DctqArgs a = make_args(ctx, d_image, h, w, row_stride, q, ctx->d_coef);
    HIPCHK(ctx, launch_dctq(a, dctq_kernel_id(TIC_KERNEL_HYBRID), ctx->stream));
    HIPCHK(ctx, pack_and_place(ctx, ctx->d_coef, n, h, w, q, ctx->d_stream_buf, ctx->d_stream_buf.cap, kEntropyEightLanes, 0u));
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->d_stream_buf, len, out_on_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, out_on_host ? hipStreamSynchronize(ctx->stream) : wait_stream(ctx));
    ctx->last_rate_waits++;
    const StreamStatus st = read_status(ctx->h_stat);
    size_t packed = 0; // (two independent walks over the same coefficients: cannot differ, in error or length)
    if (st.err || stream_result(ctx, st, len, false, &packed) != TIC_OK || packed != len)
        return set_err(ctx, TIC_E_HIP, "the packed stream (%llu bits, error %d) contradicts its probe (%zu bytes)", st.bits, st.err, len);
    *out_len = len;
    *quality = q;
    return TIC_OK;
}

static int compress_to_size_impl(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, size_t max_bytes, int qmin, int qmax,
                                 void *out, bool out_on_host, size_t cap, size_t *out_len, int *quality) {
    const size_t n = num_blocks(h, w);
    ctx->last_rate_probes = ctx->last_rate_waits = 0;
    if (n == 0) { // a header at every quality: the bisection ends at qmax
        if (max_bytes < 16) {
            *out_len = 16;
            return set_err(ctx, TIC_E_SPACE, "16 bytes at quality %d exceed the budget of %zu", qmin, max_bytes);
        }
        if (out_on_host) {
            write_header((uint8_t *)out, h, w, qmax);
        } else {
            const int rc = put_header_only(ctx, out, h, w, qmax, false);
            if (rc) return rc;
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
        *out_len = 16;
        *quality = qmax;
        return TIC_OK;
    }
    int rc = ensure_rate(ctx, 8);
    if (rc) return rc;
    RateSearch rs;
    rate_search_begin(rs, qmin, qmax, (unsigned long long)max_bytes);
    int cand[kRateMaxCandidates];
    while (const int nc = rate_search_round(rs, single_frame_depth(n), cand)) {
        rc = queue_probes(ctx, d_image, h, w, row_stride, n, cand, nc);
        if (rc) return rc;
        HIPCHK(ctx, wait_stream(ctx));
        ctx->last_rate_probes += nc;
        ctx->last_rate_waits++;
        for (int i = 0; i < nc; i++) rs.known[cand[i]] = probe_size(ctx->h_rate[i]);
        rate_search_replay(rs);
    }
    if (rs.state == kRateNoCode) return set_err(ctx, TIC_E_RANGE, "coefficient without a Huffman code at quality %d (reference raises KeyError)", qmin);
    if (rs.state == kRateTooLarge) {
        *out_len = (size_t)rs.known[qmin];
        return set_err(ctx, TIC_E_SPACE, "%lld bytes at quality %d exceed the budget of %zu", rs.known[qmin], qmin, max_bytes);
    }
    return chosen_stream(ctx, d_image, h, w, row_stride, n, rs.lo, (size_t)rs.known[rs.lo], out, out_on_host, cap, out_len, quality);
}

static int check_search_args(tic_ctx *ctx, int h, int w, ptrdiff_t row_stride, int qmin, int qmax, const void *out, size_t cap, size_t *out_len,
                             int *quality) {
    if (!ctx || !out_len || !quality) return TIC_E_ARG;
    if (qmin < 1 || qmax > 99 || qmin > qmax) return set_err(ctx, TIC_E_QUALITY, "quality range %d..%d is not inside 1..99", qmin, qmax);
    const int rc = check_geometry(ctx, h, w, row_stride, qmin);
    if (rc) return rc;
    if (!out || cap < 16) return set_err(ctx, TIC_E_SPACE, "output buffer too small");
    return TIC_OK;
}

int tic_compress_to_size_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, size_t max_bytes, int qmin, int qmax,
                             void *d_out, size_t cap, size_t *out_len, int *quality) {
    TIC_LOCK(ctx);
    int rc = check_search_args(ctx, h, w, row_stride, qmin, qmax, d_out, cap, out_len, quality);
    if (rc) return rc;
    const size_t n = num_blocks(h, w);
    if (n && !d_image) return set_err(ctx, TIC_E_ARG, "null image pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rc = ensure_scratch(ctx, 0, n * 128 + 16);
    if (rc) return rc;
    return compress_to_size_impl(ctx, d_image, h, w, row_stride, max_bytes, qmin, qmax, d_out, false, cap, out_len, quality);
}

int tic_compress_to_size(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, size_t max_bytes, int qmin, int qmax,
                         uint8_t *out, size_t cap, size_t *out_len, int *quality) {
    TIC_LOCK(ctx);
    int rc = check_search_args(ctx, h, w, row_stride, qmin, qmax, out, cap, out_len, quality);
    if (rc) return rc;
    const size_t n = num_blocks(h, w);
    if (n == 0) return compress_to_size_impl(ctx, nullptr, h, w, row_stride, max_bytes, qmin, qmax, out, true, cap, out_len, quality);
    if (!image) return set_err(ctx, TIC_E_ARG, "null image pointer");
    size_t pitch = 0;
    rc = upload_image(ctx, image, h, w, row_stride, n, &pitch);
    if (rc) return rc;
    return compress_to_size_impl(ctx, ctx->d_img, h, w, (ptrdiff_t)pitch, max_bytes, qmin, qmax, out, true, cap, out_len, quality);
}

int tic_last_rate_search(tic_ctx *ctx, int *probes, int *host_waits) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (probes) *probes = ctx->last_rate_probes;
    if (host_waits) *host_waits = ctx->last_rate_waits;
    return TIC_OK;
}

// ---- rate-distortion: the exact round-trip error without a stream or a decoded frame ------------------------------------------
// The decoder reproduces the reference's pixels bit for bit, so the squared error between a frame and decompress(compress(frame, q)) is
// an integer that depends on the quantised coefficients and the frame alone.  The measuring kernel (idct_sse_kernel: idct_kernel's
// arithmetic, an epilogue that compares instead of storing) sums it from what a rate probe leaves resident.
static int check_distortion_args(tic_ctx *ctx, int h, int w, ptrdiff_t row_stride, int quality, int scaled_exp, const void *sums) {
    if (!ctx || !sums) return TIC_E_ARG;
    if (h < 0 || w < 0) return set_err(ctx, TIC_E_ARG, "negative image size %dx%d", h, w);
    if (scaled_exp < 0 && (quality < 1 || quality > 99) && !(quality == TIC_QUALITY_CUSTOM && ctx->custom_quality != 0.0))
        return set_err(ctx, TIC_E_QUALITY, "quality %d outside 1..99", quality);
    if (scaled_exp > 62) return set_err(ctx, TIC_E_QUALITY, "scaled_dct exponent %d outside 0..62", scaled_exp);
    if (h > 0 && w > 0 && row_stride < (ptrdiff_t)w) return set_err(ctx, TIC_E_ARG, "row stride %td < width %d", row_stride, w);
    return TIC_OK;
}

// Clears result 0 of the context's rate buffer and queues the measuring kernel adding into it; read_distortion brings it back.
static int queue_distortion(tic_ctx *ctx, const void *d_coeffs_zz, const void *d_image, int h, int w, ptrdiff_t row_stride, int quality,
                            int scaled_exp, IdctArgs *ia, SseArgs *m) {
    const int rc = ensure_rate(ctx, 1);
    if (rc) return rc;
    measure_args(ctx, d_coeffs_zz, d_image, h, w, row_stride, quality, scaled_exp, dist_of(ctx->d_rate, 1), ia, m);
    HIPCHK(ctx, hipMemsetAsync(m->res, 0, sizeof(DistortionResult), ctx->stream));
    return TIC_OK;
}

static int read_distortion(tic_ctx *ctx, uint64_t sums[2]) {
    DistortionResult *h_res = dist_of(ctx->h_rate, 1);
    HIPCHK(ctx, hipMemcpyAsync(h_res, dist_of(ctx->d_rate, 1), sizeof(DistortionResult), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, wait_stream(ctx));
    sums[0] = h_res->sse;
    sums[1] = h_res->sse_wrapped;
    return TIC_OK;
}

int tic_distortion_dev(tic_ctx *ctx, const void *d_coeffs_zz, const void *d_image, int h, int w, ptrdiff_t row_stride, int quality,
                       int scaled_exponent, uint64_t sums[2]) {
    TIC_LOCK(ctx);
    int rc = check_distortion_args(ctx, h, w, row_stride, quality, scaled_exponent, sums);
    if (rc) return rc;
    sums[0] = sums[1] = 0;
    if (num_blocks(h, w) == 0) return TIC_OK;
    if (!d_coeffs_zz || !d_image) return set_err(ctx, TIC_E_ARG, "null device pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    IdctArgs ia;
    SseArgs m;
    rc = queue_distortion(ctx, d_coeffs_zz, d_image, h, w, row_stride, quality, scaled_exponent, &ia, &m);
    if (rc) return rc;
    HIPCHK(ctx, launch_idct_sse(ia, m, ctx->stream));
    return read_distortion(ctx, sums);
}

// Times `iters` back-to-back launches of the measuring kernel on resident coefficients, behind `warm` untimed ones (timed_launches).
int tic_distortion_dev_timed(tic_ctx *ctx, const void *d_coeffs_zz, const void *d_image, int h, int w, ptrdiff_t row_stride, int quality,
                             int scaled_exponent, int warm, int iters, float *ms_total) {
    TIC_LOCK(ctx);
    int rc = check_distortion_args(ctx, h, w, row_stride, quality, scaled_exponent, ms_total);
    if (rc) return rc;
    if (warm < 0 || iters <= 0) return set_err(ctx, TIC_E_ARG, "bad argument");
    if (num_blocks(h, w) && (!d_coeffs_zz || !d_image)) return set_err(ctx, TIC_E_ARG, "null device pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    IdctArgs ia;
    SseArgs m;
    rc = queue_distortion(ctx, d_coeffs_zz, d_image, h, w, row_stride, quality, scaled_exponent, &ia, &m);
    if (rc) return rc;
    return timed_launches(ctx, warm, iters, ms_total, nullptr, [&](int, hipEvent_t, hipEvent_t) { return launch_idct_sse(ia, m, ctx->stream); });
}

// Times idct_kernel alone on resident coefficients, writing pixels to d_out: the launch the measuring kernel is to be compared with.
int tic_idct_dev_timed(tic_ctx *ctx, const void *d_coeffs_zz, void *d_out, int h, int w, ptrdiff_t out_stride, int quality, int scaled_exponent,
                       int warm, int iters, float *ms_total) {
    TIC_LOCK(ctx);
    int rc = check_distortion_args(ctx, h, w, out_stride, quality, scaled_exponent, ms_total);
    if (rc) return rc;
    if (warm < 0 || iters <= 0) return set_err(ctx, TIC_E_ARG, "bad argument");
    if (num_blocks(h, w) && (!d_coeffs_zz || !d_out)) return set_err(ctx, TIC_E_ARG, "null device pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    IdctArgs ia;
    SseArgs m;
    measure_args(ctx, d_coeffs_zz, d_out, h, w, out_stride, quality, scaled_exponent, nullptr, &ia, &m);
    ia.out = (uint8_t *)d_out;
    ia.stride = (long)out_stride;
    ia.aligned8 = m.aligned8;
    return timed_launches(ctx, warm, iters, ms_total, nullptr, [&](int, hipEvent_t, hipEvent_t) { return launch_idct(ia, ctx->stream); });
}

static int check_rd_args(tic_ctx *ctx, int h, int w, ptrdiff_t row_stride, const int *qualities, int nq, long long *sizes, const uint64_t *sse,
                         const uint64_t *sse_wrapped) {
    if (ctx && nq > 0 && (!sse || !sse_wrapped)) return set_err(ctx, TIC_E_ARG, "null result pointer");
    return check_size_args(ctx, h, w, row_stride, qualities, nq, sizes);
}

int tic_rd_points_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, const int *qualities, int nq, long long *sizes,
                      uint64_t *sse, uint64_t *sse_wrapped) {
    TIC_LOCK(ctx);
    int rc = check_rd_args(ctx, h, w, row_stride, qualities, nq, sizes, sse, sse_wrapped); // (a bad quality fails here: nothing has been queued)
    if (rc || nq == 0) return rc;
    const size_t n = num_blocks(h, w);
    if (n == 0) { // header only (codec.py:151): no pixel, no error
        for (int i = 0; i < nq; i++) {
            sizes[i] = 16;
            sse[i] = sse_wrapped[i] = 0;
        }
        return TIC_OK;
    }
    if (!d_image) return set_err(ctx, TIC_E_ARG, "null image pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rc = ensure_scratch(ctx, 0, n * 128 + 16);
    if (rc) return rc;
    rc = ensure_rate(ctx, (size_t)nq);
    if (rc) return rc;
    rc = queue_probes(ctx, d_image, h, w, row_stride, n, qualities, nq, true);
    if (rc) return rc;
    HIPCHK(ctx, wait_stream(ctx));
    const DistortionResult *d = dist_of(ctx->h_rate, nq);
    for (int i = 0; i < nq; i++) {
        sizes[i] = probe_size(ctx->h_rate[i]);
        sse[i] = d[i].sse;
        sse_wrapped[i] = d[i].sse_wrapped;
    }
    return TIC_OK;
}

int tic_rd_points(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, const int *qualities, int nq, long long *sizes,
                  uint64_t *sse, uint64_t *sse_wrapped) {
    TIC_LOCK(ctx);
    int rc = check_rd_args(ctx, h, w, row_stride, qualities, nq, sizes, sse, sse_wrapped);
    if (rc || nq == 0) return rc;
    const size_t n = num_blocks(h, w);
    if (n == 0) return tic_rd_points_dev(ctx, nullptr, h, w, row_stride, qualities, nq, sizes, sse, sse_wrapped);
    if (!image) return set_err(ctx, TIC_E_ARG, "null image pointer");
    size_t pitch = 0;
    rc = upload_image(ctx, image, h, w, row_stride, n, &pitch);
    if (rc) return rc;
    return tic_rd_points_dev(ctx, ctx->d_img, h, w, (ptrdiff_t)pitch, qualities, nq, sizes, sse, sse_wrapped);
}

// The search by distortion: the mirror of compress_to_size_impl.  Contract (header, tic_compress_to_psnr_dev):
// bisect downwards to the smallest quality that meets the bound, behind a first test of qmax - as PsnrSearch (tic_rd_plan.h, shared with the
// batch form) runs it; the depth of the look-ahead per frame size is the size search's.

static int compress_to_psnr_impl(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, uint64_t max_sse, int qmin, int qmax,
                                 void *out, bool out_on_host, size_t cap, size_t *out_len, int *quality, uint64_t *sse) {
    const size_t n = num_blocks(h, w);
    ctx->last_rate_probes = ctx->last_rate_waits = 0;
    if (n == 0) { // a header and no error at every quality: the bisection ends at qmin
        if (out_on_host) {
            write_header((uint8_t *)out, h, w, qmin);
        } else {
            const int rc = put_header_only(ctx, out, h, w, qmin, false);
            if (rc) return rc;
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
        *out_len = 16;
        *quality = qmin;
        *sse = 0;
        return TIC_OK;
    }
    int rc = ensure_rate(ctx, 8);
    if (rc) return rc;
    PsnrSearch ps;
    psnr_search_begin(ps, qmin, qmax, max_sse);
    int cand[kRateMaxCandidates];
    while (const int nc = psnr_search_round(ps, single_frame_depth(n), cand)) {
        rc = queue_probes(ctx, d_image, h, w, row_stride, n, cand, nc, true);
        if (rc) return rc;
        HIPCHK(ctx, wait_stream(ctx));
        ctx->last_rate_probes += nc;
        ctx->last_rate_waits++;
        const DistortionResult *d = dist_of(ctx->h_rate, nc);
        for (int i = 0; i < nc; i++) {
            ps.known[cand[i]] = probe_size(ctx->h_rate[i]);
            ps.known_sse[cand[i]] = d[i].sse;
        }
        psnr_search_replay(ps);
    }
    if (ps.state != kPsnrMeets) {
        *quality = qmax;
        *sse = ps.known_sse[qmax];
        *out_len = 0; // (tells this TIC_E_SPACE from the one of a stream that does not fit cap, which reports its length)
        if (ps.state == kPsnrNoCode) return set_err(ctx, TIC_E_RANGE, "coefficient without a Huffman code at quality %d (reference raises KeyError)", qmax);
        return set_err(ctx, TIC_E_SPACE, "squared error %llu at quality %d exceeds the bound of %llu", (unsigned long long)ps.known_sse[qmax], qmax,
                       (unsigned long long)max_sse);
    }
    *sse = ps.known_sse[ps.lo];
    return chosen_stream(ctx, d_image, h, w, row_stride, n, ps.lo, (size_t)ps.known[ps.lo], out, out_on_host, cap, out_len, quality);
}

int tic_compress_to_psnr_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, uint64_t max_sse, int qmin, int qmax,
                             void *d_out, size_t cap, size_t *out_len, int *quality, uint64_t *sse) {
    TIC_LOCK(ctx);
    if (ctx && !sse) return TIC_E_ARG;
    int rc = check_search_args(ctx, h, w, row_stride, qmin, qmax, d_out, cap, out_len, quality);
    if (rc) return rc;
    const size_t n = num_blocks(h, w);
    if (n && !d_image) return set_err(ctx, TIC_E_ARG, "null image pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rc = ensure_scratch(ctx, 0, n * 128 + 16);
    if (rc) return rc;
    return compress_to_psnr_impl(ctx, d_image, h, w, row_stride, max_sse, qmin, qmax, d_out, false, cap, out_len, quality, sse);
}

int tic_compress_to_psnr(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, uint64_t max_sse, int qmin, int qmax,
                         uint8_t *out, size_t cap, size_t *out_len, int *quality, uint64_t *sse) {
    TIC_LOCK(ctx);
    if (ctx && !sse) return TIC_E_ARG;
    int rc = check_search_args(ctx, h, w, row_stride, qmin, qmax, out, cap, out_len, quality);
    if (rc) return rc;
    const size_t n = num_blocks(h, w);
    if (n == 0) return compress_to_psnr_impl(ctx, nullptr, h, w, row_stride, max_sse, qmin, qmax, out, true, cap, out_len, quality, sse);
    if (!image) return set_err(ctx, TIC_E_ARG, "null image pointer");
    size_t pitch = 0;
    rc = upload_image(ctx, image, h, w, row_stride, n, &pitch);
    if (rc) return rc;
    return compress_to_psnr_impl(ctx, ctx->d_img, h, w, (ptrdiff_t)pitch, max_sse, qmin, qmax, out, true, cap, out_len, quality, sse);
}

// ---- the reference's integer encoder (c/img.c, c/encode.c): scaled-DCT streams ------------------------------------------------
// Transform stage: fdctq_scaled_kernel (tic_scaled.hip).  Entropy stage: the packers and the host coder above with the stream's own
// header and end (flag 1 << 30, setting 0..3, BB_flushBits' byte).
static int check_scaled_geometry(tic_ctx *ctx, int h, int w, ptrdiff_t stride, int qf) {
    if (!ctx) return TIC_E_ARG;
    if (h < 0 || w < 0) return set_err(ctx, TIC_E_ARG, "negative image size %dx%d", h, w);
    if ((h & 7) != 0 || (w & 7) != 0) return set_err(ctx, TIC_E_ARG, "the scaled-DCT encoder takes heights and widths that are multiples of 8 (encode.c:37), not %dx%d", h, w);
    if (qf < 0 || qf > 3) return set_err(ctx, TIC_E_QUALITY, "scaled-DCT setting %d outside 0..3 (best, high, med, low)", qf);
    if (h > 0 && w > 0 && stride < (ptrdiff_t)w) return set_err(ctx, TIC_E_ARG, "row stride %td < width %d", stride, w);
    return TIC_OK;
}

static ScaledArgs make_scaled_args(const void *d_image, int h, int w, ptrdiff_t stride, int qf, void *d_out) {
    ScaledArgs a;
    a.img = (const uint8_t *)d_image;
    a.out = (int16_t *)d_out;
    a.stride = (long)stride;
    a.bw = w / 8;
    a.tiles_x = (a.bw + 7) / 8;
    a.ntiles = (h / 8) * a.tiles_x;
    a.qf = qf;
    a.aligned8 = ((((uintptr_t)d_image) | (uintptr_t)stride) & 7) == 0;
    a.nframes = 1;
    a.frame_stride_in = 0;
    a.frame_stride_out = 0;
    return a;
}

size_t tic_compress_scaled_bound(int h, int w) { return compress_bound(h, w) + 1; }

int tic_dctq_scaled_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, int qf, void *d_coeffs_zz) {
    TIC_LOCK(ctx);
    int rc = check_scaled_geometry(ctx, h, w, row_stride, qf);
    if (rc) return rc;
    if (h == 0 || w == 0) return TIC_OK;
    if (!d_image || !d_coeffs_zz) return set_err(ctx, TIC_E_ARG, "null device pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, launch_fdctq_scaled(make_scaled_args(d_image, h, w, row_stride, qf, d_coeffs_zz), ctx->stream));
    return TIC_OK;
}

int tic_dctq_scaled_dev_frames(tic_ctx *ctx, const void *d_images, int nframes, int h, int w, ptrdiff_t row_stride, ptrdiff_t frame_stride,
                               int qf, void *d_coeffs_zz, ptrdiff_t coeff_frame_stride) {
    TIC_LOCK(ctx);
    int rc = check_scaled_geometry(ctx, h, w, row_stride, qf);
    if (rc) return rc;
    if (nframes < 0) return set_err(ctx, TIC_E_ARG, "negative frame count");
    if (h == 0 || w == 0 || nframes == 0) return TIC_OK;
    if (!d_images || !d_coeffs_zz) return set_err(ctx, TIC_E_ARG, "null device pointer");
    ScaledArgs a = make_scaled_args(d_images, h, w, row_stride, qf, d_coeffs_zz);
    rc = set_frames(ctx, a, nframes, h, w, row_stride, frame_stride, coeff_frame_stride);
    if (rc) return rc;
    if ((coeff_frame_stride & 15) != 0) return set_err(ctx, TIC_E_ARG, "coefficient frame stride must be a multiple of 16");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, launch_fdctq_scaled(a, ctx->stream));
    return TIC_OK;
}

// tic_dctq_dev_timed_warm for the integer kernel: the same submission and the same per-launch stamps (timed_launches), so that the two
// figures compare.
int tic_dctq_scaled_dev_timed_warm(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, int qf, void *d_coeffs_zz, int warm,
                                   int iters, float *ms_total, float *per_launch_ms) {
    TIC_LOCK(ctx);
    int rc = check_scaled_geometry(ctx, h, w, row_stride, qf);
    if (rc) return rc;
    if (!ms_total || iters < 1 || warm < 0 || !d_image || !d_coeffs_zz || h == 0 || w == 0) return set_err(ctx, TIC_E_ARG, "bad argument");
    if (per_launch_ms && iters > 32768) return set_err(ctx, TIC_E_ARG, "per-launch times for at most 32768 launches");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const ScaledArgs a = make_scaled_args(d_image, h, w, row_stride, qf, d_coeffs_zz);
    return timed_launches(ctx, warm, iters, ms_total, per_launch_ms,
                          [&](int, hipEvent_t e0, hipEvent_t e1) { return launch_fdctq_scaled(a, ctx->stream, e0, e1); });
}

int tic_dctq_scaled(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, int qf, int16_t *coeffs_zz) {
    TIC_LOCK(ctx);
    int rc = check_scaled_geometry(ctx, h, w, row_stride, qf);
    if (rc) return rc;
    const size_t n = num_blocks(h, w);
    if (n == 0) return TIC_OK;
    if (!image || !coeffs_zz) return set_err(ctx, TIC_E_ARG, "null host pointer");
    size_t pitch = 0;
    rc = upload_image(ctx, image, h, w, row_stride, n, &pitch);
    if (rc) return rc;
    HIPCHK(ctx, launch_fdctq_scaled(make_scaled_args(ctx->d_img, h, w, (ptrdiff_t)pitch, qf, ctx->d_coef), ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(coeffs_zz, ctx->d_coef, n * 128, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TIC_OK;
}

// The distortion column of the reference's tests/cbenchmark.py: the integer encoder's coefficients through the measuring kernel at the
// exponent the stream's header would carry (the setting's index).
int tic_roundtrip_sse_scaled(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, int qf, uint64_t sums[2]) {
    TIC_LOCK(ctx);
    int rc = check_scaled_geometry(ctx, h, w, row_stride, qf);
    if (rc) return rc;
    if (!sums) return set_err(ctx, TIC_E_ARG, "null result pointer");
    sums[0] = sums[1] = 0;
    const size_t n = num_blocks(h, w);
    if (n == 0) return TIC_OK;
    if (!image) return set_err(ctx, TIC_E_ARG, "null image pointer");
    size_t pitch = 0;
    rc = upload_image(ctx, image, h, w, row_stride, n, &pitch);
    if (rc) return rc;
    HIPCHK(ctx, launch_fdctq_scaled(make_scaled_args(ctx->d_img, h, w, (ptrdiff_t)pitch, qf, ctx->d_coef), ctx->stream));
    IdctArgs ia;
    SseArgs m;
    rc = queue_distortion(ctx, ctx->d_coef, ctx->d_img, h, w, (ptrdiff_t)pitch, 50, qf, &ia, &m);
    if (rc) return rc;
    HIPCHK(ctx, launch_idct_sse(ia, m, ctx->stream));
    return read_distortion(ctx, sums);
}

int tic_entropy_encode_scaled(const int16_t *coeffs_zz, int h, int w, int qf, uint8_t *out, size_t cap, size_t *out_len) {
    return entropy_encode_scaled(coeffs_zz, h, w, qf, out, cap, out_len);
}

// A buffer of at least tic_compress_scaled_bound() bytes receives the stream from the placing kernel itself.  A smaller one is never
// handed to that kernel: the stream is placed in the context's own buffer and copied over only when it fits, so that TIC_E_SPACE leaves
// the caller's buffer untouched and a stream that fits is written to its last byte and no further.
int tic_compress_scaled_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, int qf, void *d_out, size_t cap,
                            size_t *out_len) {
    TIC_LOCK(ctx);
    int rc = check_scaled_geometry(ctx, h, w, row_stride, qf);
    if (rc) return rc;
    if (!out_len) return set_err(ctx, TIC_E_ARG, "null length pointer");
    if (!d_out || cap < 17) return set_err(ctx, TIC_E_SPACE, "output buffer too small");
    const size_t n = num_blocks(h, w);
    if (n && !d_image) return set_err(ctx, TIC_E_ARG, "null image pointer");
    rc = ensure_scratch(ctx, 0, n * 128 + 16);
    if (rc) return rc;
    rc = tic_dctq_scaled_dev(ctx, d_image, h, w, row_stride, qf, ctx->d_coef);
    if (rc) return rc;
    const size_t bound = tic_compress_scaled_bound(h, w);
    if (cap >= bound || n == 0) return entropy_encode_dev_impl(ctx, ctx->d_coef, h, w, qf, d_out, cap, out_len, true);
    rc = ctx->d_stream_buf.grow(ctx, bound);
    if (rc) return rc;
    size_t len = 0;
    rc = entropy_encode_dev_impl(ctx, ctx->d_coef, h, w, qf, ctx->d_stream_buf, ctx->d_stream_buf.cap, &len, true);
    if (rc) return rc;
    if (len > cap) return set_err(ctx, TIC_E_SPACE, "output buffer too small (%zu bytes needed, %zu given)", len, cap);
    HIPCHK(ctx, hipMemcpyAsync(d_out, ctx->d_stream_buf, len, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *out_len = len;
    return TIC_OK;
}

int tic_compress_scaled(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, int qf, uint8_t *out, size_t cap,
                        size_t *out_len) {
    TIC_LOCK(ctx);
    int rc = check_scaled_geometry(ctx, h, w, row_stride, qf);
    if (rc) return rc;
    if (!out || !out_len) return set_err(ctx, TIC_E_ARG, "null output pointer");
    const size_t n = num_blocks(h, w);
    if (n == 0) return entropy_encode_scaled(nullptr, h, w, qf, out, cap, out_len);
    if (!image) return set_err(ctx, TIC_E_ARG, "null image pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rc = ctx->d_stream_buf.grow(ctx, tic_compress_scaled_bound(h, w));
    if (rc) return rc;
    size_t pitch = 0, len = 0;
    rc = upload_image(ctx, image, h, w, row_stride, n, &pitch);
    if (rc) return rc;
    rc = tic_compress_scaled_dev(ctx, ctx->d_img, h, w, (ptrdiff_t)pitch, qf, ctx->d_stream_buf, ctx->d_stream_buf.cap, &len);
    if (rc) return rc;
    if (len > cap) return set_err(ctx, TIC_E_SPACE, "output buffer too small (%zu bytes needed, %zu given)", len, cap);
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->d_stream_buf, len, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *out_len = len;
    return TIC_OK;
}

// ---- batch pipeline (BASELINE config 3) -------------------------------------------------------------------
// Frames travel in chunks (chunk_frames): per chunk one H2D copy - from where the caller's frames lie when they are pinned, else out of the
// slot's pinned staging buffer - and ONE transform launch, on two streams in turn so that the copy of chunk c + 1 overlaps the kernels of
// chunk c.  Two pipelines share that front: tic_compress_batch with threads > 0 and tic_dctq_batch bring the coefficients back and code
// them on host worker threads (batch_host_coder); tic_compress_batch with threads <= 0 runs the entropy stage on the device and brings
// back finished streams (batch_device_entropy).  What they share is written once:
//   batch_begin     checks, frames without blocks, the plan (BatchPlan), the slots, the call's figures, the batch-wide registration
//   enqueue_chunk   upload + transform + what the pipeline adds on the chunk's stream + the chunk's `done` event
//   batch_end       joins the pipeline's threads, drains the streams, releases the call's registrations and the slots
//   SlotGate        which slot is free (Slot::pending), and the first error a pipeline thread met
//   ClosableQueue, run_strided, the decisions about the caller's memory: tic_host_pipeline.h

// The slots a context keeps, a chunk in each: one is being staged and uploaded, one is on the device, one has its results read back, one
// is handed out to the caller (the host coder's pipeline: coded by the workers).  Chunk c takes slot c % kBatchSlots once that is free.
constexpr int kBatchSlots = 4;

// (row pitch of staged frames: batch_pitch, tic_host_pipeline.h)

// What a batch call works out once: blocks per frame, the staged row pitch, bytes of a frame's pixels and coefficients, the distance of two
// streams in a slot, frames per chunk (0: the call had nothing to put through the pipeline).
struct BatchPlan {
    size_t nblk = 0, pitch = 0, img_bytes = 0, coef_bytes = 0, bound = 0;
    int chunk = 0;
};

// h rows of w bytes from one pitch to another: one memcpy when both sides are dense.
static void copy_rows(uint8_t *dst, size_t pitch, const uint8_t *src, ptrdiff_t row_stride, int h, int w) {
    if ((size_t)row_stride == pitch && pitch == (size_t)w) {
        memcpy(dst, src, (size_t)h * (size_t)w);
        return;
    }
    for (int y = 0; y < h; y++) memcpy(dst + (size_t)y * pitch, src + (ptrdiff_t)y * row_stride, (size_t)w);
}

// Stages the frames of a chunk into the slot's pinned buffer on several threads: one thread copies ~10 GB/s, which
// would cap a 1080p batch at ~5,000 frames/s - below what PCIe and the GPU take.
static void stage_chunk(const tic_ctx *ctx, uint8_t *pin, size_t img_bytes, size_t pitch, const uint8_t *const *images, int first, int cnt,
                        ptrdiff_t row_stride, int h, int w) {
    unsigned hw = std::thread::hardware_concurrency();
    int T = ctx->stage_threads > 0 ? ctx->stage_threads : (int)(hw ? hw / 2 : 4);
    T = T < 1 ? 1 : (T > 8 ? 8 : T);
    if (T > cnt) T = cnt;
    if (img_bytes * (size_t)cnt < (4u << 20)) T = 1;
    run_strided(cnt, T, [ctx]() { bind_pipeline_thread(ctx); },
                [=](int k) { copy_rows(pin + (size_t)k * img_bytes, pitch, images[first + k], row_stride, h, w); });
}

static bool host_pointer_is_pinned(const void *p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError(); // (plain malloc'ed memory: "invalid value", not an error of ours)
        return false;
    }
    return at.type == hipMemoryTypeHost;
}
// Pins [p, p + bytes), widened to whole pages, where it lies.  Returns the registered base for hipHostUnregister, or null when the runtime
// refuses (memory of another kind, part of the range registered already): not an error of ours, the caller takes its other route.
static void *pin_range(const void *p, size_t bytes) {
    const uintptr_t lo = page_floor((uintptr_t)p), hi = page_ceil((uintptr_t)p + bytes);
    if (hipHostRegister((void *)lo, hi - lo, hipHostRegisterDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return (void *)lo;
}
// Pageable input.  Copying 2 MB frames into the pinned slots costs the host 2 x the batch in DRAM traffic and eight copy threads,
// and it is what makes the host -> host rate depend on the box: 12.3 ms for 256 x 1080p on a quiet host, 18-22 ms when the copy
// threads compete with other tenants or sit on the wrong side of the socket link (profiles/r04_numa_probe.txt), while frames the
// DMA engine reads where they lie take 12.7-13.5 ms everywhere.  hipHostRegister is cheap PER CALL, not per byte - 0.03 ms for a
// chunk's 36 MB, 0.18 ms for 510 MB, the pages are validated when the copy engine first touches them - but 77 us per call: one by
// one, 256 frames cost 19.7 ms.  So the frames [first, first + cnt) are registered as ONE range, from the lowest to the highest
// address, when that range is dense enough to be mostly frames (range_is_mostly_frames) - for the whole batch if possible, else chunk
// by chunk.  Anything that cannot be registered this way (a range with a hole, memory of another kind, part of it registered by the
// caller already) is staged.  Returns true if the frames are now pinned.
static bool auto_register_frames(tic_ctx *ctx, const uint8_t *const *images, int first, int cnt, size_t img_bytes) {
    if (!ctx->auto_register || cnt < 1 || img_bytes < (256u << 10)) return false;
    // (a range over frames of which some are pinned already would overlap the caller's own registration: such a set is left alone)
    for (int k = 0; k < cnt; k++)
        if (host_pointer_is_pinned(images[first + k]) || host_pointer_is_pinned(images[first + k] + img_bytes - 1)) return false;
    uintptr_t lo = UINTPTR_MAX, hi = 0;
    for (int k = 0; k < cnt; k++) {
        const uintptr_t p = (uintptr_t)images[first + k];
        if (!p) return false;
        lo = p < lo ? p : lo;
        hi = p + img_bytes > hi ? p + img_bytes : hi;
    }
    if (!range_is_mostly_frames(lo, hi, img_bytes, (size_t)cnt)) return false;
    void *reg = pin_range((const void *)lo, hi - lo);
    if (!reg) return false;
    ctx->autoregs.push_back(reg);
    ctx->last_batch_autoreg_frames += cnt;
    return true;
}
static void auto_unregister_all(tic_ctx *ctx) { // (after the call's last copy has completed)
    for (void *r : ctx->autoregs) {
        if (hipHostUnregister(r) != hipSuccess) (void)hipGetLastError();
    }
    ctx->autoregs.clear();
}

// Host -> device copy of a chunk.  Frames the caller holds in pinned or registered memory, rows back to back, go to the device from
// where they lie (one copy for the chunk when the frames follow each other in memory, else one per frame); anything else is staged
// into the slot's pinned buffer first (pageable memory: the runtime would stage it too, synchronously and through a small bounce
// buffer).  *direct: the number of frames that took the direct path.
static hipError_t upload_chunk(tic_ctx *ctx, Slot &s, size_t img_bytes, size_t pitch, const uint8_t *const *images, int first, int cnt,
                               ptrdiff_t row_stride, int h, int w, hipStream_t st, int *direct) {
    *direct = 0;
    const bool dense = (size_t)row_stride == pitch && pitch == (size_t)w; // the device layout IS the caller's layout
    bool pinned = dense;
    for (int k = 0; k < cnt && pinned; k++)
        pinned = host_pointer_is_pinned(images[first + k]) && host_pointer_is_pinned(images[first + k] + img_bytes - 1);
    if (!pinned && dense) {
        // a chunk of pageable frames (chunk by chunk: the whole batch was tried at the call's start)
        BT_START();
        pinned = auto_register_frames(ctx, images, first, cnt, img_bytes);
        BT_STOP(0);
    }
    if (pinned) {
        // from where the frames lie: one copy for the chunk when they follow each other in memory, else one per frame.  A copy the
        // runtime refuses (frames of one chunk in two separately registered ranges make a chunk-wide copy invalid) falls back to
        // one copy per frame, and that to the staged route below - the device buffer is simply written again, in stream order
        bool contiguous = true;
        for (int k = 1; k < cnt && contiguous; k++) contiguous = images[first + k] == images[first] + (size_t)k * img_bytes;
        hipError_t e = contiguous ? hipMemcpyAsync(s.d_img, images[first], img_bytes * cnt, hipMemcpyHostToDevice, st) : hipErrorInvalidValue;
        if (e != hipSuccess) {
            (void)hipGetLastError();
            e = hipSuccess;
            for (int k = 0; k < cnt && e == hipSuccess; k++)
                e = hipMemcpyAsync((char *)s.d_img + (size_t)k * img_bytes, images[first + k], img_bytes, hipMemcpyHostToDevice, st);
        }
        if (e == hipSuccess) {
            *direct = cnt;
            return hipSuccess;
        }
        (void)hipGetLastError();
    }
    BT_START();
    stage_chunk(ctx, s.pin_in, img_bytes, pitch, images, first, cnt, row_stride, h, w);
    BT_STOP(0);
    return hipMemcpyAsync(s.d_img, s.pin_in, img_bytes * cnt, hipMemcpyHostToDevice, st);
}

// The context's slots hold at least `need` (sizes in bytes and a frame count: frames of one size and mixed frames share them).  They grow
// to the larger of what they held and what is asked for, so that calls of different shapes in turn do not allocate in turn.
static int ensure_batch_slots(tic_ctx *ctx, tic_ctx::SlotNeed need) {
    if ((int)ctx->bslots.size() == kBatchSlots && ctx->bslot_cap.covers(need)) return TIC_OK;
    const tic_ctx::SlotNeed &old = ctx->bslot_cap;
    need.img = std::max(need.img, old.img), need.coef = std::max(need.coef, old.coef), need.pin_out = std::max(need.pin_out, old.pin_out);
    need.streams = std::max(need.streams, old.streams), need.work = std::max(need.work, old.work), need.frames = std::max(need.frames, old.frames);
    for (auto &sl : ctx->bslots) sl.release(ctx);
    ctx->bslots.clear();
    ctx->bslots.resize(kBatchSlots);
    ctx->bslot_cap = tic_ctx::SlotNeed();
    const size_t nf = (size_t)need.frames;
    for (auto &sl : ctx->bslots) {
        HIPCHK(ctx, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
        HIPCHK(ctx, hipEventCreateWithFlags(&sl.rb_done, hipEventDisableTiming));
        int rc;
        if ((rc = sl.pin_in.grow(ctx, need.img)) || (rc = sl.pin_out.grow(ctx, need.pin_out)) || (rc = sl.d_img.grow(ctx, need.img)) ||
            (rc = sl.d_coef.grow(ctx, need.coef)) || (rc = sl.d_work.grow(ctx, need.work)) || (rc = sl.d_lens.grow(ctx, nf * sizeof(unsigned long long))) ||
            (rc = sl.h_lens.grow(ctx, nf * sizeof(unsigned long long))) || (rc = sl.d_err.grow(ctx, 2 * sizeof(int))) ||
            (rc = sl.h_err.grow(ctx, sizeof(int))) || (rc = sl.d_streams.grow(ctx, need.streams)) ||
            (rc = sl.h_frames.grow(ctx, sizeof(EntropyFrameTable))) || (rc = sl.d_frames.grow(ctx, sizeof(EntropyFrameTable))) ||
            (rc = sl.h_rb_off.grow(ctx, kEntropyMaxFrames * sizeof(unsigned long long))) || (rc = sl.h_sframes.grow(ctx, sizeof(ScaledFrameTable))) ||
            (rc = sl.d_sframes.grow(ctx, sizeof(ScaledFrameTable))))
            return rc;
        HIPCHK(ctx, hipMemset(sl.d_err, 0, 2 * sizeof(int))); // (two flags used in turn, state: cleared here, and they stay clear)
    }
    ctx->bslot_cap = need;
    return TIC_OK;
}
// ... for `chunk` frames of h x w
static tic_ctx::SlotNeed uniform_slot_need(int h, int w, int chunk) {
    const size_t nblk = num_blocks(h, w);
    tic_ctx::SlotNeed need;
    need.img = batch_pitch(w) * (size_t)h * chunk;
    need.coef = need.pin_out = nblk * 128 * chunk;
    need.streams = align_up(compress_bound(h, w), 16) * (size_t)chunk;
    need.work = entropy_fused_work_bytes((nblk + 8) * (size_t)chunk); // (every frame's partitions are rounded up)
    need.frames = chunk;
    return need;
}

// The front end of both pipelines: argument checks (`device_entropy`: the stricter ones of the calls whose streams the device writes),
// frames without blocks (a header each, where streams are wanted), the plan, the slots, the call's figures, and the registration of the whole
// batch as one range, if it is one.  p->chunk == 0 on return: nothing is left to do - an error, n == 0, or frames without blocks.
static int batch_begin(tic_ctx *ctx, const uint8_t *const *images, int n, int h, int w, ptrdiff_t row_stride, int quality, bool want_streams,
                       bool device_entropy, uint8_t *const *outs, const size_t *caps, size_t *out_lens, BatchPlan *p) {
    *p = BatchPlan();
    int rc = device_entropy ? check_stream_geometry(ctx, h, w, row_stride, quality) : check_geometry(ctx, h, w, row_stride, quality);
    if (rc) return rc;
    if (n < 0 || (n > 0 && !images)) return set_err(ctx, TIC_E_ARG, "bad batch arguments");
    if (want_streams && n > 0 && (!outs || !caps || !out_lens)) return set_err(ctx, TIC_E_ARG, "null output arrays");
    if (n == 0) return TIC_OK;
    const size_t nblk = num_blocks(h, w);
    if (nblk == 0) {
        for (int i = 0; i < n && want_streams; i++) {
            int r = entropy_encode(nullptr, h, w, quality, outs[i], caps[i], &out_lens[i]);
            if (r) return r;
        }
        return TIC_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t pitch = batch_pitch(w), img_bytes = pitch * (size_t)h;
    const int chunk = chunk_frames(n, img_bytes);
    rc = ensure_batch_slots(ctx, uniform_slot_need(h, w, chunk));
    if (rc) return rc;
    for (auto &sl : ctx->bslots) sl.pending = 0;
    ctx->last_batch_direct_frames = ctx->last_batch_staged_frames = ctx->last_batch_autoreg_frames = ctx->last_batch_zero_copy = 0;
    ctx->bt = BatchTrace();
    if ((size_t)row_stride == pitch && pitch == (size_t)w) { // the whole batch as one range, if it is one
        BT_START();
        (void)auto_register_frames(ctx, images, 0, n, img_bytes);
        BT_STOP(0);
    }
    p->nblk = nblk, p->pitch = pitch, p->img_bytes = img_bytes, p->coef_bytes = nblk * 128, p->bound = align_up(compress_bound(h, w), 16);
    p->chunk = chunk;
    return TIC_OK;
}

// Which slot is free, and the first error one of a pipeline's threads met.  A chunk claims its slot for `units` pieces of work (the
// device entropy pipeline: 1, the chunk; the host coder's: its frames, one per worker job); whoever finishes the last piece frees it.
struct SlotGate {
    std::mutex mu;
    std::condition_variable cv;
    int err = TIC_OK;
    void claim(tic_ctx *ctx, Slot &s, int units) { // (tic_last_batch_phases [5]: the submitting thread's wait for a free slot)
        BT_START();
        std::unique_lock<std::mutex> l(mu);
        cv.wait(l, [&] { return s.pending == 0; });
        s.pending = units;
        BT_STOP(5);
    }
    void finish(Slot &s) {
        bool freed;
        {
            std::lock_guard<std::mutex> l(mu);
            freed = --s.pending == 0;
        }
        if (freed) cv.notify_all();
    }
    void fail(int rc) {
        std::lock_guard<std::mutex> l(mu);
        if (err == TIC_OK) err = rc;
    }
    int error() {
        std::lock_guard<std::mutex> l(mu);
        return err;
    }
};

// Enqueues frames [first, first + cnt) in slot `s` on stream `st`: the upload, ONE transform launch (a grid plane per frame, or one tall
// frame where merge_frames sees one), then `rest(s, st)` - what the pipeline wants on the stream behind the transform - and the slot's
// `done` event.
extern "C++" { // (templates inside the C-ABI block)
// The order of a chunk on its stream, for frames of one size and for mixed frames alike: upload(&direct) - *direct = frames that came from
// where the caller holds them - then transform(), rest(s, st), the slot's `done` event.  `first`, `cnt`: what the slot's consumers find in it.
template <class Upload, class Transform, class Rest>
static int enqueue_on_slot(tic_ctx *ctx, Slot &s, hipStream_t st, int first, int cnt, Upload upload, Transform transform, Rest rest) {
    s.first = first;
    s.count = cnt;
    int direct = 0;
    hipError_t e = upload(&direct);
    ctx->last_batch_direct_frames += direct;
    ctx->last_batch_staged_frames += cnt - direct;
    BT_START();
    if (e == hipSuccess) e = transform();
    if (e == hipSuccess) e = rest(s, st);
    if (e == hipSuccess) e = hipEventRecord(s.done, st);
    BT_STOP(1);
    if (e != hipSuccess) return set_err(ctx, TIC_E_HIP, "batch enqueue failed at frame %d: %s", first, hipGetErrorString(e));
    return TIC_OK;
}
template <class Rest>
static int enqueue_chunk(tic_ctx *ctx, const BatchPlan &p, Slot &s, hipStream_t st, const uint8_t *const *images, int first, int cnt,
                         ptrdiff_t row_stride, int h, int w, int quality, Rest rest) {
    DctqArgs a = make_args(ctx, s.d_img, h, w, (ptrdiff_t)p.pitch, quality, s.d_coef);
    a.fallback_count = nullptr;
    const int rc = set_frames(ctx, a, cnt, h, w, (ptrdiff_t)p.pitch, (ptrdiff_t)p.img_bytes, (ptrdiff_t)p.coef_bytes);
    if (rc) return rc;
    merge_frames(a);
    return enqueue_on_slot(
        ctx, s, st, first, cnt, [&](int *direct) { return upload_chunk(ctx, s, p.img_bytes, p.pitch, images, first, cnt, row_stride, h, w, st, direct); },
        [&]() { return launch_dctq(a, 2, st); }, rest);
}

// Read-back of a chunk's streams by the SHADER, not by a DMA engine: `row` pieces of V (16 or 8 bytes) of every row from device memory into
// device-accessible host memory.  The runtime spreads the batch's uploads over both SDMA engines and queues every later copy
// behind the uploads already submitted - with four chunks of uploads in the queue a chunk's read-back started 2 ms after its kernels
// had finished, the read-backs came in bursts of four, and the uploads stalled 0.5-0.7 ms behind every burst for want of a free slot
// (rocprofv3 --memory-copy-trace, profiles/r04_batch_timeline.txt).  Stores from a kernel cross the link in the other direction while
// the engines upload.
template <class V>
__global__ __launch_bounds__(256) void readback_rows_kernel(const V *__restrict__ src, size_t src_pitch, V *__restrict__ dst, size_t dst_pitch, size_t row) {
    const V *s = src + (size_t)blockIdx.y * src_pitch;
    V *d = dst + (size_t)blockIdx.y * dst_pitch;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < row; i += (size_t)gridDim.x * 256u) __builtin_nontemporal_store(s[i], d + i);
}
// `rows` rows of `row_bytes` (rounded up to whole pieces), the pitches in bytes (multiples of the piece)
template <class V>
static hipError_t launch_readback(const void *src, size_t src_pitch, void *dst, size_t dst_pitch, size_t row_bytes, int rows, hipStream_t st) {
    hipLaunchKernelGGL(readback_rows_kernel<V>, dim3(64, (unsigned)rows), dim3(256), 0, st, (const V *)src, src_pitch / sizeof(V), (V *)dst, dst_pitch / sizeof(V),
                       (row_bytes + sizeof(V) - 1) / sizeof(V));
    return hipGetLastError();
}
}
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2v __attribute__((ext_vector_type(2)));
// ... in descriptor form (mixed batches): frame blockIdx.y's stream - lens[y] bytes at the offset its record names, whole 16-byte pieces -
// to dst + dst_off[y].  Only the bytes a stream has cross the link, whatever the frames' sizes.
__global__ __launch_bounds__(256) void readback_frames_kernel(const unsigned char *__restrict__ src, const EntropyFrameTable *__restrict__ frames,
                                                              const unsigned long long *__restrict__ lens, const unsigned long long *__restrict__ dst_off,
                                                              unsigned char *__restrict__ dst) {
    const u32x4v *sp = reinterpret_cast<const u32x4v *>(src + frames->rec[blockIdx.y].out_off);
    u32x4v *dp = reinterpret_cast<u32x4v *>(dst + dst_off[blockIdx.y]);
    const size_t pieces = (size_t)((lens[blockIdx.y] + 15ull) / 16ull);
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < pieces; i += (size_t)gridDim.x * 256u) __builtin_nontemporal_store(sp[i], dp + i);
}

// The end of a batch call: the pipeline's threads (their queues are closed: each drains its own first), the streams, the frames pinned for
// the call - behind its last copy - and the slots.
static void batch_end(tic_ctx *ctx, std::vector<std::thread> &threads) {
    BT_START();
    for (auto &t : threads) t.join();
    (void)hipStreamSynchronize(ctx->bstream[0]);
    (void)hipStreamSynchronize(ctx->bstream[1]);
    (void)hipStreamSynchronize(ctx->rstream);
    BT_STOP(6); // (tic_last_batch_phases [6]: the caller's wait for the pipeline's threads and streams, [7]: releasing the frames pinned for the call)
    BT_START();
    auto_unregister_all(ctx);
    BT_STOP(7);
    for (auto &sl : ctx->bslots) sl.pending = 0;
}

// The host coder's pipeline (tic_compress_batch with threads > 0, tic_dctq_batch): the coefficients of a chunk come back into the slot's
// pinned buffer, `threads` workers entropy-code them frame by frame (and copy them out, where the caller wants them).
static int batch_host_coder(tic_ctx *ctx, const uint8_t *const *images, int n, int h, int w, ptrdiff_t row_stride, int quality,
                            int16_t *const *coeffs, uint8_t *const *outs, const size_t *caps, size_t *out_lens, int threads, bool want_entropy) {
    BatchPlan p;
    const int rc = batch_begin(ctx, images, n, h, w, row_stride, quality, want_entropy, false, outs, caps, out_lens, &p);
    if (rc || p.chunk == 0) return rc;
    std::vector<Slot> &slots = ctx->bslots;
    const bool need_d2h = want_entropy || coeffs != nullptr;
    SlotGate gate;
    ClosableQueue<std::pair<int, int>> jobs; // (slot, frame index inside the chunk)
    auto worker = [&]() {
        bind_pipeline_thread(ctx);
        (void)hipSetDevice(ctx->device);
        std::pair<int, int> job;
        while (jobs.pop(job)) {
            Slot &s = slots[job.first];
            const int f = s.first + job.second;
            int r = hipEventSynchronize(s.done) == hipSuccess ? TIC_OK : TIC_E_HIP;
            const int16_t *zz = need_d2h ? s.pin_out + (size_t)job.second * p.nblk * 64 : nullptr;
            if (r == TIC_OK && want_entropy) r = entropy_encode(zz, h, w, quality, outs[f], caps[f], &out_lens[f]);
            if (r == TIC_OK && coeffs && coeffs[f]) memcpy(coeffs[f], zz, p.coef_bytes);
            if (r != TIC_OK) gate.fail(r);
            gate.finish(s);
        }
    };
    const int nthreads = threads < 1 ? 1 : (threads > 64 ? 64 : threads);
    std::vector<std::thread> pool;
    for (int t = 0; t < nthreads; t++) pool.emplace_back(worker);

    int result = TIC_OK, c = 0;
    for (int first = 0; first < n; first += p.chunk, c++) {
        const int cnt = n - first < p.chunk ? n - first : p.chunk, si = c % kBatchSlots;
        Slot &s = slots[si];
        gate.claim(ctx, s, cnt);
        result = enqueue_chunk(ctx, p, s, ctx->bstream[c & 1], images, first, cnt, row_stride, h, w, quality, [&](Slot &sl, hipStream_t st) {
            return need_d2h ? hipMemcpyAsync(sl.pin_out, sl.d_coef, p.coef_bytes * cnt, hipMemcpyDeviceToHost, st) : hipSuccess;
        });
        if (result != TIC_OK) break;
        for (int k = 0; k < cnt; k++) jobs.push({si, k});
    }
    jobs.close();
    batch_end(ctx, pool);
    if (result == TIC_OK && gate.error() != TIC_OK) result = set_err(ctx, gate.error(), "batch consumer failed with code %d", gate.error());
    return result;
}

// The device entropy pipeline (tic_compress_batch with threads <= 0): per chunk one H2D copy, one transform launch, the entropy
// stage, then only the finished streams (and 8 bytes of length per frame) come back.
constexpr int kRetryEightLanes = -1000; // internal: batch_device_entropy asks tic_compress_batch for another run with the 8-lane packing kernel

// Zero copy, for a batch of one chunk (it runs on the calling thread, which owns the call's registrations): where the caller's buffers are
// rows of ONE block of memory (rows_of_one_block: a pool of n x cap bytes - what compress_batch() of the Python mirror and bench.py hold),
// the block is pinned for the call and the shader stores every stream where the caller wants it, in 8-byte pieces (a row pitch of
// tic_compress_bound() bytes is a multiple of 8, not 16); the copy out of the pipeline's pinned buffer (0.12-0.28 ms for the 49 streams of
// the reference's benchmark set: a third of the call) does not happen.  The rows are written up to the chunk's longest stream rounded to 8
// bytes (all within the frames' capacities): bytes behind a stream's end are not preserved.  *done = false: not applicable, nothing was
// enqueued.
static int read_back_zero_copy(tic_ctx *ctx, const BatchPlan &p, Slot &s, hipStream_t st, uint8_t *const *outs, const size_t *caps, size_t maxlen, bool *done) {
    *done = false;
    const size_t row = (maxlen + 7) / 8 * 8;
    size_t P = 0;
    if (!ctx->auto_register || maxlen < 16 || !rows_of_one_block(outs + s.first, caps + s.first, s.count, row, &P)) return TIC_OK;
    uint8_t *base = outs[s.first];
    const size_t span = (size_t)(s.count - 1) * P + row;
    if (!(host_pointer_is_pinned(base) && host_pointer_is_pinned(base + span - 1))) {
        void *reg = pin_range(base, span);
        if (!reg) return TIC_OK;
        ctx->autoregs.push_back(reg); // (released with the call's other registrations, behind its last synchronisation)
    }
    void *d_dst = nullptr;
    if (hipHostGetDevicePointer(&d_dst, base, 0) != hipSuccess) {
        (void)hipGetLastError();
        return TIC_OK;
    }
    BT_START();
    hipError_t e = launch_readback<u32x2v>(s.d_streams, p.bound, d_dst, P, row, s.count, st);
    if (e == hipSuccess) e = hipEventRecord(s.rb_done, st);
    BT_STOP(3);
    if (e != hipSuccess) return set_err(ctx, TIC_E_HIP, "stream read-back failed: %s", hipGetErrorString(e));
    s.rb_row = 0; // (nothing to hand out)
    ctx->last_batch_zero_copy += s.count;
    *done = true;
    return TIC_OK;
}

// Finishing a chunk, part 1: wait for its lengths, then start the read-back of its streams on `st`.  The reading thread does not wait for
// the copy: it records the slot's rb_done behind it and turns to the next chunk, so that the read-backs follow each other on their stream
// without a host round trip in between; hand_out_chunk waits for the event.
static int read_back(tic_ctx *ctx, const BatchPlan &p, Slot &s, hipStream_t st, uint8_t *const *outs, const size_t *caps, size_t *out_lens, bool zero_copy) {
    BT_START();
    const hipError_t ev = hipEventSynchronize(s.done);
    BT_STOP(2);
    if (ev != hipSuccess) return set_err(ctx, TIC_E_HIP, "batch chunk failed");
    if (*s.h_err == 1) return set_err(ctx, TIC_E_RANGE, "coefficient without a Huffman code (reference raises KeyError)");
    if (*s.h_err == 4) return kRetryEightLanes; // a block exceeds the lane-per-block kernel's strings: the whole call is run again
    if (*s.h_err) return set_err(ctx, TIC_E_SPACE, "device entropy stage: stream buffer too small");
    size_t maxlen = 0;
    for (int k = 0; k < s.count; k++) {
        const size_t len = (size_t)s.h_lens[k];
        const int f = s.first + k;
        if (len > caps[f]) return set_err(ctx, TIC_E_SPACE, "output buffer of frame %d too small (%zu bytes needed)", f, len);
        out_lens[f] = len;
        if (len > maxlen) maxlen = len;
    }
    if (zero_copy) {
        bool done = false;
        const int rc = read_back_zero_copy(ctx, p, s, st, outs, caps, maxlen, &done);
        if (rc || done) return rc;
    }
    // Packed: ONE launch brings the head of every frame's stream buffer - as many bytes as the longest stream has - into the slot's pinned
    // buffer, to be handed out by a few threads (a copy straight into the caller's pageable buffers is staged by the runtime, ~0.15 ms
    // each; 16 separate copies of ~0.9 MB into pinned memory cost ~45 us each, 2.5 x their transfer time).  Frames of one batch compress
    // to similar sizes, so little more than the streams themselves crosses PCIe.  Where the rows would not fit the pinned buffer: a copy
    // per frame, straight to the caller.
    const size_t pin_cap = p.coef_bytes * (size_t)p.chunk; // size of pin_out (ensure_batch_slots)
    const size_t row = align_up(maxlen, 256);
    const bool packed = row * (size_t)s.count <= pin_cap;
    BT_START();
    hipError_t e = hipSuccess;
    if (packed) // (row and bound are multiples of 16; the bytes behind a stream are never handed out)
        e = launch_readback<u32x4v>(s.d_streams, p.bound, s.pin_out, row, maxlen, s.count, st);
    for (int k = 0; k < s.count && !packed && e == hipSuccess; k++)
        e = hipMemcpyAsync(outs[s.first + k], (char *)s.d_streams + (size_t)k * p.bound, (size_t)s.h_lens[k], hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return set_err(ctx, TIC_E_HIP, "stream read-back failed: %s", hipGetErrorString(e));
    e = hipEventRecord(s.rb_done, st);
    BT_STOP(3);
    if (e != hipSuccess) return set_err(ctx, TIC_E_HIP, "stream read-back failed");
    s.rb_row = packed ? row : 0;
    return TIC_OK;
}

// ... part 2: once the read-back has arrived, out of the slot's pinned buffer into the caller's buffers, by a few threads
static int hand_out_chunk(tic_ctx *ctx, Slot &s, uint8_t *const *outs) {
    BT_START();
    if (hipEventSynchronize(s.rb_done) != hipSuccess) return set_err(ctx, TIC_E_HIP, "stream read-back failed");
    if (const size_t row = s.rb_row) {
        const int cnt = s.count, first = s.first;
        const char *src = (const char *)s.pin_out;
        const unsigned long long *lens = s.h_lens;
        size_t total = 0;
        for (int k = 0; k < cnt; k++) total += (size_t)lens[k];
        const int T = cnt < 4 || total < (4u << 20) ? 1 : 4; // (starting and joining four threads costs 0.15-0.2 ms: more than copying 4 MB)
        run_strided(cnt, T, [ctx]() { bind_pipeline_thread(ctx); }, [=](int k) { memcpy(outs[first + k], src + (size_t)k * row, (size_t)lens[k]); });
    }
    BT_STOP(4);
    return TIC_OK;
}

// Three host threads, kBatchSlots slots: the calling thread stages chunk c into pinned memory and enqueues it (H2D, kernels, lengths), a
// second waits for each chunk in turn and starts the read-back of its streams, a third hands them out to the caller's buffers.  The
// device always has work queued while the threads copy, and a slot is claimed again only after the third thread has freed it
// (256 x 1080p host -> host: DESIGN.md section 6).
// A batch of ONE chunk (the reference's benchmark set: 49 frames of 512 x 512) runs on the calling thread: enqueue, wait, read back, hand out.
// Starting the two pipeline threads costs more than the chunk's work when the host is busy - their first wake-up came 3-10 ms late in
// one call in three on a shared box (tools/batch_small_probe.py: chunk_wait 0.008 ms, the reader found the chunk long finished).
// (The driver is written once for frames of one size and for mixed frames: enqueue(c, slot, stream, par) queues chunk c - par: which of the
// slot's two error flags it uses -, read(slot, zero_copy) is read_back, hand(slot) is hand_out_chunk.)
extern "C++" {
template <class Enqueue, class Read, class Hand>
static int device_entropy_pipeline(tic_ctx *ctx, int nchunks, Enqueue enqueue, Read read, Hand hand) {
    std::vector<Slot> &slots = ctx->bslots;
    const bool inline_path = nchunks <= 1;
    SlotGate gate;
    ClosableQueue<int> q_read, q_hand; // slots to read back / to hand out, in submission order
    std::vector<std::thread> threads;
    if (!inline_path) {
        threads.emplace_back([&]() {
            bind_pipeline_thread(ctx);
            (void)hipSetDevice(ctx->device);
            int k;
            while (q_read.pop(k)) {
                const int r = read(slots[k], false);
                if (r == TIC_OK) {
                    q_hand.push(k);
                } else { // nothing to hand out
                    gate.fail(r);
                    gate.finish(slots[k]);
                }
            }
            q_hand.close();
        });
        threads.emplace_back([&]() {
            bind_pipeline_thread(ctx);
            int k;
            while (q_hand.pop(k)) {
                const int r = hand(slots[k]);
                if (r != TIC_OK) gate.fail(r);
                gate.finish(slots[k]);
            }
        });
    }
    int result = TIC_OK;
    for (int c = 0; c < nchunks; c++) {
        const int si = c % kBatchSlots;
        Slot &s = slots[si];
        gate.claim(ctx, s, 1);
        if (gate.error() != TIC_OK) break;
        const int par = s.parity;
        s.parity ^= 1;
        result = enqueue(c, s, ctx->bstream[c & 1], par);
        if (result != TIC_OK) break;
        if (inline_path) {
            result = read(s, true);
            if (result == TIC_OK) result = hand(s);
            break;
        }
        q_read.push(si);
    }
    q_read.close();
    batch_end(ctx, threads);
    return result != TIC_OK ? result : gate.error();
}
}

static int batch_device_entropy(tic_ctx *ctx, const uint8_t *const *images, int n, int h, int w, ptrdiff_t row_stride, int quality,
                                uint8_t *const *outs, const size_t *caps, size_t *out_lens) {
    BatchPlan p;
    const int rc = batch_begin(ctx, images, n, h, w, row_stride, quality, true, true, outs, caps, out_lens, &p);
    if (rc || p.chunk == 0) return rc;
    return device_entropy_pipeline(
        ctx, (n + p.chunk - 1) / p.chunk,
        [&](int c, Slot &s, hipStream_t stream, int par) {
            const int first = c * p.chunk, cnt = n - first < p.chunk ? n - first : p.chunk;
            return enqueue_chunk(ctx, p, s, stream, images, first, cnt, row_stride, h, w, quality, [&](Slot &sl, hipStream_t st) {
                // entropy stage of the whole chunk: pack + place (headers, lengths); no zero fill
                hipError_t e = entropy_gpu_fused((const int16_t *)sl.d_coef, p.nblk, cnt, ctx->d_huff, sl.d_work, sl.d_work.cap, sl.d_streams, p.bound,
                                                 (p.bound - 16) / 4, h, w, quality, sl.d_lens, nullptr, sl.d_err + par, sl.d_err + (par ^ 1),
                                                 quality <= ctx->ent_lane_max_quality ? kEntropyLanePerBlock : kEntropyEightLanes, st);
                if (e == hipSuccess) e = hipMemcpyAsync(sl.h_lens, sl.d_lens, cnt * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
                if (e == hipSuccess) e = hipMemcpyAsync(sl.h_err, sl.d_err + par, sizeof(int), hipMemcpyDeviceToHost, st);
                return e;
            });
        },
        [&](Slot &s, bool zero_copy) { return read_back(ctx, p, s, ctx->rstream, outs, caps, out_lens, zero_copy); },
        [&](Slot &s) { return hand_out_chunk(ctx, s, outs); });
}

int tic_compress_batch(tic_ctx *ctx, const uint8_t *const *images, int n, int h, int w, ptrdiff_t row_stride, int quality,
                       uint8_t *const *outs, const size_t *caps, size_t *out_lens, int threads) {
    TIC_LOCK(ctx);
    if (threads <= 0) {
        int rc = batch_device_entropy(ctx, images, n, h, w, row_stride, quality, outs, caps, out_lens);
        if (rc == kRetryEightLanes) {
            ctx->ent_lane_max_quality = quality - 1;
            rc = batch_device_entropy(ctx, images, n, h, w, row_stride, quality, outs, caps, out_lens);
        }
        return rc;
    }
    return batch_host_coder(ctx, images, n, h, w, row_stride, quality, nullptr, outs, caps, out_lens, threads, true);
}

// ---- mixed batches: frames of any sizes and qualities in one call (tic_compress_batch_v) -----------------------------------------------------
// The plan (plan_mixed_batch, tic_host_pipeline.h) orders the frames by (quality, width, height), cuts chunks by bytes and by count and names,
// per chunk, the runs of neighbours the transform takes in one launch each.  A chunk then goes the way a chunk of equal frames goes -
// enqueue_on_slot, device_entropy_pipeline, SlotGate, batch_end - with the entropy stage in descriptor form (entropy_gpu_fused_v: ONE pack and ONE
// place launch for the chunk, whatever its frames) and a read-back that brings down each stream's own bytes.  Device entropy only; no zero-copy
// route (the streams of a mixed call are not rows of one length); no registration of the caller's frames beyond what the caller did itself:
// pinned, dense frames are copied from where they lie, everything else is staged.
struct MixedCall {
    const uint8_t *const *images;
    const ptrdiff_t *row_strides;
    uint8_t *const *outs;
    const size_t *caps;
    size_t *out_lens;
};

// Upload of a mixed chunk: every frame pinned where it lies and dense at the staged pitch - a copy per stretch of frames that follow each other in
// memory as they do in the chunk -, else all of them staged into the slot's pinned buffer by a few threads and ONE copy.
static hipError_t upload_chunk_v(tic_ctx *ctx, Slot &s, const MixedPlan &p, const MixedChunk &c, const MixedCall &io, hipStream_t st, int *direct) {
    *direct = 0;
    const MixedFrame *fr = &p.frames[(size_t)c.first];
    bool pinned = true;
    for (int k = 0; k < c.count && pinned; k++) {
        const uint8_t *img = io.images[fr[k].index];
        pinned = (size_t)io.row_strides[fr[k].index] == fr[k].pitch && host_pointer_is_pinned(img) && host_pointer_is_pinned(img + fr[k].img_bytes - 1);
    }
    if (pinned) {
        hipError_t e = hipSuccess;
        for (int k = 0; k < c.count && e == hipSuccess;) {
            int m = 1;
            size_t bytes = fr[k].img_bytes;
            while (k + m < c.count && io.images[fr[k + m].index] == io.images[fr[k].index] + bytes) bytes += fr[k + m++].img_bytes;
            e = hipMemcpyAsync((char *)s.d_img + fr[k].img_off, io.images[fr[k].index], bytes, hipMemcpyHostToDevice, st);
            k += m;
        }
        if (e == hipSuccess) {
            *direct = c.count;
            return hipSuccess;
        }
        (void)hipGetLastError(); // (a copy the runtime refuses: the staged route writes the device buffer again, in stream order)
    }
    BT_START();
    unsigned hw = std::thread::hardware_concurrency();
    int T = ctx->stage_threads > 0 ? ctx->stage_threads : (int)(hw ? hw / 2 : 4);
    T = T < 1 ? 1 : (T > 8 ? 8 : T);
    if (T > c.count) T = c.count;
    if (c.img_bytes < (4u << 20)) T = 1;
    uint8_t *pin = s.pin_in;
    run_strided(c.count, T, [ctx]() { bind_pipeline_thread(ctx); },
                [=](int k) { copy_rows(pin + fr[k].img_off, fr[k].pitch, io.images[fr[k].index], io.row_strides[fr[k].index], fr[k].h, fr[k].w); });
    BT_STOP(0);
    return hipMemcpyAsync(s.d_img, s.pin_in, c.img_bytes, hipMemcpyHostToDevice, st);
}

// Finishing a mixed chunk, part 1 (read_back's counterpart): its lengths, then ONE launch that packs every stream's own bytes into the slot's
// pinned buffer, 64 bytes apart at least.
static int read_back_v(tic_ctx *ctx, const MixedPlan &p, Slot &s, hipStream_t st, const MixedCall &io) {
    BT_START();
    const hipError_t ev = hipEventSynchronize(s.done);
    BT_STOP(2);
    if (ev != hipSuccess) return set_err(ctx, TIC_E_HIP, "batch chunk failed");
    if (*s.h_err == 1) return set_err(ctx, TIC_E_RANGE, "coefficient without a Huffman code (reference raises KeyError)");
    if (*s.h_err == 4) return kRetryEightLanes; // a block exceeds the lane-per-block kernel's strings: the call is run again (tic_compress_batch_v)
    if (*s.h_err) return set_err(ctx, TIC_E_SPACE, "device entropy stage: stream buffer too small");
    size_t off = 0, maxlen = 0;
    for (int k = 0; k < s.count; k++) {
        const MixedFrame &f = p.frames[(size_t)(s.first + k)];
        const size_t len = (size_t)s.h_lens[k];
        if (len > io.caps[f.index] || len > f.bound) return set_err(ctx, TIC_E_SPACE, "output buffer of frame %d too small (%zu bytes needed)", f.index, len);
        io.out_lens[f.index] = len;
        s.h_rb_off[k] = off;
        off += align_up(len, 64);
        maxlen = len > maxlen ? len : maxlen;
    }
    if (off > ctx->bslot_cap.pin_out) return set_err(ctx, TIC_E_HIP, "stream read-back: landing buffer too small"); // (sized for it: mixed_slot_need)
    BT_START();
    // (the shader reads the lengths and the landing offsets where the host holds them: pinned memory, complete before the launch)
    const unsigned gx = (unsigned)std::min<size_t>(64, (maxlen / 16 + 255) / 256 + 1);
    hipLaunchKernelGGL(readback_frames_kernel, dim3(gx, (unsigned)s.count), dim3(256), 0, st, (const unsigned char *)s.d_streams, s.d_frames, s.h_lens,
                       s.h_rb_off, (unsigned char *)s.pin_out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(s.rb_done, st);
    BT_STOP(3);
    if (e != hipSuccess) return set_err(ctx, TIC_E_HIP, "stream read-back failed: %s", hipGetErrorString(e));
    return TIC_OK;
}

// ... part 2: out of the pinned buffer to where the caller wants each stream
static int hand_out_chunk_v(tic_ctx *ctx, const MixedPlan &p, Slot &s, const MixedCall &io) {
    BT_START();
    if (hipEventSynchronize(s.rb_done) != hipSuccess) return set_err(ctx, TIC_E_HIP, "stream read-back failed");
    const MixedFrame *fr = &p.frames[(size_t)s.first];
    const char *src = (const char *)s.pin_out;
    const unsigned long long *lens = s.h_lens, *offs = s.h_rb_off;
    size_t total = 0;
    for (int k = 0; k < s.count; k++) total += (size_t)lens[k];
    const int T = s.count < 4 || total < (4u << 20) ? 1 : 4;
    uint8_t *const *outs = io.outs;
    run_strided(s.count, T, [ctx]() { bind_pipeline_thread(ctx); }, [=](int k) { memcpy(outs[fr[k].index], src + offs[k], (size_t)lens[k]); });
    BT_STOP(4);
    return TIC_OK;
}

// The transform of a mixed chunk: one launch per run of neighbours (a run is one tall frame).  *launches counts them.
static hipError_t transform_chunk_v(tic_ctx *ctx, Slot &s, const MixedPlan &p, const MixedChunk &c, hipStream_t stream, int *launches) {
    hipError_t e = hipSuccess;
    for (size_t r = 0; r < c.runs.size() && e == hipSuccess; r++) {
        const MixedFrame &f = p.frames[(size_t)c.runs[r].first];
        DctqArgs a = make_args(ctx, (const char *)s.d_img + f.img_off, c.runs[r].h_total, f.w, (ptrdiff_t)f.pitch, f.quality,
                               (int16_t *)s.d_coef + f.first_block * 64);
        a.fallback_count = nullptr;
        e = launch_dctq(a, 2, stream);
        (*launches)++;
    }
    return e;
}

// ... of a scaled chunk: ONE launch of the descriptor form, whatever the frames' widths and settings (the slot's table, uploaded in stream order)
static hipError_t transform_chunk_scaled(Slot &s, const MixedPlan &p, const MixedChunk &c, hipStream_t stream, int *launches) {
    unsigned long long off[kScaledMaxFrames], blk[kScaledMaxFrames];
    long long pitch[kScaledMaxFrames];
    int hs[kScaledMaxFrames], ws[kScaledMaxFrames], qfs[kScaledMaxFrames];
    for (int k = 0; k < c.count; k++) {
        const MixedFrame &f = p.frames[(size_t)(c.first + k)];
        off[k] = f.img_off, blk[k] = f.first_block, pitch[k] = (long long)f.pitch;
        hs[k] = f.h, ws[k] = f.w, qfs[k] = f.quality;
    }
    uint32_t strips = 0;
    if (!fill_scaled_table(s.h_sframes, c.count, (unsigned long long)(uintptr_t)s.d_img.p, (unsigned long long)(uintptr_t)s.d_coef.p, off, pitch, hs, ws, qfs, blk, &strips))
        return hipErrorInvalidValue;
    hipError_t e = hipMemcpyAsync(s.d_sframes, s.h_sframes, sizeof(ScaledFrameTable), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = launch_fdctq_scaled_v(s.d_sframes, strips, stream);
    (*launches)++;
    return e;
}

static tic_ctx::SlotNeed mixed_slot_need(const MixedPlan &p) {
    tic_ctx::SlotNeed need;
    need.img = p.max_img;
    need.coef = p.max_nblk * 128;
    need.streams = p.max_stream;
    need.pin_out = p.max_stream + 64 * (size_t)p.max_count; // every stream rounded up to 64 bytes (read_back_v)
    need.work = entropy_fused_work_bytes_v(p.max_nblk, (size_t)p.max_count);
    need.frames = p.max_count;
    return need;
}

// One run of the pipeline over the plan's chunks.  kRetryEightLanes: a chunk that ran the lane-per-block kernel raised code 4; *retry_quality is
// that chunk's lowest quality.  scaled: the integer encoder's streams (the plan's qualities are its settings) - the descriptor-form transform,
// the 8-lane packing kernel always (the bound learnt for the lane-per-block kernel is neither read nor written), header flag 1 << 30.
// *launches_out: transform launches.
static int batch_mixed_pipeline(tic_ctx *ctx, const MixedPlan &p, const MixedCall &io, int *retry_quality, bool scaled, int *launches_out) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = ensure_batch_slots(ctx, mixed_slot_need(p));
    if (rc) return rc;
    for (auto &sl : ctx->bslots) sl.pending = 0;
    int launches = 0;
    const int result = device_entropy_pipeline(
        ctx, (int)p.chunks.size(),
        [&](int ci, Slot &s, hipStream_t stream, int par) {
            const MixedChunk &c = p.chunks[(size_t)ci];
            const MixedFrame *fr = &p.frames[(size_t)c.first];
            // lane per block only when EVERY frame of the chunk may take it (the plan orders by quality: the first frame's is the lowest, the last
            // frame's the highest)
            const int mode = !scaled && fr[c.count - 1].quality <= ctx->ent_lane_max_quality ? kEntropyLanePerBlock : kEntropyEightLanes;
            size_t nparts, ngroups, nplaces;
            if (!mixed_chunk_table(p, c, mode, s.h_frames, &nparts, &ngroups, &nplaces)) return set_err(ctx, TIC_E_ARG, "mixed batch: chunk %d has no table", ci);
            return enqueue_on_slot(
                ctx, s, stream, c.first, c.count, [&](int *direct) { return upload_chunk_v(ctx, s, p, c, io, stream, direct); },
                [&]() { return scaled ? transform_chunk_scaled(s, p, c, stream, &launches) : transform_chunk_v(ctx, s, p, c, stream, &launches); },
                [&](Slot &sl, hipStream_t st) {
                    hipError_t e = hipMemcpyAsync(sl.d_frames, sl.h_frames, sizeof(EntropyFrameTable), hipMemcpyHostToDevice, st);
                    if (e == hipSuccess)
                        e = entropy_gpu_fused_v((const int16_t *)sl.d_coef, sl.h_frames, sl.d_frames, c.count, ctx->d_huff, sl.d_work, sl.d_work.cap, sl.d_streams,
                                                sl.d_lens, sl.d_err + par, sl.d_err + (par ^ 1), mode, st, scaled ? kFlagScaled : 0u);
                    if (e == hipSuccess) e = hipMemcpyAsync(sl.h_lens, sl.d_lens, c.count * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
                    if (e == hipSuccess) e = hipMemcpyAsync(sl.h_err, sl.d_err + par, sizeof(int), hipMemcpyDeviceToHost, st);
                    return e;
                });
        },
        [&](Slot &s, bool) {
            const int r = read_back_v(ctx, p, s, ctx->rstream, io);
            const int q = p.frames[(size_t)s.first].quality; // (the reading thread alone writes this; the caller reads it behind batch_end's join)
            if (r == kRetryEightLanes && (*retry_quality == 0 || q < *retry_quality)) *retry_quality = q;
            return r;
        },
        [&](Slot &s) { return hand_out_chunk_v(ctx, p, s, io); });
    *launches_out = launches;
    return result;
}

// The chunk limits of the calls that go by plan_mixed_batch: 64 frames and 32 MB of staged pixels, or what the test hooks say.
struct ChunkLimits {
    int frames;
    size_t bytes;
};
static ChunkLimits mixed_chunk_limits() {
    ChunkLimits lim = {kMixedChunkFrames, kMixedChunkBytes};
    if (const char *e = test_hook("TIC_BATCH_CHUNK")) lim.frames = atoi(e); // (out of range: the default)
    if (const char *e = test_hook("TIC_BATCH_CHUNK_BYTES")) lim.bytes = strtoull(e, nullptr, 10) ? (size_t)strtoull(e, nullptr, 10) : lim.bytes;
    return lim;
}

int tic_compress_batch_v(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides,
                         const int *qualities, uint8_t *const *outs, const size_t *caps, size_t *out_lens) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    // every check before any work: nothing is written while a frame of the call is unacceptable
    if (n < 0) return set_err(ctx, TIC_E_ARG, "negative frame count %d", n);
    ctx->last_vbatch_frames = ctx->last_vbatch_single = ctx->last_vbatch_chunks = ctx->last_vbatch_launches = 0;
    if (n == 0) return TIC_OK;
    if (!images || !hs || !ws || !row_strides || !qualities || !outs || !caps || !out_lens) return set_err(ctx, TIC_E_ARG, "null array argument");
    for (int i = 0; i < n; i++) {
        const int rc = check_stream_geometry(ctx, hs[i], ws[i], row_strides[i], qualities[i]);
        if (rc) return frame_err(ctx, rc, i);
        if (!outs[i]) return set_err(ctx, TIC_E_ARG, "frame %d: null output buffer", i);
        if (!images[i] && num_blocks(hs[i], ws[i]) != 0) return set_err(ctx, TIC_E_ARG, "frame %d: null image", i);
    }
    const ChunkLimits lim = mixed_chunk_limits();
    const MixedPlan p = plan_mixed_batch(hs, ws, qualities, n, lim.frames, lim.bytes);
    const MixedCall io = {images, row_strides, outs, caps, out_lens};
    ctx->last_batch_direct_frames = ctx->last_batch_staged_frames = ctx->last_batch_autoreg_frames = ctx->last_batch_zero_copy = 0;
    ctx->bt = BatchTrace();
    for (int i : p.empty) { // frames without blocks: the host's header-only stream
        const int rc = entropy_encode(nullptr, hs[i], ws[i], qualities[i], outs[i], caps[i], &out_lens[i]);
        if (rc) return set_err(ctx, rc, "frame %d: output buffer too small for a header", i);
    }
    if (!p.frames.empty()) {
        int retry_quality = 0;
        int rc = batch_mixed_pipeline(ctx, p, io, &retry_quality, false, &ctx->last_vbatch_launches);
        if (rc == kRetryEightLanes) {
            // The flag does not say which frame of the chunk has the long block, so the bound drops below the chunk's LOWEST quality: this chunk and
            // every later one (qualities ascend) then run the 8-lane kernel, the chunks in front passed as they were - one more run settles it.
            ctx->ent_lane_max_quality = retry_quality - 1;
            retry_quality = 0;
            ctx->last_batch_direct_frames = ctx->last_batch_staged_frames = 0; // (every chunk is uploaded again: the route's figures are the second run's)
            rc = batch_mixed_pipeline(ctx, p, io, &retry_quality, false, &ctx->last_vbatch_launches);
        }
        if (rc) return rc == kRetryEightLanes ? set_err(ctx, TIC_E_HIP, "mixed batch: the 8-lane packing kernel refused a block") : rc;
    }
    ctx->last_vbatch_frames = (int)p.frames.size();
    ctx->last_vbatch_chunks = (int)p.chunks.size();
    for (int i : p.single) { // what the batch kernels do not take, behind the batch, frame by frame
        const int rc = tic_compress(ctx, images[i], hs[i], ws[i], row_strides[i], qualities[i], outs[i], caps[i], &out_lens[i]);
        if (rc) return frame_err(ctx, rc, i);
        ctx->last_vbatch_single++;
    }
    return TIC_OK;
}

int tic_last_compress_batch_v(tic_ctx *ctx, int *batch_frames, int *single_frames, int *chunks, int *transform_launches) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (batch_frames) *batch_frames = ctx->last_vbatch_frames;
    if (single_frames) *single_frames = ctx->last_vbatch_single;
    if (chunks) *chunks = ctx->last_vbatch_chunks;
    if (transform_launches) *transform_launches = ctx->last_vbatch_launches;
    return TIC_OK;
}

// ---- the integer encoder for a batch (tic_compress_batch_scaled_v) --------------------------------------------------------------------------
// The mixed batch's route with the settings 0..3 as the plan's qualities: frames ordered by (setting, width, height), the same chunks, slots,
// upload, entropy stage in descriptor form, read-back and hand-out.  What differs: ONE transform launch per chunk (fdctq_scaled_kernel_v: a
// table of records instead of a launch per run of equal-width frames), the 8-lane packing kernel always, header flag 1 << 30 with its flush
// byte, and stream areas with room for that byte.  Nothing the float route learns (ent_lane_max_quality) is read or written.
// Argument checks shared with tic_rd_points_scaled_v: every frame's geometry at every setting, its image pointer.
static int check_scaled_frames(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides, const int *qfs,
                               int nq_shared) {
    for (int i = 0; i < n; i++) {
        int rc = TIC_OK;
        if (nq_shared < 0) rc = check_scaled_geometry(ctx, hs[i], ws[i], row_strides[i], qfs[i]);
        for (int j = 0; j < nq_shared && rc == TIC_OK; j++) rc = check_scaled_geometry(ctx, hs[i], ws[i], row_strides[i], qfs[j]);
        if (rc) return frame_err(ctx, rc, i);
        if (!images[i] && num_blocks(hs[i], ws[i]) != 0) return set_err(ctx, TIC_E_ARG, "frame %d: null image", i);
    }
    return TIC_OK;
}

int tic_compress_batch_scaled_v(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides,
                                const int *qfs, uint8_t *const *outs, const size_t *caps, size_t *out_lens) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    // every check before any work: nothing is written while a frame of the call is unacceptable
    if (n < 0) return set_err(ctx, TIC_E_ARG, "negative frame count %d", n);
    ctx->last_sbatch_frames = ctx->last_sbatch_single = ctx->last_sbatch_chunks = ctx->last_sbatch_launches = 0;
    if (n == 0) return TIC_OK;
    if (!images || !hs || !ws || !row_strides || !qfs || !outs || !caps || !out_lens) return set_err(ctx, TIC_E_ARG, "null array argument");
    int rc = check_scaled_frames(ctx, images, n, hs, ws, row_strides, qfs, -1);
    if (rc) return rc;
    for (int i = 0; i < n; i++)
        if (!outs[i]) return set_err(ctx, TIC_E_ARG, "frame %d: null output buffer", i);
    const ChunkLimits lim = mixed_chunk_limits();
    const MixedPlan p = plan_mixed_batch(hs, ws, qfs, n, lim.frames, lim.bytes, 1); // (+ 1: the flush byte)
    for (const MixedFrame &f : p.frames)
        if (f.bound < tic_compress_scaled_bound(f.h, f.w)) return set_err(ctx, TIC_E_ARG, "frame %d: stream area without room for the flush byte", f.index);
    const MixedCall io = {images, row_strides, outs, caps, out_lens};
    ctx->last_batch_direct_frames = ctx->last_batch_staged_frames = ctx->last_batch_autoreg_frames = ctx->last_batch_zero_copy = 0;
    ctx->bt = BatchTrace();
    for (int i : p.empty) { // frames without blocks: the host's 17-byte stream
        rc = entropy_encode_scaled(nullptr, hs[i], ws[i], qfs[i], outs[i], caps[i], &out_lens[i]);
        if (rc) return set_err(ctx, rc, "frame %d: output buffer too small for a header and the flush byte", i);
    }
    if (!p.frames.empty()) {
        int retry_quality = 0;
        rc = batch_mixed_pipeline(ctx, p, io, &retry_quality, true, &ctx->last_sbatch_launches);
        if (rc) return rc == kRetryEightLanes ? set_err(ctx, TIC_E_HIP, "scaled batch: the 8-lane packing kernel refused a block") : rc;
    }
    ctx->last_sbatch_frames = (int)p.frames.size();
    ctx->last_sbatch_chunks = (int)p.chunks.size();
    for (int i : p.single) { // what the batch kernels do not take, behind the batch, frame by frame
        rc = tic_compress_scaled(ctx, images[i], hs[i], ws[i], row_strides[i], qfs[i], outs[i], caps[i], &out_lens[i]);
        if (rc) return frame_err(ctx, rc, i);
        ctx->last_sbatch_single++;
    }
    return TIC_OK;
}

int tic_last_compress_batch_scaled(tic_ctx *ctx, int *batch_frames, int *single_frames, int *chunks, int *transform_launches) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (batch_frames) *batch_frames = ctx->last_sbatch_frames;
    if (single_frames) *single_frames = ctx->last_sbatch_single;
    if (chunks) *chunks = ctx->last_sbatch_chunks;
    if (transform_launches) *transform_launches = ctx->last_sbatch_launches;
    return TIC_OK;
}

// Room for `ntabs` tables of the transform's descriptor form outside the batch slots.  Nothing of an earlier call may be in flight.
static int ensure_scaled_tabs(tic_ctx *ctx, size_t ntabs) {
    const size_t bytes = ntabs * sizeof(ScaledFrameTable), alloc = align_up(bytes, 16384);
    const int rc = ctx->h_scaled_tabs.grow(ctx, bytes, alloc);
    return rc ? rc : ctx->d_scaled_tabs.grow(ctx, bytes, alloc);
}

// The kernel alone, synchronous: frames resident anywhere on the device, the coefficients of all of them back to back at d_coeffs_zz in the
// caller's order (a frame without blocks takes none), one launch per kScaledMaxFrames frames.
int tic_dctq_scaled_v_dev(tic_ctx *ctx, const void *const *d_images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides, const int *qfs,
                          void *d_coeffs_zz) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (n < 0) return set_err(ctx, TIC_E_ARG, "negative frame count %d", n);
    if (n == 0) return TIC_OK;
    if (!d_images || !hs || !ws || !row_strides || !qfs) return set_err(ctx, TIC_E_ARG, "null array argument");
    int rc = check_scaled_frames(ctx, (const uint8_t *const *)d_images, n, hs, ws, row_strides, qfs, -1);
    if (rc) return rc;
    std::vector<int> with_blocks;
    for (int i = 0; i < n; i++)
        if (num_blocks(hs[i], ws[i]) != 0) with_blocks.push_back(i);
    if (with_blocks.empty()) return TIC_OK;
    if (!d_coeffs_zz || ((uintptr_t)d_coeffs_zz & 15) != 0) return set_err(ctx, TIC_E_ARG, "coefficient buffer null or not 16-byte aligned");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t m = with_blocks.size(), ntabs = (m + kScaledMaxFrames - 1) / kScaledMaxFrames;
    rc = ensure_scaled_tabs(ctx, ntabs);
    if (rc) return rc;
    std::vector<uint32_t> strips(ntabs);
    unsigned long long block = 0;
    for (size_t t = 0; t < ntabs; t++) {
        unsigned long long off[kScaledMaxFrames], blk[kScaledMaxFrames];
        long long pitch[kScaledMaxFrames];
        int fh[kScaledMaxFrames], fw[kScaledMaxFrames], fq[kScaledMaxFrames];
        const int cnt = (int)std::min<size_t>(kScaledMaxFrames, m - t * kScaledMaxFrames);
        for (int k = 0; k < cnt; k++) {
            const int i = with_blocks[t * kScaledMaxFrames + (size_t)k];
            off[k] = (unsigned long long)(uintptr_t)d_images[i], blk[k] = block, pitch[k] = (long long)row_strides[i]; // (addresses: the table's base is 0)
            fh[k] = hs[i], fw[k] = ws[i], fq[k] = qfs[i];
            block += num_blocks(hs[i], ws[i]);
        }
        if (!fill_scaled_table(&ctx->h_scaled_tabs[t], cnt, 0ull, (unsigned long long)(uintptr_t)d_coeffs_zz, off, pitch, fh, fw, fq, blk, &strips[t]))
            return set_err(ctx, TIC_E_ARG, "frames %d..: more strips than one launch walks", with_blocks[t * kScaledMaxFrames]);
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_scaled_tabs, ctx->h_scaled_tabs, ntabs * sizeof(ScaledFrameTable), hipMemcpyHostToDevice, ctx->stream));
    for (size_t t = 0; t < ntabs; t++) HIPCHK(ctx, launch_fdctq_scaled_v(ctx->d_scaled_tabs + t, strips[t], ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TIC_OK;
}

// ---- rate control for a batch: the sizes of n frames at a list of qualities, and the best stream of each within its own byte budget -----------
// (tic_stream_sizes_v, tic_compress_batch_to_size.)  The plan (tic_rate_plan.h) cuts the call into the mixed batch's chunks, ordered by
// (width, height).  A chunk is staged and uploaded ONCE into the context's scratch image; a SUBMISSION then queues any number of probes of its
// frames on the context's stream - a transform launch per probe (neighbours of one transform run at one quality: one launch) into the
// probe's own area of the coefficient workspace, then ONE launch of the size kernel's descriptor form per 64 probes - behind one memset of
// the results and one copy of the probe tables, and ends in one read-back.  Where a submission's coefficients exceed kRateWorkspaceBytes
// it goes in passes over the same workspace; the stream orders them.
struct RateCall {
    const uint8_t *const *images;
    const int *hs, *ws;
    const ptrdiff_t *row_strides;
};

// Argument checks the two calls share: every frame's geometry at `quality`, its image pointer.  "frame i: ..." for the first offender.
static int check_rate_frames(tic_ctx *ctx, const RateCall &io, int n, int quality) {
    for (int i = 0; i < n; i++) {
        const int rc = check_stream_geometry(ctx, io.hs[i], io.ws[i], io.row_strides[i], quality);
        if (rc) return frame_err(ctx, rc, i);
        if (!io.images[i] && num_blocks(io.hs[i], io.ws[i]) != 0) return set_err(ctx, TIC_E_ARG, "frame %d: null image", i);
    }
    return TIC_OK;
}

// Stages chunk `c` at the plan's pitches and queues its ONE upload into the context's scratch image.
static int upload_rate_chunk(tic_ctx *ctx, const MixedPlan &p, const MixedChunk &c, const RateCall &io) {
    int rc = ensure_scratch(ctx, c.img_bytes, 0);
    if (rc) return rc;
    rc = ctx->h_rate_pix.grow(ctx, c.img_bytes);
    if (rc) return rc;
    const MixedFrame *fr = &p.frames[(size_t)c.first];
    uint8_t *pin = ctx->h_rate_pix;
    const int T = c.count < 4 || c.img_bytes < (4u << 20) ? 1 : 4;
    run_strided(c.count, T, [ctx]() { bind_pipeline_thread(ctx); },
                [=](int k) { copy_rows(pin + fr[k].img_off, fr[k].pitch, io.images[fr[k].index], io.row_strides[fr[k].index], fr[k].h, fr[k].w); });
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_img, pin, c.img_bytes, hipMemcpyHostToDevice, ctx->stream));
    return TIC_OK;
}

// Queues the probes of `s` (frames of the chunk resident in the scratch image) and the copy of their results into ctx->h_rate, entry i for
// probe i; the caller waits for the stream.  Nothing of an earlier submission may be in flight: the buffers may grow.
// distortion: a rate-distortion submission - behind every size launch ONE launch of the measuring kernel's descriptor form on the same probes
// (idct_sse_kernel_v), its results behind the size results (dist_of(ctx->h_rate, probes)): the same memset clears both, the same copy brings
// both back.
static size_t sse_group_cap() { // (TIC_SSE_MAX_GROUPS, a test hook, lowers the cap so that the walk can be tested on frames of a few blocks)
    if (const char *e = test_hook("TIC_SSE_MAX_GROUPS")) {
        const long v = atol(e);
        if (v >= 1 && v <= (long)kSseMaxGroups) return (size_t)v;
    }
    return kSseMaxGroups;
}

// Room for the probe tables of a submission, on the host and on the device: `size_tabs` of the size kernel's, `sse_tabs` of the measuring
// kernel's (0: that kernel is not launched, its buffers stay as they are).  Nothing of an earlier submission may be in flight.
static int ensure_probe_tabs(tic_ctx *ctx, size_t size_tabs, size_t sse_tabs) {
    const size_t size_bytes = size_tabs * sizeof(SizeProbeTable), sse_bytes = sse_tabs * sizeof(SseProbeTable);
    int rc = ctx->h_rate_tabs.grow(ctx, size_bytes, align_up(size_bytes, 16384));
    if (rc == TIC_OK) rc = ctx->d_rate_tabs.grow(ctx, size_bytes, align_up(size_bytes, 16384));
    if (rc == TIC_OK) rc = ctx->h_rd_tabs.grow(ctx, sse_bytes, align_up(sse_bytes, 16384));
    if (rc == TIC_OK) rc = ctx->d_rd_tabs.grow(ctx, sse_bytes, align_up(sse_bytes, 16384));
    return rc;
}

// The transforms of probes [first, end) of `s` - one pass - into their areas of the coefficient workspace: a launch per transform run.  The
// frames' pixels lie at img_base + MixedFrame::img_off.
static int queue_rate_transforms(tic_ctx *ctx, const RatePlan &p, const RateSubmission &s, int first, int end, const void *img_base) {
    for (int k = first; k < end;) {
        int h_total = 0;
        const int m = rate_transform_run(p, s, k, end, &h_total);
        const MixedFrame &f = p.mixed.frames[(size_t)s.probes[(size_t)k].frame];
        DctqArgs a = make_args(ctx, (const char *)img_base + f.img_off, h_total, f.w, (ptrdiff_t)f.pitch, s.probes[(size_t)k].quality,
                               (int16_t *)ctx->d_coef + s.first_block[(size_t)k] * 64);
        a.fallback_count = nullptr;
        HIPCHK(ctx, launch_dctq(a, 2, ctx->stream));
        k += m;
    }
    return TIC_OK;
}

static int submit_rate_probes(tic_ctx *ctx, const RatePlan &p, RateSubmission &s, bool distortion = false) {
    const int np = (int)s.probes.size();
    layout_rate_submission(p.mixed, s, kRateWorkspaceBytes / 128);
    int rc = ensure_scratch(ctx, 0, s.max_pass_blocks * 128 + 16);
    if (rc) return rc;
    rc = ensure_rate(ctx, (size_t)np);
    if (rc) return rc;
    size_t ntabs = 0;
    for (size_t i = 0; i + 1 < s.pass_first.size(); i++) ntabs += (size_t)(s.pass_first[i + 1] - s.pass_first[i] + kSizeMaxProbes - 1) / kSizeMaxProbes;
    rc = ensure_probe_tabs(ctx, ntabs, distortion ? ntabs : 0);
    if (rc) return rc;
    const size_t tab_bytes = ntabs * sizeof(SizeProbeTable), sse_tab_bytes = distortion ? ntabs * sizeof(SseProbeTable) : 0;
    const size_t sse_cap = sse_group_cap();
    // the tables of every size launch (and of the measuring launch behind it), in launch order
    std::vector<size_t> tab_groups(ntabs), sse_groups(ntabs);
    size_t t = 0;
    for (size_t i = 0; i + 1 < s.pass_first.size(); i++)
        for (int first = s.pass_first[i]; first < s.pass_first[i + 1]; first += kSizeMaxProbes, t++) {
            const int cnt = std::min(kSizeMaxProbes, s.pass_first[i + 1] - first);
            size_t nblk[kSizeMaxProbes], total = 0;
            uint32_t result[kSizeMaxProbes];
            for (int k = 0; k < cnt; k++) nblk[k] = p.mixed.frames[(size_t)s.probes[(size_t)(first + k)].frame].nblk, result[k] = (uint32_t)(first + k);
            if (!fill_size_probe_table(&ctx->h_rate_tabs[t], cnt, nblk, result, &tab_groups[t], &total))
                return set_err(ctx, TIC_E_ARG, "rate batch: probes %d.. have no table", first);
            if (distortion) {
                SseProbeIn in[kSseMaxProbes];
                for (int k = 0; k < cnt; k++) {
                    const RateProbe &pr = s.probes[(size_t)(first + k)];
                    const MixedFrame &f = p.mixed.frames[(size_t)pr.frame];
                    in[k] = SseProbeIn{(const int16_t *)ctx->d_coef + s.first_block[(size_t)(first + k)] * 64, (const uint8_t *)ctx->d_img + f.img_off,
                                       ctx->d_consts + pr.quality, (long long)f.pitch, f.h, f.w, (uint32_t)(first + k)};
                }
                if (!fill_sse_probe_table(&ctx->h_rd_tabs[t], cnt, in, sse_cap, &sse_groups[t]))
                    return set_err(ctx, TIC_E_ARG, "rate-distortion batch: probes %d.. have no table", first);
            }
        }
    const size_t res_bytes = (size_t)np * (sizeof(SizeResult) + (distortion ? sizeof(DistortionResult) : 0));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_rate, 0, res_bytes, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_rate_tabs, ctx->h_rate_tabs, tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (distortion) HIPCHK(ctx, hipMemcpyAsync(ctx->d_rd_tabs, ctx->h_rd_tabs, sse_tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    t = 0;
    for (size_t i = 0; i + 1 < s.pass_first.size(); i++) {
        const int end = s.pass_first[i + 1];
        rc = queue_rate_transforms(ctx, p, s, s.pass_first[i], end, ctx->d_img);
        if (rc) return rc;
        for (int first = s.pass_first[i]; first < end; first += kSizeMaxProbes, t++) {
            HIPCHK(ctx, stream_size_gpu_v((const int16_t *)ctx->d_coef + s.first_block[(size_t)first] * 64, ctx->d_rate_tabs + t, tab_groups[t], ctx->d_size_tab,
                                          ctx->d_rate, ctx->stream));
            ctx->last_rbatch_launches++;
            if (distortion) {
                HIPCHK(ctx, launch_idct_sse_v(ctx->d_rd_tabs + t, sse_groups[t], dist_of(ctx->d_rate, np), ctx->stream));
                ctx->last_rbatch_sse_launches++;
            }
        }
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_rate, ctx->d_rate, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    ctx->last_rbatch_probes += np;
    return TIC_OK;
}

static void reset_rate_batch(tic_ctx *ctx) {
    ctx->last_rbatch_frames = ctx->last_rbatch_single = ctx->last_rbatch_chunks = 0;
    ctx->last_rbatch_probes = ctx->last_rbatch_waits = ctx->last_rbatch_launches = ctx->last_rbatch_sse_launches = 0;
}

// The chunk loop of the calls that probe every frame at every quality of a list (tic_stream_sizes_v, tic_rd_points_v, tic_adaptive_sizes_v).
// Per chunk: its upload, ONE submission of np = count x nq probes - submit(s) - one wait, counted in *waits, and take(pr, np, at) for
// every probe: probe pr of the submission's np is the result at = frame index x nq + j of the caller's tables.  A take that fails ends the call with
// "frame i: " in front of its message.
extern "C++" template <class Submit, class Take>
static int probe_every_quality(tic_ctx *ctx, const RatePlan &p, const RateCall &io, const int *qualities, int nq, int *waits, Submit submit, Take take) {
    RateSubmission s;
    for (const MixedChunk &c : p.mixed.chunks) {
        int rc = upload_rate_chunk(ctx, p.mixed, c, io);
        if (rc) return rc;
        s.probes.clear();
        for (int j = 0; j < nq; j++) // quality by quality: the frames of a transform run are neighbours in the queue
            for (int k = 0; k < c.count; k++) s.probes.push_back(RateProbe{c.first + k, qualities[j]});
        rc = submit(s);
        if (rc) return rc;
        HIPCHK(ctx, wait_stream(ctx));
        (*waits)++;
        for (int j = 0; j < nq; j++)
            for (int k = 0; k < c.count; k++) {
                const int i = p.mixed.frames[(size_t)(c.first + k)].index;
                rc = take((size_t)j * c.count + k, c.count * nq, (size_t)i * nq + j);
                if (rc) return frame_err(ctx, rc, i);
            }
    }
    return TIC_OK;
}

int tic_stream_sizes_v(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides, const int *qualities,
                       int nq, long long *sizes) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    // every check before any work
    if (n < 0) return set_err(ctx, TIC_E_ARG, "negative frame count %d", n);
    if (nq < 0 || (nq > 0 && !qualities)) return set_err(ctx, TIC_E_ARG, "bad quality list");
    reset_rate_batch(ctx);
    if (n == 0 || nq == 0) return TIC_OK;
    if (!images || !hs || !ws || !row_strides || !sizes) return set_err(ctx, TIC_E_ARG, "null array argument");
    const RateCall io = {images, hs, ws, row_strides};
    for (int j = 0; j < nq; j++) {
        const int rc = check_rate_frames(ctx, io, n, qualities[j]);
        if (rc) return rc;
    }
    const ChunkLimits lim = mixed_chunk_limits();
    const RatePlan p = plan_rate_batch(hs, ws, n, lim.frames, lim.bytes);
    for (int i : p.mixed.empty) // header only (codec.py:151)
        for (int j = 0; j < nq; j++) sizes[(size_t)i * nq + j] = 16;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = probe_every_quality(
        ctx, p, io, qualities, nq, &ctx->last_rbatch_waits, [&](RateSubmission &s) { return submit_rate_probes(ctx, p, s); },
        [&](size_t pr, int, size_t at) {
            sizes[at] = probe_size(ctx->h_rate[pr]);
            return TIC_OK;
        });
    if (rc) return rc;
    ctx->last_rbatch_frames = (int)p.mixed.frames.size();
    ctx->last_rbatch_chunks = (int)p.mixed.chunks.size();
    for (int i : p.mixed.single) { // what the batch does not take, behind it, frame by frame
        const int rc = tic_stream_sizes(ctx, images[i], hs[i], ws[i], row_strides[i], qualities, nq, sizes + (size_t)i * nq);
        if (rc) return frame_err(ctx, rc, i);
        ctx->last_rbatch_single++;
    }
    return TIC_OK;
}

// ---- the two batch searches (tic_compress_batch_to_size, tic_compress_batch_to_psnr): what they share ----------------------------------------
// A call is: the prologue (search_batch_begin), its own rule for block-less frames, phase 1 - the searches, chunk by chunk
// (search_chunks) - its own classification of every finished search into a failure or a stream to pack, phase 2 - the streams
// (search_batch_pack) - and the frames the batch does not take with the call's verdict behind them (search_batch_end).
struct SearchBatch {
    tic_ctx *ctx;
    RateCall io;
    int n;
    uint8_t *const *outs;
    const size_t *caps;
    size_t *out_lens;
    int *qualities, *status;
    RatePlan plan;
    std::string first_err; // the message of the first failing frame, in frame order
    int first_bad;
    // Frame i failed with `code`, its message in ctx->err; the call goes on.
    void fail(int i, int code) {
        status[i] = code;
        if (i < first_bad) first_bad = i, first_err = ctx->err;
    }
};
// A plan frame whose search ended at `quality` with a probe of `len` bytes that fit its buffer: it gets a stream.
struct SettledFrame {
    int frame, quality;
    size_t len;
};

// Every check before any work: nothing is written while an argument of the call is unacceptable.  arrays_ok: the call's own arrays are there.
// Then the plan and status[] = TIC_OK.  The caller returns at once on a code, and on n == 0.
static int search_batch_begin(SearchBatch &b, bool arrays_ok, int qmin, int qmax) {
    tic_ctx *ctx = b.ctx;
    const int n = b.n;
    if (n < 0) return set_err(ctx, TIC_E_ARG, "negative frame count %d", n);
    if (qmin < 1 || qmax > 99 || qmin > qmax) return set_err(ctx, TIC_E_QUALITY, "quality range %d..%d is not inside 1..99", qmin, qmax);
    reset_rate_batch(ctx);
    if (n == 0) return TIC_OK;
    if (!b.io.images || !b.io.hs || !b.io.ws || !b.io.row_strides || !arrays_ok || !b.outs || !b.caps || !b.out_lens || !b.qualities || !b.status)
        return set_err(ctx, TIC_E_ARG, "null array argument");
    const int rc = check_rate_frames(ctx, b.io, n, qmin);
    if (rc) return rc;
    for (int i = 0; i < n; i++)
        if (!b.outs[i]) return set_err(ctx, TIC_E_ARG, "frame %d: null output buffer", i);
    const ChunkLimits lim = mixed_chunk_limits();
    b.plan = plan_rate_batch(b.io.hs, b.io.ws, n, lim.frames, lim.bytes);
    for (int i = 0; i < n; i++) b.status[i] = TIC_OK;
    b.first_bad = n;
    return TIC_OK;
}

// Phase 1: per chunk its upload, then the bisections of all its frames in lockstep - a round is one submission of every unsettled frame's
// candidates (round_probes), one read-back, one wait and the replay.  search[f]: plan frame f, begun by the caller; store(r, q, i, np):
// probe i of the round's np is what state r learns about quality q.
extern "C++" template <class Search, class Store>
static int search_chunks(tic_ctx *ctx, const RatePlan &p, const RateCall &io, Search *search, bool distortion, Store store) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RateSubmission s;
    for (size_t ci = 0; ci < p.mixed.chunks.size(); ci++) {
        const MixedChunk &c = p.mixed.chunks[ci];
        int rc = upload_rate_chunk(ctx, p.mixed, c, io);
        if (rc) return rc;
        for (;;) {
            round_probes(c, search, p.depth[ci], s.probes);
            if (s.probes.empty()) break;
            rc = submit_rate_probes(ctx, p, s, distortion);
            if (rc) return rc;
            HIPCHK(ctx, wait_stream(ctx));
            ctx->last_rbatch_waits++;
            for (size_t i = 0; i < s.probes.size(); i++) store(search[s.probes[i].frame], s.probes[i].quality, i, (int)s.probes.size());
            for (int k = 0; k < c.count; k++) search_replay(search[c.first + k]);
        }
    }
    ctx->last_rbatch_frames = (int)p.mixed.frames.size();
    ctx->last_rbatch_chunks = (int)p.mixed.chunks.size();
    return TIC_OK;
}

// Phase 2: the streams of the settled frames, at the qualities found, by the mixed batch (which uploads their pixels again); then their
// out_lens and qualities.
static int search_batch_pack(SearchBatch &b, const std::vector<SettledFrame> &sub) {
    tic_ctx *ctx = b.ctx;
    if (sub.empty()) return TIC_OK;
    const size_t m = sub.size();
    std::vector<const uint8_t *> im(m);
    std::vector<int> sh(m), sw(m), sq(m);
    std::vector<ptrdiff_t> ss(m);
    std::vector<uint8_t *> so(m);
    std::vector<size_t> sc(m), sl(m);
    for (size_t k = 0; k < m; k++) {
        const int i = b.plan.mixed.frames[(size_t)sub[k].frame].index;
        im[k] = b.io.images[i], sh[k] = b.io.hs[i], sw[k] = b.io.ws[i], ss[k] = b.io.row_strides[i], sq[k] = sub[k].quality;
        so[k] = b.outs[i], sc[k] = sub[k].len, sl[k] = 0; // (the capacity is the probe's length: a longer stream fails before it is written)
    }
    const int rc = tic_compress_batch_v(ctx, im.data(), (int)m, sh.data(), sw.data(), ss.data(), sq.data(), so.data(), sc.data(), sl.data());
    if (rc == TIC_E_SPACE || rc == TIC_E_RANGE) { // (a stream longer than its probe, or no code where the probe found one)
        const std::string why = ctx->err;
        return set_err(ctx, TIC_E_HIP, "the packed streams contradict their probes: %s", why.c_str());
    }
    if (rc) return rc;
    for (size_t k = 0; k < m; k++) {
        const int i = b.plan.mixed.frames[(size_t)sub[k].frame].index;
        if (sl[k] != sc[k]) // (two independent walks over the same coefficients: cannot differ)
            return set_err(ctx, TIC_E_HIP, "frame %d: the packed stream (%zu bytes) contradicts its probe (%zu bytes)", i, sl[k], sc[k]);
        b.out_lens[i] = sl[k], b.qualities[i] = sq[k];
    }
    return TIC_OK;
}

// What the batch does not take, behind it: the single-frame search one(i) of each such frame.  Then the call's code: the first failing
// frame's, in frame order, with its message.
extern "C++" template <class One> static int search_batch_end(SearchBatch &b, One one) {
    tic_ctx *ctx = b.ctx;
    for (int i : b.plan.mixed.single) {
        const int rc = one(i);
        if (rc) b.fail(i, frame_err(ctx, rc, i));
        ctx->last_rbatch_single++;
    }
    if (b.first_bad < b.n) {
        ctx->err = b.first_err;
        return b.status[b.first_bad];
    }
    return TIC_OK;
}

int tic_compress_batch_to_size(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides,
                               const size_t *max_bytes, int qmin, int qmax, uint8_t *const *outs, const size_t *caps, size_t *out_lens, int *qualities,
                               int *status) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    SearchBatch b = {ctx, {images, hs, ws, row_strides}, n, outs, caps, out_lens, qualities, status};
    int rc = search_batch_begin(b, max_bytes != nullptr, qmin, qmax);
    if (rc || n == 0) return rc;
    const MixedPlan &mp = b.plan.mixed;
    for (int i : mp.empty) { // a header at every quality: the bisection ends at qmax
        if (max_bytes[i] < 16) {
            out_lens[i] = 16;
            b.fail(i, set_err(ctx, TIC_E_SPACE, "frame %d: 16 bytes at quality %d exceed the budget of %zu", i, qmin, max_bytes[i]));
        } else if (caps[i] < 16) {
            out_lens[i] = 16;
            b.fail(i, set_err(ctx, TIC_E_SPACE, "frame %d: output buffer too small (16 bytes needed, %zu given)", i, caps[i]));
        } else {
            write_header(outs[i], hs[i], ws[i], qmax);
            out_lens[i] = 16, qualities[i] = qmax;
        }
    }
    std::vector<RateSearch> search(mp.frames.size());
    for (size_t f = 0; f < search.size(); f++) rate_search_begin(search[f], qmin, qmax, (unsigned long long)max_bytes[mp.frames[f].index]);
    rc = search_chunks(ctx, b.plan, b.io, search.data(), false, [&](RateSearch &r, int q, size_t i, int) { r.known[q] = probe_size(ctx->h_rate[i]); });
    if (rc) return rc;
    std::vector<SettledFrame> sub;
    for (size_t f = 0; f < search.size(); f++) {
        const RateSearch &r = search[f];
        const int i = mp.frames[f].index;
        if (r.state == kRateNoCode) {
            b.fail(i, set_err(ctx, TIC_E_RANGE, "frame %d: coefficient without a Huffman code at quality %d (reference raises KeyError)", i, qmin));
        } else if (r.state == kRateTooLarge) {
            out_lens[i] = (size_t)r.known[qmin];
            b.fail(i, set_err(ctx, TIC_E_SPACE, "frame %d: %lld bytes at quality %d exceed the budget of %zu", i, r.known[qmin], qmin, max_bytes[i]));
        } else if ((size_t)r.known[r.lo] > caps[i]) {
            out_lens[i] = (size_t)r.known[r.lo];
            b.fail(i, set_err(ctx, TIC_E_SPACE, "frame %d: output buffer too small (%lld bytes needed, %zu given)", i, r.known[r.lo], caps[i]));
        } else {
            sub.push_back(SettledFrame{(int)f, r.lo, (size_t)r.known[r.lo]});
        }
    }
    rc = search_batch_pack(b, sub);
    if (rc) return rc;
    return search_batch_end(b, [&](int i) {
        return tic_compress_to_size(ctx, images[i], hs[i], ws[i], row_strides[i], max_bytes[i], qmin, qmax, outs[i], caps[i], &out_lens[i], &qualities[i]);
    });
}

int tic_last_rate_batch(tic_ctx *ctx, int *batch_frames, int *single_frames, int *chunks, int *probes, int *search_waits, int *size_launches) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (batch_frames) *batch_frames = ctx->last_rbatch_frames;
    if (single_frames) *single_frames = ctx->last_rbatch_single;
    if (chunks) *chunks = ctx->last_rbatch_chunks;
    if (probes) *probes = ctx->last_rbatch_probes;
    if (search_waits) *search_waits = ctx->last_rbatch_waits;
    if (size_launches) *size_launches = ctx->last_rbatch_launches;
    return TIC_OK;
}

// ---- rate-distortion for a batch: the (size, error) tables of n frames, and the smallest stream of each at no more than its own error --------
// (tic_rd_points_v, tic_compress_batch_to_psnr.)  The routes are the two above with a rate-distortion submission (submit_rate_probes,
// distortion = true): the chunks, the one upload per chunk, the passes over the workspace and the look-ahead depth are the rate plan's; the
// search by distortion is tic_rd_plan.h's, the mirror of the search by size.
int tic_rd_points_v(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides, const int *qualities,
                    int nq, long long *sizes, uint64_t *sse, uint64_t *sse_wrapped) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    // every check before any work
    if (n < 0) return set_err(ctx, TIC_E_ARG, "negative frame count %d", n);
    if (nq < 0 || (nq > 0 && !qualities)) return set_err(ctx, TIC_E_ARG, "bad quality list");
    reset_rate_batch(ctx);
    if (n == 0 || nq == 0) return TIC_OK;
    if (!images || !hs || !ws || !row_strides || !sizes) return set_err(ctx, TIC_E_ARG, "null array argument");
    if (!sse || !sse_wrapped) return set_err(ctx, TIC_E_ARG, "null result pointer");
    const RateCall io = {images, hs, ws, row_strides};
    for (int j = 0; j < nq; j++) {
        const int rc = check_rate_frames(ctx, io, n, qualities[j]);
        if (rc) return rc;
    }
    const ChunkLimits lim = mixed_chunk_limits();
    const RatePlan p = plan_rate_batch(hs, ws, n, lim.frames, lim.bytes);
    for (int i : p.mixed.empty) // header only (codec.py:151): no pixel, no error
        for (int j = 0; j < nq; j++) {
            sizes[(size_t)i * nq + j] = 16;
            sse[(size_t)i * nq + j] = sse_wrapped[(size_t)i * nq + j] = 0;
        }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = probe_every_quality(
        ctx, p, io, qualities, nq, &ctx->last_rbatch_waits, [&](RateSubmission &s) { return submit_rate_probes(ctx, p, s, true); },
        [&](size_t pr, int np, size_t at) {
            const DistortionResult &d = dist_of(ctx->h_rate, np)[pr];
            sizes[at] = probe_size(ctx->h_rate[pr]);
            sse[at] = d.sse;
            sse_wrapped[at] = d.sse_wrapped;
            return TIC_OK;
        });
    if (rc) return rc;
    ctx->last_rbatch_frames = (int)p.mixed.frames.size();
    ctx->last_rbatch_chunks = (int)p.mixed.chunks.size();
    for (int i : p.mixed.single) { // what the batch does not take, behind it, frame by frame
        const int rc = tic_rd_points(ctx, images[i], hs[i], ws[i], row_strides[i], qualities, nq, sizes + (size_t)i * nq, sse + (size_t)i * nq,
                                     sse_wrapped + (size_t)i * nq);
        if (rc) return frame_err(ctx, rc, i);
        ctx->last_rbatch_single++;
    }
    return TIC_OK;
}

int tic_compress_batch_to_psnr(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides,
                               const uint64_t *max_sse, int qmin, int qmax, uint8_t *const *outs, const size_t *caps, size_t *out_lens, int *qualities,
                               uint64_t *sse, int *status) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    SearchBatch b = {ctx, {images, hs, ws, row_strides}, n, outs, caps, out_lens, qualities, status};
    int rc = search_batch_begin(b, max_sse && sse, qmin, qmax);
    if (rc || n == 0) return rc;
    const MixedPlan &mp = b.plan.mixed;
    for (int i : mp.empty) { // a header and no error at every quality: the bisection ends at qmin
        if (caps[i] < 16) {
            out_lens[i] = 16;
            b.fail(i, set_err(ctx, TIC_E_SPACE, "frame %d: output buffer too small (16 bytes needed, %zu given)", i, caps[i]));
        } else {
            write_header(outs[i], hs[i], ws[i], qmin);
            out_lens[i] = 16, qualities[i] = qmin, sse[i] = 0;
        }
    }
    std::vector<PsnrSearch> search(mp.frames.size());
    for (size_t f = 0; f < search.size(); f++) psnr_search_begin(search[f], qmin, qmax, max_sse[mp.frames[f].index]);
    rc = search_chunks(ctx, b.plan, b.io, search.data(), true, [&](PsnrSearch &r, int q, size_t i, int np) {
        r.known[q] = probe_size(ctx->h_rate[i]);
        r.known_sse[q] = dist_of(ctx->h_rate, np)[i].sse;
    });
    if (rc) return rc;
    std::vector<SettledFrame> sub;
    for (size_t f = 0; f < search.size(); f++) {
        const PsnrSearch &r = search[f];
        const int i = mp.frames[f].index;
        if (r.state == kPsnrNoCode || r.state == kPsnrOutOfReach) { // the single call's side values: the quality and the error of qmax, no length
            qualities[i] = qmax, sse[i] = r.known_sse[qmax], out_lens[i] = 0;
            if (r.state == kPsnrNoCode)
                b.fail(i, set_err(ctx, TIC_E_RANGE, "frame %d: coefficient without a Huffman code at quality %d (reference raises KeyError)", i, qmax));
            else
                b.fail(i, set_err(ctx, TIC_E_SPACE, "frame %d: squared error %llu at quality %d exceeds the bound of %llu", i,
                                  (unsigned long long)r.known_sse[qmax], qmax, (unsigned long long)max_sse[i]));
        } else if ((size_t)r.known[r.lo] > caps[i]) {
            sse[i] = r.known_sse[r.lo], out_lens[i] = (size_t)r.known[r.lo];
            b.fail(i, set_err(ctx, TIC_E_SPACE, "frame %d: output buffer too small (%lld bytes needed, %zu given)", i, r.known[r.lo], caps[i]));
        } else {
            sub.push_back(SettledFrame{(int)f, r.lo, (size_t)r.known[r.lo]});
        }
    }
    rc = search_batch_pack(b, sub);
    if (rc) return rc;
    for (const SettledFrame &t : sub) sse[mp.frames[(size_t)t.frame].index] = search[(size_t)t.frame].known_sse[t.quality];
    return search_batch_end(b, [&](int i) {
        return tic_compress_to_psnr(ctx, images[i], hs[i], ws[i], row_strides[i], max_sse[i], qmin, qmax, outs[i], caps[i], &out_lens[i], &qualities[i], &sse[i]);
    });
}

int tic_last_rd_batch(tic_ctx *ctx, int *sse_launches) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (sse_launches) *sse_launches = ctx->last_rbatch_sse_launches;
    return TIC_OK;
}

// ---- the table of the reference's tests/cbenchmark.py in one call (tic_rd_points_scaled_v) -----------------------------------------------------
// Length and round-trip error of the integer encoder's stream for every frame x setting pair.  The chunks are the mixed plan's (frames ordered
// by width and height), cut so that the coefficients of a chunk's probes - nq areas per frame - fit the rate workspace.  Per chunk: one
// upload into the scratch image, one memset of the results, and per 64 probes ONE launch of the transform's descriptor form (a record per
// probe: the nq records of a frame name the same pixels with their own setting and output area), one of the size kernel's and one of the
// measuring kernel's (scaled branch per probe), then one read-back.  The probes are queued setting by setting, so a wave of the transform
// meets a new setting - and reloads its table words - at most nq - 1 times.
// Length of the integer encoder's stream: header, whole payload bytes, BB_flushBits' byte; -1: a coefficient without a code.
static inline long long scaled_probe_size(const SizeResult &r) { return r.nocode ? -1ll : (long long)(16ull + (r.bits >> 3) + 1ull); }

int tic_rd_points_scaled_v(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides, const int *qfs,
                           int nq, long long *sizes, uint64_t *sse, uint64_t *sse_wrapped) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    // every check before any work
    if (n < 0) return set_err(ctx, TIC_E_ARG, "negative frame count %d", n);
    if (nq < 0 || (nq > 0 && !qfs)) return set_err(ctx, TIC_E_ARG, "bad setting list");
    ctx->last_srd_frames = ctx->last_srd_single = ctx->last_srd_chunks = ctx->last_srd_launches = ctx->last_srd_size_launches = ctx->last_srd_sse_launches = 0;
    if (n == 0 || nq == 0) return TIC_OK;
    if (!images || !hs || !ws || !row_strides) return set_err(ctx, TIC_E_ARG, "null array argument");
    for (int j = 0; j < nq; j++)
        if (qfs[j] < 0 || qfs[j] > 3) return set_err(ctx, TIC_E_QUALITY, "scaled-DCT setting %d outside 0..3 (best, high, med, low)", qfs[j]);
    int rc = check_scaled_frames(ctx, images, n, hs, ws, row_strides, qfs, nq);
    if (rc) return rc;
    auto put = [&](int i, int j, long long size, uint64_t s0, uint64_t s1) {
        const size_t at = (size_t)i * (size_t)nq + (size_t)j;
        if (sizes) sizes[at] = size;
        if (sse) sse[at] = s0;
        if (sse_wrapped) sse_wrapped[at] = s1;
    };
    ChunkLimits lim = mixed_chunk_limits();
    // (a block is 64 bytes of pixels and 128 of coefficients: a chunk's probes take 2 * nq times its pixels)
    lim.bytes = std::min(lim.bytes, std::max<size_t>(kRateWorkspaceBytes / (2 * (size_t)nq), 64));
    const std::vector<int> zeros((size_t)n, 0);
    const MixedPlan p = plan_mixed_batch(hs, ws, zeros.data(), n, lim.frames, lim.bytes);
    for (int i : p.empty)
        for (int j = 0; j < nq; j++) put(i, j, 17, 0, 0);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const RateCall io = {images, hs, ws, row_strides};
    const size_t sse_cap = sse_group_cap();
    for (const MixedChunk &c : p.chunks) {
        const int np = c.count * nq;
        const size_t ntabs = ((size_t)np + kScaledMaxFrames - 1) / kScaledMaxFrames;
        static_assert(kScaledMaxFrames == kSizeMaxProbes && kScaledMaxFrames == kSseMaxProbes, "one group of probes is one launch of each kernel");
        rc = ensure_scratch(ctx, c.img_bytes, c.nblk * (size_t)nq * 128 + 16);
        if (rc) return rc;
        rc = ensure_rate(ctx, (size_t)np);
        if (rc) return rc;
        rc = ensure_scaled_tabs(ctx, ntabs);
        if (rc) return rc;
        const size_t size_bytes = ntabs * sizeof(SizeProbeTable), sse_bytes = ntabs * sizeof(SseProbeTable);
        rc = ensure_probe_tabs(ctx, ntabs, ntabs);
        if (rc) return rc;
        rc = upload_rate_chunk(ctx, p, c, io);
        if (rc) return rc;
        // probe j * count + k: frame k of the chunk at setting j, its coefficients behind those of the probes in front
        std::vector<size_t> size_groups(ntabs), sse_groups(ntabs), tab_first_block(ntabs);
        std::vector<uint32_t> strips(ntabs);
        size_t block = 0;
        for (size_t t = 0; t < ntabs; t++) {
            const int first = (int)t * kScaledMaxFrames, cnt = std::min(kScaledMaxFrames, np - first);
            unsigned long long off[kScaledMaxFrames], blk[kScaledMaxFrames];
            long long pitch[kScaledMaxFrames];
            int fh[kScaledMaxFrames], fw[kScaledMaxFrames], fq[kScaledMaxFrames];
            size_t nblk[kSizeMaxProbes], total = 0;
            uint32_t result[kSizeMaxProbes];
            SseProbeIn in[kSseMaxProbes];
            tab_first_block[t] = block;
            for (int k = 0; k < cnt; k++) {
                const int pi = first + k, j = pi / c.count;
                const MixedFrame &f = p.frames[(size_t)(c.first + pi % c.count)];
                off[k] = f.img_off, blk[k] = block, pitch[k] = (long long)f.pitch, fh[k] = f.h, fw[k] = f.w, fq[k] = qfs[j];
                nblk[k] = f.nblk, result[k] = (uint32_t)pi;
                in[k] = SseProbeIn{(const int16_t *)ctx->d_coef + block * 64, (const uint8_t *)ctx->d_img + f.img_off, ctx->d_consts + 50, (long long)f.pitch,
                                   f.h, f.w, (uint32_t)pi, qfs[j]};
                block += f.nblk;
            }
            if (!fill_scaled_table(&ctx->h_scaled_tabs[t], cnt, (unsigned long long)(uintptr_t)ctx->d_img.p, (unsigned long long)(uintptr_t)ctx->d_coef.p, off, pitch, fh,
                                   fw, fq, blk, &strips[t]) ||
                !fill_size_probe_table(&ctx->h_rate_tabs[t], cnt, nblk, result, &size_groups[t], &total) ||
                !fill_sse_probe_table(&ctx->h_rd_tabs[t], cnt, in, sse_cap, &sse_groups[t]))
                return set_err(ctx, TIC_E_ARG, "scaled rate-distortion batch: probes %d.. have no table", first);
        }
        const size_t res_bytes = (size_t)np * (sizeof(SizeResult) + sizeof(DistortionResult));
        HIPCHK(ctx, hipMemsetAsync(ctx->d_rate, 0, res_bytes, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_scaled_tabs, ctx->h_scaled_tabs, ntabs * sizeof(ScaledFrameTable), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_rate_tabs, ctx->h_rate_tabs, size_bytes, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_rd_tabs, ctx->h_rd_tabs, sse_bytes, hipMemcpyHostToDevice, ctx->stream));
        for (size_t t = 0; t < ntabs; t++) {
            HIPCHK(ctx, launch_fdctq_scaled_v(ctx->d_scaled_tabs + t, strips[t], ctx->stream));
            HIPCHK(ctx, stream_size_gpu_v((const int16_t *)ctx->d_coef + tab_first_block[t] * 64, ctx->d_rate_tabs + t, size_groups[t], ctx->d_size_tab, ctx->d_rate,
                                          ctx->stream));
            HIPCHK(ctx, launch_idct_sse_v(ctx->d_rd_tabs + t, sse_groups[t], dist_of(ctx->d_rate, np), ctx->stream, true));
            ctx->last_srd_launches++, ctx->last_srd_size_launches++, ctx->last_srd_sse_launches++;
        }
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_rate, ctx->d_rate, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, wait_stream(ctx));
        const DistortionResult *dist = dist_of(ctx->h_rate, np);
        for (int pi = 0; pi < np; pi++)
            put(p.frames[(size_t)(c.first + pi % c.count)].index, pi / c.count, scaled_probe_size(ctx->h_rate[pi]), dist[pi].sse, dist[pi].sse_wrapped);
    }
    ctx->last_srd_frames = (int)p.frames.size();
    ctx->last_srd_chunks = (int)p.chunks.size();
    for (int i : p.single) { // what a chunk cannot hold, behind the batch, frame by frame and setting by setting
        const size_t nblk = num_blocks(hs[i], ws[i]);
        for (int j = 0; j < nq; j++) {
            uint64_t sums[2] = {0, 0};
            rc = tic_roundtrip_sse_scaled(ctx, images[i], hs[i], ws[i], row_strides[i], qfs[j], sums);
            if (rc) return frame_err(ctx, rc, i);
            // (its coefficients are still in the scratch buffer: the size kernel on them)
            rc = ensure_rate(ctx, 1);
            if (rc) return rc;
            HIPCHK(ctx, hipMemsetAsync(ctx->d_rate, 0, sizeof(SizeResult), ctx->stream));
            HIPCHK(ctx, stream_size_gpu((const int16_t *)ctx->d_coef, nblk, 1, ctx->d_size_tab, ctx->d_rate, ctx->stream));
            HIPCHK(ctx, hipMemcpyAsync(ctx->h_rate, ctx->d_rate, sizeof(SizeResult), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, wait_stream(ctx));
            put(i, j, scaled_probe_size(ctx->h_rate[0]), sums[0], sums[1]);
        }
        ctx->last_srd_single++;
    }
    return TIC_OK;
}

int tic_last_rd_scaled_batch(tic_ctx *ctx, int *batch_frames, int *single_frames, int *chunks, int *transform_launches, int *size_launches,
                             int *sse_launches) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (batch_frames) *batch_frames = ctx->last_srd_frames;
    if (single_frames) *single_frames = ctx->last_srd_single;
    if (chunks) *chunks = ctx->last_srd_chunks;
    if (transform_launches) *transform_launches = ctx->last_srd_launches;
    if (size_launches) *size_launches = ctx->last_srd_size_launches;
    if (sse_launches) *sse_launches = ctx->last_srd_sse_launches;
    return TIC_OK;
}

// The measuring kernel's descriptor form alone, on n probes whose coefficients lie back to back on the device: the tables (one per 64 probes
// with blocks) into the context's table buffers, the results cleared.  launches[t]: the grid of table t.
static int queue_distortion_v(tic_ctx *ctx, const void *d_coeffs_zz, const void *const *d_images, int n, const int *hs, const int *ws,
                              const ptrdiff_t *row_strides, const int *qualities, std::vector<size_t> &launches) {
    int rc = ensure_rate(ctx, (size_t)n);
    if (rc) return rc;
    const size_t ntabs = ((size_t)n + kSseMaxProbes - 1) / kSseMaxProbes; // (an upper bound: probes without blocks take no entry)
    rc = ensure_probe_tabs(ctx, 0, ntabs); // (no size launch: the size kernel's tables are not touched)
    if (rc) return rc;
    const size_t cap = sse_group_cap();
    launches.clear();
    SseProbeIn in[kSseMaxProbes];
    int cnt = 0;
    size_t blk = 0;
    auto flush = [&]() {
        if (cnt == 0) return true;
        size_t groups = 0;
        if (!fill_sse_probe_table(&ctx->h_rd_tabs[launches.size()], cnt, in, cap, &groups)) return false;
        launches.push_back(groups);
        cnt = 0;
        return true;
    };
    for (int i = 0; i < n; i++) {
        const size_t nb = num_blocks(hs[i], ws[i]);
        if (nb == 0) continue;
        in[cnt++] = SseProbeIn{(const int16_t *)d_coeffs_zz + blk * 64, (const uint8_t *)d_images[i], ctx->d_consts + qualities[i], (long long)row_strides[i],
                               hs[i], ws[i], (uint32_t)i};
        blk += nb;
        if (cnt == kSseMaxProbes && !flush()) return set_err(ctx, TIC_E_ARG, "probe %d: no table", i);
    }
    if (!flush()) return set_err(ctx, TIC_E_ARG, "probes have no table");
    HIPCHK(ctx, hipMemsetAsync(dist_of(ctx->d_rate, n), 0, (size_t)n * sizeof(DistortionResult), ctx->stream));
    if (!launches.empty())
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_rd_tabs, ctx->h_rd_tabs, launches.size() * sizeof(SseProbeTable), hipMemcpyHostToDevice, ctx->stream));
    return TIC_OK;
}

static int check_distortion_v_args(tic_ctx *ctx, const void *d_coeffs_zz, const void *const *d_images, int n, const int *hs, const int *ws,
                                   const ptrdiff_t *row_strides, const int *qualities, const void *result) {
    if (!ctx) return TIC_E_ARG;
    if (n < 0) return set_err(ctx, TIC_E_ARG, "negative probe count %d", n);
    if (n == 0) return TIC_OK;
    if (!d_images || !hs || !ws || !row_strides || !qualities || !result) return set_err(ctx, TIC_E_ARG, "null array argument");
    for (int i = 0; i < n; i++) {
        const int rc = check_distortion_args(ctx, hs[i], ws[i], row_strides[i], qualities[i], -1, result);
        if (rc) {
            const std::string why = ctx->err;
            return set_err(ctx, rc, "probe %d: %s", i, why.c_str());
        }
        if (num_blocks(hs[i], ws[i]) && (!d_coeffs_zz || !d_images[i])) return set_err(ctx, TIC_E_ARG, "probe %d: null device pointer", i);
    }
    return TIC_OK;
}

int tic_distortion_v_dev(tic_ctx *ctx, const void *d_coeffs_zz, const void *const *d_images, int n, const int *hs, const int *ws,
                         const ptrdiff_t *row_strides, const int *qualities, uint64_t *sums) {
    TIC_LOCK(ctx);
    int rc = check_distortion_v_args(ctx, d_coeffs_zz, d_images, n, hs, ws, row_strides, qualities, sums);
    if (rc || n == 0) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<size_t> launches;
    rc = queue_distortion_v(ctx, d_coeffs_zz, d_images, n, hs, ws, row_strides, qualities, launches);
    if (rc) return rc;
    ctx->last_rbatch_sse_launches = 0;
    for (size_t t = 0; t < launches.size(); t++) {
        HIPCHK(ctx, launch_idct_sse_v(ctx->d_rd_tabs + t, launches[t], dist_of(ctx->d_rate, n), ctx->stream));
        ctx->last_rbatch_sse_launches++;
    }
    DistortionResult *h_res = dist_of(ctx->h_rate, n);
    HIPCHK(ctx, hipMemcpyAsync(h_res, dist_of(ctx->d_rate, n), (size_t)n * sizeof(DistortionResult), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, wait_stream(ctx));
    for (int i = 0; i < n; i++) {
        sums[2 * i] = h_res[i].sse;
        sums[2 * i + 1] = h_res[i].sse_wrapped;
    }
    return TIC_OK;
}

// Times `iters` back-to-back rounds of its launches on resident coefficients, behind `warm` untimed ones (timed_launches).
int tic_distortion_v_dev_timed(tic_ctx *ctx, const void *d_coeffs_zz, const void *const *d_images, int n, const int *hs, const int *ws,
                               const ptrdiff_t *row_strides, const int *qualities, int warm, int iters, float *ms_total) {
    TIC_LOCK(ctx);
    int rc = check_distortion_v_args(ctx, d_coeffs_zz, d_images, n, hs, ws, row_strides, qualities, ms_total);
    if (rc) return rc;
    if (!ms_total || warm < 0 || iters <= 0) return set_err(ctx, TIC_E_ARG, "bad argument");
    *ms_total = 0.0f;
    if (n == 0) return TIC_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<size_t> launches;
    rc = queue_distortion_v(ctx, d_coeffs_zz, d_images, n, hs, ws, row_strides, qualities, launches);
    if (rc) return rc;
    return timed_launches(ctx, warm, iters, ms_total, nullptr, [&](int, hipEvent_t, hipEvent_t) {
        for (size_t t = 0; t < launches.size(); t++) {
            const hipError_t e = launch_idct_sse_v(ctx->d_rd_tabs + t, launches[t], dist_of(ctx->d_rate, n), ctx->stream);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    });
}

// One batch over several contexts - normally one per GPU of the node - from ONE process: a host thread per context, contiguous shards
// (frame i of n goes to context i / ceil(n / nctx): the partition of DESIGN.md 7 and of tinyimgcodec_amd/distributed.py
// shard_range), every thread runs the stream-overlapped pipeline of tic_compress_batch on its shard.  Sizes come back in frame
// order in out_lens; there is no data-path exchange between the shards.  The first failing shard's code is returned (its message:
// tic_last_error of that context); *failed_ctx (may be null) receives its index, -1 when all succeeded.  Two contexts may sit on the
// same device (each has its own streams, slots and scratch): that is how a one-GPU box tests this path.
int tic_compress_batch_multi(tic_ctx *const *ctxs, int nctx, const uint8_t *const *images, int n, int h, int w, ptrdiff_t row_stride,
                             int quality, uint8_t *const *outs, const size_t *caps, size_t *out_lens, int threads, int *failed_ctx) {
    if (failed_ctx) *failed_ctx = -1;
    if (!ctxs || nctx < 1 || n < 0) return TIC_E_ARG;
    for (int k = 0; k < nctx; k++) {
        if (!ctxs[k]) return TIC_E_ARG;
        for (int j = 0; j < k; j++)
            if (ctxs[j] == ctxs[k]) return set_err(ctxs[k], TIC_E_ARG, "context %d and %d of a multi-context batch are the same", j, k);
    }
    if (n == 0) return TIC_OK;
    if (!images || !outs || !caps || !out_lens) return set_err(ctxs[0], TIC_E_ARG, "null pointer argument");
    const int per = (n + nctx - 1) / nctx;
    std::vector<int> rcs((size_t)nctx, TIC_OK);
    std::vector<std::thread> th;
    for (int k = 0; k < nctx; k++) {
        const int lo = std::min(k * per, n), hi = std::min(lo + per, n);
        if (hi <= lo) continue;
        th.emplace_back([=, &rcs] { rcs[(size_t)k] = tic_compress_batch(ctxs[k], images + lo, hi - lo, h, w, row_stride, quality, outs + lo, caps + lo, out_lens + lo, threads); });
    }
    for (auto &t : th) t.join();
    for (int k = 0; k < nctx; k++)
        if (rcs[(size_t)k] != TIC_OK) {
            if (failed_ctx) *failed_ctx = k;
            return rcs[(size_t)k];
        }
    return TIC_OK;
}

int tic_dctq_batch(tic_ctx *ctx, const uint8_t *const *images, int n, int h, int w, ptrdiff_t row_stride, int quality,
                   int16_t *const *coeffs) {
    TIC_LOCK(ctx);
    return batch_host_coder(ctx, images, n, h, w, row_stride, quality, coeffs, nullptr, nullptr, nullptr, 4, false);
}

// ---- decode ---------------------------------------------------------------------------------------------
// What a stream's 16-byte header asks for.  scaled_exp < 0: decode() proper; >= 0: its scaled_dct branch with 2 ** scaled_exp
// (codec.py:59-62), whose constants are those of quality 50 - `quality` is the one the constants are taken at.
struct StreamHead {
    int h, w, quality, scaled_exp;
};

// The header checks of tic_decompress, tic_decompress_batch and tic_decompress_dev (tic_decompress_adaptive, the strict decoder, has
// its own).  frame >= 0: the messages name the frame of a batch.
static int check_header(tic_ctx *ctx, const uint8_t *data, size_t len, StreamHead *sh, int frame = -1) {
    char pre[32] = "";
    if (frame >= 0) snprintf(pre, sizeof pre, "frame %d: ", frame);
    int h, w, quality;
    uint32_t flag;
    if (parse_header(data, len, &h, &w, &quality, &flag) != TIC_OK) return set_err(ctx, TIC_E_STREAM, "%sstream shorter than the 16-byte header", pre);
    if (flag & (1u << 31)) return set_err(ctx, TIC_E_STREAM, "%sstreams with an embedded Huffman table are not supported", pre);
    const bool scaled = (flag & (1u << 30)) != 0; // a stream of the reference's C encoder (codec.py:127-128): quality = exponent
    if (h < 0 || w < 0) return set_err(ctx, TIC_E_STREAM, "%sbad geometry in header", pre);
    if (scaled && (quality < 0 || quality > 62)) return set_err(ctx, TIC_E_QUALITY, "%sscaled_dct exponent %d in header outside 0..62", pre, quality);
    if (!scaled && (quality < 1 || quality > 99)) return set_err(ctx, TIC_E_QUALITY, "%squality %d in header outside 1..99", pre, quality);
    *sh = {h, w, scaled ? 50 : quality, scaled ? quality : -1};
    return TIC_OK;
}

// The device decoder's tables go up with the context's first device decode.  ctx->d_dec_luts is set only once they are there.
static int ensure_dec_tables(tic_ctx *ctx) {
    if (ctx->d_dec_luts) return TIC_OK;
    std::unique_ptr<DecLutsDev> l(new DecLutsDev());
    dec_luts_fill(l->dc11, l->ac11, l->ac16);
    dec_chain_luts_fill(l->mdc, l->mac, l->mlong);
    dec_pair_luts_fill(l->ac2, l->long32); // (new DecLutsDev() zeroed the entries behind the long codewords)
    const int rc = ctx->d_dec_luts.grow(ctx, sizeof(DecLutsDev));
    if (rc) return rc;
    const hipError_t e = hipMemcpy(ctx->d_dec_luts, l.get(), sizeof(DecLutsDev), hipMemcpyHostToDevice);
    if (e == hipSuccess) return TIC_OK;
    ctx->d_dec_luts.release(ctx);
    return set_err(ctx, TIC_E_HIP, "device decoder set-up failed: %s", hipGetErrorString(e));
}

// The inverse stage's arguments for the device decoder's kernels: pixels into `out`, rows `stride` bytes apart; `head` (may be null)
// is the 16-byte header h, w, quality and scaled_exp came from - the fused kernel writes pixels only under it.
static DecIdctArgs dec_idct_args(const tic_ctx *ctx, int h, int w, int quality, int scaled_exp, uint8_t *out, long stride, const uint8_t *head) {
    DecIdctArgs a{};
    a.out = out;
    a.h = h;
    a.w = w;
    a.stride = stride;
    a.bw = (w + 7) / 8;
    a.aligned8 = 1;
    a.consts = ctx->d_consts + (scaled_exp >= 0 ? 50 : quality); // codec.py:62: quality = 50 on the scaled branch
    a.scaled = scaled_exp >= 0;
    a.pow2 = scaled_exp >= 0 ? ldexp(1.0, scaled_exp) : 1.0;
    if (head) memcpy(a.head, head, 16);
    return a;
}

// ... and the same for idct_kernel, which reads the coefficients from `coeffs`: the whole frame
static IdctArgs idct_args(const DecIdctArgs &d, const int16_t *coeffs) {
    IdctArgs a;
    a.coeffs = coeffs;
    a.out = d.out;
    a.h = d.h;
    a.w = d.w;
    a.stride = d.stride;
    a.bw = d.bw;
    a.tiles_x = (a.bw + 7) / 8;
    a.ntiles = ((d.h + 7) / 8) * a.tiles_x;
    a.aligned8 = d.aligned8;
    a.consts = d.consts;
    a.scaled = d.scaled;
    a.pow2 = d.pow2;
    return a;
}

// Inverse stage on coefficients that already sit in ctx->d_coef (int16 [N][64] zig-zag, DC integrated) -> pixels in `out`.
// quality and scaled_exp as StreamHead.
// d_dc32 (may be null): the blocks' DC as int32 [N], for a frame whose running DC left int16 (IdctArgs::dc32).
static int idct_from_device(tic_ctx *ctx, int h, int w, int quality, int scaled_exp, uint8_t *out, bool out_on_device = false,
                            size_t out_stride = 0, const int32_t *d_dc32 = nullptr) {
    const size_t pitch = align_up((size_t)w, 256);
    // a device destination whose rows are 8-byte aligned takes the pixels straight from the kernel (its row stores are cropped to w)
    const bool direct = out_on_device && out_stride % 8 == 0 && (uintptr_t)out % 8 == 0;
    IdctArgs a = idct_args(dec_idct_args(ctx, h, w, quality, scaled_exp, direct ? out : (uint8_t *)ctx->d_img,
                                         direct ? (long)out_stride : (long)pitch, nullptr),
                           (const int16_t *)ctx->d_coef);
    a.dc32 = d_dc32;
    HIPCHK(ctx, launch_idct(a, ctx->stream));
    if (!direct)
        HIPCHK(ctx, hipMemcpy2DAsync(out, out_on_device ? out_stride : (size_t)w, ctx->d_img, pitch, (size_t)w, (size_t)h,
                                     out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TIC_OK;
}

static int idctq_impl(tic_ctx *ctx, const int16_t *coeffs_zz, int h, int w, int quality, int scaled_exp, uint8_t *out, size_t cap) {
    if (!ctx) return TIC_E_ARG;
    if (h < 0 || w < 0) return set_err(ctx, TIC_E_ARG, "negative image size");
    if (scaled_exp < 0 && (quality < 1 || quality > 99) && !(quality == TIC_QUALITY_CUSTOM && ctx->custom_quality != 0.0))
        return set_err(ctx, TIC_E_QUALITY, "quality %d outside 1..99", quality);
    if (scaled_exp > 62) return set_err(ctx, TIC_E_QUALITY, "scaled_dct exponent %d outside 0..62", scaled_exp);
    const size_t n = num_blocks(h, w);
    if (n == 0) return TIC_OK;
    if (!coeffs_zz) return set_err(ctx, TIC_E_ARG, "null coefficient pointer");
    if (!out || (size_t)h * (size_t)w > cap) return set_err(ctx, TIC_E_SPACE, "output buffer too small");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t pitch = align_up((size_t)w, 256);
    int rc = ensure_scratch(ctx, pitch * (size_t)h, n * 128);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_coef, coeffs_zz, n * 128, hipMemcpyHostToDevice, ctx->stream));
    return idct_from_device(ctx, h, w, quality, scaled_exp, out);
}

// Long streams: Huffman + run-length decode AND the inverse stage on the device, fused (tic_entropy_dec_gpu.hip): the stream goes
// in, pixels come out, no coefficient array in between.  `out` / `out_on_device` / `out_stride` as idct_from_device.  Returns TIC_OK
// with *done = true when the image is complete in `out`; *done = false (and TIC_OK) when the device decoder met something unusual
// or does not apply - the caller then decodes on the host, which reproduces the reference's behaviour on malformed streams (what
// the device wrote to `out` until then is overwritten).
// Streams the device decoder takes.  Long ones as in rounds 2-4 (16,384 blocks and 2 Mbit at least: the host PARALLEL decoder's own line).
// Since round 5 also short ones - at least kDevDecodeMinBlocks blocks (a 256 x 256 frame) and kDevDecodeMinBits stream bits: with two
// launches instead of four the device decoder beats the host's serial decoder far below the old line, the reference's own benchmark
// images (512 x 512, tests/benchmark.py) decompress() in 86 - 100 us instead of 132 - 387.  Round 5 kept streams below 32 bits per block
// on the host (kDevDecodeMinDensity): sparse streams hold blocks longer than the 544-bit range their average asks for, the stitch gave
// up and the second run cost more than the host decoder.  Round 6: the stitch follows the chain over such ranges (tic_entropy_dec_gpu.hip,
// the fix-up loop), every density is taken, and the bit floor is 1 KB (the benchmark set's sparsest stream at q = 5 has 4,071 bytes).
// Hooks TIC_DECODE_MIN_BLOCKS / _BITS / _DENSITY move the lines for measurements.
// The SINK (DecSink): pixels, as described - or the COEFFICIENTS themselves (tic_entropy_decode, tic_retable_adaptive): the same two launches with the
// fused kernel's phase 1 alone (entropy_decode_coef_gpu), the same tries, and the blocks of the host-decoded tail copied behind block m instead of
// transformed; `out`, ctx->d_img and ctx->h_small are not touched then.
struct DecSink {
    bool coef = false;          // false: pixels into `out`
    int16_t *d_user = nullptr;  // coef: the caller's device buffer, int16 [n][64], 16-byte aligned; null: ctx->d_coef
};
constexpr size_t kDevDecodeMinBlocks = 1024, kDevDecodeMinBits = 1u << 13, kDevDecodeMinDensity = 0;
static bool device_decoder_takes(size_t n, size_t len) {
    size_t min_blocks = kDevDecodeMinBlocks, min_bits = kDevDecodeMinBits, min_density = kDevDecodeMinDensity;
    if (const char *e = test_hook("TIC_DECODE_MIN_BLOCKS")) min_blocks = (size_t)atol(e);
    if (const char *e = test_hook("TIC_DECODE_MIN_BITS")) min_bits = (size_t)atol(e);
    if (const char *e = test_hook("TIC_DECODE_MIN_DENSITY")) min_density = (size_t)atol(e);
    if (min_bits < 8192) min_bits = 8192; // (entropy_decode_idct_gpu: a stream of at least 128 + 2 x 2,048 bits)
    const size_t bits = len * 8;
    if (bits + 8192 >= (1ull << 32) || bits < 128) return false;
    const bool long_one = n >= 16384 && bits >= 128 + (1u << 21);
    const bool short_one = n >= min_blocks && bits >= 128 + min_bits && bits - 128 >= min_density * n;
    return long_one || short_one;
}

// stream bits per lane of the device decoder: `mult` average blocks, at least `floor_words` 32-bit words, as an odd number of words up to 63
// Round 6's rule: TWO average blocks, at least 288 bits (rounds 3-5: three, at least 544 - then a range in which the walk did not fall in step with the
// chain ended the run; now it hands its exit on, and ranges below 544 bits get eight shadows in front of a wave's own).  tools/range_rule_sweep.py,
// profiles/r06_decoder.txt (7): a 512^2 stream at q = 50 / 10 76 / 71 us instead of 88 / 85, 4096^2 noise at q = 90 / 10 121 / 70 instead of 129 / 76;
// second runs in 600 stress streams 4 instead of 2 (all below 32 bits per block).
static int decode_range_bits(size_t len, size_t n, size_t mult = 2, size_t floor_words = 9) {
    // (nearly flat content - below 7 stream bits per block: DC code + end-of-block and little else - is periodic bit patterns in which a walk can stay
    //  out of step for tens of ranges: ranges twice as long there.  tools/stress_decoder.py 600: second runs on valid streams of 4-7 bits per block 1 in
    //  24 instead of 4; everywhere else the longer range only costs - the benchmark loop's decompress() +10-17 us, profiles/r06_decoder.txt)
    return dec_range_rule(len, n, mult, floor_words); // (tic_entropy_dec_gpu.h: the work buffer's self-test asks it too)
}

static int decode_on_device(tic_ctx *ctx, const uint8_t *data, size_t len, const StreamHead &sh, uint8_t *out, bool out_on_device, size_t out_stride,
                            bool *done, const uint8_t *head16 /* the 16 header bytes sh came from */, bool src_on_device = false,
                            bool head_is_guess = false, bool *guess_held = nullptr, DecSink sink = DecSink()) {
    *done = false;
    const int h = sh.h, w = sh.w;
    if (guess_held) *guess_held = false;
    const uint8_t *guessed_head = head_is_guess ? head16 : nullptr;
    const size_t n = num_blocks(h, w);
    // the host parallel decoder's own threshold: shorter streams are decoded serially in well under a millisecond
    if (!device_decoder_takes(n, len) || test_hook("TIC_DECODE_SERIAL") || test_hook("TIC_DECODE_HOST")) return TIC_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = ensure_dec_tables(ctx);
    if (rc) return rc;
    const size_t pitch = align_up((size_t)w, 256);
    rc = ensure_scratch(ctx, sink.coef ? 0 : pitch * (size_t)h, n * 128);
    if (rc) return rc;
    int16_t *const d_sink = sink.coef ? (sink.d_user ? sink.d_user : (int16_t *)ctx->d_coef) : nullptr;
    // The stream is decoded where it lies when it is in device memory at a 4-byte aligned address (the kernels mask the bytes behind
    // its end themselves); a host stream, or an odd address, goes through the context's stream buffer.
    const bool in_place = src_on_device && ((uintptr_t)data & 3u) == 0;
    if (!in_place) {
        rc = ctx->d_stream_buf.grow(ctx, align_up(len, 4) + 16);
        if (rc) return rc;
    }
    const void *d_stream = in_place ? (const void *)data : (const void *)ctx->d_stream_buf;
    rc = ctx->h_dec_tail.grow(ctx, kDecTailEnd + kDecTailCoef); // pinned: the stream's last bytes on their way down (device source), the tail's
    if (rc) return rc;                                          // coefficients on their way up
    DecWorkspace &ws = ctx->dec_ws;
    const size_t wb = entropy_decode_gpu_work_bytes(len, n);
    rc = ws.grow(ctx, wb, wb, entropy_decode_gpu_desc_words(len, n), 1, 1);
    if (rc) return rc;
    if (!in_place) HIPCHK(ctx, hipMemcpyAsync(ctx->d_stream_buf, data, len, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    // The blocks that start in the stream's last 2048 bits are decoded on the host (below): with a device source their bytes - the
    // last 256 of the stream, 512 taken - come down NOW, in front of the kernels, instead of in a synchronous copy behind them
    // (only for a run WITH the margin, i.e. the second run on a stream whose end is not what a whole stream's is: see below)
    const size_t end_bytes = len < kDecTailEnd ? len : kDecTailEnd;
    bool tail_prefetched = false;
    // where the pixels go: a device destination whose rows are 8-byte aligned takes them straight from the kernels (row stores are
    // cropped to w); anything else gets them from the context's image buffer with one strided copy at the end
    const bool direct = !sink.coef && out_on_device && out_stride % 8 == 0 && (uintptr_t)out % 8 == 0;
    // a small image on its way to host memory: the kernels store its rows (8-byte aligned, back to back) into the context's host-mapped
    // buffer, and one memcpy behind the wait that reads the status takes them to the caller - no copy command, no second wait
    // (a 512 x 512 image: 30 us between the last kernel and the end of the read-back, profiles/r05_decoder.txt)
    const size_t pitch8 = dec_pix_pitch(w);
    const bool host_pix = !sink.coef && !out_on_device && pitch8 * (size_t)h <= kDecHostPixBytes && !test_hook("TIC_DECODE_NO_HOSTPIX");
    if (host_pix) {
        rc = ensure_small(ctx, kSmallHostBytes);
        if (rc) return rc;
    }
    // (head16 is a guess, or the stream's own header)
    const DecIdctArgs ia = dec_idct_args(ctx, h, w, sh.quality, sh.scaled_exp, direct ? out : host_pix ? ctx->h_small.d : (uint8_t *)ctx->d_img,
                                         direct ? (long)out_stride : host_pix ? (long)pitch8 : (long)pitch, head16);
    // stream bits per lane (decode_range_bits): 2 average blocks, at least 288 bits, as an odd number of 32-bit words up to 63 (noise at q = 50,
    // 220 bits per block: 480; tiled Lenna, 41, and noise at q = 10, 70: 288; noise at q = 90, 404: 864).  The decoder's kernels are one
    // dependent chain per lane, so their time goes with this number (profiles/r04_decoder.txt: the measure kernel 57 us at 672 bits,
    // 76 at 1,024).  A run in which more ranges in a row than the stitch has rounds stay without a synchronisation point (periodic content),
    // or whose blocks do not follow each other where they are decoded, gives up: one more try with the longest range, then the host decoder
    size_t mult = 2, floor_words = 9;
    if (const char *e = test_hook("TIC_DECODE_RULE")) { // "<average blocks per range>,<least words per range>": measurements of the rule itself
        unsigned a = 0, b = 0;
        if (sscanf(e, "%u,%u", &a, &b) == 2 && a >= 1 && a <= 64 && b >= 9 && b <= 63) mult = a, floor_words = b | 1;
    }
    int range_bits = decode_range_bits(len, n, mult, floor_words);
    ctx->last_decode_tries = 0;
    if (const char *e = test_hook("TIC_DECODE_RANGE")) range_bits = atoi(e);
    if (!entropy_decode_gpu_range_ok(range_bits)) return set_err(ctx, TIC_E_ARG, "TIC_DECODE_RANGE=%d: not a range the device decoder takes", range_bits);
    // The first run takes the chain to the stream's END (margin 0): a whole stream then leaves nothing to the host - no second wait, no
    // upload, no extra launch (20 us of 194 for a 4096^2 stream).  If anything at all is flagged on that run the stream is not what a whole
    // one is (cut, damaged, too few blocks for its header) and it is decoded once more the way rounds 2-3 did: blocks that start in the last
    // 2,048 bits go to the host's bit-serial decoder, which reproduces the reference's behaviour at a stream's end.
    int margin_bits = test_hook("TIC_DECODE_MARGIN") ? 2048 : 0;
    int flat_grid = 4096; // (tic_entropy_dec_gpu.hip wave_lookback)
    if (const char *e = test_hook("TIC_DECODE_FLAT_GRID")) flat_grid = atoi(e) < 0 ? 0 : atoi(e);
    DecStatus st;
    for (;;) {
        if (margin_bits && src_on_device && !tail_prefetched) {
            HIPCHK(ctx, hipMemcpyAsync(ctx->h_dec_tail, (const char *)data + (len - end_bytes), end_bytes, hipMemcpyDeviceToHost, ctx->stream));
            tail_prefetched = true;
        }
        rc = ws.begin(ctx, ctx->stream, 1); // (every call ends with a drained stream)
        if (rc) return rc;
        ctx->last_decode_tries++;
        ctx->last_decode_range = range_bits;
        if (sink.coef)
            HIPCHK(ctx, entropy_decode_coef_gpu(d_stream, len, n, ctx->d_dec_luts, ws.work, ws.work.cap, ws.desc, ws.desc_words, ws.epoch, head16, d_sink,
                                                ws.h_status.d, range_bits, margin_bits, ctx->stream, flat_grid));
        else
            HIPCHK(ctx, entropy_decode_idct_gpu(d_stream, len, n, ctx->d_dec_luts, ws.work, ws.work.cap, ws.desc, ws.desc_words, ws.epoch, ia,
                                                ws.h_status.d, range_bits, margin_bits, ctx->stream, flat_grid));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(&st, ws.h_status, sizeof st); // (host-mapped: the stream has drained)
        if (guessed_head) { // geometry and quality were a guess (tic_decompress_dev): what this run produced counts only if the stream's header is the guessed one
            if (memcmp(st.head, guessed_head, 16) != 0) return TIC_OK;
            *guess_held = true;
        }
        if (test_hook("TIC_DECODE_TRACE"))
            fprintf(stderr, "device decoder run %d: range %d margin %d -> giveup %d, m %llu of %zu, pos_out %llu of %zu bits\n", ctx->last_decode_tries, range_bits,
                    margin_bits, st.giveup, st.m, n, st.pos_out, len * 8);
        // (a whole stream, walked cleanly, whose running DC left int16: no other run decodes it, the host route does.  Beside another bit the DC
        //  sums are those of a broken chain and say nothing: the tries go on as ever)
        if (st.giveup == kDecGiveupWideDc) break;
        if ((st.giveup & 4) && range_bits < 2016) { // (a range without a synchronisation point breaks the chain: whatever else was flagged follows from it)
            range_bits = 2016; // (one retry, with the longest range: a stream that trips the first choice has blocks far above its average)
            continue;
        }
        if (st.giveup != 0 && margin_bits == 0) {
            margin_bits = 2048;
            continue;
        }
        break;
    }
    ctx->last_decode_giveup = st.giveup | ((st.m == 0 || st.m > n) ? 64 : 0);
    if (ctx->last_decode_giveup != 0) return TIC_OK; // the host decoder takes the whole stream
    if (st.m < n) { // the blocks that start in the stream's last 2048 bits: serial on the host, a few KB uploaded, transformed by idct_kernel's block-range form
        const size_t tail_bytes = (n - (size_t)st.m) * 128;
        std::vector<int16_t> big; // (more tail blocks than the pinned buffer holds: cannot happen for a stream the device decoder accepts - 2048 bits are at most 341 blocks)
        int16_t *tail = reinterpret_cast<int16_t *>(ctx->h_dec_tail + kDecTailEnd);
        if (tail_bytes > kDecTailCoef) {
            big.resize(tail_bytes / 2);
            tail = big.data();
        }
        const size_t off = len - end_bytes; // the piece of the stream that came down in front of the kernels starts here
        std::vector<DcWide> wide;
        if (src_on_device && tail_prefetched && (size_t)st.pos_out / 8 >= off) { // (pos_out >= 8 len - 2048: always inside that piece)
            entropy_decode_tail(ctx->h_dec_tail, end_bytes, h, w, (size_t)st.m, (size_t)st.pos_out - off * 8, st.dc_out, tail, &wide);
        } else if (src_on_device) {
            const size_t o2 = (size_t)st.pos_out / 8;
            std::vector<uint8_t> end(len - o2);
            HIPCHK(ctx, hipMemcpy(end.data(), (const char *)data + o2, len - o2, hipMemcpyDeviceToHost));
            entropy_decode_tail(end.data(), len - o2, h, w, (size_t)st.m, (size_t)st.pos_out - o2 * 8, st.dc_out, tail, &wide);
        } else {
            entropy_decode_tail(data, len, h, w, (size_t)st.m, (size_t)st.pos_out, st.dc_out, tail, &wide);
        }
        if (!wide.empty()) { // the running DC leaves int16 in the tail only: the host route, as if the kernel had met it
            ctx->last_decode_giveup = kDecGiveupWideDc;
            return TIC_OK;
        }
        if (sink.coef) { // nothing is transformed: the tail's rows go behind block m, and the call ends with a drained stream
            HIPCHK(ctx, hipMemcpyAsync((char *)d_sink + (size_t)st.m * 128, tail, tail_bytes, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            *done = true;
            return TIC_OK;
        }
        HIPCHK(ctx, hipMemcpyAsync((char *)ctx->d_coef + (size_t)st.m * 128, tail, tail_bytes, hipMemcpyHostToDevice, ctx->stream));
        IdctArgs a = idct_args(ia, (const int16_t *)ctx->d_coef);
        a.first_block = (long)st.m;
        a.nblocks_sel = (long)(n - (size_t)st.m);
        a.ntiles = (int)((a.nblocks_sel + 7) / 8);
        HIPCHK(ctx, launch_idct(a, ctx->stream));
        if (direct || host_pix || !big.empty()) HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); // (the caller's pixels are complete when this returns)
    }
    if (host_pix) { // (the stream has drained: the kernels' stores have arrived)
        copy_rows(out, (size_t)w, ctx->h_small, (ptrdiff_t)pitch8, h, w);
    } else if (!direct && !sink.coef) { // (coefficient sink: every row is in place already)
        HIPCHK(ctx, hipMemcpy2DAsync(out, out_on_device ? out_stride : (size_t)w, ctx->d_img, pitch, (size_t)w, (size_t)h,
                                     out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    *done = true;
    return TIC_OK;
}

int tic_idctq(tic_ctx *ctx, const int16_t *coeffs_zz, int h, int w, int quality, uint8_t *out, size_t cap) {
    TIC_LOCK(ctx);
    return idctq_impl(ctx, coeffs_zz, h, w, quality, -1, out, cap);
}

int tic_idctq_scaled(tic_ctx *ctx, const int16_t *coeffs_zz, int h, int w, int exponent, uint8_t *out, size_t cap) {
    TIC_LOCK(ctx);
    if (ctx && exponent < 0) return set_err(ctx, TIC_E_QUALITY, "scaled_dct exponent %d outside 0..62", exponent);
    return idctq_impl(ctx, coeffs_zz, h, w, 50, exponent, out, cap);
}

// Which decoder the last tic_decompress of this context used: 1 = device Huffman decoder, 2 = host decoder (short streams,
// anything unusual in a long one), 0 = none yet.
int tic_last_decode_path(tic_ctx *ctx) {
    TIC_LOCK(ctx);
    return ctx ? ctx->last_decode_path : TIC_E_ARG;
}

// Diagnostics: the device decoder's reason for leaving the last long stream to the host decoder (0: it did not; bits: 1 an incident
// in the first range, 4 a range without a synchronisation point, 8 / 16 / 32 an incident on the true chain, 2 trace overflow, 64 no block produced).
int tic_last_decode_giveup(tic_ctx *ctx) {
    TIC_LOCK(ctx);
    return ctx ? ctx->last_decode_giveup : TIC_E_ARG;
}

// ... and the stream bits per lane its last run worked with, and how many runs the last long stream took (2: the first choice of
// range met a range without a synchronisation point and the longest range was tried).  Either pointer may be null.
int tic_last_decode_range(tic_ctx *ctx, int *range_bits, int *tries) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (range_bits) *range_bits = ctx->last_decode_range;
    if (tries) *tries = ctx->last_decode_tries;
    return TIC_OK;
}

int tic_last_decode_guess(tic_ctx *ctx) {
    TIC_LOCK(ctx);
    return ctx ? ctx->last_decode_guess : TIC_E_ARG;
}

int tic_set_decode_guess(tic_ctx *ctx, int enable) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    ctx->dec_guess_on = enable != 0;
    return TIC_OK;
}

// The host decoder (short streams, anything the device decoder hands back: the reference's behaviour on malformed streams lives there),
// then the inverse stage on the device; `data` is in host memory, `out` / `out_on_device` / `out_stride` as idct_from_device.
static int decode_on_host(tic_ctx *ctx, const uint8_t *data, size_t len, const StreamHead &sh, uint8_t *out, bool out_on_device,
                          size_t out_stride) {
    const size_t n = num_blocks(sh.h, sh.w);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // coefficients land in a pinned buffer kept on the context: no page faults on a fresh 32 MB vector per call, and the upload
    // runs at PCIe speed instead of through the runtime's staging of pageable memory
    int rc = ctx->h_zz.grow(ctx, n * 128);
    if (rc) return rc;
    std::vector<DcWide> wide;
    entropy_decode(data, len, sh.h, sh.w, ctx->h_zz, &wide);
    ctx->last_decode_path = 2;
    rc = ensure_scratch(ctx, align_up((size_t)sh.w, 256) * (size_t)sh.h, n * 128);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_coef, ctx->h_zz, n * 128, hipMemcpyHostToDevice, ctx->stream));
    // The running DC left int16 somewhere (np.cumsum keeps int32, codec.py:53, and the reference transforms what it holds): the int16
    // layout holds the saturated value, so every block's DC goes up once more as int32 and the wide-DC form of idct_kernel reads it
    // from there.  No stream of our encoders comes here (their DC is an int16 coefficient).
    const int32_t *d_dc32 = nullptr;
    if (!wide.empty()) {
        std::vector<int32_t> dc32(n);
        for (size_t b = 0; b < n; b++) dc32[b] = ctx->h_zz[b * 64];
        for (const DcWide &x : wide) dc32[x.block] = x.dc;
        rc = ctx->d_dc32.grow(ctx, n * sizeof(int32_t));
        if (rc) return rc;
        HIPCHK(ctx, hipMemcpy(ctx->d_dc32, dc32.data(), n * sizeof(int32_t), hipMemcpyHostToDevice)); // (pageable, synchronous: dc32 dies with this scope)
        d_dc32 = ctx->d_dc32;
    }
    return idct_from_device(ctx, sh.h, sh.w, sh.quality, sh.scaled_exp, out, out_on_device, out_stride, d_dc32);
}

int tic_decompress(tic_ctx *ctx, const uint8_t *data, size_t len, uint8_t *out, size_t cap) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    ctx->last_decode_giveup = 0;
    ctx->last_decode_tries = 0;
    StreamHead sh;
    int rc = check_header(ctx, data, len, &sh);
    if (rc) return rc;
    if (num_blocks(sh.h, sh.w) == 0) return TIC_OK;
    if (!out || (size_t)sh.h * (size_t)sh.w > cap) return set_err(ctx, TIC_E_SPACE, "output buffer too small");
    // long streams: the Huffman decode runs on the device too; only the stream goes up and the pixels come down
    bool done = false;
    rc = decode_on_device(ctx, data, len, sh, out, false, 0, &done, data);
    if (rc) return rc;
    if (!done) return decode_on_host(ctx, data, len, sh, out, false, 0);
    ctx->last_decode_path = 1;
    return TIC_OK;
}

// ---- tic_decompress_batch: a chunk's three stages.  The plan (tic_decode_plan.h) says which frames a chunk holds and where their words, ranges,
// blocks and pixels lie in its buffers; the buffers themselves are the context's (ctx->dbat).  `pf`: the chunk's frames, c.count of them.
struct DecBatchIO { // the caller's arrays
    const uint8_t *const *streams;
    const size_t *lens;
    uint8_t *const *outs;
    const size_t *caps;
};

// The buffers both batch decoders share (ctx->dbat): the pinned upload buffer and its device mirror grow together; the chunk's pixel buffer.
static int dbatch_grow(tic_ctx *ctx, size_t up_bytes, size_t pix_bytes) {
    tic_ctx::DecBatch &B = ctx->dbat;
    int rc = B.h_in.grow(ctx, up_bytes, up_bytes + up_bytes / 4);
    if (rc == TIC_OK) rc = B.d_in.grow(ctx, up_bytes, up_bytes + up_bytes / 4);
    return rc ? rc : B.d_pix.grow(ctx, pix_bytes, pix_bytes + pix_bytes / 4);
}

// Descriptors, buffers, ONE upload - descriptors, the frame of every measure wave, the frame of every fused workgroup, the streams - and the two
// launches.  *refused: the launcher's host-side checks said no (every one of them comes before its first launch): nothing runs, and the stream
// has drained - the upload still read the pinned buffer the next chunk is packed into.
// The SINK: d_coef == nullptr pixels into ctx->dbat.d_pix, as described - else (the batch transcoders) the chunk's coefficient rows to d_coef, c.blocks
// of them, frame k's from row pf[k].blk0 on: the same descriptors with the header alone in DecFrame::idct, no pixel buffer, the batch form of the
// coefficient sink behind the same measure launch; nothing is waited for, and tic_last_decompress_batch_work does not hear of it (TBatchCall keeps the phase times).
static int dbatch_enqueue(tic_ctx *ctx, const DecBatchIO &io, const DecPlanFrame *pf, const DecPlanChunk &c, bool *refused, int16_t *d_coef = nullptr) {
    tic_ctx::DecBatch &B = ctx->dbat;
    const uint32_t F = (uint32_t)c.count;
    std::vector<DecFrame> frames(F);
    uint32_t tiles = 0, wgs = 0;
    for (uint32_t k = 0; k < F; k++) {
        const DecPlanFrame &f = pf[k];
        DecFrame &d = frames[k];
        d.word0 = f.word0, d.nwords = f.nwords, d.last_mask = f.last_mask;
        d.stream_bits = d.fast_end = f.stream_bits;
        d.nranges = f.nranges, d.range0 = f.range0;
        d.tile0 = tiles, d.ntiles = entropy_decode_batch_tiles(f.nranges, c.range_bits);
        d.blk0 = f.blk0, d.nblocks = (uint32_t)f.nblk;
        d.wg0 = wgs, d.nwgs = entropy_decode_batch_wgs(f.nblk);
        d.pad_ = 0;
        if (d_coef) {
            memset(&d.idct, 0, sizeof d.idct);
            memcpy(d.idct.head, io.streams[f.index], 16); // (the sink stores a frame's rows only under the header its geometry came from)
        } else {
            d.idct = dec_idct_args(ctx, f.h, f.w, f.quality, -1, nullptr /* set below, when the pixel buffer exists */, (long)f.pitch, io.streams[f.index]);
        }
        tiles += d.ntiles, wgs += d.nwgs;
    }
    const DecUploadLayout up(F, tiles, wgs, c.words);
    int rc;
    rc = dbatch_grow(ctx, up.up_bytes, d_coef ? 0 : c.pix_bytes);
    if (rc) return rc;
    const size_t wb = dec_work_provision_bytes(F, c.ranges288, c.blocks);
    rc = B.ws.grow(ctx, wb, wb + wb / 4, 4 * (size_t)((tiles > wgs ? tiles : wgs) + 2), F, F < 256 ? 256 : 2 * (size_t)F);
    if (rc) return rc;
    BT_START();
    for (uint32_t k = 0; k < F && !d_coef; k++) frames[k].idct.out = B.d_pix + pf[k].pix_off;
    memcpy(B.h_in + up.o_frames, frames.data(), F * sizeof(DecFrame));
    uint32_t *tf = (uint32_t *)(B.h_in + up.o_tiles), *wf = (uint32_t *)(B.h_in + up.o_wgs);
    for (uint32_t k = 0; k < F; k++) {
        for (uint32_t t = 0; t < frames[k].ntiles; t++) tf[frames[k].tile0 + t] = k;
        for (uint32_t g = 0; g < frames[k].nwgs; g++) wf[frames[k].wg0 + g] = k;
    }
    for (uint32_t k = 0; k < F; k++) // (the bytes behind a stream's last word are never read: no need to clear them)
        memcpy(B.h_in + up.o_streams + (size_t)pf[k].word0 * 4, io.streams[pf[k].index], pf[k].len);
    rc = B.ws.begin(ctx, ctx->stream, F);
    if (rc) return rc;
    BT_STOP(0);
    BT_START();
    size_t work_held = B.ws.work.cap;
    if (const char *e = test_hook("TIC_DBATCH_WORK_CAP")) work_held = (size_t)atoll(e) < work_held ? (size_t)atoll(e) : work_held; // (tests: a launcher that refuses)
    if (!d_coef) {
        ctx->last_dbatch_range = c.range_bits;
        ctx->last_dbatch_work_used = dec_work_carve_bytes(F, c.ranges, c.blocks, c.range_bits);
        ctx->last_dbatch_work_held = work_held;
    }
    HIPCHK(ctx, hipMemcpyAsync(B.d_in, B.h_in, up.up_bytes, hipMemcpyHostToDevice, ctx->stream));
    const hipError_t le =
        d_coef ? entropy_decode_coef_gpu_batch(B.d_in + up.o_streams, (const DecFrame *)(B.d_in + up.o_frames), (const uint32_t *)(B.d_in + up.o_tiles),
                                               (const uint32_t *)(B.d_in + up.o_wgs), F, tiles, wgs, c.ranges, c.blocks, c.small_win, ctx->d_dec_luts, B.ws.work, work_held, B.ws.desc,
                                               B.ws.desc_words, B.ws.epoch, B.ws.h_status.d, c.range_bits, d_coef, ctx->stream)
               : entropy_decode_idct_gpu_batch(B.d_in + up.o_streams, (const DecFrame *)(B.d_in + up.o_frames), (const uint32_t *)(B.d_in + up.o_tiles),
                                               (const uint32_t *)(B.d_in + up.o_wgs), F, tiles, wgs, c.ranges, c.blocks, c.small_win, ctx->d_dec_luts, B.ws.work, work_held, B.ws.desc,
                                               B.ws.desc_words, B.ws.epoch, B.ws.h_status.d, c.range_bits, ctx->stream);
    if (le == hipErrorInvalidValue) {
        (void)hipGetLastError();
        *refused = true;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return TIC_OK;
    }
    HIPCHK(ctx, le);
    BT_STOP(1);
    return TIC_OK;
}

// The pixels come down: one copy into the caller's memory where the frames are dense and follow each other there (*direct), else one copy
// into pinned memory (dbatch_settle hands it out).
// (the direct copy is `total` bytes long, the device buffer's padding between two frames included: it may only cover bytes the caller gave away -
//  a frame of a whole number of 256 B has none behind it, elsewhere caps[] must reach to the next frame; an arena of frames at
//  256-byte aligned distances with caps[i] = h * w takes the pinned route, and the bytes between its frames stay the caller's)
// (shared by tic_decompress_batch and tic_decompress_batch_adaptive: Frame is a frame of either plan - index, h, w, pitch, pix_off)
extern "C++" template <class Frame> static int dbatch_pixels_down(tic_ctx *ctx, const DecBatchIO &io, const Frame *pf, size_t F, size_t pix_bytes, bool *direct) {
    tic_ctx::DecBatch &B = ctx->dbat;
    BT_START();
    bool dense = true;
    for (size_t k = 0; k < F && dense; k++) dense = pf[k].pitch == (size_t)pf[k].w;
    dense = dense && frames_are_one_arena(F, [&](size_t k) {
                return ArenaFrame{io.outs[pf[k].index], pf[k].pix_off, (size_t)pf[k].h * (size_t)pf[k].w, io.caps[pf[k].index]};
            });
    *direct = false;
    if (dense && ctx->auto_register) {
        uint8_t *const out0 = io.outs[pf[0].index];
        const size_t total = pf[F - 1].pix_off + (size_t)pf[F - 1].h * (size_t)pf[F - 1].w;
        bool pinned = host_pointer_is_pinned(out0) && host_pointer_is_pinned(out0 + total - 1);
        void *reg = nullptr;
        if (!pinned && total >= (256u << 10)) pinned = (reg = pin_range(out0, total)) != nullptr;
        if (pinned) {
            hipError_t e = hipMemcpyAsync(out0, B.d_pix, total, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            *direct = e == hipSuccess;
            if (!*direct) (void)hipGetLastError();
        }
        if (reg && hipHostUnregister(reg) != hipSuccess) (void)hipGetLastError();
    }
    if (!*direct) {
        const int rc = B.h_pix.grow(ctx, pix_bytes, pix_bytes + pix_bytes / 4);
        if (rc) return rc;
        HIPCHK(ctx, hipMemcpyAsync(B.h_pix, B.d_pix, pix_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    BT_STOP(2);
    return TIC_OK;
}
static int dbatch_download(tic_ctx *ctx, const DecBatchIO &io, const DecPlanFrame *pf, const DecPlanChunk &c, bool *direct) {
    const int rc = dbatch_pixels_down(ctx, io, pf, (size_t)c.count, c.pix_bytes, direct);
    if (rc) return rc;
    ctx->last_dbatch_chunks++;
    ctx->last_dbatch_direct += *direct ? c.count : 0;
    return TIC_OK;
}

// The complete frames (good[k]) leave the pinned buffer on a few threads, unless the download was direct.
extern "C++" template <class Frame> static void dbatch_hand_out(tic_ctx *ctx, const DecBatchIO &io, const Frame *pf, int F, size_t pix_bytes, bool direct, const std::vector<char> &good) {
    tic_ctx::DecBatch &B = ctx->dbat;
    BT_START();
    if (!direct) {
        const int T = pix_bytes < (2u << 20) || F < 2 ? 1 : (F < 8 ? F : 8);
        run_strided(F, T, [ctx]() { bind_pipeline_thread(ctx); }, [&](int k) {
            const Frame &f = pf[k];
            if (good[(size_t)k]) copy_rows(io.outs[f.index], (size_t)f.w, B.h_pix + f.pix_off, (ptrdiff_t)f.pitch, f.h, f.w);
        });
    }
    BT_STOP(4);
}

// What the kernels report, frame by frame (dec_status_complete): a frame that is complete counts, any other goes to `later`; then the complete
// ones are handed out.
static void dbatch_settle(tic_ctx *ctx, const DecBatchIO &io, const DecPlanFrame *pf, const DecPlanChunk &c, bool direct, std::vector<int> *later) {
    tic_ctx::DecBatch &B = ctx->dbat;
    const int F = c.count;
    std::vector<char> good((size_t)F);
    for (int k = 0; k < F; k++) {
        good[(size_t)k] = dec_status_complete(B.ws.h_status[k], io.streams[pf[k].index], pf[k].nblk);
        if (good[(size_t)k]) ctx->last_dbatch_frames++;
        else later->push_back(pf[k].index);
    }
    dbatch_hand_out(ctx, io, pf, F, c.pix_bytes, direct, good);
}

// decompress() of MANY streams at once (the mirror of tic_compress_batch; the reference's benchmark loop, tests/benchmark.py:12-23, decodes
// 49 streams of 512 x 512 per quality one call after the other: 94-105 us each, launch and copy latency).  The streams of a chunk are packed
// into one pinned buffer behind their descriptors and go up in ONE copy; ONE measure launch and ONE fused launch decode all of them (the
// batch forms of the two kernels: every wave and workgroup looks up its frame, nothing crosses a frame - the DC sum starts over with every
// frame, codec.py:53); the pixels of the chunk come down in ONE copy - straight into the caller's buffers where they follow each other in
// memory (pinned for the call by one hipHostRegister), else through the context's pinned buffer and a few copy threads.
// Frame i: what tic_decompress(ctx, streams[i], lens[i], outs[i], caps[i]) gives, geometry in hs[i] / ws[i] (either may be null).  A frame the
// batch kernels do not take (a short or damaged stream, a C-encoder stream, anything the device decoder flags) is decoded by that very
// call afterwards - and so is every frame of a chunk the batch launcher refuses (its host-side checks, before any kernel: a work buffer
// too small for the chunk) or that fails on the way.  Errors: headers are checked before any work (the first bad frame's error, nothing
// decoded); an error while decoding is the first one met, and every frame that did not fail itself is complete: an error inside a chunk
// ends the chunks, not the call - the frames it leaves still go to the single-frame call.
int tic_decompress_batch(tic_ctx *ctx, const uint8_t *const *streams, const size_t *lens, int n, uint8_t *const *outs, const size_t *caps, int *hs, int *ws) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (n < 0 || (n > 0 && (!streams || !lens || !outs || !caps))) return set_err(ctx, TIC_E_ARG, "bad batch arguments");
    ctx->last_dbatch_frames = ctx->last_dbatch_fallback = ctx->last_dbatch_chunks = ctx->last_dbatch_direct = 0;
    ctx->last_dbatch_range = 0;
    ctx->last_dbatch_work_used = ctx->last_dbatch_work_held = 0;
    ctx->bt = BatchTrace(); // (tic_last_batch_phases: [0] packing the upload buffer, [1] enqueue, [2] wait + download, [4] hand-out, [5] single-frame calls)
    if (n == 0) return TIC_OK;
    // ---- the checks of tic_decompress, for every frame, before any work
    std::vector<DecPlanIn> in((size_t)n);
    std::vector<int> later; // frames for the single-frame call
    for (int i = 0; i < n; i++) {
        StreamHead sh;
        const int rc = check_header(ctx, streams[i], lens[i], &sh, i);
        if (rc) return rc;
        const size_t nb = num_blocks(sh.h, sh.w);
        if (nb && (!outs[i] || (size_t)sh.h * (size_t)sh.w > caps[i])) return set_err(ctx, TIC_E_SPACE, "frame %d: output buffer too small", i);
        if (hs) hs[i] = sh.h;
        if (ws) ws[i] = sh.w;
        in[(size_t)i] = {sh.h, sh.w, sh.quality, lens[i],
                         nb != 0 && sh.scaled_exp < 0 && device_decoder_takes(nb, lens[i]) && !test_hook("TIC_DECODE_HOST") && !test_hook("TIC_DECODE_SERIAL")};
        if (nb && !in[(size_t)i].takes) later.push_back(i);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = ensure_dec_tables(ctx);
    if (rc) return rc;
    // ---- the plan: chunks of frames in order, inside the limits (one 512 x 512 benchmark set - 49 frames, 12.8 MB of pixels - is one chunk;
    // sixteen 4096^2 frames are one)
    DecPlanLimits lim = {(size_t)96 << 20, (size_t)288 << 20, 1024};
    if (const char *e = test_hook("TIC_DBATCH_CHUNK")) lim.frames = atoi(e) >= 1 && atoi(e) <= 1024 ? atoi(e) : lim.frames; // (tests: several chunks)
    const DecPlan plan = plan_decode_batch(in.data(), n, lim);
    // ---- the chunks, one after the other
    const DecBatchIO io = {streams, lens, outs, caps};
    int result = TIC_OK;
    std::string first_err; // (the text of an error inside a chunk: the single-frame calls behind it write their own)
    auto fail = [&](int rc) { if (result == TIC_OK) result = rc; };
    for (const DecPlanChunk &c : plan.chunks) {
        const DecPlanFrame *pf = &plan.frames[(size_t)c.first];
        bool refused = false, direct = false;
        int crc = dbatch_enqueue(ctx, io, pf, c, &refused);
        if (crc == TIC_OK && !refused) crc = dbatch_download(ctx, io, pf, c, &direct);
        if (crc == TIC_OK && !refused) {
            dbatch_settle(ctx, io, pf, c, direct, &later);
            continue;
        }
        // refused, or ended early by a failed allocation, copy or launch (every such way out lies in front of the status words: none of the
        // chunk's frames is counted or queued yet): its frames go one by one.  An error is the first and stands (its text too: kept below); no
        // further chunk is tried, what they would have held goes one by one as well
        const size_t last = crc != TIC_OK ? plan.frames.size() : (size_t)(c.first + c.count);
        for (size_t k = (size_t)c.first; k < last; k++) later.push_back(plan.frames[k].index);
        if (crc == TIC_OK) continue;
        fail(crc);
        first_err = ctx->err;
        break;
    }
    // ---- frames the batch did not take, or did not finish: the single-frame call, with everything it knows (second run, host decoders)
    std::sort(later.begin(), later.end());
    for (int i : later) {
        const int rc = tic_decompress(ctx, streams[i], lens[i], outs[i], caps[i]);
        ctx->last_dbatch_fallback++;
        if (rc != TIC_OK) {
            if (result == TIC_OK) {
                const std::string m = ctx->err;
                set_err(ctx, rc, "frame %d: %s", i, m.c_str());
            }
            fail(rc);
        }
    }
    if (!first_err.empty()) ctx->err = first_err;
    return result;
}

// How the last tic_decompress_batch went: frames decoded by the batch kernels, frames that took the single-frame call (too short for the
// device decoder, C-encoder streams, anything flagged), chunks, frames whose pixels were copied straight into the caller's memory.
int tic_last_decompress_batch(tic_ctx *ctx, int *batch_frames, int *single_frames, int *chunks, int *direct_frames) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (batch_frames) *batch_frames = ctx->last_dbatch_frames;
    if (single_frames) *single_frames = ctx->last_dbatch_fallback;
    if (chunks) *chunks = ctx->last_dbatch_chunks;
    if (direct_frames) *direct_frames = ctx->last_dbatch_direct;
    return TIC_OK;
}

// ... and the work buffer of the last chunk it handed to the batch launcher: the chunk's range (stream bits per lane, the largest of its
// frames' choices), the bytes the launcher carves for it and the bytes the context held for it (0 / 0 / 0: no chunk).  Any pointer may be null.
int tic_last_decompress_batch_work(tic_ctx *ctx, int *range_bits, size_t *work_used, size_t *work_held) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (range_bits) *range_bits = ctx->last_dbatch_range;
    if (work_used) *work_used = ctx->last_dbatch_work_used;
    if (work_held) *work_held = ctx->last_dbatch_work_held;
    return TIC_OK;
}

// The device decoder's work buffer for `nframes` streams of `total_ranges` ranges of `range_bits` bits and `total_blocks` blocks in all: the
// launchers' own carve-up (tic_entropy_dec_gpu.h dec_work_carve_bytes); 0 for a range the decoder does not take.
size_t tic_decode_work_bytes(size_t nframes, size_t total_ranges, size_t total_blocks, int range_bits) {
    return dec_range_ok(range_bits) ? dec_work_carve_bytes(nframes, total_ranges, total_blocks, range_bits) : 0;
}

// decompress() with stream and pixels both resident in HBM (the counterpart of tic_compress_dev): only the 16-byte header, the
// status and - for the blocks that start in the stream's last 2048 bits - a few hundred bytes cross PCIe.  Short streams and streams
// the device decoder gives up on come down to the host decoder and their coefficients go back up (the reference's behaviour on
// malformed streams lives there).  d_out: h rows of w pixels, out_stride bytes apart.
int tic_decompress_dev(tic_ctx *ctx, const void *d_stream, size_t len, void *d_out, ptrdiff_t out_stride, size_t out_cap, int *h_out, int *w_out) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    ctx->last_decode_giveup = 0;
    ctx->last_decode_tries = 0;
    ctx->last_decode_guess = 0;
    if (!d_stream && len) return set_err(ctx, TIC_E_ARG, "null stream pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (len < 16) return set_err(ctx, TIC_E_STREAM, "stream shorter than the 16-byte header");
    // Geometry and quality are in the stream's header - in device memory; a synchronous 16-byte read in front of the first launch is a
    // sixth of the call for a 4096^2 stream.  A long stream is therefore decoded on a GUESS - the header of the stream this context decoded
    // last (frames of a sequence, the images of a batch) - and the first kernel echoes the real header into the status words: when it is
    // the guessed one, everything the run produced stands, without the read; when it is not (or the guess does not fit this call's
    // buffers), the header is read and the stream decoded again.  A run on a wrong guess writes NO pixel: the fused kernel compares
    // the stream's first 16 bytes with the header its geometry came from before it stores anything (DecIdctArgs::head), so nothing
    // outside the real h x w is ever touched - a destination that is a window of a larger surface keeps its neighbours
    // (test_decompress_dev_wrong_guess_writes_nothing_outside_the_image).  (On an error return the contents of d_out are unspecified.)
    // ... and only after two streams in a row came with the same header (dec_head_streak): alternating geometries never pay for a guess,
    // a change behind a run of equal frames pays once.  tic_set_decode_guess(ctx, 0) turns the guessing off.
    const bool may_guess = ctx->dec_guess_on && ctx->dec_head_valid && ctx->dec_head_streak >= 1 && device_decoder_takes(kDevDecodeMinBlocks, len) &&
                           !test_hook("TIC_DECODE_NO_GUESS");
    for (int attempt = may_guess ? 0 : 1; attempt < 2; attempt++) {
        const bool guess = attempt == 0;
        uint8_t head[16] = {0};
        if (guess)
            memcpy(head, ctx->dec_head, 16);
        else
            HIPCHK(ctx, hipMemcpy(head, d_stream, 16, hipMemcpyDeviceToHost));
        StreamHead sh;
        int rc = check_header(ctx, head, 16, &sh); // (a cached header passed these checks when it was cached)
        if (rc) return rc;
        const int h = sh.h, w = sh.w;
        const size_t n = num_blocks(h, w);
        if (guess && (n == 0 || out_stride < (ptrdiff_t)w || !d_out || (size_t)(h - 1) * (size_t)out_stride + (size_t)w > out_cap)) { // the guess does not fit this call
            ctx->last_decode_guess = -1;
            continue;
        }
        if (!guess) {
            if (h_out) *h_out = h;
            if (w_out) *w_out = w;
            if (n == 0) return TIC_OK;
            if (out_stride < (ptrdiff_t)w) return set_err(ctx, TIC_E_ARG, "row stride %td smaller than the width %d", out_stride, w);
            if (!d_out || (size_t)(h - 1) * (size_t)out_stride + (size_t)w > out_cap) return set_err(ctx, TIC_E_SPACE, "output buffer too small");
        }
        bool done = false, held = false;
        rc = decode_on_device(ctx, (const uint8_t *)d_stream, len, sh, (uint8_t *)d_out, true, (size_t)out_stride, &done, head, true, guess,
                              guess ? &held : nullptr);
        if (rc) return rc;
        if (guess) {
            ctx->last_decode_guess = held ? 1 : -1;
            if (!held) continue; // another header (or the device decoder does not take this stream): read it
            if (h_out) *h_out = h;
            if (w_out) *w_out = w;
        }
        if (done) {
            ctx->last_decode_path = 1;
            ctx->dec_head_streak = ctx->dec_head_valid && memcmp(ctx->dec_head, head, 16) == 0 ? (ctx->dec_head_streak < 1000 ? ctx->dec_head_streak + 1 : 1000) : 0;
            memcpy(ctx->dec_head, head, 16);
            ctx->dec_head_valid = true;
            return TIC_OK;
        }
        std::vector<uint8_t> host(len);
        HIPCHK(ctx, hipMemcpy(host.data(), d_stream, len, hipMemcpyDeviceToHost));
        return decode_on_host(ctx, host.data(), len, sh, (uint8_t *)d_out, true, (size_t)out_stride);
    }
    return set_err(ctx, TIC_E_ARG, "tic_decompress_dev: unreachable");
}

// tic_decompress_dev, asynchronously.  A long stream is LAUNCHED on the guess of its header (tic_decompress_dev above) on a stream of
// the ticket's own and the call returns; tic_decompress_async_result waits for it and checks what the kernels reported - the header they
// saw, nothing unusual on the chain, every block produced; if any of that fails (another header, a damaged or cut stream) the stream is
// decoded again there, synchronously, by tic_decompress_dev itself, so the outcome of a ticket is always that of the synchronous call.
// A call that cannot be launched on a guess (no stream decoded yet on this context, a short stream, a destination the kernels cannot
// write directly or the guessed geometry does not fit) runs synchronously right away and its ticket only carries the outcome.
int tic_decompress_dev_async(tic_ctx *ctx, const void *d_stream, size_t len, void *d_out, ptrdiff_t out_stride, size_t out_cap, long long *ticket) {
    TIC_LOCK(ctx);
    if (!ctx || !ticket) return TIC_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long long t = ctx->dec_async_next;
    tic_ctx::DecSlot &sl = ctx->dec_slots[t % kDecSlots];
    if (sl.ticket >= 0) return set_err(ctx, TIC_E_ARG, "%d asynchronous decodes are open: collect results (tic_decompress_async_result) first", kDecSlots);
    sl.launched = false;
    sl.d_stream = d_stream;
    sl.len = len;
    sl.d_out = d_out;
    sl.out_stride = out_stride;
    sl.out_cap = out_cap;
    StreamHead sh = {0, 0, 0, -1};
    bool launch = ctx->dec_guess_on && ctx->dec_head_valid && ctx->dec_head_streak >= 1 && d_stream && d_out && ((uintptr_t)d_stream & 3u) == 0 &&
                  out_stride % 8 == 0 && (uintptr_t)d_out % 8 == 0 && ctx->d_dec_luts && !test_hook("TIC_DECODE_NO_GUESS") && !test_hook("TIC_DECODE_HOST") &&
                  !test_hook("TIC_DECODE_SERIAL") && check_header(ctx, ctx->dec_head, 16, &sh) == TIC_OK; // (it passed when it was cached)
    const int h = sh.h, w = sh.w;
    const size_t n = launch ? num_blocks(h, w) : 0;
    launch = launch && device_decoder_takes(n, len) && out_stride >= (ptrdiff_t)w && (size_t)(h - 1) * (size_t)out_stride + (size_t)w <= out_cap;
    if (launch) {
        if (!sl.stream) HIPCHK(ctx, hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
        if (!sl.done) HIPCHK(ctx, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
        if (!ctx->dec_order) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->dec_order, hipEventDisableTiming));
        const size_t wb = entropy_decode_gpu_work_bytes(len, n);
        int rc = sl.ws.grow(ctx, wb, wb, entropy_decode_gpu_desc_words(len, n), 1, 1); // (nothing of this slot is in flight: its ticket is closed)
        if (rc) return rc;
        rc = sl.ws.begin(ctx, sl.stream, 1);
        if (rc) return rc;
        // (the guess: pixels are written only if the stream really starts with it)
        const DecIdctArgs ia = dec_idct_args(ctx, h, w, sh.quality, sh.scaled_exp, (uint8_t *)d_out, (long)out_stride, ctx->dec_head);
        // behind everything queued on the context's stream so far (the stream may just have been written there: tic_compress_dev_async)
        HIPCHK(ctx, hipEventRecord(ctx->dec_order, ctx->stream));
        HIPCHK(ctx, hipStreamWaitEvent(sl.stream, ctx->dec_order, 0));
        HIPCHK(ctx, entropy_decode_idct_gpu(d_stream, len, n, ctx->d_dec_luts, sl.ws.work, sl.ws.work.cap, sl.ws.desc, sl.ws.desc_words, sl.ws.epoch, ia,
                                            sl.ws.h_status.d, decode_range_bits(len, n), 0, sl.stream));
        HIPCHK(ctx, hipEventRecord(sl.done, sl.stream));
        memcpy(sl.head, ctx->dec_head, 16);
        sl.n = n;
        sl.h = h;
        sl.w = w;
        sl.launched = true;
    } else {
        sl.rc = tic_decompress_dev(ctx, d_stream, len, d_out, out_stride, out_cap, &sl.h, &sl.w);
    }
    sl.ticket = t;
    ctx->dec_async_next = t + 1;
    *ticket = t;
    return TIC_OK;
}

// Outcome of an asynchronous decode: what tic_decompress_dev would have returned for the same arguments (and *h_out / *w_out, either
// may be null).  wait == 0: TIC_E_BUSY while the frame is still in flight.  A ticket is closed by the call that returns anything else.
int tic_decompress_async_result(tic_ctx *ctx, long long ticket, int wait, int *h_out, int *w_out) {
    TIC_LOCK(ctx);
    if (!ctx || ticket < 0) return TIC_E_ARG;
    tic_ctx::DecSlot &sl = ctx->dec_slots[ticket % kDecSlots];
    if (sl.ticket != ticket) return set_err(ctx, TIC_E_ARG, "decode ticket %lld is not open", ticket);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (sl.launched) {
        {   // (as tic_async_result: a failing event call closes the ticket too)
            const hipError_t q = wait ? hipEventSynchronize(sl.done) : hipEventQuery(sl.done);
            if (!wait && q == hipErrorNotReady) return TIC_E_BUSY;
            if (q != hipSuccess) sl.ticket = -1;
            HIPCHK(ctx, q);
        }
        DecStatus st;
        memcpy(&st, sl.ws.h_status, sizeof st); // (host-mapped: the slot's stream has drained)
        if (dec_status_complete(st, sl.head, sl.n)) {
            ctx->last_decode_path = 1;
            ctx->last_decode_giveup = 0;
            ctx->last_decode_guess = 1;
            ctx->last_decode_tries = 1;
            sl.rc = TIC_OK;
        } else { // another header, or something unusual in the stream: the synchronous call settles it (and overwrites what this run wrote)
            const bool on = ctx->dec_guess_on;
            ctx->dec_guess_on = false; // (the launch on the guess is what just failed: this time the header is read first)
            sl.rc = tic_decompress_dev(ctx, sl.d_stream, sl.len, sl.d_out, sl.out_stride, sl.out_cap, &sl.h, &sl.w);
            ctx->dec_guess_on = on;
            ctx->last_decode_guess = -1;
        }
    }
    sl.ticket = -1;
    if (h_out) *h_out = sl.h;
    if (w_out) *w_out = sl.w;
    if (test_hooks_enabled() && sl.rc == TIC_OK) // (hooks build: what became of the ticket, where a test can read it)
        set_err(ctx, TIC_OK, "decode ticket %lld: slot %d, launched %d, guess held %d, epoch %u", ticket, (int)(ticket % kDecSlots), sl.launched ? 1 : 0,
                sl.launched && ctx->last_decode_guess == 1 ? 1 : 0, sl.ws.epoch);
    return sl.rc;
}

// ---- self test hook (used by tests/ only; not part of the drop-in surface) --------------------------------
int tic_selftest_transpose(tic_ctx *ctx, const void *host_in, void *host_dpp, void *host_ref, int nthreads) {
    TIC_LOCK(ctx);
    if (!ctx || nthreads <= 0 || nthreads % 256) return TIC_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    void *d_in, *d_a, *d_b;
    size_t bytes = (size_t)nthreads * 8;
    HIPCHK(ctx, hipMalloc(&d_in, bytes));
    HIPCHK(ctx, hipMalloc(&d_a, bytes));
    HIPCHK(ctx, hipMalloc(&d_b, bytes));
    HIPCHK(ctx, hipMemcpy(d_in, host_in, bytes, hipMemcpyHostToDevice));
    HIPCHK(ctx, launch_selftest_transpose(d_in, d_a, d_b, nthreads, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(host_dpp, d_a, bytes, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(host_ref, d_b, bytes, hipMemcpyDeviceToHost));
    (void)hipFree(d_in);
    (void)hipFree(d_a);
    (void)hipFree(d_b);
    return TIC_OK;
}

// ---- per-image Huffman tables: compress(..., auto_generate_huffman_table=True), codec.py:133-164 / huffman.py:101-194 ----------------
size_t tic_compress_adaptive_bound(int h, int w) {
    // header, the largest table, and per block at most 65 symbols (DC, 63 AC, EOB) of at most kAdaptMaxSymbolBits each
    return 16 + kAdaptMaxTableBytes + num_blocks(h, w) * (65 * kAdaptMaxSymbolBits / 8) + 8;
}

int tic_huffman_table_build(const uint64_t *dc_count, const uint64_t *dc_first, const uint64_t *ac_count, const uint64_t *ac_first,
                            uint64_t *dc_code, uint8_t *dc_len, uint64_t *ac_code, uint8_t *ac_len, uint8_t *table, size_t table_cap,
                            size_t *table_bits) {
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "64-bit words");
    return huffman_table_build((const unsigned long long *)dc_count, (const unsigned long long *)dc_first, (const unsigned long long *)ac_count,
                               (const unsigned long long *)ac_first, (unsigned long long *)dc_code, dc_len, (unsigned long long *)ac_code, ac_len,
                               table, table_cap, table_bits);
}

// Statistics, table, packing of the n blocks in ctx->d_coef; the stream goes to the caller's host buffer.  One read-back in between:
// the 4.4 KB of statistics the host builds the table from (it also yields the stream's exact length, checked against `cap` before
// anything is packed).
static int adaptive_encode_dev(tic_ctx *ctx, size_t n, int h, int w, int quality, uint8_t *out, size_t cap, size_t *out_len) {
    const size_t a = align_up(sizeof(AdaptStats), 256), b = align_up(sizeof(HuffWide), 256);
    int rc = ctx->d_adapt_stats.grow(ctx, a + b + 256); // (statistics, table and error word: all three rewritten per call)
    if (rc) return rc;
    ctx->d_adapt_tab = (HuffWide *)((char *)ctx->d_adapt_stats + a);
    ctx->d_adapt_err = (uint32_t *)((char *)ctx->d_adapt_stats + a + b);
    rc = ctx->d_adapt_work.grow(ctx, adaptive_work_bytes(n));
    if (rc) return rc;
    AdaptStats *st = ctx->d_adapt_stats;
    HIPCHK(ctx, hipMemsetAsync(st, 0, sizeof(AdaptStats), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(st->first, 0xff, sizeof(st->first), ctx->stream));
    HIPCHK(ctx, adaptive_stats((const int16_t *)ctx->d_coef, n, st, ctx->stream));
    AdaptStats hs;
    HIPCHK(ctx, hipMemcpyAsync(&hs, st, sizeof hs, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (hs.err) return set_err(ctx, TIC_E_RANGE, "a DC category or AC size above 15 (write_huffman_table has 4 bits for it, codec.py:73-84)");
    std::vector<uint8_t> head(16 + kAdaptMaxTableBytes, 0);
    write_header(head.data(), h, w, quality);
    head[12] = 0x80; // write_uint(1 << 31, 32): most significant bit first (codec.py:111)
    unsigned long long dc_code[16], ac_code[256];
    uint8_t dc_len[16], ac_len[256];
    size_t tbits = 0;
    rc = huffman_table_build(hs.count + kAdaptDcBin, hs.first + kAdaptDcBin, hs.count, hs.first, dc_code, dc_len, ac_code, ac_len,
                                 head.data() + 16, kAdaptMaxTableBytes, &tbits);
    if (rc == TIC_E_RANGE)
        return set_err(ctx, rc, "a Huffman code of this frame and its value bits exceed %d bits", kAdaptMaxSymbolBits);
    if (rc) return set_err(ctx, rc, "Huffman table build failed");
    HuffWide tab;
    for (int i = 0; i < kAdaptBins; i++) {
        const bool dc = i >= kAdaptDcBin;
        tab.code[i] = dc ? dc_code[i - kAdaptDcBin] : ac_code[i];
        tab.len[i] = dc ? dc_len[i - kAdaptDcBin] : ac_len[i];
    }
    const unsigned long long base = 128 + tbits, total = adaptive_stream_bits(hs.count + kAdaptDcBin, hs.count, dc_len, ac_len, tbits);
    const size_t bytes = (size_t)((total + 7) / 8), words = (size_t)((total + 31) / 32);
    if (bytes > cap) {
        *out_len = bytes;
        return set_err(ctx, TIC_E_SPACE, "output buffer too small (%zu bytes needed, %zu given)", bytes, cap);
    }
    rc = ctx->d_adapt_out.grow(ctx, words * 4);
    if (rc) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->d_adapt_out, 0, words * 4, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_adapt_out, head.data(), (size_t)((base + 7) / 8), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_adapt_tab, &tab, sizeof tab, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_adapt_err, 0, 4, ctx->stream));
    HIPCHK(ctx, adaptive_pack((const int16_t *)ctx->d_coef, n, ctx->d_adapt_tab, ctx->d_adapt_work, ctx->d_adapt_out, base, words,
                              ctx->d_adapt_err, ctx->stream));
    uint32_t herr = 0;
    HIPCHK(ctx, hipMemcpyAsync(&herr, ctx->d_adapt_err, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->d_adapt_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (herr) return set_err(ctx, TIC_E_HIP, "packing reached past the stream's computed length (statistics and packing disagree)");
    *out_len = bytes;
    return TIC_OK;
}

int tic_compress_adaptive(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, int quality, uint8_t *out, size_t cap,
                          size_t *out_len) {
    TIC_LOCK(ctx);
    int rc = check_stream_geometry(ctx, h, w, row_stride, quality);
    if (rc) return rc;
    if (!out || !out_len) return set_err(ctx, TIC_E_ARG, "null output pointer");
    const size_t n = num_blocks(h, w);
    if (n == 0) return set_err(ctx, TIC_E_ARG, "an image without blocks has no symbols to build a table from (the reference raises IndexError)");
    if (!image) return set_err(ctx, TIC_E_ARG, "null image pointer");
    size_t pitch = 0;
    rc = upload_image(ctx, image, h, w, row_stride, n, &pitch);
    if (rc) return rc;
    DctqArgs a = make_args(ctx, ctx->d_img, h, w, (ptrdiff_t)pitch, quality, ctx->d_coef);
    HIPCHK(ctx, launch_dctq(a, 2, ctx->stream));
    return adaptive_encode_dev(ctx, n, h, w, quality, out, cap, out_len);
}

int tic_entropy_encode_adaptive(tic_ctx *ctx, const int16_t *coeffs_zz, int h, int w, int quality, uint8_t *out, size_t cap,
                                size_t *out_len) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (h < 0 || w < 0) return set_err(ctx, TIC_E_ARG, "negative image size");
    if (quality < 1 || quality > 99) return set_err(ctx, TIC_E_QUALITY, "quality %d outside 1..99", quality);
    if (!out || !out_len) return set_err(ctx, TIC_E_ARG, "null output pointer");
    const size_t n = num_blocks(h, w);
    if (n == 0) return set_err(ctx, TIC_E_ARG, "an image without blocks has no symbols to build a table from (the reference raises IndexError)");
    if (!coeffs_zz) return set_err(ctx, TIC_E_ARG, "null coefficient pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = ensure_scratch(ctx, 0, n * 128);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_coef, coeffs_zz, n * 128, hipMemcpyHostToDevice, ctx->stream));
    return adaptive_encode_dev(ctx, n, h, w, quality, out, cap, out_len);
}

// ---- adaptive batches: per-image tables for frames of any sizes and qualities in one call (tic_compress_batch_adaptive_v) ----------------------
// The mixed batch's plan, slots and pipeline (plan_mixed_batch, enqueue_on_slot, device_entropy_pipeline) with the adaptive encoder's two device
// halves in descriptor form (adaptive_stats_v, adaptive_pack_v) around the host's table build:
//   enqueue (calling thread)  upload, transform runs, the chunk's frame table, statistics (the launch resets them), ONE copy of the chunk's
//                             statistics into the slot's pinned mirror, the slot's `done` event;
//   read (second thread)      per frame the table (huffman_table_build) and the exact stream length from counts x lengths; stream areas from
//                             those lengths; ONE upload of frame table, code tables and headers + serialized tables; bits / scan / write; the
//                             read-back of every stream's own bytes into the pinned landing buffer; `rb_done`;
//   hand-out (third thread)   hand_out_chunk_v.
// A frame whose stream does not fit the caller's buffer is not packed: its out_lens entry holds the need and the call ends in TIC_E_SPACE.
struct AdaptCall {
    const int16_t *const *coeffs; // the coefficient entry's frames (null: `io.images` are pixels)
    MixedCall io;
    int short_frames;             // frames left unwritten for want of space (the reading thread counts; read behind batch_end's join)
};

struct AdaptSlotView { // a slot's adaptive buffers as chunk of `count` frames carves them
    AdaptSlotLayout l;
    AdaptStats *h_stats, *d_stats;
    AdaptFrameTable *h_frames, *d_frames;
    EntropyFrameTable *h_rb, *d_rb;
    HuffWide *h_tabs, *d_tabs;
    uint8_t *h_heads, *d_heads;
    uint32_t *h_err, *d_err;
};
static AdaptSlotView adapt_view(const Slot &s, size_t count, size_t nblk, size_t ngroups) {
    AdaptSlotView v;
    v.l = adaptive_slot_layout(count, nblk, ngroups);
    v.h_stats = (AdaptStats *)(s.h_adapt + v.l.stats), v.d_stats = (AdaptStats *)(s.d_adapt + v.l.stats);
    v.h_frames = (AdaptFrameTable *)(s.h_adapt + v.l.frames), v.d_frames = (AdaptFrameTable *)(s.d_adapt + v.l.frames);
    v.h_rb = (EntropyFrameTable *)(s.h_adapt + v.l.rb_frames), v.d_rb = (EntropyFrameTable *)(s.d_adapt + v.l.rb_frames);
    v.h_tabs = (HuffWide *)(s.h_adapt + v.l.tabs), v.d_tabs = (HuffWide *)(s.d_adapt + v.l.tabs);
    v.h_heads = (uint8_t *)(s.h_adapt + v.l.heads), v.d_heads = (uint8_t *)(s.d_adapt + v.l.heads);
    v.h_err = (uint32_t *)(s.h_adapt + v.l.err), v.d_err = (uint32_t *)(s.d_adapt + v.l.err);
    return v;
}

// Every slot holds the largest chunk's adaptive buffers (a frame's workgroups are rounded up: at most one more per frame).
static int ensure_adapt_slots(tic_ctx *ctx, const MixedPlan &p) {
    const AdaptSlotLayout l = adaptive_slot_layout((size_t)p.max_count, p.max_nblk, p.max_nblk / kAdaptGroupBlocks + (size_t)p.max_count);
    for (auto &sl : ctx->bslots) {
        int rc = sl.d_adapt.grow(ctx, l.end);
        if (rc == TIC_OK) rc = sl.h_adapt.grow(ctx, l.upload_end);
        if (rc) return rc;
    }
    return TIC_OK;
}

// The read stage of an adaptive chunk (see above).  Only this slot's buffers are written.
static int adaptive_pack_chunk(tic_ctx *ctx, const MixedPlan &p, Slot &s, hipStream_t st, AdaptCall &call) {
    BT_START();
    const hipError_t ev = hipEventSynchronize(s.done);
    BT_STOP(2);
    if (ev != hipSuccess) return set_err(ctx, TIC_E_HIP, "batch chunk failed");
    BT_START();
    const MixedFrame *fr = &p.frames[(size_t)s.first];
    const int count = s.count;
    size_t nblk = 0, ngroups = 0;
    for (int k = 0; k < count; k++) nblk += fr[k].nblk, ngroups += (fr[k].nblk + kAdaptGroupBlocks - 1) / kAdaptGroupBlocks;
    const AdaptSlotView v = adapt_view(s, (size_t)count, nblk, ngroups);
    unsigned long long total_bits[kEntropyMaxFrames];
    uint32_t base_bits[kEntropyMaxFrames];
    for (int k = 0; k < count; k++) {
        const MixedFrame &f = fr[k];
        const AdaptStats &hs = v.h_stats[k];
        if (hs.err)
            return set_err(ctx, TIC_E_RANGE, "frame %d: a DC category or AC size above 15 (write_huffman_table has 4 bits for it, codec.py:73-84)", f.index);
        uint8_t *head = v.h_heads + (size_t)k * kAdaptHeadStride;
        memset(head, 0, kAdaptHeadStride);
        write_header(head, f.h, f.w, f.quality);
        head[12] = 0x80; // write_uint(1 << 31, 32): most significant bit first (codec.py:111)
        unsigned long long dc_code[16], ac_code[256];
        uint8_t dc_len[16], ac_len[256];
        size_t tbits = 0;
        const int rc = huffman_table_build(hs.count + kAdaptDcBin, hs.first + kAdaptDcBin, hs.count, hs.first, dc_code, dc_len, ac_code, ac_len, head + 16,
                                           kAdaptMaxTableBytes, &tbits);
        if (rc == TIC_E_RANGE) return set_err(ctx, rc, "frame %d: a Huffman code of this frame and its value bits exceed %d bits", f.index, kAdaptMaxSymbolBits);
        if (rc) return set_err(ctx, rc, "frame %d: Huffman table build failed", f.index);
        HuffWide &tab = v.h_tabs[k];
        for (int i = 0; i < kAdaptBins; i++) {
            const bool dc = i >= kAdaptDcBin;
            tab.code[i] = dc ? dc_code[i - kAdaptDcBin] : ac_code[i];
            tab.len[i] = dc ? dc_len[i - kAdaptDcBin] : ac_len[i];
        }
        base_bits[k] = (uint32_t)(128 + tbits);
        const unsigned long long total = adaptive_stream_bits(hs.count + kAdaptDcBin, hs.count, dc_len, ac_len, tbits);
        const size_t bytes = (size_t)((total + 7) / 8);
        call.io.out_lens[f.index] = bytes;
        const bool fits = bytes <= call.io.caps[f.index];
        if (!fits) call.short_frames++;
        total_bits[k] = fits ? total : 0ull;
        s.h_lens[k] = fits ? bytes : 0ull; // (nothing of an unpacked frame is read back or handed out)
    }
    size_t stream_bytes = 0, landing = 0, maxlen = 0;
    assign_adaptive_streams(v.h_frames, count, total_bits, base_bits, &stream_bytes);
    for (int k = 0; k < count; k++) {
        v.h_rb->rec[k].out_off = v.h_frames->rec[k].out_off; // (all the read-back kernel reads of its table)
        s.h_rb_off[k] = landing;
        landing += align_up((size_t)s.h_lens[k], 64);
        maxlen = std::max(maxlen, (size_t)s.h_lens[k]);
    }
    // (nothing is in flight on this slot's buffers: its previous chunk was handed out before this one claimed it)
    int rc = s.d_streams.grow(ctx, stream_bytes, stream_bytes + stream_bytes / 4);
    if (rc == TIC_OK) rc = s.pin_out.grow(ctx, landing, landing + landing / 4);
    if (rc) return rc;
    *v.h_err = 0u;
    hipError_t e = stream_bytes ? hipMemsetAsync(s.d_streams, 0, stream_bytes, st) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_adapt + v.l.err, s.h_adapt + v.l.err, v.l.upload_end - v.l.err, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = adaptive_pack_v((const int16_t *)s.d_coef, v.d_frames, count, ngroups, v.d_tabs, v.d_heads, (uint32_t *)(s.d_adapt + v.l.bbits),
                            (unsigned long long *)(s.d_adapt + v.l.gsum), s.d_streams, v.d_err, st);
    if (e == hipSuccess) e = hipMemcpyAsync(s.h_err, v.d_err, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) {
        const unsigned gx = (unsigned)std::min<size_t>(64, (maxlen / 16 + 255) / 256 + 1);
        hipLaunchKernelGGL(readback_frames_kernel, dim3(gx, (unsigned)count), dim3(256), 0, st, (const unsigned char *)s.d_streams, v.d_rb, s.h_lens, s.h_rb_off,
                           (unsigned char *)s.pin_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(s.rb_done, st);
    BT_STOP(3);
    if (e != hipSuccess) return set_err(ctx, TIC_E_HIP, "adaptive batch: packing or read-back of the chunk at frame %d failed: %s", s.first, hipGetErrorString(e));
    return TIC_OK;
}

static int batch_adaptive_pipeline(tic_ctx *ctx, const MixedPlan &p, AdaptCall &call) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = ensure_batch_slots(ctx, mixed_slot_need(p));
    if (rc == TIC_OK) rc = ensure_adapt_slots(ctx, p);
    if (rc) return rc;
    for (auto &sl : ctx->bslots) sl.pending = 0;
    int launches = 0;
    return device_entropy_pipeline(
        ctx, (int)p.chunks.size(),
        [&](int ci, Slot &s, hipStream_t stream, int) {
            const MixedChunk &c = p.chunks[(size_t)ci];
            const MixedFrame *fr = &p.frames[(size_t)c.first];
            AdaptFrameTable t;
            size_t nblk, ngroups;
            if (!adaptive_chunk_table(p, c, &t, &nblk, &ngroups)) return set_err(ctx, TIC_E_ARG, "adaptive batch: chunk %d has no table", ci);
            const AdaptSlotView v = adapt_view(s, (size_t)c.count, nblk, ngroups);
            if (v.l.end > s.d_adapt.cap || v.l.upload_end > s.h_adapt.cap) return set_err(ctx, TIC_E_HIP, "adaptive batch: slot buffers too small for chunk %d", ci);
            *v.h_frames = t;
            return enqueue_on_slot(
                ctx, s, stream, c.first, c.count,
                [&](int *direct) {
                    if (!call.coeffs) return upload_chunk_v(ctx, s, p, c, call.io, stream, direct);
                    hipError_t e = hipSuccess;
                    for (int k = 0; k < c.count && e == hipSuccess; k++)
                        e = hipMemcpyAsync((int16_t *)s.d_coef + fr[k].first_block * 64, call.coeffs[fr[k].index], fr[k].nblk * 128, hipMemcpyHostToDevice, stream);
                    *direct = c.count;
                    return e;
                },
                [&]() { return call.coeffs ? hipSuccess : transform_chunk_v(ctx, s, p, c, stream, &launches); },
                [&](Slot &sl, hipStream_t st) {
                    hipError_t e = hipMemcpyAsync(v.d_frames, v.h_frames, sizeof(AdaptFrameTable), hipMemcpyHostToDevice, st);
                    if (e == hipSuccess) e = adaptive_stats_v((const int16_t *)sl.d_coef, v.d_frames, c.count, ngroups, v.d_stats, st);
                    if (e == hipSuccess) e = hipMemcpyAsync(v.h_stats, v.d_stats, (size_t)c.count * sizeof(AdaptStats), hipMemcpyDeviceToHost, st);
                    return e;
                });
        },
        [&](Slot &s, bool) { return adaptive_pack_chunk(ctx, p, s, ctx->rstream, call); },
        [&](Slot &s) {
            if (hipEventSynchronize(s.rb_done) != hipSuccess) return set_err(ctx, TIC_E_HIP, "stream read-back failed");
            if (*s.h_err) return set_err(ctx, TIC_E_HIP, "packing reached past a stream's computed length (statistics and packing disagree)");
            return hand_out_chunk_v(ctx, p, s, call.io);
        });
}

// Both entries: `images` (pixels, row_strides) or `coeffs` (int16 [N_i][64], absolute DC).  Every check before any work.
static int compress_batch_adaptive_impl(tic_ctx *ctx, const uint8_t *const *images, const int16_t *const *coeffs, int n, const int *hs, const int *ws,
                                        const ptrdiff_t *row_strides, const int *qualities, uint8_t *const *outs, const size_t *caps, size_t *out_lens) {
    if (n < 0) return set_err(ctx, TIC_E_ARG, "negative frame count %d", n);
    ctx->last_abatch_frames = ctx->last_abatch_single = ctx->last_abatch_chunks = 0;
    if (n == 0) return TIC_OK;
    if ((!images && !coeffs) || !hs || !ws || (images && !row_strides) || !qualities || !outs || !caps || !out_lens)
        return set_err(ctx, TIC_E_ARG, "null array argument");
    for (int i = 0; i < n; i++) {
        int rc = TIC_OK;
        if (images)
            rc = check_stream_geometry(ctx, hs[i], ws[i], row_strides[i], qualities[i]);
        else if (hs[i] < 0 || ws[i] < 0)
            rc = set_err(ctx, TIC_E_ARG, "negative image size");
        else if (qualities[i] < 1 || qualities[i] > 99)
            rc = set_err(ctx, TIC_E_QUALITY, "quality %d outside 1..99", qualities[i]);
        if (rc) return frame_err(ctx, rc, i);
        if (num_blocks(hs[i], ws[i]) == 0)
            return set_err(ctx, TIC_E_ARG, "frame %d: an image without blocks has no symbols to build a table from (the reference raises IndexError)", i);
        if (!outs[i]) return set_err(ctx, TIC_E_ARG, "frame %d: null output buffer", i);
        if (images ? !images[i] : !coeffs[i]) return set_err(ctx, TIC_E_ARG, images ? "frame %d: null image" : "frame %d: null coefficient pointer", i);
    }
    const ChunkLimits lim = mixed_chunk_limits();
    const MixedPlan p = plan_mixed_batch(hs, ws, qualities, n, lim.frames, lim.bytes);
    AdaptCall call = {coeffs, {images, row_strides, outs, caps, out_lens}, 0};
    ctx->last_batch_direct_frames = ctx->last_batch_staged_frames = ctx->last_batch_autoreg_frames = ctx->last_batch_zero_copy = 0;
    ctx->bt = BatchTrace();
    if (!p.frames.empty()) {
        const int rc = batch_adaptive_pipeline(ctx, p, call);
        if (rc) return rc;
    }
    ctx->last_abatch_frames = (int)p.frames.size();
    ctx->last_abatch_chunks = (int)p.chunks.size();
    for (int i : p.single) { // what a chunk does not hold, behind the batch, frame by frame
        const int rc = images ? tic_compress_adaptive(ctx, images[i], hs[i], ws[i], row_strides[i], qualities[i], outs[i], caps[i], &out_lens[i])
                              : tic_entropy_encode_adaptive(ctx, coeffs[i], hs[i], ws[i], qualities[i], outs[i], caps[i], &out_lens[i]);
        ctx->last_abatch_single++;
        if (rc == TIC_E_SPACE && out_lens[i] > caps[i]) {
            call.short_frames++;
            continue;
        }
        if (rc) return frame_err(ctx, rc, i);
    }
    if (call.short_frames)
        return set_err(ctx, TIC_E_SPACE, "%d frame(s) not written: output buffer too small (out_lens holds the sizes needed)", call.short_frames);
    return TIC_OK;
}

int tic_compress_batch_adaptive_v(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides,
                                  const int *qualities, uint8_t *const *outs, const size_t *caps, size_t *out_lens) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (n > 0 && !images) return set_err(ctx, TIC_E_ARG, "null array argument");
    return compress_batch_adaptive_impl(ctx, images, nullptr, n, hs, ws, row_strides, qualities, outs, caps, out_lens);
}

int tic_entropy_encode_adaptive_batch(tic_ctx *ctx, const int16_t *const *coeffs, int n, const int *hs, const int *ws, const int *qualities,
                                      uint8_t *const *outs, const size_t *caps, size_t *out_lens) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (n > 0 && !coeffs) return set_err(ctx, TIC_E_ARG, "null array argument");
    return compress_batch_adaptive_impl(ctx, nullptr, coeffs, n, hs, ws, nullptr, qualities, outs, caps, out_lens);
}

int tic_last_compress_batch_adaptive(tic_ctx *ctx, int *batch_frames, int *single_frames, int *chunks) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (batch_frames) *batch_frames = ctx->last_abatch_frames;
    if (single_frames) *single_frames = ctx->last_abatch_single;
    if (chunks) *chunks = ctx->last_abatch_chunks;
    return TIC_OK;
}

// Streams with an embedded table the DEVICE decoder takes (tic_adaptive_dec_gpu.hip): every stream of at least 16,384 blocks, and
// shorter ones from kAdaptDevMinBlocks blocks and kAdaptDevMinBits payload bits (32 KB) on - the crossover against the host's
// bit-serial decoder measured in profiles/adaptive_decode.txt: a device decode of a small stream costs 0.45-0.65 ms whatever its
// length, the host 25-30 us per KB; 512^2 at q = 5 (4 KB) stays on the host, at q = 90 (72 KB) goes to the device - provided no code
// of its tables has length zero (a one-symbol tree: nothing to synchronise on) and the stream's bit positions fit 32 bits.  The hooks build moves the lines with TIC_DECODE_MIN_BLOCKS /
// TIC_DECODE_MIN_BITS and sends everything to the host with TIC_DECODE_HOST, as for default-table streams.
constexpr size_t kAdaptDevMinBlocks = 1024, kAdaptDevMinBits = 1u << 18;
static bool adaptive_device_takes(size_t n, size_t len, size_t payload_bit) {
    size_t min_blocks = kAdaptDevMinBlocks, min_bits = kAdaptDevMinBits;
    if (const char *e = test_hook("TIC_DECODE_MIN_BLOCKS")) min_blocks = (size_t)atol(e);
    if (const char *e = test_hook("TIC_DECODE_MIN_BITS")) min_bits = (size_t)atol(e);
    if (test_hook("TIC_DECODE_HOST")) return false;
    if (!adaptive_dec_fits(n, len, payload_bit)) return false;
    return n >= 16384 || (n >= min_blocks && len * 8 - payload_bit >= min_bits);
}

// The device decoder on a stream it takes, with the tables in ctx->adec_tab: coefficients into ctx->d_coef.  *done = false (and TIC_OK) after a give-up
// (ctx->last_decode_giveup says why): the caller runs the host decoder.
static int adaptive_decode_on_device(tic_ctx *ctx, const uint8_t *data, size_t len, bool src_on_device, const AdaptTable &t, size_t n, bool *done) {
    *done = false;
    // decoded where it lies when it is in device memory at a 4-byte aligned address, else through the context's stream buffer
    const bool in_place = src_on_device && ((uintptr_t)data & 3u) == 0;
    int rc = TIC_OK;
    if (!in_place) {
        rc = ctx->d_stream_buf.grow(ctx, align_up(len, 4) + 16);
        if (rc) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_stream_buf, data, len, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    }
    const void *d_stream = in_place ? (const void *)data : (const void *)ctx->d_stream_buf;
    const size_t tab_bytes = align_up(sizeof(AdaptDecTab), 256);
    rc = ctx->d_adec_tab.grow(ctx, tab_bytes + align_up(sizeof(AdaptDecStatus), 256)); // tables (uploaded per call) and status words in one allocation
    if (rc) return rc;
    ctx->d_adec_status = (AdaptDecStatus *)((char *)ctx->d_adec_tab + tab_bytes);
    const int range = adaptive_dec_range_bits(len, t.payload_bit, n);
    const size_t wb = adaptive_dec_work_bytes(len, t.payload_bit, n, range);
    rc = ctx->d_adec_work.grow(ctx, wb, wb + wb / 8); // (room for a longer stream of the same geometry)
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_adec_tab, &ctx->adec_tab, sizeof ctx->adec_tab, hipMemcpyHostToDevice, ctx->stream));
    // Three launches of the stitch settle nearly every stream (the last one only proves it), so the passes behind them are launched
    // right away and one synchronisation shows both.  A stream with stretches in which no walk falls in step gets more rounds, 16 at a
    // time and nothing else, until the chain has crossed them a workgroup per launch; then the passes run once.
    AdaptDecStatus st{};
    const auto run = [&](int round0, int nrounds, bool finish) -> int {
        HIPCHK(ctx, adaptive_decode_gpu(d_stream, len, t.payload_bit, n, range, ctx->d_adec_tab, ctx->d_adec_work, ctx->d_adec_status,
                                        (int16_t *)ctx->d_coef, round0, nrounds, finish, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(&st, ctx->d_adec_status, sizeof st, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, wait_stream(ctx));
        if (test_hook("TIC_DECODE_TRACE")) {
            fprintf(stderr, "adaptive decode: %zu blocks, range %d, rounds %d..%d%s, exits moved:", n, range, round0, round0 + nrounds - 1,
                    finish ? " and the passes" : "");
            for (int r = round0; r < round0 + nrounds; r++) fprintf(stderr, " %u", st.changed[r]);
            fprintf(stderr, ", give-up %u, blocks on the chain %u\n", st.giveup, st.blocks);
        }
        return TIC_OK;
    };
    int rounds = 3;
    rc = run(0, rounds, true);
    if (rc) return rc;
    if (st.changed[rounds - 1]) {
        while (st.changed[rounds - 1] && rounds < kAdaptDecMaxRounds) {
            const int more = kAdaptDecMaxRounds - rounds < 16 ? kAdaptDecMaxRounds - rounds : 16;
            rc = run(rounds, more, false);
            if (rc) return rc;
            rounds += more;
        }
        if (st.changed[rounds - 1]) {
            st.giveup = kAdaptGiveupNoSync; // (whatever the passes of the first launches reported is void)
        } else {
            rc = run(rounds, 0, true);
            if (rc) return rc;
        }
    }
    ctx->last_decode_giveup = (int)st.giveup;
    *done = st.giveup == 0;
    return TIC_OK;
}

// tic_decompress_adaptive / _dev behind their argument checks.  The stream: `len` bytes at `data`, in host or device memory; `head`:
// its first `head_len` bytes in host memory (all of it, or 16 + kAdaptMaxTableBytes: header and table).  Pixels as idct_from_device.
// The host decoder runs for the streams the device decoder does not take, after a give-up, and whenever the table does not parse:
// it alone decides between pixels and TIC_E_STREAM and words the message.
// The front half, which the coefficient calls share (tic_entropy_decode_adaptive, tic_retable_default): the stream's coefficients into ctx->d_coef
// (*in_h_zz = false: the device decoder wrote them) or into ctx->h_zz (*in_h_zz = true: the host decoder did; the caller uploads them where it needs
// them on the device).  img_bytes: the scratch image provisioned beside the coefficients (0: none).
static int adaptive_read_coefs(tic_ctx *ctx, const uint8_t *data, size_t len, bool src_on_device, const uint8_t *head, size_t head_len, int h, int w,
                               size_t img_bytes, bool *in_h_zz) {
    const size_t n = num_blocks(h, w);
    *in_h_zz = false;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = n ? ensure_scratch(ctx, img_bytes, n * 128) : TIC_OK;
    if (rc) return rc;
    {
        AdaptTable t;
        if (adaptive_parse_table(head, head_len, &t, nullptr) == TIC_OK && adaptive_device_takes(n, len, t.payload_bit) &&
            adaptive_dec_tab_build(t, &ctx->adec_tab)) {
            bool done = false;
            rc = adaptive_decode_on_device(ctx, data, len, src_on_device, t, n, &done);
            if (rc) return rc;
            if (done) {
                ctx->last_decode_path = 1;
                return TIC_OK;
            }
        }
    }
    ctx->last_decode_path = 2;
    std::vector<uint8_t> host;
    if (src_on_device && len > head_len) {
        try {
            host.resize(len);
        } catch (...) {
            return set_err(ctx, TIC_E_ARG, "out of host memory for a stream of %zu bytes", len);
        }
        HIPCHK(ctx, hipMemcpy(host.data(), data, len, hipMemcpyDeviceToHost));
        head = host.data();
    } else if (!src_on_device) {
        head = data;
    }
    rc = ctx->h_zz.grow(ctx, n * 128); // (the landing buffer of decode_on_host)
    if (rc) return rc;
    const char *why = "";
    rc = adaptive_decode(head, len, h, w, ctx->h_zz, &why);
    if (rc) return set_err(ctx, rc, "adaptive stream: %s", why);
    *in_h_zz = true;
    return TIC_OK;
}

static int decompress_adaptive_impl(tic_ctx *ctx, const uint8_t *data, size_t len, bool src_on_device, const uint8_t *head, size_t head_len, int h, int w,
                                    int q, uint8_t *out, bool out_on_device, size_t out_stride) {
    const size_t n = num_blocks(h, w);
    bool in_h_zz = false;
    const int rc = adaptive_read_coefs(ctx, data, len, src_on_device, head, head_len, h, w, align_up((size_t)w, 256) * (size_t)h, &in_h_zz);
    if (rc) return rc;
    if (n == 0) return TIC_OK;
    if (in_h_zz) HIPCHK(ctx, hipMemcpyAsync(ctx->d_coef, ctx->h_zz, n * 128, hipMemcpyHostToDevice, ctx->stream));
    return idct_from_device(ctx, h, w, q, -1, out, out_on_device, out_stride);
}

// The header checks of tic_decompress_adaptive and tic_decompress_batch_adaptive.  frame >= 0: the messages name the frame of a batch.
static int check_adaptive_header(tic_ctx *ctx, const uint8_t *data, size_t len, const uint8_t *out, size_t cap, int *h_out, int *w_out, int *q_out, int frame = -1) {
    char pre[32] = "";
    if (frame >= 0) snprintf(pre, sizeof pre, "frame %d: ", frame);
    int h = 0, w = 0, q = 0;
    uint32_t flag = 0;
    if (parse_header(data, len, &h, &w, &q, &flag) != TIC_OK) return set_err(ctx, TIC_E_STREAM, "%sstream shorter than its 16-byte header", pre);
    if (h < 0 || w < 0) return set_err(ctx, TIC_E_STREAM, "%snegative image size in the header", pre);
    if (q < 1 || q > 99) return set_err(ctx, TIC_E_STREAM, "%squality %d in the header outside 1..99", pre, q);
    if ((size_t)h * (size_t)w > cap || (!out && h && w)) return set_err(ctx, TIC_E_SPACE, "%soutput buffer too small", pre);
    *h_out = h, *w_out = w, *q_out = q;
    return TIC_OK;
}

int tic_decompress_adaptive(tic_ctx *ctx, const uint8_t *data, size_t len, uint8_t *out, size_t cap) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    ctx->last_decode_giveup = 0;
    int h = 0, w = 0, q = 0;
    const int rc = check_adaptive_header(ctx, data, len, out, cap, &h, &w, &q);
    if (rc) return rc;
    return decompress_adaptive_impl(ctx, data, len, false, data, len, h, w, q, out, false, 0);
}

// ---- transcoding (tinyimgcodec_hip_transcode.h): a stream's coefficients, and the stream of the other table family from them -----------------------
// The reader of default-table and scaled_dct streams: decode_on_device with the coefficient sink - *on_device = true, the n rows are at d_user (null:
// ctx->d_coef) - or, for everything the device reader does not take or gives up on, the host decoder as in decode_on_host: *on_device = false, the
// rows are in ctx->h_zz.  A running DC outside int16 (the device run's give-up bit 512 comes here too) is TIC_E_RANGE: the layout cannot hold it.
// `data` in host or device memory; head16: the stream's own 16 header bytes, in host memory.
static int read_default_coefs(tic_ctx *ctx, const uint8_t *data, size_t len, bool src_on_device, const StreamHead &sh, const uint8_t *head16,
                              int16_t *d_user, bool *on_device) {
    const size_t n = num_blocks(sh.h, sh.w);
    DecSink sink;
    sink.coef = true;
    sink.d_user = d_user;
    int rc = decode_on_device(ctx, data, len, sh, nullptr, false, 0, on_device, head16, src_on_device, false, nullptr, sink);
    if (rc) return rc;
    if (*on_device) {
        ctx->last_decode_path = 1;
        return TIC_OK;
    }
    std::vector<uint8_t> host;
    if (src_on_device) {
        try {
            host.resize(len);
        } catch (...) {
            return set_err(ctx, TIC_E_ARG, "out of host memory for a stream of %zu bytes", len);
        }
        HIPCHK(ctx, hipSetDevice(ctx->device));
        HIPCHK(ctx, hipMemcpy(host.data(), data, len, hipMemcpyDeviceToHost));
        data = host.data();
    }
    rc = ctx->h_zz.grow(ctx, n * 128);
    if (rc) return rc;
    std::vector<DcWide> wide;
    entropy_decode(data, len, sh.h, sh.w, ctx->h_zz, &wide);
    ctx->last_decode_path = 2;
    if (!wide.empty())
        return set_err(ctx, TIC_E_RANGE, "the running DC left int16 at block %zu (%d): the int16 coefficient layout cannot hold it", wide[0].block,
                       (int)wide[0].dc);
    return TIC_OK;
}

// the header's fields as the caller gets them (quality: the exponent of a scaled_dct stream)
static void head_out(const StreamHead &sh, int *h, int *w, int *quality, uint32_t *flag) {
    if (h) *h = sh.h;
    if (w) *w = sh.w;
    if (quality) *quality = sh.scaled_exp >= 0 ? sh.scaled_exp : sh.quality;
    if (flag) *flag = sh.scaled_exp >= 0 ? kFlagScaled : 0u;
}

static int entropy_decode_impl(tic_ctx *ctx, const uint8_t *data, size_t len, bool on_device, void *coeffs_zz, size_t cap_blocks, int *h, int *w,
                               int *quality, uint32_t *flag) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    ctx->last_decode_giveup = 0;
    ctx->last_decode_tries = 0;
    if (!data && len) return set_err(ctx, TIC_E_ARG, "null stream pointer");
    uint8_t head[16] = {0};
    if (on_device) {
        if (len < 16) return set_err(ctx, TIC_E_STREAM, "stream shorter than the 16-byte header");
        HIPCHK(ctx, hipSetDevice(ctx->device));
        HIPCHK(ctx, hipMemcpy(head, data, 16, hipMemcpyDeviceToHost));
    }
    StreamHead sh;
    int rc = check_header(ctx, on_device ? head : data, on_device ? 16 : len, &sh);
    if (rc) return rc;
    head_out(sh, h, w, quality, flag);
    const size_t n = num_blocks(sh.h, sh.w);
    if (n == 0) return TIC_OK;
    if (!coeffs_zz || cap_blocks < n) return set_err(ctx, TIC_E_SPACE, "coefficient buffer too small (%zu blocks needed)", n);
    if (on_device && ((uintptr_t)coeffs_zz & 15u)) return set_err(ctx, TIC_E_ARG, "device coefficient buffer must be 16-byte aligned");
    bool dev = false;
    rc = read_default_coefs(ctx, data, len, on_device, sh, on_device ? head : data, on_device ? (int16_t *)coeffs_zz : nullptr, &dev);
    if (rc) return rc;
    if (dev && on_device) return TIC_OK; // (the rows are where the caller wants them, behind a drained stream)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (dev) HIPCHK(ctx, hipMemcpyAsync(coeffs_zz, ctx->d_coef, n * 128, hipMemcpyDeviceToHost, ctx->stream));
    else if (on_device) HIPCHK(ctx, hipMemcpyAsync(coeffs_zz, ctx->h_zz, n * 128, hipMemcpyHostToDevice, ctx->stream));
    else memcpy(coeffs_zz, ctx->h_zz, n * 128);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TIC_OK;
}

int tic_entropy_decode(tic_ctx *ctx, const uint8_t *data, size_t len, int16_t *coeffs_zz, size_t cap_blocks, int *h, int *w, int *quality,
                       uint32_t *flag) {
    return entropy_decode_impl(ctx, data, len, false, coeffs_zz, cap_blocks, h, w, quality, flag);
}

int tic_entropy_decode_dev(tic_ctx *ctx, const void *d_stream, size_t len, void *d_coeffs_zz, size_t cap_blocks, int *h, int *w, int *quality,
                           uint32_t *flag) {
    return entropy_decode_impl(ctx, (const uint8_t *)d_stream, len, true, d_coeffs_zz, cap_blocks, h, w, quality, flag);
}

int tic_entropy_decode_dev_timed(tic_ctx *ctx, const void *d_stream, size_t len, void *d_coeffs_zz, size_t cap_blocks, int warm, int iters,
                                 float *ms_total) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (!ms_total || warm < 0 || iters <= 0 || !d_stream || !d_coeffs_zz || len < 16) return set_err(ctx, TIC_E_ARG, "bad argument");
    if (((uintptr_t)d_stream & 3u) || ((uintptr_t)d_coeffs_zz & 15u)) return set_err(ctx, TIC_E_ARG, "stream 4-byte, coefficients 16-byte aligned");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    uint8_t head[16];
    HIPCHK(ctx, hipMemcpy(head, d_stream, 16, hipMemcpyDeviceToHost));
    StreamHead sh;
    int rc = check_header(ctx, head, 16, &sh);
    if (rc) return rc;
    const size_t n = num_blocks(sh.h, sh.w);
    if (cap_blocks < n) return set_err(ctx, TIC_E_SPACE, "coefficient buffer too small (%zu blocks needed)", n);
    if (!device_decoder_takes(n, len)) return set_err(ctx, TIC_E_ARG, "the device reader does not take this stream");
    rc = ensure_dec_tables(ctx);
    if (rc) return rc;
    DecWorkspace &ws = ctx->dec_ws;
    const size_t wb = entropy_decode_gpu_work_bytes(len, n);
    rc = ws.grow(ctx, wb, wb, entropy_decode_gpu_desc_words(len, n), 1, 1);
    if (rc) return rc;
    const int range_bits = decode_range_bits(len, n);
    rc = timed_launches(ctx, warm, iters, ms_total, nullptr, [&](int, hipEvent_t, hipEvent_t) {
        if (ws.begin(ctx, ctx->stream, 1)) return hipErrorUnknown; // (a new epoch per run; the status words are the last run's when the stream has drained)
        return entropy_decode_coef_gpu(d_stream, len, n, ctx->d_dec_luts, ws.work, ws.work.cap, ws.desc, ws.desc_words, ws.epoch, head,
                                       (int16_t *)d_coeffs_zz, ws.h_status.d, range_bits, 0, ctx->stream);
    });
    if (rc) return rc;
    DecStatus st;
    memcpy(&st, ws.h_status, sizeof st);
    if (!dec_status_complete(st, head, n)) return set_err(ctx, TIC_E_ARG, "the device reader gave up on this stream (flags %d): nothing to time", st.giveup);
    return TIC_OK;
}

int tic_entropy_decode_adaptive(tic_ctx *ctx, const uint8_t *data, size_t len, int16_t *coeffs_zz, size_t cap_blocks, int *h_out, int *w_out,
                                int *quality) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    ctx->last_decode_giveup = 0;
    int h = 0, w = 0, q = 0;
    int rc = check_adaptive_header(ctx, data, len, data, ~(size_t)0 >> 1, &h, &w, &q); // (no pixels: the capacity that counts is cap_blocks, below)
    if (rc) return rc;
    if (h_out) *h_out = h;
    if (w_out) *w_out = w;
    if (quality) *quality = q;
    const size_t n = num_blocks(h, w);
    if (n && (!coeffs_zz || cap_blocks < n)) return set_err(ctx, TIC_E_SPACE, "coefficient buffer too small (%zu blocks needed)", n);
    bool in_h_zz = false;
    rc = adaptive_read_coefs(ctx, data, len, false, data, len, h, w, 0, &in_h_zz);
    if (rc || n == 0) return rc;
    if (in_h_zz) {
        memcpy(coeffs_zz, ctx->h_zz, n * 128);
        return TIC_OK;
    }
    HIPCHK(ctx, hipMemcpyAsync(coeffs_zz, ctx->d_coef, n * 128, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TIC_OK;
}

int tic_retable_adaptive(tic_ctx *ctx, const uint8_t *data, size_t len, uint8_t *out, size_t cap, size_t *out_len) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    ctx->last_decode_giveup = 0;
    ctx->last_decode_tries = 0;
    if (!out || !out_len) return set_err(ctx, TIC_E_ARG, "null output pointer");
    int h = 0, w = 0, q = 0;
    uint32_t flag = 0;
    if (parse_header(data, len, &h, &w, &q, &flag) != TIC_OK) return set_err(ctx, TIC_E_STREAM, "stream shorter than the 16-byte header");
    if (flag & (1u << 31)) return set_err(ctx, TIC_E_STREAM, "the stream has an embedded Huffman table already");
    if (flag & kFlagScaled) return set_err(ctx, TIC_E_STREAM, "a scaled_dct stream cannot carry an embedded table: the flag word has room for one family");
    if (h < 0 || w < 0) return set_err(ctx, TIC_E_STREAM, "negative image size in the header");
    if (q < 1 || q > 99) return set_err(ctx, TIC_E_STREAM, "quality %d in the header outside 1..99", q);
    const size_t n = num_blocks(h, w);
    if (n == 0) return set_err(ctx, TIC_E_ARG, "an image without blocks has no symbols to build a table from (the reference raises IndexError)");
    const StreamHead sh = {h, w, q, -1};
    bool dev = false;
    int rc = read_default_coefs(ctx, data, len, false, sh, data, nullptr, &dev);
    if (rc) return rc;
    if (!dev) { // the host reader's rows go up; the device reader's never left
        HIPCHK(ctx, hipSetDevice(ctx->device));
        rc = ensure_scratch(ctx, 0, n * 128);
        if (rc) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_coef, ctx->h_zz, n * 128, hipMemcpyHostToDevice, ctx->stream));
    }
    return adaptive_encode_dev(ctx, n, h, w, q, out, cap, out_len);
}

int tic_retable_default(tic_ctx *ctx, const uint8_t *data, size_t len, uint8_t *out, size_t cap, size_t *out_len) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    ctx->last_decode_giveup = 0;
    if (!out || !out_len) return set_err(ctx, TIC_E_ARG, "null output pointer");
    int h = 0, w = 0, q = 0;
    int rc = check_adaptive_header(ctx, data, len, data, ~(size_t)0 >> 1, &h, &w, &q); // (no pixels: `cap` is the stream's, checked against its length)
    if (rc) return rc;
    const size_t n = num_blocks(h, w);
    bool in_h_zz = false;
    rc = adaptive_read_coefs(ctx, data, len, false, data, len, h, w, 0, &in_h_zz);
    if (rc) return rc;
    if (n == 0) return entropy_encode(nullptr, h, w, q, out, cap, out_len); // the header alone (codec.py:151)
    if (in_h_zz) HIPCHK(ctx, hipMemcpyAsync(ctx->d_coef, ctx->h_zz, n * 128, hipMemcpyHostToDevice, ctx->stream));
    // the default device entropy stage on the context's workspace; the input stream's copy in d_stream_buf (if the device reader made one) is done with
    rc = ctx->d_stream_buf.grow(ctx, compress_bound(h, w));
    if (rc) return rc;
    size_t packed = 0;
    rc = entropy_encode_dev_impl(ctx, ctx->d_coef, h, w, q, ctx->d_stream_buf, ctx->d_stream_buf.cap, &packed, false);
    if (rc) return rc;
    if (packed > cap) {
        *out_len = packed;
        return set_err(ctx, TIC_E_SPACE, "output buffer too small (%zu bytes needed, %zu given)", packed, cap);
    }
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->d_stream_buf, packed, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *out_len = packed;
    return TIC_OK;
}

// ---- tic_decompress_batch_adaptive: decompress_adaptive() of MANY streams at once ---------------------------------------------------------------
// The fixed cost of a device decode of an adaptive stream - seven launches, a table upload, a status read-back, a synchronisation
// (profiles/adaptive_decode.txt section 1) - is per submission, not per frame: the frames of a chunk (tic_adaptive_decode_plan.h) share ONE
// upload (descriptors, workgroup tables, a look-up table per frame built on the host, the streams), one launch per kernel of the descriptor
// form (tic_adaptive_dec_gpu.hip), one launch of the inverse transform (idct_batch_kernel) and one download (dbatch_pixels_down).

// Which frames the batch kernels take: blocks, a table that parses and builds (no code of length zero: the flat and one-block frames are
// the host decoder's), bit positions that fit 32 bits, and no TIC_DECODE_HOST in the hooks build.  The size thresholds of
// adaptive_device_takes (kAdaptDevMinBlocks / kAdaptDevMinBits) do NOT apply: they were measured against the fixed cost of a submission, and
// the frames of a batch share that cost.  No floor on frames or payload per call is applied beyond "two taken frames at least" (a call
// with fewer is the single call, thresholds included): tools/adaptive_decode_batch_timing.py measures the batch against the loop on small
// and large frames (profiles/adaptive_decode_batch.txt), and a floor is to be settled from there, not guessed here.
static bool adaptive_batch_takes(size_t nblocks, const uint8_t *data, size_t len, AdaptTable *t) {
    if (nblocks == 0 || test_hook("TIC_DECODE_HOST")) return false;
    if (adaptive_parse_table(data, len < 16 + kAdaptMaxTableBytes ? len : 16 + kAdaptMaxTableBytes, t, nullptr) != TIC_OK) return false;
    return adaptive_dec_tab_buildable(*t) && adaptive_dec_fits(nblocks, len, t->payload_bit);
}

// A chunk through the kernels: buffers, ONE upload, the rounds protocol (tic_adaptive_dec_gpu.hip header comment), the pixels in ctx->dbat.d_pix.
// good[k]: frame k is complete there.  Every way out with an error lies in front of `good`.
// pixels = false (tic_retable_default_batch): the reader stage alone - no inverse transform is set up or launched, the chunk's coefficients stay at
// ctx->adbat.d_work + AdaptDecWorkLayout(c).o_coef, frame k's rows from row pf[k].d.blk0 on.
static int adbatch_decode(tic_ctx *ctx, const DecBatchIO &io, const AdaptDecPlanFrame *pf, const AdaptDecPlanChunk &c, const AdaptTable *tabs, std::vector<char> *good,
                          bool pixels = true) {
    tic_ctx::DecBatch &B = ctx->dbat;
    tic_ctx::AdaptDecBatchBuf &A = ctx->adbat;
    const uint32_t F = (uint32_t)c.count;
    size_t iwgs = 0;
    std::vector<IdctArgs> ia(F);
    for (uint32_t k = 0; k < F && pixels; k++) {
        ia[k] = idct_args(dec_idct_args(ctx, pf[k].h, pf[k].w, pf[k].quality, -1, nullptr, (long)pf[k].pitch, nullptr), nullptr);
        iwgs += (size_t)idct_batch_wgs(ia[k].ntiles);
    }
    const AdaptDecUploadLayout up(c, sizeof(IdctArgs), iwgs);
    const AdaptDecWorkLayout wl(c);
    int rc = dbatch_grow(ctx, up.up_bytes, pixels ? c.pix_bytes : 0);
    if (rc) return rc;
    rc = A.d_work.grow(ctx, wl.bytes, wl.bytes + wl.bytes / 4);
    if (rc) return rc;
    rc = A.h_status.grow(ctx, wl.status_bytes, 2 * wl.status_bytes);
    if (rc) return rc;
    BT_START();
    AdaptDecFrame *hf = (AdaptDecFrame *)(B.h_in + up.o_frames);
    IdctArgs *hia = (IdctArgs *)(B.h_in + up.o_idct_args);
    uint2 *hiw = (uint2 *)(B.h_in + up.o_idct_wgs);
    adec_plan_fill_wg_tables(pf, c.count, (uint32_t *)(B.h_in + up.o_rwg), (uint32_t *)(B.h_in + up.o_bwg));
    size_t g = 0;
    for (uint32_t k = 0; k < F; k++) {
        const AdaptDecPlanFrame &f = pf[k];
        hf[k] = f.d;
        if (pixels) {
            ia[k].coeffs = (const int16_t *)(A.d_work + wl.o_coef) + (size_t)f.d.blk0 * 64;
            ia[k].out = B.d_pix + f.pix_off;
            memcpy(&hia[k], &ia[k], sizeof(IdctArgs));
            for (int t = 0; t < ia[k].ntiles; t += idct_batch_tiles_per_wg()) hiw[g++] = make_uint2(k, (uint32_t)t);
        }
        if (!adaptive_dec_tab_build(tabs[k], (AdaptDecTab *)(B.h_in + up.o_tabs + f.tab_off))) return set_err(ctx, TIC_E_ARG, "frame %d: no look-up table for a table that parsed", f.index);
        memcpy(B.h_in + up.o_streams + (size_t)f.d.word0 * 4, io.streams[f.index], f.len); // (the bytes behind a stream's last word are never read)
    }
    BT_STOP(0);
    BT_START();
    HIPCHK(ctx, hipMemcpyAsync(B.d_in, B.h_in, up.up_bytes, hipMemcpyHostToDevice, ctx->stream));
    AdaptDecBatch a;
    a.frames = (const AdaptDecFrame *)(B.d_in + up.o_frames);
    a.rwg_frame = (const uint32_t *)(B.d_in + up.o_rwg), a.bwg_frame = (const uint32_t *)(B.d_in + up.o_bwg);
    a.tabs = (const char *)(B.d_in + up.o_tabs);
    a.words = (const uint32_t *)(B.d_in + up.o_streams);
    a.work = A.d_work + wl.o_work;
    a.cs = (AdaptDecChunkStatus *)(A.d_work + wl.o_status);
    a.fs = (AdaptDecFrameStatus *)(a.cs + 1);
    a.zz = (int16_t *)(A.d_work + wl.o_coef);
    a.nframes = F, a.ranges = c.ranges, a.blocks = (uint32_t)c.blocks, a.range_wgs = c.range_wgs, a.block_wgs = c.block_wgs;
    const AdaptDecChunkStatus *cs = (const AdaptDecChunkStatus *)A.h_status;
    const AdaptDecFrameStatus *fs = (const AdaptDecFrameStatus *)(cs + 1);
    const auto run = [&](int round0, int nrounds, bool finish) -> int {
        HIPCHK(ctx, adaptive_decode_gpu_batch(a, round0, nrounds, finish, ctx->stream));
        if (finish && pixels) HIPCHK(ctx, launch_idct_batch((const IdctArgs *)(B.d_in + up.o_idct_args), (const uint2 *)(B.d_in + up.o_idct_wgs), iwgs, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(A.h_status, a.cs, wl.status_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (test_hook("TIC_DECODE_TRACE")) {
            const int lastr = round0 + nrounds - 1; // (the last round launched so far: round0 >= 1 where nrounds is 0)
            uint32_t moving = 0;
            for (uint32_t k = 0; k < F; k++) moving += fs[k].changed[lastr] != 0;
            fprintf(stderr, "adaptive batch decode: %u frames, rounds %d..%d%s, exits moved in round %d: %u, frames still moving: %u\n", F, round0, lastr,
                    finish ? " and the passes" : "", lastr, cs->changed[lastr], moving);
        }
        return TIC_OK;
    };
    int last = kAdaptBatchRounds0 - 1;
    rc = run(0, kAdaptBatchRounds0, true);
    if (rc) return rc;
    if (cs->changed[last]) {
        rc = run(kAdaptBatchRounds0, kAdaptBatchRoundsMore, false);
        if (rc) return rc;
        last = kAdaptBatchRounds - 1;
        rc = run(kAdaptBatchRounds, 0, true); // (a frame round 18 still moved is marked below: whatever the passes leave of it is never handed out)
        if (rc) return rc;
    }
    BT_STOP(1);
    good->assign(F, 0);
    // (a frame that settled early keeps zeros in the rounds it left at once)
    for (uint32_t k = 0; k < F; k++) (*good)[k] = (fs[k].giveup | (fs[k].changed[last] ? kAdaptGiveupNoSync : 0u)) == 0;
    return TIC_OK;
}

int tic_decompress_batch_adaptive(tic_ctx *ctx, const uint8_t *const *streams, const size_t *lens, int n, uint8_t *const *outs, const size_t *caps, int *hs, int *ws) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (n < 0 || (n > 0 && (!streams || !lens || !outs || !caps))) return set_err(ctx, TIC_E_ARG, "bad batch arguments");
    ctx->last_adbatch_frames = ctx->last_adbatch_single = ctx->last_adbatch_chunks = ctx->last_adbatch_direct = 0;
    ctx->bt = BatchTrace(); // (tic_last_batch_phases: [0] packing the upload buffer, [1] upload, kernels and status, [2] download, [4] hand-out, [5] single-frame calls)
    if (n == 0) return TIC_OK;
    if (n == 1) { // exactly the single call
        const int rc = tic_decompress_adaptive(ctx, streams[0], lens[0], outs[0], caps[0]);
        if (rc == TIC_OK || lens[0] >= 16) {
            int h = 0, w = 0, q = 0;
            uint32_t flag = 0;
            (void)parse_header(streams[0], lens[0], &h, &w, &q, &flag);
            if (hs) hs[0] = h;
            if (ws) ws[0] = w;
        }
        ctx->last_adbatch_single = 1;
        return rc;
    }
    // ---- the checks of tic_decompress_adaptive, for every frame, before any work
    std::vector<AdaptDecPlanIn> in((size_t)n);
    std::vector<AdaptTable> tabs; // of the frames taken, in order
    std::vector<int> later;       // frames for the single-frame call
    {
        AdaptTable t;
        for (int i = 0; i < n; i++) {
            int h = 0, w = 0, q = 0;
            const int rc = check_adaptive_header(ctx, streams[i], lens[i], outs[i], caps[i], &h, &w, &q, i);
            if (rc) return rc;
            if (hs) hs[i] = h;
            if (ws) ws[i] = w;
            in[(size_t)i] = {h, w, q, lens[i], 0, adaptive_batch_takes(num_blocks(h, w), streams[i], lens[i], &t)};
            if (in[(size_t)i].takes) in[(size_t)i].payload_bit = t.payload_bit, tabs.push_back(t);
        }
    }
    if (tabs.size() < 2) { // (adaptive_batch_takes: no batch of one)
        for (AdaptDecPlanIn &f : in) f.takes = false;
        tabs.clear();
    }
    for (int i = 0; i < n; i++)
        if (!in[(size_t)i].takes) later.push_back(i);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // ---- the plan: chunks of frames in order, inside the limits (the 294 frames of the benchmark set - 77 MB of pixels, 154 MB of coefficients,
    // 4 MB of tables - are one chunk; so are sixteen 1080p frames)
    AdaptDecPlanLimits lim = {(size_t)96 << 20, (size_t)288 << 20, (size_t)256 << 20, (size_t)16 << 20, 1024};
    if (const char *e = test_hook("TIC_ADBATCH_CHUNK")) lim.frames = atoi(e) >= 1 && atoi(e) <= 1024 ? atoi(e) : lim.frames; // (tests: several chunks)
    const AdaptDecPlan plan = plan_adaptive_decode_batch(in.data(), n, lim);
    const DecBatchIO io = {streams, lens, outs, caps};
    int result = TIC_OK;
    std::string first_err; // (the text of an error inside a chunk: the single-frame calls behind it write their own)
    for (const AdaptDecPlanChunk &c : plan.chunks) {
        const AdaptDecPlanFrame *pf = &plan.frames[(size_t)c.first];
        std::vector<char> good;
        bool direct = false;
        int crc = adbatch_decode(ctx, io, pf, c, &tabs[(size_t)c.first], &good);
        if (crc == TIC_OK) crc = dbatch_pixels_down(ctx, io, pf, (size_t)c.count, c.pix_bytes, &direct);
        if (crc == TIC_OK) {
            ctx->last_adbatch_chunks++;
            ctx->last_adbatch_direct += direct ? c.count : 0;
            for (int k = 0; k < c.count; k++) {
                if (good[(size_t)k]) ctx->last_adbatch_frames++;
                else later.push_back(pf[k].index);
            }
            dbatch_hand_out(ctx, io, pf, c.count, c.pix_bytes, direct, good);
            continue;
        }
        // ended early by a failed allocation, copy or launch: its frames and those of the chunks behind it go one by one; the error is the first and stands
        for (size_t k = (size_t)c.first; k < plan.frames.size(); k++) later.push_back(plan.frames[k].index);
        result = crc;
        first_err = ctx->err;
        break;
    }
    // ---- frames the batch did not take, or gave up on: the single call, which alone decides between pixels and TIC_E_STREAM and words the message.
    // (after a direct download a given-up frame's bytes in the caller's buffer hold what the kernels left: the single call overwrites them, or fails)
    std::sort(later.begin(), later.end());
    BT_START();
    for (int i : later) {
        const int rc = tic_decompress_adaptive(ctx, streams[i], lens[i], outs[i], caps[i]);
        ctx->last_adbatch_single++;
        if (rc != TIC_OK && result == TIC_OK) {
            const std::string m = ctx->err;
            result = set_err(ctx, rc, "frame %d: %s", i, m.c_str());
            first_err = ctx->err;
        }
    }
    BT_STOP(5);
    if (!first_err.empty()) ctx->err = first_err;
    return result;
}

// How the last tic_decompress_batch_adaptive went: frames decoded by the batch kernels, frames that took the single call (not taken, or given
// up on), chunks.  Any pointer may be null.
int tic_last_decompress_batch_adaptive(tic_ctx *ctx, int *batch_frames, int *single_frames, int *chunks) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (batch_frames) *batch_frames = ctx->last_adbatch_frames;
    if (single_frames) *single_frames = ctx->last_adbatch_single;
    if (chunks) *chunks = ctx->last_adbatch_chunks;
    return TIC_OK;
}

// ... and the frames of its chunks whose pixels were copied straight into the caller's memory (the direct download)
int tic_last_decompress_batch_adaptive_direct(tic_ctx *ctx) {
    TIC_LOCK(ctx);
    return ctx ? ctx->last_adbatch_direct : TIC_E_ARG;
}

// The device decoder's geometry for a stream of `len` bytes whose payload starts at bit `payload_bit` and holds `nblocks` blocks: stream
// bits per lane (adaptive_dec_range_bits) and the number of ranges - a workgroup of the range grid holds 256 of them.  Pure arithmetic.
int tic_adaptive_decode_geometry(size_t len, size_t payload_bit, size_t nblocks, int *range_bits, size_t *nranges) {
    if (!adaptive_dec_fits(nblocks, len, payload_bit)) return TIC_E_ARG;
    const int r = adaptive_dec_range_rule(len, payload_bit, nblocks);
    if (range_bits) *range_bits = r;
    if (nranges) *nranges = adaptive_dec_ranges_of(len, payload_bit, r);
    return TIC_OK;
}

int tic_decompress_adaptive_dev(tic_ctx *ctx, const void *d_stream, size_t len, void *d_out, ptrdiff_t out_stride, size_t out_cap, int *h_out, int *w_out) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    ctx->last_decode_giveup = 0;
    if (!d_stream && len) return set_err(ctx, TIC_E_ARG, "null stream pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (len < 16) return set_err(ctx, TIC_E_STREAM, "stream shorter than its 16-byte header");
    // header and table come down (2.6 KB at most); the payload stays where it is
    uint8_t head[16 + kAdaptMaxTableBytes];
    const size_t head_len = len < sizeof head ? len : sizeof head;
    HIPCHK(ctx, hipMemcpy(head, d_stream, head_len, hipMemcpyDeviceToHost));
    int h = 0, w = 0, q = 0;
    uint32_t flag = 0;
    (void)parse_header(head, head_len, &h, &w, &q, &flag);
    if (h < 0 || w < 0) return set_err(ctx, TIC_E_STREAM, "negative image size in the header");
    if (q < 1 || q > 99) return set_err(ctx, TIC_E_STREAM, "quality %d in the header outside 1..99", q);
    if (h_out) *h_out = h;
    if (w_out) *w_out = w;
    if (num_blocks(h, w) != 0) {
        if (out_stride < (ptrdiff_t)w) return set_err(ctx, TIC_E_ARG, "row stride %td smaller than the width %d", out_stride, w);
        if (!d_out || (size_t)(h - 1) * (size_t)out_stride + (size_t)w > out_cap) return set_err(ctx, TIC_E_SPACE, "output buffer too small");
    }
    return decompress_adaptive_impl(ctx, (const uint8_t *)d_stream, len, true, head, head_len, h, w, q, (uint8_t *)d_out, true, (size_t)out_stride);
}

// ---- batch transcoding (tinyimgcodec_hip_transcode_batch.h): tic_entropy_decode / tic_retable_adaptive / tic_retable_default of MANY streams ------
// A single transcoding call of a small stream is per-call cost and little else (profiles/transcode.txt: 0.21-0.24 ms for a 512^2 stream whose reader
// kernel takes 12.5 us).  The frames of a chunk (tic_transcode_plan.h: up to kEntropyMaxFrames of them) share ONE upload, one launch per kernel of the
// reader's descriptor form, one launch per kernel of the writer's, and one download; their coefficients lie back to back in one device buffer, frame
// k's rows from row blk0 on, and never leave the device between the reader and the writer.
// Frame i's result is the single call's.  The batch kernels finish a frame or they do not: a frame they do not take, give up on or flag is not
// written at all here and goes through the single call behind the chunks, which alone words errors - so do the frames of a chunk that fails on the
// way (an allocation, a copy, a launch).  The calls leave tic_last_decode_* as they found them.
extern "C++" {
struct TBatchCall {
    tic_ctx *ctx;
    int n;
    std::vector<int> rc;     // per frame: the code so far
    std::vector<char> done;  // per frame: finished (by the batch kernels, or refused for space from their figures)
    std::vector<std::pair<int, std::string>> errs; // failing frames and their messages
    int saved[4];
    BatchTrace saved_bt; // (the readers' stages time their phases: tic_last_batch_phases keeps the last batch call's)
    TBatchCall(tic_ctx *c, int frames) : ctx(c), n(frames), rc((size_t)frames, TIC_OK), done((size_t)frames, 0) {
        saved[0] = c->last_decode_path, saved[1] = c->last_decode_giveup, saved[2] = c->last_decode_range, saved[3] = c->last_decode_tries;
        saved_bt = c->bt;
        c->last_tbatch_frames = c->last_tbatch_single = c->last_tbatch_chunks = 0;
    }
    void finished(int i) { done[(size_t)i] = 1, ctx->last_tbatch_frames++; }
    void failed(int i, int code, const std::string &msg) { done[(size_t)i] = 1, rc[(size_t)i] = code, errs.emplace_back(i, msg), ctx->last_tbatch_frames++; } // (refused from the kernels' own figures)
    // The frames the chunks left, through `single(i)` in ascending order; then the call's result: the code and message of the lowest failing index.
    template <class Single> int end(Single single, int *rcs) {
        for (int i = 0; i < n; i++) {
            if (done[(size_t)i]) continue;
            const int r = single(i);
            ctx->last_tbatch_single++;
            rc[(size_t)i] = r;
            if (r != TIC_OK) errs.emplace_back(i, ctx->err);
        }
        ctx->last_decode_path = saved[0], ctx->last_decode_giveup = saved[1], ctx->last_decode_range = saved[2], ctx->last_decode_tries = saved[3];
        ctx->bt = saved_bt;
        if (rcs) memcpy(rcs, rc.data(), (size_t)n * sizeof(int));
        if (errs.empty()) return TIC_OK;
        const auto first = std::min_element(errs.begin(), errs.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        return set_err(ctx, rc[(size_t)first->first], "frame %d: %s", first->first, first->second.c_str());
    }
};
}

static TranscodeLimits tbatch_limits() {
    TranscodeLimits lim = transcode_default_limits();
    if (const char *e = test_hook("TIC_TBATCH_CHUNK")) lim.frames = atoi(e) >= 1 && atoi(e) <= kEntropyMaxFrames ? atoi(e) : lim.frames; // (tests: several chunks)
    return lim;
}

// Which frames the default-table reader's batch kernels take: a header tic_entropy_decode accepts (`scaled_ok`: or a scaled_dct one), blocks, the
// device decoder's size rule, no host-decoder hook.  Silent: the single call words what is wrong with a frame.
static bool tbatch_default_takes(const uint8_t *data, size_t len, bool scaled_ok, DecPlanIn *in, uint32_t *flag_out) {
    int h = 0, w = 0, q = 0;
    uint32_t flag = 0;
    if (!data || parse_header(data, len, &h, &w, &q, &flag) != TIC_OK || (flag & (1u << 31)) || h < 0 || w < 0) return false;
    const bool scaled = (flag & kFlagScaled) != 0;
    if (scaled ? (!scaled_ok || q < 0 || q > 62) : (q < 1 || q > 99)) return false;
    const size_t nb = num_blocks(h, w);
    *in = {h, w, q, len, nb != 0 && device_decoder_takes(nb, len) && !test_hook("TIC_DECODE_HOST") && !test_hook("TIC_DECODE_SERIAL")};
    *flag_out = scaled ? kFlagScaled : 0u;
    return in->takes;
}

// The default-table reader's stage of a chunk: dbatch_enqueue with the coefficient sink - descriptors, buffers, ONE upload and the two launches (the
// unchanged measure / stitch kernel, the batch form of the coefficient sink), queued on the context's stream; nothing is waited for.  The chunk's
// rows go to d_coef (c.blocks of them); frame k's status lands in ctx->dbat.ws.h_status[k] when the stream has drained.  *refused: the launcher's
// host-side checks said no, nothing runs.
static int tbatch_read_default(tic_ctx *ctx, const uint8_t *const *streams, const DecPlanFrame *pf, const DecPlanChunk &c, int16_t *d_coef, bool *refused) {
    const DecBatchIO io = {streams, nullptr, nullptr, nullptr};
    return dbatch_enqueue(ctx, io, pf, c, refused, d_coef);
}

static const char *const kTBatchShort = "output buffer too small (%zu bytes needed, %zu given)"; // (the single calls' wording)
static std::string tbatch_short_msg(size_t need, size_t cap) {
    char buf[128];
    snprintf(buf, sizeof buf, kTBatchShort, need, cap);
    return buf;
}

int tic_entropy_decode_batch(tic_ctx *ctx, const uint8_t *const *streams, const size_t *lens, int n, int16_t *const *coeffs, const size_t *cap_blocks,
                             int *hs, int *ws, int *qualities, uint32_t *flags, int *rcs) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (n < 0 || (n > 0 && (!streams || !lens || !coeffs || !cap_blocks))) return set_err(ctx, TIC_E_ARG, "bad batch arguments");
    TBatchCall call(ctx, n);
    if (n == 0) return TIC_OK;
    const auto single = [&](int i) {
        return tic_entropy_decode(ctx, streams[i], lens[i], coeffs[i], cap_blocks[i], hs ? hs + i : nullptr, ws ? ws + i : nullptr, qualities ? qualities + i : nullptr,
                                  flags ? flags + i : nullptr);
    };
    if (n == 1) return call.end(single, rcs);
    std::vector<DecPlanIn> in((size_t)n);
    std::vector<uint32_t> flag((size_t)n, 0u);
    for (int i = 0; i < n; i++) {
        in[(size_t)i] = DecPlanIn{0, 0, 0, 0, false};
        if (tbatch_default_takes(streams[i], lens[i], true, &in[(size_t)i], &flag[(size_t)i]))
            in[(size_t)i].takes = coeffs[i] && cap_blocks[i] >= num_blocks(in[(size_t)i].h, in[(size_t)i].w); // (else: the single call's TIC_E_SPACE)
    }
    // (a failure in front of the chunks leaves every frame to the single call, as a failure inside one does: only the arguments fail the whole call)
    int rc = hipSetDevice(ctx->device) == hipSuccess ? ensure_dec_tables(ctx) : TIC_E_HIP;
    const DecPlan plan = rc == TIC_OK ? plan_transcode_default_reader(in.data(), n, tbatch_limits()) : DecPlan();
    for (const DecPlanChunk &c : plan.chunks) {
        const DecPlanFrame *pf = &plan.frames[(size_t)c.first];
        // coefficients: the context's scratch on the device, the host decoder's pinned landing buffer for the ONE download
        if ((rc = ensure_scratch(ctx, 0, c.blocks * 128)) || (rc = ctx->h_zz.grow(ctx, c.blocks * 128))) break;
        bool refused = false;
        if ((rc = tbatch_read_default(ctx, streams, pf, c, (int16_t *)ctx->d_coef.p, &refused))) break;
        if (refused) continue;
        if (hipMemcpyAsync(ctx->h_zz, ctx->d_coef, c.blocks * 128, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
            (void)hipGetLastError();
            break;
        }
        ctx->last_tbatch_chunks++;
        for (int k = 0; k < c.count; k++) {
            const DecPlanFrame &f = pf[k];
            if (!dec_status_complete(ctx->dbat.ws.h_status[k], streams[f.index], f.nblk)) continue;
            memcpy(coeffs[f.index], ctx->h_zz + (size_t)f.blk0 * 64, f.nblk * 128);
            if (hs) hs[f.index] = f.h;
            if (ws) ws[f.index] = f.w;
            if (qualities) qualities[f.index] = f.quality;
            if (flags) flags[f.index] = flag[(size_t)f.index];
            call.finished(f.index);
        }
    }
    return call.end(single, rcs);
}

// The adaptive writer's stage of a chunk whose coefficients are resident at d_coef (rows as the reader's plan says) and whose statistics launch has
// run on all its frames with slot table `v` (tf[k].skip: the reader did not complete frame k - its statistics are not looked at, it is not packed):
// tables on the host, ONE upload, bits / scan / write, ONE download of the streams.  A frame whose stream does not fit caps[] gets TIC_E_SPACE and
// the needed length; a frame the table build refuses is left to the single call.
static int tbatch_write_adaptive(tic_ctx *ctx, TBatchCall &call, Slot &s, const AdaptSlotView &v, TranscodeFrame *tf, int count, size_t ngroups, const int16_t *d_coef,
                                 uint8_t *const *outs, const size_t *caps, size_t *out_lens) {
    unsigned long long total_bits[kEntropyMaxFrames];
    uint32_t base_bits[kEntropyMaxFrames];
    bool any = false;
    for (int k = 0; k < count; k++) {
        total_bits[k] = 0ull, base_bits[k] = 0u, s.h_lens[k] = 0ull;
        if (tf[k].skip) continue;
        const AdaptStats &hs = v.h_stats[k];
        uint8_t *head = v.h_heads + (size_t)k * kAdaptHeadStride;
        memset(head, 0, kAdaptHeadStride);
        write_header(head, tf[k].h, tf[k].w, tf[k].quality);
        head[12] = 0x80; // write_uint(1 << 31, 32): most significant bit first (codec.py:111)
        unsigned long long dc_code[16], ac_code[256];
        uint8_t dc_len[16], ac_len[256];
        size_t tbits = 0;
        if (hs.err || huffman_table_build(hs.count + kAdaptDcBin, hs.first + kAdaptDcBin, hs.count, hs.first, dc_code, dc_len, ac_code, ac_len, head + 16,
                                          kAdaptMaxTableBytes, &tbits) != TIC_OK) {
            tf[k].skip = true; // (the single call words it)
            continue;
        }
        HuffWide &tab = v.h_tabs[k];
        for (int i = 0; i < kAdaptBins; i++) {
            const bool dc = i >= kAdaptDcBin;
            tab.code[i] = dc ? dc_code[i - kAdaptDcBin] : ac_code[i];
            tab.len[i] = dc ? dc_len[i - kAdaptDcBin] : ac_len[i];
        }
        base_bits[k] = (uint32_t)(128 + tbits);
        const unsigned long long total = adaptive_stream_bits(hs.count + kAdaptDcBin, hs.count, dc_len, ac_len, tbits);
        const size_t bytes = (size_t)((total + 7) / 8), cap = caps[tf[k].index];
        if (bytes > cap) { // tic_retable_adaptive's refusal, from the same figures
            out_lens[tf[k].index] = bytes;
            call.failed(tf[k].index, TIC_E_SPACE, tbatch_short_msg(bytes, cap));
            tf[k].skip = true;
            continue;
        }
        total_bits[k] = total, s.h_lens[k] = bytes;
        any = true;
    }
    if (!any) return TIC_OK;
    size_t stream_bytes = 0, landing = 0, maxlen = 0;
    assign_adaptive_streams(v.h_frames, count, total_bits, base_bits, &stream_bytes);
    for (int k = 0; k < count; k++) {
        v.h_rb->rec[k].out_off = v.h_frames->rec[k].out_off; // (all the read-back kernel reads of its table)
        s.h_rb_off[k] = landing;
        landing += align_up((size_t)s.h_lens[k], 64);
        maxlen = std::max(maxlen, (size_t)s.h_lens[k]);
    }
    int rc = s.d_streams.grow(ctx, stream_bytes, stream_bytes + stream_bytes / 4);
    if (rc == TIC_OK) rc = s.pin_out.grow(ctx, landing, landing + landing / 4);
    if (rc) return rc;
    *v.h_err = 0u;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemsetAsync(s.d_streams, 0, stream_bytes, st));
    HIPCHK(ctx, hipMemcpyAsync(s.d_adapt + v.l.err, s.h_adapt + v.l.err, v.l.upload_end - v.l.err, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, adaptive_pack_v(d_coef, v.d_frames, count, ngroups, v.d_tabs, v.d_heads, (uint32_t *)(s.d_adapt + v.l.bbits), (unsigned long long *)(s.d_adapt + v.l.gsum),
                                s.d_streams, v.d_err, st));
    HIPCHK(ctx, hipMemcpyAsync(s.h_err, v.d_err, sizeof(int), hipMemcpyDeviceToHost, st));
    const unsigned gx = (unsigned)std::min<size_t>(64, (maxlen / 16 + 255) / 256 + 1);
    hipLaunchKernelGGL(readback_frames_kernel, dim3(gx, (unsigned)count), dim3(256), 0, st, (const unsigned char *)s.d_streams, v.d_rb, s.h_lens, s.h_rb_off,
                       (unsigned char *)s.pin_out);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (*s.h_err) return set_err(ctx, TIC_E_HIP, "packing reached past a stream's computed length (statistics and packing disagree)");
    for (int k = 0; k < count; k++) {
        if (tf[k].skip) continue;
        memcpy(outs[tf[k].index], (const char *)s.pin_out.p + s.h_rb_off[k], (size_t)s.h_lens[k]);
        out_lens[tf[k].index] = (size_t)s.h_lens[k];
        call.finished(tf[k].index);
    }
    return TIC_OK;
}

// The batch slot the writers borrow (slot 0: its tables, length words, error flags, stream areas and landing buffer; no batch call is in flight
// while a transcoding call holds the context's lock).
static int tbatch_slot(tic_ctx *ctx, size_t work_bytes, size_t stream_bytes, Slot **s) {
    tic_ctx::SlotNeed need;
    need.frames = kEntropyMaxFrames, need.work = work_bytes, need.streams = stream_bytes, need.pin_out = stream_bytes ? stream_bytes + 64 * (size_t)kEntropyMaxFrames : 0;
    const int rc = ensure_batch_slots(ctx, need);
    if (rc) return rc;
    *s = &ctx->bslots[0];
    return TIC_OK;
}

int tic_retable_adaptive_batch(tic_ctx *ctx, const uint8_t *const *streams, const size_t *lens, int n, uint8_t *const *outs, const size_t *caps,
                               size_t *out_lens, int *rcs) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (n < 0 || (n > 0 && (!streams || !lens || !outs || !caps || !out_lens))) return set_err(ctx, TIC_E_ARG, "bad batch arguments");
    TBatchCall call(ctx, n);
    if (n == 0) return TIC_OK;
    const auto single = [&](int i) { return tic_retable_adaptive(ctx, streams[i], lens[i], outs[i], caps[i], &out_lens[i]); };
    if (n == 1) return call.end(single, rcs);
    std::vector<DecPlanIn> in((size_t)n);
    for (int i = 0; i < n; i++) {
        uint32_t flag = 0;
        in[(size_t)i] = DecPlanIn{0, 0, 0, 0, false};
        if (tbatch_default_takes(streams[i], lens[i], false, &in[(size_t)i], &flag)) in[(size_t)i].takes = outs[i] != nullptr;
    }
    int rc = hipSetDevice(ctx->device) == hipSuccess ? ensure_dec_tables(ctx) : TIC_E_HIP; // (a failure here: every frame to the single call)
    Slot *sp = nullptr;
    if (rc == TIC_OK) rc = tbatch_slot(ctx, 0, 0, &sp);
    const DecPlan plan = rc == TIC_OK ? plan_transcode_default_reader(in.data(), n, tbatch_limits()) : DecPlan();
    for (const DecPlanChunk &c : plan.chunks) {
        const DecPlanFrame *pf = &plan.frames[(size_t)c.first];
        Slot &s = *sp;
        TranscodeFrame tf[kEntropyMaxFrames];
        for (int k = 0; k < c.count; k++) tf[k] = transcode_frame(pf[k]);
        size_t span = 0, ngroups = 0;
        AdaptFrameTable table;
        if (!transcode_adaptive_table(&table, tf, c.count, &span, &ngroups)) continue; // (its frames go one by one)
        const AdaptSlotLayout l = adaptive_slot_layout((size_t)c.count, span, ngroups);
        if ((rc = ensure_scratch(ctx, 0, c.blocks * 128)) || (rc = s.d_adapt.grow(ctx, l.end, l.end + l.end / 4)) || (rc = s.h_adapt.grow(ctx, l.upload_end, l.upload_end + l.upload_end / 4))) break;
        const AdaptSlotView v = adapt_view(s, (size_t)c.count, span, ngroups);
        *v.h_frames = table;
        // 1. one upload, 2. the reader's two launches, 3. the statistics of every frame on the resident rows, 4. ONE read-back: the statistics by copy,
        // the reader's status words through host-mapped memory
        bool refused = false;
        const int16_t *d_coef = (const int16_t *)ctx->d_coef.p;
        if ((rc = tbatch_read_default(ctx, streams, pf, c, (int16_t *)ctx->d_coef.p, &refused))) break;
        if (refused) continue;
        hipError_t e = hipMemcpyAsync(v.d_frames, v.h_frames, sizeof(AdaptFrameTable), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = adaptive_stats_v(d_coef, v.d_frames, c.count, ngroups, v.d_stats, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(v.h_stats, v.d_stats, (size_t)c.count * sizeof(AdaptStats), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            break;
        }
        ctx->last_tbatch_chunks++;
        for (int k = 0; k < c.count; k++) tf[k].skip = !dec_status_complete(ctx->dbat.ws.h_status[k], streams[pf[k].index], pf[k].nblk);
        // 5. tables on the host, 6. one upload, 7. bits / scan / write, 8. one download
        if ((rc = tbatch_write_adaptive(ctx, call, s, v, tf, c.count, ngroups, d_coef, outs, caps, out_lens))) break;
    }
    return call.end(single, rcs);
}

// The default writer's stage of a chunk whose coefficients are resident at d_coef: the mixed batch's descriptor-form pack and place launches on the
// frames that are not skipped, ONE read-back of the lengths and the flag, the streams' own bytes into the slot's landing buffer, hand-out.  The
// launch has ONE error flag for all its frames: where it says that a coefficient has no default code (1), the frames [lo, hi) it ran on are halved and
// each half is launched again - the coefficients are still resident - until the flagged frames stand alone; those are left to the single call, which
// words the error.  (One such frame among 64: twelve more launches, no reader run again.)
static int tbatch_write_default(tic_ctx *ctx, TBatchCall &call, Slot &s, const TranscodeFrame *chunk, int count, int lo, int hi, size_t blocks, const int16_t *d_coef,
                                uint8_t *const *outs, const size_t *caps, size_t *out_lens) {
    TranscodeFrame tf[kEntropyMaxFrames];
    for (int k = 0; k < count; k++) {
        tf[k] = chunk[k];
        tf[k].skip = tf[k].skip || k < lo || k >= hi;
    }
    int qmax = 0;
    for (int k = 0; k < count; k++) qmax = !tf[k].skip && tf[k].quality > qmax ? tf[k].quality : qmax;
    int mode = qmax <= ctx->ent_lane_max_quality ? kEntropyLanePerBlock : kEntropyEightLanes;
    int entry[kEntropyMaxFrames], m = 0;
    hipStream_t st = ctx->stream;
    for (;;) {
        size_t stream_bytes = 0, nparts, ngroups, nplaces;
        if (!transcode_entropy_table(s.h_frames, mode, tf, count, entry, &m, &stream_bytes, &nparts, &ngroups, &nplaces)) return TIC_OK; // (no frame left, or one too large: one by one)
        int rc = s.d_streams.grow(ctx, stream_bytes, stream_bytes + stream_bytes / 4);
        if (rc == TIC_OK) rc = s.pin_out.grow(ctx, stream_bytes + 64 * (size_t)m);
        const size_t wb = entropy_fused_work_bytes_v(blocks, (size_t)m);
        if (rc == TIC_OK) rc = s.d_work.grow(ctx, wb, wb + wb / 4);
        if (rc) return rc;
        const int par = s.parity;
        s.parity ^= 1;
        HIPCHK(ctx, hipMemcpyAsync(s.d_frames, s.h_frames, sizeof(EntropyFrameTable), hipMemcpyHostToDevice, st));
        HIPCHK(ctx, entropy_gpu_fused_v(d_coef, s.h_frames, s.d_frames, m, ctx->d_huff, s.d_work, s.d_work.cap, s.d_streams, s.d_lens, s.d_err + par, s.d_err + (par ^ 1), mode, st));
        HIPCHK(ctx, hipMemcpyAsync(s.h_lens, s.d_lens, (size_t)m * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(s.h_err, s.d_err + par, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (*s.h_err == 4 && mode == kEntropyLanePerBlock) { // a block exceeds the lane-per-block kernel's strings: once more with the 8-lane kernel
            mode = kEntropyEightLanes;
            continue;
        }
        break;
    }
    if (*s.h_err) { // (1: a symbol without a default code somewhere in [lo, hi))
        if (hi - lo <= 1) return TIC_OK;
        const int mid = lo + (hi - lo) / 2;
        const int rc = tbatch_write_default(ctx, call, s, chunk, count, lo, mid, blocks, d_coef, outs, caps, out_lens);
        return rc ? rc : tbatch_write_default(ctx, call, s, chunk, count, mid, hi, blocks, d_coef, outs, caps, out_lens);
    }
    size_t off = 0, maxlen = 0;
    for (int k = 0; k < count; k++) {
        const int j = entry[k];
        if (j < 0) continue;
        const size_t len = (size_t)s.h_lens[j], cap = caps[tf[k].index];
        if (len > cap) { // tic_retable_default's refusal, from the same length
            out_lens[tf[k].index] = len;
            call.failed(tf[k].index, TIC_E_SPACE, tbatch_short_msg(len, cap));
            s.h_lens[j] = 0ull;
            entry[k] = -1;
        }
        s.h_rb_off[j] = off;
        off += align_up((size_t)s.h_lens[j], 64);
        maxlen = std::max(maxlen, (size_t)s.h_lens[j]);
    }
    if (maxlen == 0) return TIC_OK;
    const unsigned gx = (unsigned)std::min<size_t>(64, (maxlen / 16 + 255) / 256 + 1);
    hipLaunchKernelGGL(readback_frames_kernel, dim3(gx, (unsigned)m), dim3(256), 0, st, (const unsigned char *)s.d_streams, s.d_frames, s.h_lens, s.h_rb_off,
                       (unsigned char *)s.pin_out);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int k = 0; k < count; k++) {
        const int j = entry[k];
        if (j < 0) continue;
        memcpy(outs[tf[k].index], (const char *)s.pin_out.p + s.h_rb_off[j], (size_t)s.h_lens[j]);
        out_lens[tf[k].index] = (size_t)s.h_lens[j];
        call.finished(tf[k].index);
    }
    return TIC_OK;
}

int tic_retable_default_batch(tic_ctx *ctx, const uint8_t *const *streams, const size_t *lens, int n, uint8_t *const *outs, const size_t *caps,
                              size_t *out_lens, int *rcs) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (n < 0 || (n > 0 && (!streams || !lens || !outs || !caps || !out_lens))) return set_err(ctx, TIC_E_ARG, "bad batch arguments");
    TBatchCall call(ctx, n);
    if (n == 0) return TIC_OK;
    const auto single = [&](int i) { return tic_retable_default(ctx, streams[i], lens[i], outs[i], caps[i], &out_lens[i]); };
    if (n == 1) return call.end(single, rcs);
    // the frames tic_decompress_batch_adaptive's reader takes (adaptive_batch_takes), behind the header checks of tic_retable_default
    std::vector<AdaptDecPlanIn> in((size_t)n);
    std::vector<AdaptTable> tabs; // of the frames taken, in order
    {
        AdaptTable t;
        for (int i = 0; i < n; i++) {
            int h = 0, w = 0, q = 0;
            uint32_t flag = 0;
            in[(size_t)i] = AdaptDecPlanIn{0, 0, 0, 0, 0, false};
            if (!streams[i] || !outs[i] || parse_header(streams[i], lens[i], &h, &w, &q, &flag) != TIC_OK || h < 0 || w < 0 || q < 1 || q > 99) continue;
            in[(size_t)i] = AdaptDecPlanIn{h, w, q, lens[i], 0, adaptive_batch_takes(num_blocks(h, w), streams[i], lens[i], &t)};
            if (in[(size_t)i].takes) in[(size_t)i].payload_bit = t.payload_bit, tabs.push_back(t);
        }
    }
    if (tabs.size() < 2) { // (adaptive_batch_takes: no batch of one)
        for (AdaptDecPlanIn &f : in) f.takes = false;
        tabs.clear();
    }
    Slot *sp = nullptr;
    int rc = hipSetDevice(ctx->device) == hipSuccess ? tbatch_slot(ctx, 0, 0, &sp) : TIC_E_HIP; // (a failure here: every frame to the single call)
    const AdaptDecPlan plan = rc == TIC_OK ? plan_transcode_adaptive_reader(in.data(), n, tbatch_limits()) : AdaptDecPlan();
    const DecBatchIO io = {streams, lens, outs, caps};
    for (const AdaptDecPlanChunk &c : plan.chunks) {
        const AdaptDecPlanFrame *pf = &plan.frames[(size_t)c.first];
        std::vector<char> good;
        if ((rc = adbatch_decode(ctx, io, pf, c, &tabs[(size_t)c.first], &good, false))) break;
        ctx->last_tbatch_chunks++;
        TranscodeFrame tf[kEntropyMaxFrames];
        for (int k = 0; k < c.count; k++) {
            tf[k] = transcode_frame(pf[k]);
            tf[k].skip = !good[(size_t)k];
        }
        const int16_t *d_coef = (const int16_t *)(ctx->adbat.d_work + AdaptDecWorkLayout(c).o_coef);
        if ((rc = tbatch_write_default(ctx, call, *sp, tf, c.count, 0, c.count, c.blocks, d_coef, outs, caps, out_lens))) break;
    }
    return call.end(single, rcs);
}

int tic_last_transcode_batch(tic_ctx *ctx, int *batch_frames, int *single_frames, int *chunks) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (batch_frames) *batch_frames = ctx->last_tbatch_frames;
    if (single_frames) *single_frames = ctx->last_tbatch_single;
    if (chunks) *chunks = ctx->last_tbatch_chunks;
    return TIC_OK;
}

// ---- rate control of the adaptive family (include/tinyimgcodec_hip_adaptive_rate.h) ------------------------------------------------------------
// The length of an adaptive stream is a function of its symbol statistics alone (adaptive_stream_size, tic_adaptive.cpp), so a PROBE here is
// the transform into the coefficient workspace and the statistics of what it left: the probes of a submission lie back to back in the
// workspace (layout_rate_submission: passes where they exceed it), one statistics launch takes up to kSizeMaxProbes of them, ONE read-back
// brings all their statistics, and the host builds a table and a length per probe.  Plan, chunks, uploads, transform runs and the bisection
// are rate control's (tic_rate_plan.h); a single frame is a plan of one frame.
int tic_adaptive_stream_size(const uint64_t *dc_count, const uint64_t *dc_first, const uint64_t *ac_count, const uint64_t *ac_first, size_t *bytes) {
    return adaptive_stream_size((const unsigned long long *)dc_count, (const unsigned long long *)dc_first, (const unsigned long long *)ac_count,
                                (const unsigned long long *)ac_first, bytes);
}

int tic_entropy_size_adaptive(const int16_t *coeffs_zz, int h, int w, size_t *bytes) { return entropy_size_adaptive(coeffs_zz, h, w, bytes); }

// The statistics kernel of the size and search routes: 0 = adaptive_stats_probe_kernel_v, 1 = adaptive_stats_v_kernel (profiles/adaptive_rate.txt).
static constexpr int kAdaptRateKernel = 0;

// One statistics launch: probes [first, first + count) of a submission, back to back from block `first_block` of the coefficients.
struct AdaptStatsLaunch {
    size_t first_block;
    int first, count;
};

// Buffers and tables of a submission of np probes (nblk[i] blocks each) cut into `launches`, queued on the context's stream: the statistics
// reset (kernel 0; adaptive_stats_v resets its own), ONE upload of every launch's table.  groups[t]: launch t's grid.  Nothing of an
// earlier submission may be in flight: the buffers may grow.
static int prepare_adaptive_stats(tic_ctx *ctx, const std::vector<AdaptStatsLaunch> &launches, const size_t *nblk, int np, int kernel, int max_groups,
                                  std::vector<size_t> &groups) {
    const size_t st_bytes = (size_t)np * sizeof(AdaptStats), st_alloc = align_up(st_bytes, 65536);
    int rc = ctx->d_arate_stats.grow(ctx, st_bytes, st_alloc);
    if (rc) return rc;
    rc = ctx->h_arate_stats.grow(ctx, st_bytes, st_alloc);
    if (rc) return rc;
    const size_t nt = launches.size();
    groups.assign(nt, 0);
    if (kernel == 0) {
        const size_t tab_bytes = nt * sizeof(SizeProbeTable), tab_alloc = align_up(tab_bytes, 16384);
        rc = ctx->h_rate_tabs.grow(ctx, tab_bytes, tab_alloc);
        if (rc) return rc;
        rc = ctx->d_rate_tabs.grow(ctx, tab_bytes, tab_alloc);
        if (rc) return rc;
        for (size_t t = 0; t < nt; t++) {
            const AdaptStatsLaunch &l = launches[t];
            uint32_t result[kSizeMaxProbes];
            size_t total = 0;
            for (int k = 0; k < l.count && k < kSizeMaxProbes; k++) result[k] = (uint32_t)(l.first + k);
            if (!fill_size_probe_table(&ctx->h_rate_tabs[t], l.count, nblk + l.first, result, &groups[t], &total) ||
                !cap_probe_groups(&ctx->h_rate_tabs[t], l.count, max_groups, &groups[t]))
                return set_err(ctx, TIC_E_ARG, "adaptive statistics: probes %d.. have no table", l.first);
        }
        HIPCHK(ctx, adaptive_stats_probe_reset(ctx->d_arate_stats, np, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_rate_tabs, ctx->h_rate_tabs, tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    } else {
        const size_t tab_bytes = nt * sizeof(AdaptFrameTable), tab_alloc = align_up(tab_bytes, 16384);
        rc = ctx->h_arate_frames.grow(ctx, tab_bytes, tab_alloc);
        if (rc) return rc;
        rc = ctx->d_arate_frames.grow(ctx, tab_bytes, tab_alloc);
        if (rc) return rc;
        for (size_t t = 0; t < nt; t++) {
            size_t total = 0;
            if (!fill_adaptive_table(&ctx->h_arate_frames[t], launches[t].count, nblk + launches[t].first, &total, &groups[t]))
                return set_err(ctx, TIC_E_ARG, "adaptive statistics: probes %d.. have no table", launches[t].first);
        }
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_arate_frames, ctx->h_arate_frames, tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    return TIC_OK;
}

// Launch t of a prepared submission on the coefficients at d_zz (block 0 of the submission's layout).
static hipError_t launch_adaptive_stats(tic_ctx *ctx, const int16_t *d_zz, const AdaptStatsLaunch &l, size_t t, int kernel, size_t groups) {
    ctx->last_arate_launches++;
    if (kernel == 0) return adaptive_stats_probe_v(d_zz + l.first_block * 64, ctx->d_rate_tabs + t, groups, ctx->d_arate_stats, ctx->stream);
    return adaptive_stats_v(d_zz + l.first_block * 64, ctx->d_arate_frames + t, l.count, groups, ctx->d_arate_stats + l.first, ctx->stream);
}

static int check_stats_v_args(tic_ctx *ctx, const void *d_coeffs_zz, int nprobes, const size_t *nblocks, int kernel, int max_groups) {
    if (nprobes < 1 || nprobes > kSizeMaxProbes) return set_err(ctx, TIC_E_ARG, "probe count %d outside 1..%d", nprobes, kSizeMaxProbes);
    if (!d_coeffs_zz || !nblocks) return set_err(ctx, TIC_E_ARG, "null coefficient pointer or block counts");
    if (kernel != 0 && kernel != 1) return set_err(ctx, TIC_E_ARG, "kernel %d is neither 0 (probe kernel) nor 1 (adaptive_stats_v_kernel)", kernel);
    if (max_groups < 0) return set_err(ctx, TIC_E_ARG, "negative workgroup cap %d", max_groups);
    for (int k = 0; k < nprobes; k++)
        if (nblocks[k] == 0) return set_err(ctx, TIC_E_ARG, "probe %d has no blocks", k);
    return TIC_OK;
}

int tic_adaptive_stats_v_dev(tic_ctx *ctx, const void *d_coeffs_zz, int nprobes, const size_t *nblocks, int kernel, int max_groups, uint64_t *count,
                             uint64_t *first, uint32_t *err) {
    TIC_LOCK(ctx);
    if (!ctx || !count || !first || !err) return TIC_E_ARG;
    int rc = check_stats_v_args(ctx, d_coeffs_zz, nprobes, nblocks, kernel, max_groups);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const std::vector<AdaptStatsLaunch> launches{{0, 0, nprobes}};
    std::vector<size_t> groups;
    rc = prepare_adaptive_stats(ctx, launches, nblocks, nprobes, kernel, max_groups, groups);
    if (rc) return rc;
    HIPCHK(ctx, launch_adaptive_stats(ctx, (const int16_t *)d_coeffs_zz, launches[0], 0, kernel, groups[0]));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_arate_stats, ctx->d_arate_stats, (size_t)nprobes * sizeof(AdaptStats), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, wait_stream(ctx));
    for (int k = 0; k < nprobes; k++) {
        const AdaptStats &s = ctx->h_arate_stats[k];
        memcpy(count + (size_t)k * kAdaptBins, s.count, sizeof s.count);
        memcpy(first + (size_t)k * kAdaptBins, s.first, sizeof s.first);
        err[k] = s.err;
    }
    return TIC_OK;
}

int tic_adaptive_stats_v_dev_timed(tic_ctx *ctx, const void *d_coeffs_zz, int nprobes, const size_t *nblocks, int kernel, int max_groups, int warm,
                                   int iters, float *ms_total) {
    TIC_LOCK(ctx);
    if (!ctx || !ms_total || warm < 0 || iters <= 0) return TIC_E_ARG;
    int rc = check_stats_v_args(ctx, d_coeffs_zz, nprobes, nblocks, kernel, max_groups);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const std::vector<AdaptStatsLaunch> launches{{0, 0, nprobes}};
    std::vector<size_t> groups;
    rc = prepare_adaptive_stats(ctx, launches, nblocks, nprobes, kernel, max_groups, groups);
    if (rc) return rc;
    return timed_launches(ctx, warm, iters, ms_total, nullptr, [&](int, hipEvent_t, hipEvent_t) {
        if (kernel == 0) {
            const hipError_t e = adaptive_stats_probe_reset(ctx->d_arate_stats, nprobes, ctx->stream);
            if (e != hipSuccess) return e;
        }
        return launch_adaptive_stats(ctx, (const int16_t *)d_coeffs_zz, launches[0], 0, kernel, groups[0]);
    });
}

// Stream length from a probe's statistics: -1 where tic_compress_adaptive returns TIC_E_RANGE (a category or size above 15, or a code
// and its value bits beyond kAdaptMaxSymbolBits); any other failure of the table build is the call's.
static int adaptive_probe_size(tic_ctx *ctx, const AdaptStats &st, long long *size) {
    if (st.err) {
        *size = -1;
        return TIC_OK;
    }
    size_t bytes = 0;
    const int rc = adaptive_stream_size(st.count + kAdaptDcBin, st.first + kAdaptDcBin, st.count, st.first, &bytes);
    if (rc == TIC_E_RANGE) {
        *size = -1;
        return TIC_OK;
    }
    if (rc) return set_err(ctx, rc, "Huffman table build failed");
    *size = (long long)bytes;
    return TIC_OK;
}

// Queues the probes of `s` - frames of plan `p`, their pixels at img_base + MixedFrame::img_off - and the copy of their statistics into
// ctx->h_arate_stats, entry i for probe i; the caller waits for the stream.  No host wait in here.
static int submit_adaptive_probes(tic_ctx *ctx, const RatePlan &p, RateSubmission &s, const void *img_base) {
    const int np = (int)s.probes.size();
    layout_rate_submission(p.mixed, s, kRateWorkspaceBytes / 128);
    int rc = ensure_scratch(ctx, 0, s.max_pass_blocks * 128 + 16);
    if (rc) return rc;
    std::vector<size_t> nblk((size_t)np);
    for (int i = 0; i < np; i++) nblk[(size_t)i] = p.mixed.frames[(size_t)s.probes[(size_t)i].frame].nblk;
    std::vector<AdaptStatsLaunch> launches;
    for (size_t i = 0; i + 1 < s.pass_first.size(); i++)
        for (int first = s.pass_first[i]; first < s.pass_first[i + 1]; first += kSizeMaxProbes)
            launches.push_back(AdaptStatsLaunch{s.first_block[(size_t)first], first, std::min(kSizeMaxProbes, s.pass_first[i + 1] - first)});
    std::vector<size_t> groups;
    rc = prepare_adaptive_stats(ctx, launches, nblk.data(), np, kAdaptRateKernel, 0, groups);
    if (rc) return rc;
    size_t t = 0;
    for (size_t i = 0; i + 1 < s.pass_first.size(); i++) {
        const int end = s.pass_first[i + 1];
        rc = queue_rate_transforms(ctx, p, s, s.pass_first[i], end, img_base);
        if (rc) return rc;
        for (int first = s.pass_first[i]; first < end; first += kSizeMaxProbes, t++)
            HIPCHK(ctx, launch_adaptive_stats(ctx, (const int16_t *)ctx->d_coef, launches[t], t, kAdaptRateKernel, groups[t]));
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_arate_stats, ctx->d_arate_stats, (size_t)np * sizeof(AdaptStats), hipMemcpyDeviceToHost, ctx->stream));
    ctx->last_arate_probes += np;
    return TIC_OK;
}

// A plan of ONE frame whose pixels lie at the submission's img_base with their own row stride.
static RatePlan single_frame_rate_plan(int h, int w, ptrdiff_t row_stride, size_t n) {
    RatePlan p;
    MixedFrame f = MixedFrame();
    f.index = 0, f.h = h, f.w = w, f.quality = 0;
    f.nblk = n, f.pitch = (size_t)row_stride, f.img_bytes = (size_t)row_stride * (size_t)h;
    p.mixed.frames.push_back(f);
    p.run_of.push_back(0);
    p.depth.push_back(rate_depth(n));
    return p;
}

static void reset_adaptive_rate(tic_ctx *ctx) { ctx->last_arate_probes = ctx->last_arate_waits = ctx->last_arate_launches = 0; }

static const char *const kAdaptNoBlocks = "an image without blocks has no symbols to build a table from (the reference raises IndexError)";

// The probes of q[0 .. nq) on one resident frame: sizes[i], -1 where the encoder returns TIC_E_RANGE.  One submission, one wait.
static int adaptive_sizes_impl(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, size_t n, const int *q, int nq, long long *sizes) {
    const RatePlan p = single_frame_rate_plan(h, w, row_stride, n);
    RateSubmission s;
    for (int i = 0; i < nq; i++) s.probes.push_back(RateProbe{0, q[i]});
    int rc = submit_adaptive_probes(ctx, p, s, d_image);
    if (rc) return rc;
    HIPCHK(ctx, wait_stream(ctx));
    ctx->last_arate_waits++;
    for (int i = 0; i < nq; i++) {
        rc = adaptive_probe_size(ctx, ctx->h_arate_stats[i], &sizes[i]);
        if (rc) return rc;
    }
    return TIC_OK;
}

int tic_adaptive_sizes_dev(tic_ctx *ctx, const void *d_image, int h, int w, ptrdiff_t row_stride, const int *qualities, int nq, long long *sizes) {
    TIC_LOCK(ctx);
    int rc = check_size_args(ctx, h, w, row_stride, qualities, nq, sizes); // (a bad quality fails here: nothing has been queued)
    if (rc) return rc;
    reset_adaptive_rate(ctx);
    const size_t n = num_blocks(h, w);
    if (n == 0) return set_err(ctx, TIC_E_ARG, "%s", kAdaptNoBlocks);
    if (nq == 0) return TIC_OK;
    if (!d_image) return set_err(ctx, TIC_E_ARG, "null image pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return adaptive_sizes_impl(ctx, d_image, h, w, row_stride, n, qualities, nq, sizes);
}

int tic_adaptive_sizes(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, const int *qualities, int nq, long long *sizes) {
    TIC_LOCK(ctx);
    int rc = check_size_args(ctx, h, w, row_stride, qualities, nq, sizes);
    if (rc) return rc;
    reset_adaptive_rate(ctx);
    const size_t n = num_blocks(h, w);
    if (n == 0) return set_err(ctx, TIC_E_ARG, "%s", kAdaptNoBlocks);
    if (nq == 0) return TIC_OK;
    if (!image) return set_err(ctx, TIC_E_ARG, "null image pointer");
    size_t pitch = 0;
    rc = upload_image(ctx, image, h, w, row_stride, n, &pitch);
    if (rc) return rc;
    return adaptive_sizes_impl(ctx, ctx->d_img, h, w, (ptrdiff_t)pitch, n, qualities, nq, sizes);
}

int tic_compress_adaptive_to_size(tic_ctx *ctx, const uint8_t *image, int h, int w, ptrdiff_t row_stride, size_t max_bytes, int qmin, int qmax,
                                  uint8_t *out, size_t cap, size_t *out_len, int *quality) {
    TIC_LOCK(ctx);
    int rc = check_search_args(ctx, h, w, row_stride, qmin, qmax, out, cap, out_len, quality);
    if (rc) return rc;
    reset_adaptive_rate(ctx);
    const size_t n = num_blocks(h, w);
    if (n == 0) return set_err(ctx, TIC_E_ARG, "%s", kAdaptNoBlocks);
    if (!image) return set_err(ctx, TIC_E_ARG, "null image pointer");
    size_t pitch = 0;
    rc = upload_image(ctx, image, h, w, row_stride, n, &pitch);
    if (rc) return rc;
    const RatePlan p = single_frame_rate_plan(h, w, (ptrdiff_t)pitch, n);
    RateSearch rs;
    rate_search_begin(rs, qmin, qmax, (unsigned long long)max_bytes);
    RateSubmission s;
    for (;;) {
        int cand[kRateMaxCandidates];
        const int nc = rate_search_round(rs, p.depth[0], cand);
        if (nc == 0) break;
        s.probes.clear();
        for (int i = 0; i < nc; i++) s.probes.push_back(RateProbe{0, cand[i]});
        rc = submit_adaptive_probes(ctx, p, s, ctx->d_img);
        if (rc) return rc;
        HIPCHK(ctx, wait_stream(ctx));
        ctx->last_arate_waits++;
        for (int i = 0; i < nc; i++) {
            rc = adaptive_probe_size(ctx, ctx->h_arate_stats[i], &rs.known[cand[i]]);
            if (rc) return rc;
        }
        rate_search_replay(rs);
    }
    if (rs.state == kRateNoCode)
        return set_err(ctx, TIC_E_RANGE, "no adaptive stream at quality %d: a DC category or AC size above 15, or a code and its value bits beyond %d bits",
                       qmin, kAdaptMaxSymbolBits);
    if (rs.state == kRateTooLarge) {
        *out_len = (size_t)rs.known[qmin];
        return set_err(ctx, TIC_E_SPACE, "%lld bytes at quality %d exceed the budget of %zu", rs.known[qmin], qmin, max_bytes);
    }
    // the stream: the adaptive encoder itself at the quality found (its own statistics, table and length: independent of the probe's)
    const int q = rs.lo;
    const size_t len = (size_t)rs.known[q];
    if (len > cap) {
        *out_len = len;
        return set_err(ctx, TIC_E_SPACE, "output buffer too small (%zu bytes needed, %zu given)", len, cap);
    }
    DctqArgs a = make_args(ctx, ctx->d_img, h, w, (ptrdiff_t)pitch, q, ctx->d_coef);
    HIPCHK(ctx, launch_dctq(a, 2, ctx->stream));
    size_t packed = 0;
    rc = adaptive_encode_dev(ctx, n, h, w, q, out, cap, &packed);
    ctx->last_arate_waits++;
    if (rc) return rc;
    if (packed != len) return set_err(ctx, TIC_E_HIP, "the encoded stream (%zu bytes) contradicts its probe (%zu bytes)", packed, len);
    *out_len = len;
    *quality = q;
    return TIC_OK;
}

int tic_adaptive_sizes_v(tic_ctx *ctx, const uint8_t *const *images, int n, const int *hs, const int *ws, const ptrdiff_t *row_strides, const int *qualities,
                         int nq, long long *sizes) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    // every check before any work
    if (n < 0) return set_err(ctx, TIC_E_ARG, "negative frame count %d", n);
    if (nq < 0 || (nq > 0 && !qualities)) return set_err(ctx, TIC_E_ARG, "bad quality list");
    reset_adaptive_rate(ctx);
    if (n == 0) return TIC_OK;
    if (!images || !hs || !ws || !row_strides || (nq > 0 && !sizes)) return set_err(ctx, TIC_E_ARG, "null array argument");
    const RateCall io = {images, hs, ws, row_strides};
    for (int j = 0; j < std::max(nq, 1); j++) {
        const int rc = check_rate_frames(ctx, io, n, nq ? qualities[j] : 50);
        if (rc) return rc;
    }
    for (int i = 0; i < n; i++)
        if (num_blocks(hs[i], ws[i]) == 0) return set_err(ctx, TIC_E_ARG, "frame %d: %s", i, kAdaptNoBlocks);
    if (nq == 0) return TIC_OK;
    const ChunkLimits lim = mixed_chunk_limits();
    const RatePlan p = plan_rate_batch(hs, ws, n, lim.frames, lim.bytes);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int brc = probe_every_quality(
        ctx, p, io, qualities, nq, &ctx->last_arate_waits, [&](RateSubmission &s) { return submit_adaptive_probes(ctx, p, s, ctx->d_img); },
        [&](size_t pr, int, size_t at) { return adaptive_probe_size(ctx, ctx->h_arate_stats[pr], &sizes[at]); });
    if (brc) return brc;
    int probes = ctx->last_arate_probes, waits = ctx->last_arate_waits, launches = ctx->last_arate_launches;
    for (int i : p.mixed.single) { // what the batch does not take, behind it, frame by frame
        const int rc = tic_adaptive_sizes(ctx, images[i], hs[i], ws[i], row_strides[i], qualities, nq, sizes + (size_t)i * nq);
        probes += ctx->last_arate_probes, waits += ctx->last_arate_waits, launches += ctx->last_arate_launches;
        if (rc) return frame_err(ctx, rc, i);
    }
    ctx->last_arate_probes = probes, ctx->last_arate_waits = waits, ctx->last_arate_launches = launches;
    return TIC_OK;
}

int tic_last_adaptive_rate(tic_ctx *ctx, int *probes, int *host_waits, int *stats_launches) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (probes) *probes = ctx->last_arate_probes;
    if (host_waits) *host_waits = ctx->last_arate_waits;
    if (stats_launches) *stats_launches = ctx->last_arate_launches;
    return TIC_OK;
}

// ---- requantisation (tinyimgcodec_hip_requantize.h): a stream's coefficients at another quality, and the streams written from them -------------
// The reader is tic_entropy_decode's (read_default_coefs), the writers are tic_retable_default's and tic_retable_adaptive's; in between the
// store kernel (tic_requant_gpu.hip) works IN PLACE on ctx->d_coef for a stream that is written; a size table or a search runs the measuring
// kernel on ctx->d_coef, which stores nothing: the source stays where the reader left it, so the stream is read once whatever the number
// of qualities.
static void reset_requant(tic_ctx *ctx) { ctx->last_rq_route = ctx->last_rq_measure = ctx->last_rq_store = ctx->last_rq_rounds = 0; }

static int ensure_requant_tabs(tic_ctx *ctx, size_t launches) {
    const size_t bytes = launches * sizeof(RequantLaunch);
    const int rc = ctx->h_requant_tabs.grow(ctx, bytes, align_up(bytes, 16384));
    return rc ? rc : ctx->d_requant_tabs.grow(ctx, bytes, align_up(bytes, 16384));
}

// Launch t of a call, queued: the n jobs go up in its table together with their zeroed flags, the kernel runs, the flags come back into
// ctx->h_requant_tabs[t].flags.  The caller waits for the stream before it reads them, and before it fills table t again.
static int queue_requant(tic_ctx *ctx, size_t t, const RequantJobIn *jobs, int n, const int16_t *d_src, size_t src_cap, int16_t *d_dst, size_t dst_cap) {
    RequantLaunch *h = ctx->h_requant_tabs + t, *d = ctx->d_requant_tabs + t;
    size_t ngroups = 0;
    if (!fill_requant_job_table(&h->tab, n, jobs, src_cap, dst_cap, &ngroups)) return set_err(ctx, TIC_E_ARG, "requantise: %d jobs have no table", n);
    memset(h->flags, 0, sizeof h->flags);
    HIPCHK(ctx, hipMemcpyAsync(d, h, sizeof *h, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, requant_gpu_v(d_src, d_dst, &d->tab, ngroups, ctx->d_consts, d->flags, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(h->flags, d->flags, sizeof h->flags, hipMemcpyDeviceToHost, ctx->stream));
    ctx->last_rq_store++;
    return TIC_OK;
}

static int check_requant_quality(tic_ctx *ctx, int q, const char *which) {
    return q < 1 || q > 99 ? set_err(ctx, TIC_E_QUALITY, "%s quality %d outside 1..99", which, q) : TIC_OK;
}

static int requantize_zz_impl(tic_ctx *ctx, const void *coeffs, size_t n, int q_from, int q_to, void *out, bool on_device) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    reset_requant(ctx);
    int rc = check_requant_quality(ctx, q_from, "source");
    if (rc == TIC_OK) rc = check_requant_quality(ctx, q_to, "target");
    if (rc) return rc;
    if (n == 0) return TIC_OK;
    if (!coeffs || !out) return set_err(ctx, TIC_E_ARG, "null coefficient pointer");
    if (n > (~(size_t)0 >> 8)) return set_err(ctx, TIC_E_ARG, "%zu blocks are more than an address holds", n);
    const int16_t *d_src = (const int16_t *)coeffs;
    int16_t *d_dst = (int16_t *)out;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (on_device) {
        if ((((uintptr_t)coeffs) | ((uintptr_t)out)) & 15u) return set_err(ctx, TIC_E_ARG, "device coefficient buffers must be 16-byte aligned");
        const uintptr_t a = (uintptr_t)coeffs, b = (uintptr_t)out;
        if (a != b && a < b + n * 128 && b < a + n * 128) return set_err(ctx, TIC_E_ARG, "source and destination overlap without being the same buffer");
    } else {
        rc = ensure_scratch(ctx, 0, n * 128);
        if (rc) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_coef, coeffs, n * 128, hipMemcpyHostToDevice, ctx->stream));
        d_src = d_dst = (int16_t *)ctx->d_coef;
    }
    rc = ensure_requant_tabs(ctx, 1);
    if (rc) return rc;
    const RequantJobIn job = {0, 0, n, q_from, q_to, 0};
    rc = queue_requant(ctx, 0, &job, 1, d_src, n, d_dst, n);
    if (rc) return rc;
    if (!on_device) HIPCHK(ctx, hipMemcpyAsync(out, ctx->d_coef, n * 128, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->h_requant_tabs[0].flags[0]) return set_err(ctx, TIC_E_RANGE, "a coefficient requantised from quality %d to %d leaves int16", q_from, q_to);
    return TIC_OK;
}

int tic_requantize_zz(tic_ctx *ctx, const int16_t *coeffs_zz, size_t nblocks, int from_quality, int to_quality, int16_t *out_zz) {
    return requantize_zz_impl(ctx, coeffs_zz, nblocks, from_quality, to_quality, out_zz, false);
}

int tic_requantize_zz_dev(tic_ctx *ctx, const void *d_coeffs_zz, size_t nblocks, int from_quality, int to_quality, void *d_out_zz) {
    return requantize_zz_impl(ctx, d_coeffs_zz, nblocks, from_quality, to_quality, d_out_zz, true);
}

int tic_requantize_zz_v_dev(tic_ctx *ctx, const void *d_coeffs_zz, size_t src_blocks, int njobs, const size_t *src_block, const size_t *nblocks,
                            const int *from_quality, const int *to_quality, void *d_out_zz, size_t out_blocks, int *range) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    reset_requant(ctx);
    if (njobs < 0 || (njobs > 0 && (!src_block || !nblocks || !from_quality || !to_quality || !range))) return set_err(ctx, TIC_E_ARG, "bad job list");
    if (njobs == 0) return TIC_OK;
    if (src_blocks > (~(size_t)0 >> 8) || out_blocks > (~(size_t)0 >> 8)) return set_err(ctx, TIC_E_ARG, "more blocks than an address holds");
    size_t total = 0;
    for (int k = 0; k < njobs; k++) {
        int rc = check_requant_quality(ctx, from_quality[k], "source");
        if (rc == TIC_OK) rc = check_requant_quality(ctx, to_quality[k], "target");
        if (rc) return rc;
        if (nblocks[k] == 0) return set_err(ctx, TIC_E_ARG, "job %d has no blocks", k);
        if (src_block[k] > src_blocks || nblocks[k] > src_blocks - src_block[k])
            return set_err(ctx, TIC_E_ARG, "job %d reads blocks %zu + %zu of %zu", k, src_block[k], nblocks[k], src_blocks);
        if (nblocks[k] > out_blocks - total) return set_err(ctx, TIC_E_SPACE, "coefficient buffer too small (job %d ends at block %zu)", k, total + nblocks[k]);
        total += nblocks[k];
    }
    if (!d_coeffs_zz || !d_out_zz) return set_err(ctx, TIC_E_ARG, "null coefficient pointer");
    if ((((uintptr_t)d_coeffs_zz) | ((uintptr_t)d_out_zz)) & 15u) return set_err(ctx, TIC_E_ARG, "device coefficient buffers must be 16-byte aligned");
    const uintptr_t a = (uintptr_t)d_coeffs_zz, b = (uintptr_t)d_out_zz;
    if (a < b + out_blocks * 128 && b < a + src_blocks * 128) return set_err(ctx, TIC_E_ARG, "source and destination overlap");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t launches = ((size_t)njobs + kSizeMaxProbes - 1) / kSizeMaxProbes;
    int rc = ensure_requant_tabs(ctx, launches);
    if (rc) return rc;
    size_t at = 0;
    for (size_t t = 0; t < launches; t++) {
        RequantJobIn jobs[kSizeMaxProbes];
        const int first = (int)t * kSizeMaxProbes, cnt = std::min(kSizeMaxProbes, njobs - first);
        for (int k = 0; k < cnt; k++) {
            jobs[k] = RequantJobIn{src_block[first + k], at, nblocks[first + k], from_quality[first + k], to_quality[first + k], (uint32_t)k};
            at += nblocks[first + k];
        }
        rc = queue_requant(ctx, t, jobs, cnt, (const int16_t *)d_coeffs_zz, src_blocks, (int16_t *)d_out_zz, out_blocks);
        if (rc) break;
    }
    if (const hipError_t e = hipStreamSynchronize(ctx->stream); e != hipSuccess && rc == TIC_OK) // (the call ends drained, also one that could not queue all its launches)
        rc = set_err(ctx, TIC_E_HIP, "waiting for the stream failed: %s", hipGetErrorString(e));
    if (rc) return rc;
    for (int k = 0; k < njobs; k++) range[k] = ctx->h_requant_tabs[k / kSizeMaxProbes].flags[k % kSizeMaxProbes] ? 1 : 0;
    return TIC_OK;
}

// The refusals the stream calls share (tic_retable_adaptive's, in its order), all before GPU work.
static int check_requant_header(tic_ctx *ctx, const uint8_t *data, size_t len, StreamHead *sh) {
    if (!data && len) return set_err(ctx, TIC_E_ARG, "null stream pointer");
    int h = 0, w = 0, q = 0;
    uint32_t flag = 0;
    if (parse_header(data, len, &h, &w, &q, &flag) != TIC_OK) return set_err(ctx, TIC_E_STREAM, "stream shorter than the 16-byte header");
    if (flag & (1u << 31)) return set_err(ctx, TIC_E_STREAM, "the stream has an embedded Huffman table: requantisation reads default-table streams");
    if (flag & kFlagScaled) return set_err(ctx, TIC_E_STREAM, "a scaled_dct stream has no quality to requantise from");
    if (h < 0 || w < 0) return set_err(ctx, TIC_E_STREAM, "negative image size in the header");
    if (q < 1 || q > 99) return set_err(ctx, TIC_E_STREAM, "quality %d in the header outside 1..99", q);
    *sh = {h, w, q, -1};
    return TIC_OK;
}

// The stream's n >= 1 blocks into ctx->d_coef: the device reader's never left, the host reader's go up.
static int requant_read(tic_ctx *ctx, const uint8_t *data, size_t len, const StreamHead &sh, size_t n) {
    ctx->last_decode_giveup = 0;
    ctx->last_decode_tries = 0;
    bool dev = false;
    int rc = read_default_coefs(ctx, data, len, false, sh, data, nullptr, &dev);
    if (rc) return rc;
    ctx->last_rq_route = dev ? 1 : 2;
    if (dev) return TIC_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rc = ensure_scratch(ctx, 0, n * 128);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_coef, ctx->h_zz, n * 128, hipMemcpyHostToDevice, ctx->stream));
    return TIC_OK;
}

// The n blocks in ctx->d_coef from quality q_from to q_to in place, then the stream of quality q_to into the caller's host buffer.
static int requant_write(tic_ctx *ctx, size_t n, int h, int w, int q_from, int q_to, bool adaptive, uint8_t *out, size_t cap, size_t *out_len) {
    int rc = ensure_requant_tabs(ctx, 1);
    if (rc) return rc;
    const RequantJobIn job = {0, 0, n, q_from, q_to, 0};
    rc = queue_requant(ctx, 0, &job, 1, (const int16_t *)ctx->d_coef, n, (int16_t *)ctx->d_coef, n);
    if (rc) return rc;
    // the range flag decides before anything is written: a value that left int16 is unspecified in d_coef, and so would its stream be
    HIPCHK(ctx, wait_stream(ctx));
    if (ctx->h_requant_tabs[0].flags[0]) return set_err(ctx, TIC_E_RANGE, "a coefficient requantised from quality %d to %d leaves int16", q_from, q_to);
    if (adaptive) return adaptive_encode_dev(ctx, n, h, w, q_to, out, cap, out_len);
    rc = ctx->d_stream_buf.grow(ctx, compress_bound(h, w)); // (the input stream's copy there, if the device reader made one, is done with)
    if (rc) return rc;
    size_t packed = 0;
    rc = entropy_encode_dev_impl(ctx, ctx->d_coef, h, w, q_to, ctx->d_stream_buf, ctx->d_stream_buf.cap, &packed, false);
    if (rc) return rc;
    if (packed > cap) {
        *out_len = packed;
        return set_err(ctx, TIC_E_SPACE, "output buffer too small (%zu bytes needed, %zu given)", packed, cap);
    }
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->d_stream_buf, packed, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *out_len = packed;
    return TIC_OK;
}

int tic_requantize(tic_ctx *ctx, const uint8_t *data, size_t len, int to_quality, int adaptive, uint8_t *out, size_t cap, size_t *out_len) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    reset_requant(ctx);
    if (!out || !out_len) return set_err(ctx, TIC_E_ARG, "null output pointer");
    StreamHead sh;
    int rc = check_requant_header(ctx, data, len, &sh);
    if (rc == TIC_OK) rc = check_requant_quality(ctx, to_quality, "target");
    if (rc) return rc;
    const size_t n = num_blocks(sh.h, sh.w);
    if (n == 0) {
        if (adaptive) return set_err(ctx, TIC_E_ARG, "an image without blocks has no symbols to build a table from (the reference raises IndexError)");
        *out_len = 16;
        if (cap < 16) return set_err(ctx, TIC_E_SPACE, "output buffer too small (16 bytes needed, %zu given)", cap);
        write_header(out, sh.h, sh.w, to_quality); // the header alone (codec.py:151)
        return TIC_OK;
    }
    rc = requant_read(ctx, data, len, sh, n);
    if (rc) return rc;
    return requant_write(ctx, n, sh.h, sh.w, sh.quality, to_quality, adaptive != 0, out, cap, out_len);
}

// One measuring launch, queued: the sizes of the frame of n blocks at d_src at the nq qualities q[0 .. nq) (at most kSizeMaxProbes), added
// into ctx->d_rate[res0 .. res0 + nq) by the measuring kernel; nothing is stored.  The caller has zeroed and provisioned the results
// (ensure_rate); it waits.  (The composition this replaced - the store kernel into a workspace, then the size kernel's descriptor form -
// lives on in tic_requant_kernels_timed alone, where the two are timed side by side: DESIGN.md 5.14.)
static int queue_requant_sizes(tic_ctx *ctx, const int16_t *d_src, size_t n, int q_from, const int *q, int nq, uint32_t res0) {
    RequantQualities qs;
    qs.nq = nq, qs.q_from = q_from;
    for (int k = 0; k < kSizeMaxProbes; k++) qs.q_to[k] = (uint8_t)(k < nq ? q[k] : 0);
    HIPCHK(ctx, requant_size_gpu_v(d_src, n, qs, ctx->d_consts, ctx->d_size_tab, ctx->d_rate + res0, ctx->stream));
    ctx->last_rq_measure++;
    return TIC_OK;
}

int tic_requantized_sizes(tic_ctx *ctx, const uint8_t *data, size_t len, const int *qualities, int nq, long long *sizes) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    reset_requant(ctx);
    if (nq < 0 || (nq > 0 && (!qualities || !sizes))) return set_err(ctx, TIC_E_ARG, "bad quality list");
    StreamHead sh;
    int rc = check_requant_header(ctx, data, len, &sh);
    for (int i = 0; i < nq && rc == TIC_OK; i++) rc = check_requant_quality(ctx, qualities[i], "target");
    if (rc || nq == 0) return rc;
    const size_t n = num_blocks(sh.h, sh.w);
    if (n == 0) { // header only (codec.py:151)
        for (int i = 0; i < nq; i++) sizes[i] = 16;
        return TIC_OK;
    }
    rc = requant_read(ctx, data, len, sh, n);
    if (rc) return rc;
    // (the measuring kernel writes nothing: a launch takes as many qualities as its table holds)
    const size_t per = (size_t)kSizeMaxProbes, launches = ((size_t)nq + per - 1) / per;
    rc = ensure_rate(ctx, (size_t)nq);
    if (rc == TIC_OK && hipMemsetAsync(ctx->d_rate, 0, (size_t)nq * sizeof(SizeResult), ctx->stream) != hipSuccess)
        rc = set_err(ctx, TIC_E_HIP, "hipMemsetAsync of the size results failed");
    for (size_t t = 0; t < launches && rc == TIC_OK; t++) {
        const size_t first = t * per;
        rc = queue_requant_sizes(ctx, (const int16_t *)ctx->d_coef, n, sh.quality, qualities + first, (int)std::min(per, (size_t)nq - first), (uint32_t)first);
    }
    if (rc == TIC_OK && hipMemcpyAsync(ctx->h_rate, ctx->d_rate, (size_t)nq * sizeof(SizeResult), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = set_err(ctx, TIC_E_HIP, "hipMemcpyAsync of the size results failed");
    if (const hipError_t e = wait_stream(ctx); e != hipSuccess && rc == TIC_OK) // (the call ends drained, also one that could not queue all its passes)
        rc = set_err(ctx, TIC_E_HIP, "waiting for the stream failed: %s", hipGetErrorString(e));
    if (rc) return rc;
    ctx->last_rq_rounds = 1;
    for (int i = 0; i < nq; i++) sizes[i] = probe_size(ctx->h_rate[i]); // (-1: a value without a code or outside int16)
    return TIC_OK;
}

int tic_requantize_to_size(tic_ctx *ctx, const uint8_t *data, size_t len, size_t max_bytes, int qmin, int qmax, uint8_t *out, size_t cap,
                           size_t *out_len, int *quality) {
    TIC_LOCK(ctx);
    if (!ctx || !out_len || !quality) return TIC_E_ARG;
    reset_requant(ctx);
    StreamHead sh;
    int rc = check_requant_header(ctx, data, len, &sh);
    if (rc) return rc;
    if (qmax == 0) qmax = sh.quality;
    if (qmin < 1 || qmax > 99 || qmin > qmax) return set_err(ctx, TIC_E_QUALITY, "quality range %d..%d is not inside 1..99", qmin, qmax);
    if (!out || cap < 16) return set_err(ctx, TIC_E_SPACE, "output buffer too small");
    const size_t n = num_blocks(sh.h, sh.w);
    if (n == 0) { // a header at every quality: the bisection ends at qmax
        *out_len = 16;
        if (max_bytes < 16) return set_err(ctx, TIC_E_SPACE, "16 bytes at quality %d exceed the budget of %zu", qmin, max_bytes);
        write_header(out, sh.h, sh.w, qmax);
        *quality = qmax;
        return TIC_OK;
    }
    rc = requant_read(ctx, data, len, sh, n);
    if (rc) return rc;
    RateSearch rs;
    rate_search_begin(rs, qmin, qmax, (unsigned long long)max_bytes);
    int cand[kRateMaxCandidates];
    while (const int nc = rate_search_round(rs, single_frame_depth(n), cand)) {
        rc = ensure_rate(ctx, (size_t)nc);
        if (rc) return rc;
        if (hipMemsetAsync(ctx->d_rate, 0, (size_t)nc * sizeof(SizeResult), ctx->stream) != hipSuccess)
            rc = set_err(ctx, TIC_E_HIP, "hipMemsetAsync of the size results failed");
        if (rc == TIC_OK) rc = queue_requant_sizes(ctx, (const int16_t *)ctx->d_coef, n, sh.quality, cand, nc, 0);
        if (rc == TIC_OK && hipMemcpyAsync(ctx->h_rate, ctx->d_rate, (size_t)nc * sizeof(SizeResult), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            rc = set_err(ctx, TIC_E_HIP, "hipMemcpyAsync of the size results failed");
        if (const hipError_t e = wait_stream(ctx); e != hipSuccess && rc == TIC_OK) // (a round ends drained, also one that could not queue all of itself)
            rc = set_err(ctx, TIC_E_HIP, "waiting for the stream failed: %s", hipGetErrorString(e));
        if (rc) return rc;
        ctx->last_rq_rounds++;
        for (int i = 0; i < nc; i++) rs.known[cand[i]] = probe_size(ctx->h_rate[i]); // (-1: a value without a code or outside int16)
        rate_search_replay(rs);
    }
    if (rs.state == kRateNoCode)
        return set_err(ctx, TIC_E_RANGE, "a coefficient outside int16 or without a Huffman code at quality %d (reference raises KeyError)", qmin);
    if (rs.state == kRateTooLarge) {
        *out_len = (size_t)rs.known[qmin];
        return set_err(ctx, TIC_E_SPACE, "%lld bytes at quality %d exceed the budget of %zu", rs.known[qmin], qmin, max_bytes);
    }
    const size_t want = (size_t)rs.known[rs.lo];
    if (want > cap) {
        *out_len = want;
        return set_err(ctx, TIC_E_SPACE, "output buffer too small (%zu bytes needed, %zu given)", want, cap);
    }
    rc = requant_write(ctx, n, sh.h, sh.w, sh.quality, rs.lo, false, out, cap, out_len);
    if (rc) return rc;
    if (*out_len != want) // (two independent walks over the same coefficients: cannot differ)
        return set_err(ctx, TIC_E_HIP, "the packed stream (%zu bytes) contradicts its probe (%zu bytes)", *out_len, want);
    *quality = rs.lo;
    return TIC_OK;
}

int tic_requant_kernels_timed(tic_ctx *ctx, const void *d_coeffs_zz, size_t nblocks, int from_quality, const int *qualities, int nq, int mode,
                              int warm, int iters, float *ms_total, long long *sizes) {
    TIC_LOCK(ctx);
    if (!ctx || !ms_total || warm < 0 || iters <= 0) return TIC_E_ARG;
    if (!d_coeffs_zz || ((uintptr_t)d_coeffs_zz & 15u) || nblocks == 0 || nblocks > (~(size_t)0 >> 8) || !qualities || nq < 1 || nq > kSizeMaxProbes ||
        mode < 0 || mode > 2)
        return set_err(ctx, TIC_E_ARG, "bad argument");
    int rc = check_requant_quality(ctx, from_quality, "source");
    for (int i = 0; i < nq && rc == TIC_OK; i++) rc = check_requant_quality(ctx, qualities[i], "target");
    if (rc) return rc;
    reset_requant(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rc = ensure_rate(ctx, (size_t)nq);
    if (rc == TIC_OK && mode != 1) rc = ctx->d_requant.grow(ctx, (size_t)nq * nblocks * 128); // the composition's workspace, tables and flags
    if (rc == TIC_OK && mode != 1) rc = ensure_probe_tabs(ctx, 1, 0);
    if (rc == TIC_OK && mode != 1) rc = ensure_requant_tabs(ctx, 1);
    if (rc) return rc;
    // tables once, in front of the timed interval: what is timed is the kernels (and the memset every measuring run begins with)
    size_t job_groups = 0, size_groups = 0;
    RequantLaunch *const hl = ctx->h_requant_tabs, *const dl = ctx->d_requant_tabs; // (null for mode 1, which uses neither)
    RequantQualities qs;
    qs.nq = nq, qs.q_from = from_quality;
    for (int k = 0; k < kSizeMaxProbes; k++) qs.q_to[k] = (uint8_t)(k < nq ? qualities[k] : 0);
    if (mode != 1) {
        RequantJobIn jobs[kSizeMaxProbes];
        size_t nblk[kSizeMaxProbes], total = 0;
        uint32_t result[kSizeMaxProbes];
        for (int k = 0; k < nq; k++) {
            jobs[k] = RequantJobIn{0, (size_t)k * nblocks, nblocks, from_quality, qualities[k], (uint32_t)k};
            nblk[k] = nblocks, result[k] = (uint32_t)k;
        }
        if (!fill_requant_job_table(&hl->tab, nq, jobs, nblocks, ctx->d_requant.cap / 128, &job_groups) ||
            !fill_size_probe_table(ctx->h_rate_tabs, nq, nblk, result, &size_groups, &total))
            return set_err(ctx, TIC_E_ARG, "requantise: %d jobs have no table", nq);
        memset(hl->flags, 0, sizeof hl->flags);
        HIPCHK(ctx, hipMemcpyAsync(dl, hl, sizeof *hl, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_rate_tabs, ctx->h_rate_tabs, sizeof(SizeProbeTable), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    rc = timed_launches(ctx, warm, iters, ms_total, nullptr, [&](int, hipEvent_t, hipEvent_t) {
        if (mode == 0) return requant_gpu_v((const int16_t *)d_coeffs_zz, ctx->d_requant, &dl->tab, job_groups, ctx->d_consts, dl->flags, ctx->stream);
        hipError_t e = hipMemsetAsync(ctx->d_rate, 0, (size_t)nq * sizeof(SizeResult), ctx->stream); // (every run starts from zeroed results)
        if (e != hipSuccess) return e;
        if (mode == 1) return requant_size_gpu_v((const int16_t *)d_coeffs_zz, nblocks, qs, ctx->d_consts, ctx->d_size_tab, ctx->d_rate, ctx->stream);
        e = requant_gpu_v((const int16_t *)d_coeffs_zz, ctx->d_requant, &dl->tab, job_groups, ctx->d_consts, dl->flags, ctx->stream);
        return e != hipSuccess ? e : stream_size_gpu_v(ctx->d_requant, ctx->d_rate_tabs, size_groups, ctx->d_size_tab, ctx->d_rate, ctx->stream);
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_rate, ctx->d_rate, (size_t)nq * sizeof(SizeResult), hipMemcpyDeviceToHost, ctx->stream));
    if (mode != 1) HIPCHK(ctx, hipMemcpyAsync(hl->flags, dl->flags, sizeof hl->flags, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; sizes && i < nq; i++)
        sizes[i] = mode == 0 ? 0 : (mode == 2 && hl->flags[i]) ? -1ll : probe_size(ctx->h_rate[i]);
    return TIC_OK;
}

int tic_last_requantize(tic_ctx *ctx, int *route, int *measure_launches, int *store_launches, int *rounds) {
    TIC_LOCK(ctx);
    if (!ctx) return TIC_E_ARG;
    if (route) *route = ctx->last_rq_route;
    if (measure_launches) *measure_launches = ctx->last_rq_measure;
    if (store_launches) *store_launches = ctx->last_rq_store;
    if (rounds) *rounds = ctx->last_rq_rounds;
    return TIC_OK;
}

} // extern "C"
