// tic_host_pipeline.h - the host-side pieces the batch entry points of tic_api.hip share, free of HIP and of the context: the queue between
// the pipeline's threads, the loop that spreads a chunk's frames over a few copy threads, and the three decisions about a caller's buffers
// that are functions of addresses and sizes alone.  tests/native/pipeline_selftest.cpp runs all of it on the CPU, under the thread and the
// address sanitizer.
#pragma once
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace tic {

// A FIFO that can be closed.  pop() blocks while the queue is empty and open; it returns false once the queue is closed AND drained: what
// was pushed before close() is still delivered.  close() wakes every waiting consumer.
template <class T> class ClosableQueue {
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<T> q_;
    bool closed_ = false;

  public:
    void push(T v) {
        {
            std::lock_guard<std::mutex> l(mu_);
            q_.push_back(std::move(v));
        }
        cv_.notify_one();
    }
    void close() {
        {
            std::lock_guard<std::mutex> l(mu_);
            closed_ = true;
        }
        cv_.notify_all();
    }
    bool pop(T &v) {
        std::unique_lock<std::mutex> l(mu_);
        cv_.wait(l, [&] { return closed_ || !q_.empty(); });
        if (q_.empty()) return false;
        v = std::move(q_.front());
        q_.pop_front();
        return true;
    }
};

// fn(k) for k in [0, cnt) on T threads, thread t taking k = t, t + T, ...; on the calling thread when T <= 1.  Every thread started here
// calls bind() first (the caller's thread never does).
template <class Bind, class Fn> void run_strided(int cnt, int T, Bind bind, Fn fn) {
    if (T <= 1) {
        for (int k = 0; k < cnt; k++) fn(k);
        return;
    }
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++)
        th.emplace_back([=]() {
            bind();
            for (int k = t; k < cnt; k += T) fn(k);
        });
    for (auto &x : th) x.join();
}

// [p, p + bytes) widened to whole pages: what a registration of the range covers.
constexpr uintptr_t kPageBytes = 4096;
inline uintptr_t page_floor(uintptr_t a) { return a & ~(kPageBytes - 1); }
inline uintptr_t page_ceil(uintptr_t a) { return (a + kPageBytes - 1) & ~(kPageBytes - 1); }

// The density rule of the in-place registration: `cnt` frames of `frame_bytes` between lo and hi (lowest first byte, highest last byte + 1)
// are registered as one range only if the range, in pages, is mostly frames - at most a quarter more plus 1 MiB (arrays allocated one after
// the other lie 16 bytes to a few pages apart); a range over scattered frames would pin memory that is not theirs.
inline bool range_is_mostly_frames(uintptr_t lo, uintptr_t hi, size_t frame_bytes, size_t cnt) {
    const size_t span = page_ceil(hi) - page_floor(lo), frames = frame_bytes * cnt;
    return span <= frames + frames / 4 + ((size_t)1 << 20);
}

// Are the `cnt` buffers rows of ONE block of memory, fit for 8-byte stores of `row_bytes` (a multiple of 8) each?  Equal positive
// distance P between neighbours, P a multiple of 8, the first buffer 8-byte aligned, P and every capacity at least a row.  *pitch = P.
inline bool rows_of_one_block(uint8_t *const *outs, const size_t *caps, int cnt, size_t row_bytes, size_t *pitch) {
    if (cnt < 2 || outs[1] <= outs[0]) return false;
    const uint8_t *base = outs[0];
    const size_t P = (size_t)(outs[1] - outs[0]);
    if (P % 8 != 0 || (uintptr_t)base % 8 != 0 || P < row_bytes) return false;
    for (int k = 0; k < cnt; k++)
        if (outs[k] != base + (size_t)k * P || caps[k] < row_bytes) return false;
    *pitch = P;
    return true;
}

// A decoded frame as the device buffer holds it and as the caller wants it: `bytes` of pixels at offset `off` of the device buffer (frames
// start at multiples of 256 there), to go to `out`, where the caller gave away `cap` bytes.
struct ArenaFrame {
    const uint8_t *out;
    size_t off, bytes, cap;
};
// May ONE copy of the device buffer, from its start to the last frame's end, land at the first frame's address?  The frames must lie in the
// caller's memory at the device buffer's distances, and the copy - the padding between two frames included - may only cover bytes the
// caller gave away: a frame of a whole number of 256 bytes has no padding behind it, behind any other (but the last) `cap` must reach to
// the next frame.  at(k) gives frame k.
template <class At> bool frames_are_one_arena(size_t n, At at) {
    for (size_t k = 0; k < n; k++) {
        const ArenaFrame f = at(k);
        if (k > 0) {
            const ArenaFrame p = at(k - 1);
            if (f.out != p.out + (f.off - p.off)) return false;
        }
        if (k + 1 < n && f.bytes % 256 != 0 && f.cap < at(k + 1).off - f.off) return false;
    }
    return true;
}

} // namespace tic
