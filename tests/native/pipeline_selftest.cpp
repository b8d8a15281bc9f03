// pipeline_selftest - the host-side pieces of the batch pipeline (tinyimgcodec_amd/csrc/tic_host_pipeline.h: no HIP, no context) on the CPU:
// the closable queue between the pipeline's threads, the strided copy-thread loop, and the three decisions about a caller's buffers.
// tests/test_host_cpu.py builds it twice - thread sanitizer, address + undefined-behaviour sanitizer - and runs both.
//   pipeline_selftest   -> "pipeline_selftest ok", exit 0; the first failed check is printed, exit 1
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "../../tinyimgcodec_amd/csrc/tic_host_pipeline.h"

using namespace tic;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            printf("pipeline_selftest FAILED: %s (line %d)\n", #cond, __LINE__);      \
            exit(1);                                                                  \
        }                                                                             \
    } while (0)

static void queue_checks() {
    // one producer, three consumers: every one of 10,000 items is popped exactly once, the ones pushed before close() included
    {
        constexpr int kItems = 10000;
        ClosableQueue<int> q;
        std::vector<std::atomic<int>> seen(kItems);
        for (auto &s : seen) s = 0;
        std::atomic<int> ended{0};
        std::vector<std::thread> consumers;
        for (int t = 0; t < 3; t++)
            consumers.emplace_back([&]() {
                int v;
                while (q.pop(v)) seen[(size_t)v]++;
                ended++;
            });
        for (int i = 0; i < kItems; i++) q.push(i);
        q.close();
        for (auto &c : consumers) c.join();
        CHECK(ended == 3);
        for (int i = 0; i < kItems; i++) CHECK(seen[(size_t)i] == 1);
        int v = -1;
        CHECK(!q.pop(v) && v == -1); // closed and drained: at once, nothing delivered
    }
    // close() wakes every consumer that waits on an empty queue
    {
        ClosableQueue<int> q;
        std::atomic<int> waiting{0}, woken{0};
        std::vector<std::thread> consumers;
        for (int t = 0; t < 3; t++)
            consumers.emplace_back([&]() {
                int v;
                waiting++;
                CHECK(!q.pop(v));
                woken++;
            });
        while (waiting < 3) std::this_thread::yield();
        std::this_thread::sleep_for(std::chrono::milliseconds(20)); // (let them reach the wait; a consumer that comes later sees `closed` itself)
        q.close();
        for (auto &c : consumers) c.join();
        CHECK(woken == 3);
    }
    // items pushed before close() are delivered behind it, in order, to a consumer that only starts then
    {
        ClosableQueue<int> q;
        for (int i = 0; i < 5; i++) q.push(i);
        q.close();
        int v = -1;
        for (int i = 0; i < 5; i++) CHECK(q.pop(v) && v == i);
        CHECK(!q.pop(v));
    }
}

static void strided_checks() {
    for (int cnt = 0; cnt <= 9; cnt++)
        for (int T = 1; T <= 9; T++) {
            std::vector<std::atomic<int>> visits(10);
            for (auto &v : visits) v = 0;
            std::atomic<int> bound{0};
            const std::thread::id me = std::this_thread::get_id();
            std::atomic<int> on_caller{0};
            run_strided(cnt, T, [&]() { bound++; },
                        [&](int k) {
                            visits[(size_t)k]++;
                            if (std::this_thread::get_id() == me) on_caller++;
                        });
            for (int k = 0; k < 10; k++) CHECK(visits[(size_t)k] == (k < cnt ? 1 : 0));
            CHECK(bound == (T == 1 ? 0 : T));          // every started thread binds itself, the caller's never
            CHECK(on_caller == (T == 1 ? cnt : 0));    // inline when T == 1
        }
}

static void decision_checks() {
    // ---- the density rule: span (whole pages) <= frames + frames / 4 + 1 MiB
    {
        const size_t fb = 1u << 20; // 8 frames of 1 MiB: the limit is 8 + 2 + 1 = 11 MiB
        const uintptr_t lo = 0x10000000;
        CHECK(range_is_mostly_frames(lo, lo + 8 * fb, fb, 8));                       // back to back
        CHECK(range_is_mostly_frames(lo, lo + 11 * fb, fb, 8));                      // exactly at the limit
        CHECK(!range_is_mostly_frames(lo, lo + 11 * fb + 1, fb, 8));                 // one byte over: one page more
        CHECK(range_is_mostly_frames(lo + 1, lo + 11 * fb, fb, 8));                  // page rounding: [lo + 1, ...) still starts at lo's page
        CHECK(!range_is_mostly_frames(lo - 1, lo + 11 * fb, fb, 8));                 // ... and one byte lower takes a page more
        CHECK(page_floor(0x1fff) == 0x1000 && page_ceil(0x1001) == 0x2000 && page_ceil(0x2000) == 0x2000);
    }
    // ---- rows of one block
    {
        alignas(8) static uint8_t pool[8 * 104 + 16];
        uint8_t *outs[4];
        size_t caps[4], P = 0;
        auto rows = [&](uint8_t *base, size_t pitch) {
            for (int k = 0; k < 4; k++) outs[k] = base + (size_t)k * pitch, caps[k] = pitch;
        };
        rows(pool, 104);
        CHECK(rows_of_one_block(outs, caps, 4, 96, &P) && P == 104);                 // a pool of 4 x 104 bytes, rows of 96
        CHECK(rows_of_one_block(outs, caps, 4, 104, &P));                            // a row as long as the pitch
        CHECK(!rows_of_one_block(outs, caps, 4, 112, &P));                           // ... and longer
        CHECK(!rows_of_one_block(outs, caps, 1, 96, &P));                            // one buffer is no block of rows
        outs[2] += 8;
        CHECK(!rows_of_one_block(outs, caps, 4, 96, &P));                            // unequal distance
        rows(pool, 100);
        CHECK(!rows_of_one_block(outs, caps, 4, 96, &P));                            // P % 8 != 0
        rows(pool + 4, 104);
        CHECK(!rows_of_one_block(outs, caps, 4, 96, &P));                            // a misaligned base
        rows(pool, 104);
        caps[3] = 95;
        CHECK(!rows_of_one_block(outs, caps, 4, 96, &P));                            // a capacity one byte short
        rows(pool + 3 * 104, 104);
        outs[1] = pool;
        CHECK(!rows_of_one_block(outs, caps, 2, 96, &P));                            // descending addresses
    }
    // ---- the dense arena: frames at the device buffer's distances (multiples of 256), the padding inside the caller's capacities
    {
        static uint8_t mem[4096];
        std::vector<ArenaFrame> fr;
        auto at = [&](size_t k) { return fr[k]; };
        fr = {{mem, 0, 512, 512}, {mem + 512, 512, 512, 512}, {mem + 1024, 1024, 300, 300}};
        CHECK(frames_are_one_arena(fr.size(), at));                                  // whole 256s, the ragged frame last
        fr = {{mem, 0, 300, 512}, {mem + 512, 512, 300, 512}, {mem + 1024, 1024, 300, 300}};
        CHECK(frames_are_one_arena(fr.size(), at));                                  // ragged frames whose capacities reach the next frame
        fr = {{mem, 0, 300, 300}, {mem + 512, 512, 300, 300}};
        CHECK(!frames_are_one_arena(fr.size(), at));                                 // a gap the capacity does not reach over
        fr = {{mem, 0, 300, 511}, {mem + 512, 512, 300, 300}};
        CHECK(!frames_are_one_arena(fr.size(), at));                                 // ... one byte short of it
        fr = {{mem, 0, 512, 512}, {mem + 512, 512, 300, 300}, {mem + 1024, 1024, 300, 300}};
        CHECK(!frames_are_one_arena(fr.size(), at));                                 // a whole number of 256 bytes, then a frame that is not
        fr = {{mem, 0, 512, 512}, {mem + 768, 512, 512, 512}};
        CHECK(!frames_are_one_arena(fr.size(), at));                                 // not at the device buffer's distance
        fr = {{mem, 0, 300, 300}};
        CHECK(frames_are_one_arena(fr.size(), at));                                  // a single frame
    }
}

int main() {
    queue_checks();
    strided_checks();
    decision_checks();
    printf("pipeline_selftest ok\n");
    return 0;
}
