// decws_selftest - the device decoder's work buffer: what is PROVIDED for a launch (dec_work_provision_bytes, from the stream lengths
// alone) against what the launchers CARVE out of it (dec_work_carve_bytes, at the range the call ends up with), both taken from
// tinyimgcodec_amd/csrc/tic_entropy_dec_gpu.h - the functions the library itself calls.  Host only: no HIP header, no device.
//
//   decws_selftest            the header's provision                      -> "decws_selftest ok", exit 0
//   decws_selftest --parent   the two expressions the provision replaced  -> counts its counterexamples, prints the smallest, exit 1
//
// The second form is what shows that the sweep can fail: with (bits / 288 + 2) * cap_of(288) entries per frame and 16 KiB of slack for
// the whole batch, a batch of short sparse frames whose range is long needs more than it is given.
#define TIC_DEC_WORKSPACE_ONLY
#include "../../tinyimgcodec_amd/csrc/tic_entropy_dec_gpu.h"

#include <stdio.h>
#include <string.h>

#include <vector>

using namespace tic;

namespace {

bool g_parent = false;

struct Frame {
    size_t len, nblk; // stream bytes (header included), blocks
};

// ---- the two sides
size_t provision_batch(size_t nframes, size_t ranges288, size_t blocks) {
    if (g_parent) return ranges288 * ((size_t)dec_cap_of(kDecRangeMin) * 2 * 2) + blocks * 4 + nframes * 8 + 16384;
    return dec_work_provision_bytes(nframes, ranges288, blocks);
}
size_t provision_single(size_t len, size_t nblk) {
    if (g_parent) return (len * 8 / kDecRangeMin + 2) * ((size_t)dec_cap_of(kDecRangeMin) * 2 * 2) + nblk * 4 + 16384;
    return dec_work_provision_bytes(1, dec_ranges_288(len), nblk);
}

// ---- what a stream can be.  The device decoder takes streams of at least 1,024 blocks and 128 + 8,192 bits (tic_api.hip
// device_decoder_takes).  A block has at least 6 bits (2-bit DC code, 4-bit end-of-block) and at most 9 + 11 bits of DC and
// 63 x (16 + 10) bits of AC: that is what the tables allow.
constexpr size_t kMinLen = 16 + 1024, kMinBlocks = 1024, kMaxBlockBits = 20 + 63 * 26;
size_t sparsest(size_t len) { return (len - 16) * 8 / 6; } // most blocks a stream of this length can hold
size_t densest(size_t len) {
    const size_t b = ((len - 16) * 8 + kMaxBlockBits - 1) / kMaxBlockBits;
    return b < kMinBlocks ? kMinBlocks : b;
}

struct Rng { // xorshift64*: the same cases on every run
    unsigned long long s;
    unsigned long long next() {
        s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
        return s * 2685821657736338717ull;
    }
    size_t in(size_t lo, size_t hi) { return lo + (size_t)(next() % (unsigned long long)(hi - lo + 1)); } // [lo, hi]
};

struct Tally {
    const char *name;
    unsigned long long cases = 0, bad = 0;
    // the smallest counterexample: fewest frames, then the shortest stream, then the shortest range
    size_t f = 0, len = 0, nblk = 0, have = 0, need = 0;
    int range = 0;
    void see(size_t nframes, size_t len_, size_t nblk_, int range_, size_t have_, size_t need_) {
        cases++;
        if (have_ >= need_) return;
        if (!bad || nframes < f || (nframes == f && (len_ < len || (len_ == len && range_ < range))))
            f = nframes, len = len_, nblk = nblk_, range = range_, have = have_, need = need_;
        bad++;
    }
    void report() const {
        printf("%s: %llu cases, %llu counterexamples\n", name, cases, bad);
        if (bad)
            printf("  smallest: %zu frame(s) of %zu bytes and %zu blocks (the chunk's largest, where they differ) at range %d: %zu bytes provided, %zu carved (%zu short)\n", f, len, nblk,
                   range, have, need, need - have);
    }
};

std::vector<int> legal_ranges() {
    std::vector<int> r;
    for (int b = 0; b <= 4096; b++)
        if (dec_range_ok(b)) r.push_back(b);
    return r;
}

void equal_batches(Tally &t, size_t len, size_t nblk, const std::vector<int> &ranges) {
    static const size_t kFrames[] = {1, 2, 79, 200, 1024};
    for (int R : ranges)
        for (size_t F : kFrames)
            t.see(F, len, nblk, R, provision_batch(F, F * dec_ranges_288(len), F * nblk), dec_work_carve_bytes(F, F * dec_ranges_of(len * 8, R), F * nblk, R));
}

void block_counts(size_t len, size_t out[4]) {
    const size_t lo = densest(len), hi = sparsest(len) < kMinBlocks ? kMinBlocks : sparsest(len);
    out[0] = kMinBlocks, out[1] = lo, out[2] = hi, out[3] = lo + (hi - lo) / 2;
}

} // namespace

int main(int argc, char **argv) {
    g_parent = argc > 1 && strcmp(argv[1], "--parent") == 0;
    const std::vector<int> ranges = legal_ranges();
    if (ranges.size() != 28 || ranges.front() != 288 || ranges.back() != 2016) { // odd word counts 9 .. 63
        printf("decws_selftest FAILED: %zu legal ranges\n", ranges.size());
        return 2;
    }
    for (int R : ranges)
        if (dec_cap_of((uint32_t)R) > dec_cap_of(kDecRangeMax)) return 2;
    // the layout itself: pieces in order, 256-byte aligned, nothing overlaps, dec_work_carve_bytes() is the end
    {
        const DecWorkCarve c(3, 1000, 5000, 480);
        const size_t trace = 1000 * (size_t)dec_cap_of(480) * 2;
        if (c.totals != 0 || c.starts < 3 * 8 || c.hand < c.starts + trace || c.bpos < c.hand + trace || c.end < c.bpos + 5000 * 4 ||
            (c.starts | c.hand | c.bpos | c.end) % 256 != 0 || c.end != dec_work_carve_bytes(3, 1000, 5000, 480) || c.end > 3 * 8 + 2 * trace + 5000 * 4 + 4 * 255) {
            printf("decws_selftest FAILED: the carve-up's layout\n");
            return 2;
        }
    }

    // ---- the frame the finding was made on, by construction: flat 192 x 472 at pixel value 128 - 1,416 blocks of 6 bits, 1,078 bytes, below
    // 7 bits per block and so at 33 words per range.  Per frame 9 ranges of 178 entries against 31 x 50 provided: 208 bytes short, and
    // from 76 frames on the parent's 16 KiB of slack is gone (79 without the pieces' rounding up to 256 B).
    Tally flat{"the flat 192 x 472 frame"};
    {
        const size_t len = 16 + (1416 * 6 + 7) / 8, nblk = 1416;
        const int R = dec_range_rule(len, nblk);
        if (len != 1078 || sparsest(len) != nblk || R != 1056 || dec_ranges_of(len * 8, R) != 9 ||
            9 * (size_t)dec_cap_of(1056) * 4 - dec_ranges_288(len) * dec_cap_of(288) * 4 != 208) {
            printf("decws_selftest FAILED: the flat frame is not what it was (%zu bytes, range %d)\n", len, R);
            return 2;
        }
        for (size_t F = 1; F <= 1024; F++)
            flat.see(F, len, nblk, R, provision_batch(F, F * dec_ranges_288(len), F * nblk), dec_work_carve_bytes(F, F * dec_ranges_of(len * 8, R), F * nblk, R));
    }

    // ---- batches of equal frames: every legal range x every stream length up to 64 KiB x {fewest, densest, sparsest, middling} block counts
    // x 1, 2, 79, 200, 1,024 frames; then a seeded sample of lengths up to 64 MiB
    Tally eq{"batch sweep, equal frames"};
    size_t nb[4];
    for (size_t len = kMinLen; len <= (64u << 10); len++) {
        block_counts(len, nb);
        for (size_t b : nb) equal_batches(eq, len, b, ranges);
    }
    Rng rng{0x9E3779B97F4A7C15ull};
    for (int i = 0; i < 20000; i++) {
        const size_t top = (size_t)1 << rng.in(17, 26); // (so that every octave gets its share)
        const size_t len = rng.in(top / 2, top);
        block_counts(len, nb);
        for (size_t b : nb) equal_batches(eq, len, b, ranges);
    }

    // ---- mixed batches: 1 .. 1,024 frames of unequal lengths and densities; the range is the whole chunk's - one dense frame sets it for all
    // the others, so every legal range is tried on every batch, whatever its frames would choose for themselves
    Tally mix{"batch sweep, mixed frames"};
    for (int i = 0; i < 4000; i++) {
        const size_t F = i < 64 ? (size_t)i + 1 : rng.in(1, 1024);
        const size_t top = i % 4 == 0 ? (64u << 10) : (i % 4 == 1 ? 4800 : 1600); // (long tails; the short sparse streams of the finding; the shortest)
        size_t r288 = 0, blocks = 0, longest = 0, longest_blk = 0;
        std::vector<Frame> fr(F);
        for (Frame &f : fr) {
            f.len = rng.in(kMinLen, top);
            const size_t hi = sparsest(f.len) < kMinBlocks ? kMinBlocks : sparsest(f.len);
            f.nblk = i % 2 ? hi : rng.in(densest(f.len), hi);
            r288 += dec_ranges_288(f.len), blocks += f.nblk;
            if (f.len > longest) longest = f.len, longest_blk = f.nblk;
        }
        const size_t have = provision_batch(F, r288, blocks);
        for (int R : ranges) {
            size_t nr = 0;
            for (const Frame &f : fr) nr += dec_ranges_of(f.len * 8, R);
            mix.see(F, longest, longest_blk, R, have, dec_work_carve_bytes(F, nr, blocks, R));
        }
    }

    // ---- the single-frame pair: the first run at the range of the rule, the second at 2,016 bits, a hook at any - and either with the
    // 2,048-bit margin (fewer ranges) or without
    Tally one{"single-frame sweep"};
    auto single = [&](size_t len) {
        block_counts(len, nb);
        for (size_t b : nb)
            for (int R : ranges)
                for (size_t margin : {(size_t)0, (size_t)2048})
                    one.see(1, len, b, R, provision_single(len, b), dec_work_carve_bytes(1, dec_ranges_of(len * 8 - margin, R), b, R));
    };
    for (size_t len = kMinLen; len <= (64u << 10); len++) single(len);
    for (int i = 0; i < 20000; i++) {
        const size_t top = (size_t)1 << rng.in(17, 26);
        single(rng.in(top / 2, top));
    }

    const Tally *all[] = {&flat, &eq, &mix, &one};
    unsigned long long bad = 0;
    for (const Tally *t : all) t->report(), bad += t->bad;
    if (bad) {
        printf("decws_selftest FAILED (%s formulas): %llu counterexamples\n", g_parent ? "parent" : "header", bad);
        return 1;
    }
    printf("decws_selftest ok\n");
    return 0;
}
