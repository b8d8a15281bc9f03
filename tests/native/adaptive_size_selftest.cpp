// adaptive_size_selftest.cpp - the host half of rate control for per-image Huffman tables, as a stand-alone program for the address and
// undefined-behaviour sanitizers (tests/test_adaptive_rate_cpu.py builds and runs it):
//   * adaptive_host_stats / entropy_size_adaptive / adaptive_stream_size (csrc/tic_adaptive.cpp) on built blocks - zero runs of 15, 16, 17,
//     31, 32, 47, 48 and 62, an entry at index 63 only, all-zero blocks, DC differences of +-65535, an AC of -32768 - against a walk written
//     here from the run-length LIST of huffman.py:12-33 (the list first, symbols from the list), on exact-size heap copies;
//   * cap_probe_groups (csrc/tic_adaptive_rate_plan.h) swept over random probe lists and caps: the grid is tiled without gap or overlap, no
//     probe loses its blocks or its result, no probe exceeds the cap.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <utility>
#include <vector>

#include "../../include/tinyimgcodec_hip.h"
#include "../../tinyimgcodec_amd/csrc/tic_adaptive.h"
#include "../../tinyimgcodec_amd/csrc/tic_adaptive_rate_plan.h"

using namespace tic;

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            failures++;                                    \
            printf("FAIL %s:%d: ", __FILE__, __LINE__);    \
            printf(__VA_ARGS__);                           \
            printf("\n");                                  \
        }                                                  \
    } while (0)

static int bit_length(long v) {
    unsigned long a = (unsigned long)(v < 0 ? -v : v);
    int n = 0;
    for (; a; a >>= 1) n++;
    return n;
}

// huffman.py:12-33: the run-length list of a block's 63 AC entries, then the symbols of the list.
static std::vector<std::pair<int, int>> run_length_list(const int16_t *ac) {
    int last = 62;
    while (last >= 0 && ac[last] == 0) last--;
    std::vector<std::pair<int, int>> out;
    int run = 0;
    for (int i = 0; i <= last; i++) {
        if (ac[i] == 0) {
            run++;
            continue;
        }
        while (run > 15) {
            out.push_back({15, 0});
            run -= 16;
        }
        out.push_back({run, (int)ac[i]});
        run = 0;
    }
    out.push_back({0, 0});
    return out;
}

static void model_stats(const std::vector<int16_t> &zz, size_t n, AdaptStats *st) {
    for (int i = 0; i < kAdaptBins; i++) st->count[i] = 0, st->first[i] = ~0ull;
    st->err = 0;
    long prev = 0;
    for (size_t b = 0; b < n; b++) {
        const int16_t *c = zz.data() + b * 64;
        const int dsz = bit_length((long)c[0] - prev);
        prev = c[0];
        if (dsz > 15) st->err = 1;
        const int dbin = kAdaptDcBin + (dsz & 15);
        if (st->count[dbin]++ == 0) st->first[dbin] = b;
        const auto list = run_length_list(c + 1);
        for (size_t k = 0; k < list.size(); k++) {
            const int sz = bit_length(list[k].second);
            if (sz > 15) st->err = 1;
            const int bin = (list[k].first << 4) | (sz & 15);
            if (st->count[bin]++ == 0) st->first[bin] = b * 64 + k;
        }
    }
}

static void check_frame(const char *name, const std::vector<int16_t> &blocks) {
    const size_t n = blocks.size() / 64;
    int16_t *heap = (int16_t *)malloc(blocks.size() * 2); // exact size: a read past the last coefficient is the sanitizer's
    memcpy(heap, blocks.data(), blocks.size() * 2);
    AdaptStats got, want;
    adaptive_host_stats(heap, n, &got);
    model_stats(blocks, n, &want);
    CHECK(got.err == want.err, "%s: err %u, model %u", name, got.err, want.err);
    for (int i = 0; i < kAdaptBins; i++)
        CHECK(got.count[i] == want.count[i] && got.first[i] == want.first[i], "%s: bin %d count %llu first %llu, model %llu %llu", name, i, got.count[i],
              got.first[i], want.count[i], want.first[i]);
    size_t bytes = 0, from_stats = 0;
    const int rc = entropy_size_adaptive(heap, 8, (int)(8 * n), &bytes);
    const int rc2 = adaptive_stream_size(want.count + kAdaptDcBin, want.first + kAdaptDcBin, want.count, want.first, &from_stats);
    if (want.err) {
        CHECK(rc == TIC_E_RANGE, "%s: a size above 15 gives %d", name, rc);
    } else {
        CHECK(rc == rc2 && (rc != TIC_OK || bytes == from_stats), "%s: walk %d %zu, statistics %d %zu", name, rc, bytes, rc2, from_stats);
        if (rc == TIC_OK) { // the identity, from the table itself
            unsigned long long dc_code[16], ac_code[256], bits = 0;
            uint8_t dc_len[16], ac_len[256], table[kAdaptMaxTableBytes];
            size_t tbits = 0;
            CHECK(huffman_table_build(want.count + kAdaptDcBin, want.first + kAdaptDcBin, want.count, want.first, dc_code, dc_len, ac_code, ac_len, table,
                                      sizeof table, &tbits) == TIC_OK, "%s: table", name);
            for (int i = 0; i < 256; i++) bits += want.count[i] * (ac_len[i] + (i & 15));
            for (int i = 0; i < 16; i++) bits += want.count[kAdaptDcBin + i] * (dc_len[i] + i);
            CHECK(bytes == 16 + (tbits + bits + 7) / 8, "%s: %zu bytes, identity %llu", name, bytes, 16 + (tbits + bits + 7) / 8);
        }
    }
    free(heap);
}

static std::vector<int16_t> block(int dc, std::initializer_list<std::pair<int, int>> entries) {
    std::vector<int16_t> b(64, 0);
    b[0] = (int16_t)dc;
    for (auto e : entries) b[(size_t)e.first] = (int16_t)e.second;
    return b;
}
static void append(std::vector<int16_t> &f, const std::vector<int16_t> &b) { f.insert(f.end(), b.begin(), b.end()); }

static void built_blocks() {
    for (int run : {15, 16, 17, 31, 32, 47, 48, 62}) {
        char name[64];
        snprintf(name, sizeof name, "run %d", run);
        std::vector<int16_t> f;
        append(f, block(3, {{1 + run, -5}}));             // the run from entry 1 on
        if (run < 62) append(f, block(-4, {{1, 2}, {2 + run, 1}})); // ... and behind an entry
        append(f, block(0, {}));
        check_frame(name, f);
    }
    check_frame("entry 63 only", block(0, {{63, 1}}));
    check_frame("entry 63 only, twice", [] { auto f = block(9, {{63, -1}}); append(f, block(9, {{63, 7}})); return f; }());
    check_frame("all zero", std::vector<int16_t>(64 * 5, 0));
    {
        std::vector<int16_t> f;
        append(f, block(-32768, {}));
        append(f, block(32767, {{5, 1}})); // + 65535
        append(f, block(-32768, {}));      // - 65535
        check_frame("DC steps of 65535", f);
    }
    check_frame("AC -32768", block(1, {{1, -32768}, {40, 32767}}));
    check_frame("AC -32768 behind a run", block(1, {{20, -32768}}));
    {
        std::vector<int16_t> f; // every size 1..15, both signs
        for (int s = 1; s <= 15; s++) append(f, block(s, {{s, (1 << (s - 1))}, {63 - s, -((1 << s) - 1)}}));
        check_frame("sizes 1..15", f);
    }
    {
        std::vector<int16_t> f(64, 0); // a full block: 63 entries, EOB ordinal 63
        for (int k = 0; k < 64; k++) f[(size_t)k] = (int16_t)(k % 7 - 3 ? k % 7 - 3 : 1);
        check_frame("full block", f);
    }
    std::mt19937 rng(12345);
    for (int t = 0; t < 200; t++) {
        const size_t n = 1 + rng() % 20;
        std::vector<int16_t> f(n * 64, 0);
        const int density = 1 + (int)(rng() % 40);
        for (auto &v : f)
            if ((int)(rng() % 40) < density) v = (int16_t)((int)(rng() % 2001) - 1000);
        check_frame("random", f);
    }
    // errors
    size_t bytes = 0;
    const std::vector<int16_t> z(64, 0);
    CHECK(entropy_size_adaptive(z.data(), 0, 8, &bytes) == TIC_E_ARG, "a frame without blocks");
    CHECK(entropy_size_adaptive(nullptr, 8, 8, &bytes) == TIC_E_ARG, "null coefficients");
    CHECK(entropy_size_adaptive(z.data(), 8, 8, nullptr) == TIC_E_ARG, "null result");
    CHECK(entropy_size_adaptive(z.data(), -8, 8, &bytes) == TIC_E_ARG, "negative size");
    unsigned long long zero[272] = {0}, first[272];
    for (auto &v : first) v = ~0ull;
    CHECK(adaptive_stream_size(zero + 256, first + 256, zero, first, &bytes) == TIC_E_ARG, "an empty histogram");
}

static void sweep_cap() {
    std::mt19937_64 rng(777);
    int tables = 0;
    for (int t = 0; t < 3000; t++) {
        const int n = 1 + (int)(rng() % kSizeMaxProbes);
        size_t nblocks[kSizeMaxProbes];
        uint32_t result[kSizeMaxProbes];
        for (int k = 0; k < n; k++) {
            const int kind = (int)(rng() % 4);
            nblocks[k] = kind == 0 ? 1 + rng() % 9 : kind == 1 ? 1 + rng() % 300 : kind == 2 ? 1 + rng() % 70000 : 1 + rng() % 3000000;
            result[k] = (uint32_t)(rng() % 1000);
        }
        SizeProbeTable *tab = (SizeProbeTable *)malloc(sizeof(SizeProbeTable)), *ref = (SizeProbeTable *)malloc(sizeof(SizeProbeTable));
        size_t groups = 0, blocks = 0, capped = 0;
        CHECK(fill_size_probe_table(tab, n, nblocks, result, &groups, &blocks), "fill");
        memcpy(ref, tab, sizeof *tab);
        const int cap = (int)(rng() % 5 == 0 ? 0 : 1 + rng() % 40);
        CHECK(cap_probe_groups(tab, n, cap, &capped), "cap");
        size_t grp = 0;
        for (int k = 0; k < n; k++) {
            const SizeProbeRec &r = tab->rec[k], &o = ref->rec[k];
            CHECK(r.first_block == o.first_block && r.nblocks == o.nblocks && r.result == o.result, "probe %d lost its blocks or result", k);
            CHECK(r.first_group == grp && tab->first_group[k] == grp, "probe %d starts at group %u, not %zu", k, r.first_group, grp);
            CHECK(r.ngroups >= 1 && r.ngroups <= o.ngroups && (cap == 0 ? r.ngroups == o.ngroups : r.ngroups == (o.ngroups < (uint32_t)cap ? o.ngroups : (uint32_t)cap)),
                  "probe %d: %u groups of %u under cap %d", k, r.ngroups, o.ngroups, cap);
            grp += r.ngroups;
        }
        CHECK(grp == capped && (cap != 0 || capped == groups), "grid %zu, table says %zu", grp, capped);
        for (int k = n; k < kSizeMaxProbes; k++) CHECK(tab->first_group[k] == 0xffffffffu, "entry %d behind the last probe", k);
        free(tab);
        free(ref);
        tables++;
    }
    SizeProbeTable tab;
    size_t nb = ((size_t)1 << 25) + 1, g = 0, b = 0;
    uint32_t res = 0;
    CHECK(fill_size_probe_table(&tab, 1, &nb, &res, &g, &b) && cap_probe_groups(&tab, 1, 0, &g), "the plan's own groups always do");
    nb = ((size_t)1 << 26);
    CHECK(fill_size_probe_table(&tab, 1, &nb, &res, &g, &b) && !cap_probe_groups(&tab, 1, 1, &g), "one workgroup for 2^26 blocks is refused");
    CHECK(!cap_probe_groups(&tab, 0, 0, &g) && !cap_probe_groups(&tab, 65, 0, &g) && !cap_probe_groups(&tab, 1, -1, &g), "bad arguments");
    printf("cap_probe_groups: %d tables\n", tables);
}

int main() {
    built_blocks();
    sweep_cap();
    if (failures) {
        printf("adaptive_size_selftest: %d failures\n", failures);
        return 1;
    }
    printf("adaptive_size_selftest ok\n");
    return 0;
}
