// rdplan_selftest - the host plan of the batch forms of rate-distortion control (tinyimgcodec_amd/csrc/tic_rd_plan.h: fill_sse_probe_table,
// the lockstep search by distortion) on the CPU.  tests/test_rd_batch_cpu.py builds it with the address and undefined-behaviour sanitizers
// (with tic_entropy.cpp for num_blocks) and runs it.
//   rdplan_selftest   -> "rdplan_selftest ok: <n> tables, <m> searches, <p> lockstep rounds", exit 0; the first failed check is printed, exit 1
// The probe table, on random probe lists with 1..64 probes of 1..300,000 blocks at group caps 1, 2, 3 and 1,024:
//   - groups tile the grid without gap or overlap, no group spans two probes: every workgroup index finds - by the kernel's rule, the
//     number of entries <= index, minus one - the probe whose groups contain it;
//   - a probe has min(ceil(tiles / 4), cap) groups, tiles = block rows x ceil(blocks per row / 8); striding by its own group count, its
//     groups reach every workgroup-tile - and with it every tile, one per wave - exactly once;
//   - entries behind the last probe are 0xffffffff; every probe carries its pointers, pitch, geometry, alignment and result entry.
// No bound on the length of a walk is checked because none was chosen: the kernel's sums are 64 bits from the lane on (tic_kernels.hip,
// SseAcc); what is checked is that the longest walk the sweep meets times a tile's largest sum still fits the 64 bits many times over.
// The lockstep search, on synthetic error tables (monotone, saw-toothed, null-topped, never reaching the bound, reaching it everywhere) at
// depths 1..3 and random (qmin, qmax, bound): the result is the plain bisection's, or its failure kind with qmax's error; no quality is
// probed twice; every quality the plain bisection tests is probed; rounds are at most 1 + ceil(7 / depth), exactly 1 when qmin == qmax.  And
// against the hand-rolled loop the single-frame search once was (inline_psnr_search): the same candidates round by round, the same end.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

#include "../../tinyimgcodec_amd/csrc/tic_rd_plan.h"

using namespace tic;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            printf("rdplan_selftest FAILED: %s (line %d)\n", #cond, __LINE__);      \
            exit(1);                                                                \
        }                                                                           \
    } while (0)

static std::mt19937_64 rng(20261019);
static int tables = 0, searches = 0, lockstep_rounds = 0;
static size_t longest_walk = 0;
static int rnd(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }

// The kernel's lookup: the number of entries <= idx, minus one.
static int find_probe(const uint32_t *first, uint32_t idx) {
    int c = 0;
    for (int l = 0; l < kSseMaxProbes; l++) c += first[l] <= idx;
    return c - 1;
}

static void check_table(const std::vector<SseProbeIn> &in, size_t cap) {
    const int n = (int)in.size();
    SseProbeTable t;
    size_t ngroups = 0;
    CHECK(fill_sse_probe_table(&t, n, in.data(), cap, &ngroups));
    size_t grp = 0;
    for (int k = 0; k < n; k++) {
        const SseProbeRec &r = t.rec[k];
        const SseProbeIn &p = in[(size_t)k];
        const int bw = (p.w + 7) / 8, bh = (p.h + 7) / 8, tiles_x = (bw + 7) / 8;
        const size_t ntiles = (size_t)bh * (size_t)tiles_x, wgt = (ntiles + 3) / 4, want = std::min(wgt, cap);
        CHECK(r.h == p.h && r.w == p.w && r.bw == bw && r.tiles_x == tiles_x && (size_t)r.ntiles == ntiles);
        CHECK((size_t)bw * (size_t)bh == num_blocks(p.h, p.w) && ntiles * 8 >= num_blocks(p.h, p.w));
        CHECK(r.coeffs == p.coeffs && r.img == p.img && r.consts == p.consts && r.stride == p.stride && r.result == p.result);
        CHECK(r.aligned8 == (int)(((uintptr_t)p.img % 8 == 0) && (p.stride % 8 == 0)));
        CHECK(r.ngroups == want && r.ngroups >= 1 && r.ngroups <= cap && r.ngroups == sse_probe_groups(ntiles, cap));
        CHECK(r.first_group == grp && t.first_group[k] == grp); // no gap, no overlap
        // every group of the probe finds the probe; the groups in front and behind do not
        for (size_t g : {grp, grp + want / 2, grp + want - 1}) CHECK(find_probe(t.first_group, (uint32_t)g) == k);
        if (k > 0) CHECK(find_probe(t.first_group, (uint32_t)grp - 1) == k - 1);
        // the walk: group g takes workgroup-tiles g, g + ngroups, ... of its own probe; wave v of it tile 4 * t + v
        std::vector<unsigned char> seen(ntiles, 0);
        for (size_t g = 0; g < want; g++) {
            size_t steps = 0;
            for (size_t wt = g; wt < wgt; wt += want, steps++)
                for (size_t v = 0; v < 4; v++)
                    if (wt * 4 + v < ntiles) seen[wt * 4 + v]++;
            CHECK(steps >= 1);
            longest_walk = std::max(longest_walk, steps);
        }
        for (unsigned char c : seen) CHECK(c == 1);
        grp += want;
    }
    CHECK(grp == ngroups && ngroups <= (size_t)kSseMaxProbes * kSseMaxGroups);
    CHECK(find_probe(t.first_group, (uint32_t)ngroups - 1) == n - 1);
    for (int k = n; k < kSseMaxProbes; k++) CHECK(t.first_group[k] == 0xffffffffu && t.rec[k].ntiles == 0 && t.rec[k].ngroups == 0);
    tables++;
}

static SseProbeIn make_probe(int h, int w, int k) {
    static const int16_t coeffs[8] = {0};
    static const uint8_t img[16] = {0};
    static const double consts[4] = {0};
    // (the pointers are carried, never followed: distinct, and aligned or not by the probe's number)
    return SseProbeIn{coeffs + (k & 7), img + (k % 3 ? 8 : k & 7), consts + (k & 3), (long long)(k % 5 ? (w + 7) / 8 * 8 : w), h, w, (uint32_t)(1000 + 3 * k)};
}

static void check_tables() {
    SseProbeTable t;
    size_t a = 0;
    const SseProbeIn one = make_probe(8, 8, 0), none = make_probe(0, 8, 0), flat = make_probe(8, 0, 0);
    CHECK(!fill_sse_probe_table(&t, 0, &one, 1024, &a) && !fill_sse_probe_table(&t, 65, &one, 1024, &a));
    CHECK(!fill_sse_probe_table(&t, 1, &one, 0, &a) && !fill_sse_probe_table(&t, 1, &one, 1025, &a));
    CHECK(!fill_sse_probe_table(&t, 1, &none, 1024, &a) && !fill_sse_probe_table(&t, 1, &flat, 1024, &a));
    const size_t caps[] = {1, 2, 3, 1024};
    // edges: one block, one tile, 33 blocks in a row (5 tiles, a second workgroup), 4 and 5 workgroup-tiles, 264 x 256 (33 of them),
    // 4096^2 (the cap of 1,024 with a walk of 8), 300,000 blocks
    const int edges[][2] = {{1, 1}, {8, 64}, {8, 264}, {8, 1024}, {8, 1032}, {264, 256}, {4096, 4096}, {8, 2400000}, {4800, 4000}};
    for (auto &e : edges)
        for (size_t cap : caps) check_table({make_probe(e[0], e[1], 1)}, cap);
    for (int it = 0; it < 160; it++) {
        const int n = it < 8 ? 64 : rnd(1, 64);
        std::vector<SseProbeIn> in;
        for (int k = 0; k < n; k++) {
            const int kind = rnd(0, 3);
            const int max_blocks = kind == 0 ? 40 : kind == 1 ? 5000 : 300000;
            const int bw = rnd(1, std::min(max_blocks, 2000)), bh = rnd(1, std::max(1, max_blocks / bw));
            in.push_back(make_probe(bh * 8 - rnd(0, 7), bw * 8 - rnd(0, 7), k));
            CHECK(num_blocks(in.back().h, in.back().w) >= 1 && num_blocks(in.back().h, in.back().w) <= 300000);
        }
        check_table(in, caps[it % 4]);
    }
    // 64-bit sums: the longest walk of the sweep (cap 1 on 300,000 blocks) times a lane's largest tile sum, times a workgroup's 256 lanes
    CHECK(longest_walk >= 9000 && (unsigned long long)longest_walk * 520200ull * 256ull < (1ull << 50));
}

// ---- the search ----
enum { kMonotone, kSaw, kNullTop, kNeverMeets, kAlwaysMeets, kKinds };
static void make_errors(int kind, long long *size /*[100]*/, uint64_t *err /*[100]*/) {
    uint64_t e = 2000000 + (uint64_t)rnd(0, 100000);
    const int first_null = kind == kNullTop ? rnd(1, 99) : 100;
    for (int q = 1; q <= 99; q++) {
        if (kind == kSaw)
            e = (uint64_t)rnd(0, 2000000); // no order at all
        else
            e -= std::min<uint64_t>(e, (uint64_t)rnd(kind == kMonotone || kind == kNullTop ? 1 : 0, 40000));
        err[q] = e;
        size[q] = q >= first_null ? -1 : 16 + q * 10;
    }
    size[0] = -1, err[0] = 0;
}

struct Plain {
    int state, q;
    std::set<int> tested;
};
static Plain plain_bisection(const long long *size, const uint64_t *err, int qmin, int qmax, uint64_t max_sse) {
    Plain r;
    auto meets = [&](int q) {
        r.tested.insert(q);
        return size[q] >= 0 && err[q] <= max_sse;
    };
    if (!meets(qmax)) {
        r.state = size[qmax] < 0 ? kPsnrNoCode : kPsnrOutOfReach, r.q = qmax;
        return r;
    }
    int lo = qmin, hi = qmax;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (meets(mid)) hi = mid; else lo = mid + 1;
    }
    r.state = kPsnrMeets, r.q = lo;
    return r;
}

// The single-frame search as tic_compress_to_psnr ran it before it drove a PsnrSearch, kept as the model of "the same probes in the same
// order": a hand-rolled loop over known[], known_sse[], lo, hi and a first-round flag.  rounds: the candidates of every round, in queue order.
struct Inline {
    int state, q;
    std::vector<std::vector<int>> rounds;
};
static Inline inline_psnr_search(const long long *size, const uint64_t *err, int qmin, int qmax, uint64_t max_sse, int depth) {
    Inline r;
    long long known[100];
    uint64_t known_sse[100];
    for (auto &k : known) k = kRateUnknown;
    auto meets = [&](int q) { return known[q] >= 0 && known_sse[q] <= max_sse; };
    int lo = qmin, hi = qmax;
    for (bool first = true;; first = false) {
        int cand[8], nc = 0;
        if (first) cand[nc++] = qmax; // (never a middle: mid < hi <= qmax)
        psnr_candidates(lo, hi, depth, known, cand, &nc);
        if (nc == 0) break;
        r.rounds.push_back(std::vector<int>(cand, cand + nc));
        for (int i = 0; i < nc; i++) known[cand[i]] = size[cand[i]], known_sse[cand[i]] = err[cand[i]];
        if (first && !meets(qmax)) {
            r.state = known[qmax] < 0 ? kPsnrNoCode : kPsnrOutOfReach, r.q = qmax;
            return r;
        }
        while (lo < hi) { // the bisection, as far as the known results carry it
            const int mid = (lo + hi) / 2;
            if (known[mid] == kRateUnknown) break;
            if (meets(mid)) hi = mid; else lo = mid + 1;
        }
    }
    r.state = kPsnrMeets, r.q = lo;
    return r;
}

static void check_search(const long long *size, const uint64_t *err, int qmin, int qmax, uint64_t max_sse, int depth) {
    const Plain want = plain_bisection(size, err, qmin, qmax, max_sse);
    const Inline model = inline_psnr_search(size, err, qmin, qmax, max_sse, depth);
    PsnrSearch s;
    psnr_search_begin(s, qmin, qmax, max_sse);
    std::set<int> probed;
    int rounds = 0;
    for (;;) {
        int cand[kRateMaxCandidates];
        const int nc = psnr_search_round(s, depth, cand);
        if (nc == 0) break;
        CHECK(nc <= (rounds == 0 ? 1 << depth : (1 << depth) - 1) && nc <= kRateMaxCandidates && s.state == kPsnrSearching);
        if (rounds == 0) CHECK(cand[0] == qmax);
        CHECK((size_t)rounds < model.rounds.size() && model.rounds[(size_t)rounds] == std::vector<int>(cand, cand + nc)); // the same probes, in order
        rounds++;
        for (int i = 0; i < nc; i++) {
            CHECK(cand[i] >= qmin && cand[i] <= qmax);
            CHECK(probed.insert(cand[i]).second); // never twice
            s.known[cand[i]] = size[cand[i]];
            s.known_sse[cand[i]] = err[cand[i]];
        }
        psnr_search_replay(s);
        CHECK(rounds <= 8);
    }
    CHECK((size_t)rounds == model.rounds.size() && s.state == model.state && (s.state == kPsnrMeets ? s.lo : s.qmax) == model.q);
    CHECK(s.state == want.state);
    if (want.state == kPsnrMeets) CHECK(s.lo == want.q && s.hi == want.q && s.known[s.lo] == size[want.q] && s.known_sse[s.lo] == err[want.q]);
    else CHECK(s.known[qmax] == size[qmax] && s.known_sse[qmax] == err[qmax] && rounds == 1); // settled after the first round
    for (int q : want.tested) CHECK(probed.count(q) == 1);
    if (qmin == qmax) CHECK(rounds == 1);
    else CHECK(rounds >= 1 && rounds <= 1 + (7 + depth - 1) / depth);
    searches++;
}

static void check_searches() {
    long long size[100];
    uint64_t err[100];
    for (int it = 0; it < 3000; it++) {
        const int kind = it % kKinds;
        make_errors(kind, size, err);
        int qmin = rnd(1, 99), qmax = rnd(1, 99);
        if (it % 7 == 0) qmin = 1, qmax = 99;
        if (it % 11 == 0) qmax = qmin;
        if (qmin > qmax) std::swap(qmin, qmax);
        uint64_t bound;
        if (kind == kAlwaysMeets) bound = 1ull << 63;
        else if (kind == kNeverMeets) bound = 0;
        else if (it % 3 == 0) { // exactly an error of the range, or one less
            const uint64_t v = err[rnd(qmin, qmax)];
            bound = v < 1 ? 0 : v - (uint64_t)rnd(0, 1);
        }
        else bound = (uint64_t)rnd(0, 2100000);
        if (kind == kNeverMeets)
            for (int q = 1; q <= 99; q++) err[q] += 1; // (an error of 0 would meet a bound of 0)
        for (int depth = 1; depth <= 3; depth++) check_search(size, err, qmin, qmax, bound, depth);
    }
}

// The lockstep queue (round_probes, tic_rate_plan.h) on searches by distortion, as rateplan_selftest checks it on searches by size: in the
// first round every frame of a chunk asks for the same qualities - count << depth probes, queued candidate by candidate in chunk order.
static void check_round_probes() {
    const int shapes[][2] = {{1, 1}, {8, 8}, {7, 9}, {15, 17}, {24, 8}, {72, 8}, {128, 8}, {136, 8}, {40, 52}, {203, 317}, {0, 8}, {8, 0}};
    std::vector<int> hs, ws;
    for (auto &s : shapes) hs.push_back(s[0]), ws.push_back(s[1]);
    for (int chunk_frames : {64, 5, 1}) {
        const RatePlan p = plan_rate_batch(hs.data(), ws.data(), (int)hs.size(), chunk_frames, kMixedChunkBytes);
        CHECK(!p.mixed.chunks.empty());
        for (const MixedChunk &c : p.mixed.chunks)
            for (int d = 1; d <= 3; d++) {
                std::vector<PsnrSearch> search(p.mixed.frames.size());
                for (auto &r : search) psnr_search_begin(r, 1, 99, 1000);
                std::vector<RateProbe> probes;
                round_probes(c, search.data(), d, probes);
                CHECK(probes.size() == (size_t)c.count << d && probes[0].quality == 99);
                for (size_t i = 0; i < probes.size(); i++)
                    CHECK(probes[i].frame == c.first + (int)(i % (size_t)c.count) && probes[i].quality == probes[i - i % (size_t)c.count].quality);
                // a settled frame asks for nothing more: the others keep their order
                search[(size_t)c.first].state = kPsnrMeets;
                round_probes(c, search.data(), d, probes);
                CHECK(probes.size() == (size_t)(c.count - 1) << d);
                for (const RateProbe &pr : probes) CHECK(pr.frame != c.first);
                lockstep_rounds++;
            }
    }
}

int main() {
    check_tables();
    check_searches();
    check_round_probes();
    printf("rdplan_selftest ok: %d tables, %d searches, %d lockstep rounds\n", tables, searches, lockstep_rounds);
    return 0;
}
