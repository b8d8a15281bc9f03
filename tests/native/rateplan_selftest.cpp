// rateplan_selftest - the host plan of the batch forms of rate control (tinyimgcodec_amd/csrc/tic_rate_plan.h: fill_size_probe_table,
// plan_rate_batch, layout_rate_submission, rate_transform_run, the lockstep search) on the CPU.  tests/test_rate_batch_cpu.py builds it
// with the address and undefined-behaviour sanitizers (with tic_entropy.cpp for num_blocks / compress_bound) and runs it.
//   rateplan_selftest   -> "rateplan_selftest ok: <n> tables, <m> searches, <p> plans", exit 0; the first failed check is printed, exit 1
// The probe table, on random probe lists with 1..64 probes of 1..300,000 blocks:
//   - groups tile the grid without gap or overlap, no group spans two probes: every workgroup index finds - by the kernel's rule, the
//     number of entries <= index, minus one - the probe whose groups contain it;
//   - a probe has min(ceil(chunks / 16), 1024) groups, chunks = ceil(blocks / 8); striding by its own group count, its waves reach every
//     chunk exactly once;
//   - entries behind the last probe are 0xffffffff; coefficient areas tile the launch's blocks; every probe names its result entry.
// The lockstep search, on synthetic size tables (monotone, null-topped, saw-toothed, all-fit, none-fit) at depths 1..3 and random
// (qmin, qmax, budget): the result is the plain bisection's, or its failure kind; no quality is probed twice; every quality the plain
// bisection tests is probed; rounds are at most ceil(ceil(log2(qmax - qmin + 1)) / depth), exactly 1 when qmin == qmax.  And against the
// hand-rolled loop the single-frame search once was (inline_size_search): the same candidates round by round, the same end.
// The plan and a submission's layout, on random frame lists: every frame exactly once; passes hold at most the workspace (or one probe);
// probes of a pass lie back to back; a merged transform launch covers neighbours of one run at one quality, contiguous in pixels and
// coefficients; the depth of a chunk keeps blocks x 128 B x 2^depth within kRateWorkspaceBytes.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

#include "../../tinyimgcodec_amd/csrc/tic_rate_plan.h"

using namespace tic;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            printf("rateplan_selftest FAILED: %s (line %d)\n", #cond, __LINE__);      \
            exit(1);                                                                  \
        }                                                                             \
    } while (0)

static std::mt19937_64 rng(20261019);
static int tables = 0, searches = 0, plans = 0;
static int rnd(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }

// The kernel's lookup: the number of entries <= idx, minus one.
static int find_probe(const uint32_t *first, uint32_t idx) {
    int c = 0;
    for (int l = 0; l < kSizeMaxProbes; l++) c += first[l] <= idx;
    return c - 1;
}

static void check_table(int n, const std::vector<size_t> &nblocks) {
    SizeProbeTable t;
    std::vector<uint32_t> result((size_t)n);
    for (int k = 0; k < n; k++) result[(size_t)k] = (uint32_t)(1000 + 3 * k);
    size_t ngroups = 0, nblk = 0;
    CHECK(fill_size_probe_table(&t, n, nblocks.data(), result.data(), &ngroups, &nblk));
    size_t grp = 0, blk = 0;
    for (int k = 0; k < n; k++) {
        const SizeProbeRec &r = t.rec[k];
        const size_t chunks = (nblocks[(size_t)k] + 7) / 8, want = std::min<size_t>((chunks + 15) / 16, 1024);
        CHECK(r.ngroups == want && r.ngroups >= 1 && r.ngroups == size_probe_groups(nblocks[(size_t)k]));
        CHECK(r.first_group == grp && t.first_group[k] == grp); // no gap, no overlap
        CHECK(r.first_block == blk && r.nblocks == nblocks[(size_t)k]);
        CHECK(r.result == result[(size_t)k]);
        // every group of the probe finds the probe; the groups in front and behind do not
        for (size_t g : {grp, grp + want / 2, grp + want - 1}) CHECK(find_probe(t.first_group, (uint32_t)g) == k);
        if (k > 0) CHECK(find_probe(t.first_group, (uint32_t)grp - 1) == k - 1);
        // the waves' loop (4 waves per group, 4 chunks in flight, the stride the probe's own wave count) reaches every chunk once
        const size_t nwaves = want * 4;
        size_t reached = 0;
        for (size_t w = 0; w < nwaves; w++)
            for (size_t base = w; base < chunks; base += nwaves * 4)
                for (size_t u = 0; u < 4; u++) reached += base + u * nwaves < chunks;
        CHECK(reached == chunks);
        grp += want, blk += nblocks[(size_t)k];
    }
    CHECK(grp == ngroups && blk == nblk);
    CHECK(find_probe(t.first_group, (uint32_t)ngroups - 1) == n - 1);
    for (int k = n; k < kSizeMaxProbes; k++) CHECK(t.first_group[k] == 0xffffffffu && t.rec[k].nblocks == 0);
    tables++;
}

static void check_tables() {
    SizeProbeTable t;
    size_t a, b;
    const size_t one = 1, zero = 0;
    const uint32_t r0 = 0;
    CHECK(!fill_size_probe_table(&t, 0, &one, &r0, &a, &b) && !fill_size_probe_table(&t, 65, &one, &r0, &a, &b));
    CHECK(!fill_size_probe_table(&t, 1, &zero, &r0, &a, &b));
    for (size_t edge : {(size_t)1, (size_t)8, (size_t)9, (size_t)128, (size_t)129, (size_t)131072, (size_t)131073, (size_t)262144, (size_t)300000})
        check_table(1, {edge});
    for (int it = 0; it < 400; it++) {
        const int n = it < 8 ? 64 : rnd(1, 64);
        std::vector<size_t> nb((size_t)n);
        for (auto &v : nb) {
            const int kind = rnd(0, 3);
            v = kind == 0 ? (size_t)rnd(1, 40) : kind == 1 ? (size_t)rnd(1, 5000) : (size_t)rnd(1, 300000);
        }
        check_table(n, nb);
    }
}

// ---- the search ----
enum { kMonotone, kNullTop, kSaw, kAllFit, kNoneFit, kKinds };
static void make_sizes(int kind, long long *size /*[100]*/) {
    long long v = 16 + rnd(1, 500);
    const int first_null = kind == kNullTop ? rnd(1, 99) : 100;
    for (int q = 1; q <= 99; q++) {
        if (kind == kSaw)
            v = 1000 + rnd(0, 4000); // no order at all
        else
            v += rnd(kind == kMonotone || kind == kNullTop ? 1 : 0, 900);
        size[q] = q >= first_null ? -1 : v;
    }
    size[0] = -1;
}

struct Plain {
    int state, q;
    std::set<int> tested;
};
static Plain plain_bisection(const long long *size, int qmin, int qmax, unsigned long long budget) {
    Plain r;
    auto fits = [&](int q) {
        r.tested.insert(q);
        return size[q] >= 0 && (unsigned long long)size[q] <= budget;
    };
    if (!fits(qmin)) {
        r.state = size[qmin] < 0 ? kRateNoCode : kRateTooLarge, r.q = qmin;
        return r;
    }
    int lo = qmin, hi = qmax;
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (fits(mid)) lo = mid; else hi = mid - 1;
    }
    r.state = kRateFits, r.q = lo;
    return r;
}

// The single-frame search as tic_compress_to_size ran it before it drove a RateSearch, kept as the model of "the same probes in the same
// order": a hand-rolled loop over known[], lo, hi and a first-round flag.  rounds: the candidates of every round, in queue order.
struct Inline {
    int state, q;
    std::vector<std::vector<int>> rounds;
};
static Inline inline_size_search(const long long *size, int qmin, int qmax, unsigned long long budget, int depth) {
    Inline r;
    long long known[100];
    for (auto &k : known) k = kRateUnknown;
    auto fits = [&](int q) { return known[q] >= 0 && (unsigned long long)known[q] <= budget; };
    int lo = qmin, hi = qmax;
    for (bool first = true;; first = false) {
        int cand[8], nc = 0;
        if (first) cand[nc++] = qmin;
        rate_candidates(lo, hi, depth, known, cand, &nc);
        if (nc == 0) break;
        r.rounds.push_back(std::vector<int>(cand, cand + nc));
        for (int i = 0; i < nc; i++) known[cand[i]] = size[cand[i]];
        if (first && !fits(qmin)) {
            r.state = known[qmin] < 0 ? kRateNoCode : kRateTooLarge, r.q = qmin;
            return r;
        }
        while (lo < hi) { // the bisection, as far as the known sizes carry it
            const int mid = (lo + hi + 1) / 2;
            if (known[mid] == kRateUnknown) break;
            if (fits(mid)) lo = mid; else hi = mid - 1;
        }
    }
    r.state = kRateFits, r.q = lo;
    return r;
}

static void check_search(const long long *size, int qmin, int qmax, unsigned long long budget, int depth) {
    const Plain want = plain_bisection(size, qmin, qmax, budget);
    const Inline model = inline_size_search(size, qmin, qmax, budget, depth);
    RateSearch s;
    rate_search_begin(s, qmin, qmax, budget);
    std::set<int> probed;
    int rounds = 0;
    for (;;) {
        int cand[kRateMaxCandidates];
        const int nc = rate_search_round(s, depth, cand);
        if (nc == 0) break;
        CHECK(nc <= (1 << depth) && s.state == kRateSearching);
        CHECK((size_t)rounds < model.rounds.size() && model.rounds[(size_t)rounds] == std::vector<int>(cand, cand + nc)); // the same probes, in order
        rounds++;
        for (int i = 0; i < nc; i++) {
            CHECK(cand[i] >= qmin && cand[i] <= qmax);
            CHECK(probed.insert(cand[i]).second); // never twice
            s.known[cand[i]] = size[cand[i]];
        }
        rate_search_replay(s);
        CHECK(rounds <= 8);
    }
    CHECK((size_t)rounds == model.rounds.size() && s.state == model.state && (s.state == kRateFits ? s.lo : s.qmin) == model.q);
    CHECK(s.state == want.state);
    if (want.state == kRateFits) CHECK(s.lo == want.q && s.known[s.lo] == size[want.q]);
    else CHECK(s.known[qmin] == size[qmin]);
    for (int q : want.tested) CHECK(probed.count(q) == 1);
    int steps = 0;
    while ((1 << steps) < qmax - qmin + 1) steps++;
    if (qmin == qmax) CHECK(rounds == 1);
    else CHECK(rounds >= 1 && rounds <= (steps + depth - 1) / depth);
    searches++;
}

static void check_searches() {
    long long size[100];
    for (int it = 0; it < 3000; it++) {
        const int kind = it % kKinds;
        make_sizes(kind, size);
        int qmin = rnd(1, 99), qmax = rnd(1, 99);
        if (it % 7 == 0) qmin = 1, qmax = 99;
        if (it % 11 == 0) qmax = qmin;
        if (qmin > qmax) std::swap(qmin, qmax);
        unsigned long long budget;
        if (kind == kAllFit) budget = 1ull << 40;
        else if (kind == kNoneFit) budget = (unsigned long long)rnd(0, 16);
        else if (it % 3 == 0) { // exactly a size of the range, or one byte less
            const long long v = size[rnd(qmin, qmax)];
            budget = v < 1 ? 0ull : (unsigned long long)(v - rnd(0, 1));
        }
        else budget = (unsigned long long)rnd(0, 60000);
        for (int depth = 1; depth <= 3; depth++) check_search(size, qmin, qmax, budget, depth);
    }
}

// ---- the plan and a submission's layout ----
static void check_plan(const std::vector<int> &hs, const std::vector<int> &ws, int chunk_frames, size_t chunk_bytes, int nq, size_t workspace_blocks) {
    const int n = (int)hs.size();
    const RatePlan p = plan_rate_batch(hs.data(), ws.data(), n, chunk_frames, chunk_bytes);
    std::vector<int> seen((size_t)n, 0);
    for (int i : p.mixed.empty) {
        seen[(size_t)i]++;
        CHECK(num_blocks(hs[(size_t)i], ws[(size_t)i]) == 0);
    }
    for (int i : p.mixed.single) seen[(size_t)i]++;
    for (const MixedFrame &f : p.mixed.frames) {
        seen[(size_t)f.index]++;
        CHECK(f.quality == 0);
    }
    for (int v : seen) CHECK(v == 1);
    CHECK(p.run_of.size() == p.mixed.frames.size() && p.depth.size() == p.mixed.chunks.size());
    for (size_t ci = 0; ci < p.mixed.chunks.size(); ci++) {
        const MixedChunk &c = p.mixed.chunks[ci];
        const int d = p.depth[ci];
        CHECK(d >= 1 && d <= 3 && d == rate_depth(c.nblk));
        if (d > 1) CHECK((c.nblk * 128) << d <= kRateWorkspaceBytes);
        if (d < 3) CHECK((c.nblk * 128) << (d + 1) > kRateWorkspaceBytes);
        for (int k = 1; k < c.count; k++) { // ordered by (width, height)
            const MixedFrame &a = p.mixed.frames[(size_t)(c.first + k - 1)], &b = p.mixed.frames[(size_t)(c.first + k)];
            CHECK(a.w < b.w || (a.w == b.w && a.h <= b.h));
        }
        // a submission: nq qualities, quality by quality, as tic_stream_sizes_v queues them
        RateSubmission s;
        for (int j = 0; j < nq; j++)
            for (int k = 0; k < c.count; k++) s.probes.push_back(RateProbe{c.first + k, 1 + j});
        layout_rate_submission(p.mixed, s, workspace_blocks);
        CHECK(s.pass_first.front() == 0 && s.pass_first.back() == (int)s.probes.size());
        size_t most = 0;
        for (size_t i = 0; i + 1 < s.pass_first.size(); i++) {
            const int first = s.pass_first[i], end = s.pass_first[i + 1];
            CHECK(first < end);
            size_t blk = 0;
            for (int k = first; k < end; k++) {
                CHECK(s.first_block[(size_t)k] == blk); // back to back from the workspace's start
                blk += p.mixed.frames[(size_t)s.probes[(size_t)k].frame].nblk;
            }
            CHECK(blk <= workspace_blocks || end - first == 1);
            if (end < (int)s.probes.size()) CHECK(blk + p.mixed.frames[(size_t)s.probes[(size_t)end].frame].nblk > workspace_blocks); // (cut only when full)
            most = std::max(most, blk);
            int covered = first;
            for (int k = first; k < end;) {
                int h_total = 0;
                const int m = rate_transform_run(p, s, k, end, &h_total);
                CHECK(m >= 1 && k + m <= end);
                const MixedFrame &a = p.mixed.frames[(size_t)s.probes[(size_t)k].frame];
                int rows = 0;
                size_t nblk = 0;
                for (int j = 0; j < m; j++) {
                    const RateProbe &pr = s.probes[(size_t)(k + j)];
                    const MixedFrame &f = p.mixed.frames[(size_t)pr.frame];
                    CHECK(pr.quality == s.probes[(size_t)k].quality && f.w == a.w && pr.frame == s.probes[(size_t)k].frame + j);
                    CHECK(pr.frame >= c.first && pr.frame < c.first + c.count);
                    if (m > 1) CHECK(f.h % 8 == 0);
                    CHECK(f.img_off == a.img_off + (size_t)rows * a.pitch && f.pitch == a.pitch); // one tall frame of pixels ...
                    CHECK(s.first_block[(size_t)(k + j)] == s.first_block[(size_t)k] + nblk);     // ... and of coefficients
                    rows += f.h, nblk += f.nblk;
                }
                CHECK(rows == h_total && num_blocks(h_total, a.w) == nblk);
                covered += m, k += m;
            }
            CHECK(covered == end);
        }
        CHECK(most == s.max_pass_blocks);
        // the first round of a search: every frame asks for the same qualities, candidate by candidate
        std::vector<RateSearch> search(p.mixed.frames.size());
        for (auto &r : search) rate_search_begin(r, 1, 99, 1000);
        std::vector<RateProbe> probes;
        round_probes(c, search.data(), d, probes);
        CHECK(probes.size() == (size_t)c.count << d);
        for (size_t i = 0; i < probes.size(); i++) CHECK(probes[i].frame == c.first + (int)(i % (size_t)c.count) && probes[i].quality == probes[i - i % (size_t)c.count].quality);
    }
    plans++;
}

static void check_plans() {
    const int shapes[][2] = {{1, 1}, {8, 8}, {7, 9}, {15, 17}, {24, 8}, {72, 8}, {128, 8}, {136, 8}, {40, 52}, {203, 317}, {0, 8}, {8, 0}};
    std::vector<int> hs, ws;
    for (auto &s : shapes) hs.push_back(s[0]), ws.push_back(s[1]);
    check_plan(hs, ws, 64, kMixedChunkBytes, 3, kRateWorkspaceBytes / 128);
    check_plan(hs, ws, 5, kMixedChunkBytes, 3, 100);
    check_plan(hs, ws, 64, 65536, 99, 700);
    for (int it = 0; it < 200; it++) {
        const int n = rnd(1, 150);
        hs.assign((size_t)n, 0), ws.assign((size_t)n, 0);
        for (int i = 0; i < n; i++) {
            const int kind = rnd(0, 5);
            hs[(size_t)i] = kind == 0 ? 8 * rnd(0, 40) : kind == 1 ? 512 : rnd(0, 700);
            ws[(size_t)i] = kind <= 1 ? 8 * rnd(1, 64) : rnd(0, 700);
        }
        check_plan(hs, ws, rnd(0, 70), it % 3 ? kMixedChunkBytes : (size_t)rnd(1000, 2000000), rnd(1, 7), it % 2 ? kRateWorkspaceBytes / 128 : (size_t)rnd(1, 20000));
    }
    CHECK(rate_depth(1) == 3 && rate_depth(131072) == 3 && rate_depth(131073) == 2 && rate_depth(262144) == 2 && rate_depth(262145) == 1);
    CHECK(single_frame_depth(1) == 3 && single_frame_depth(16384) == 3 && single_frame_depth(16385) == 2 && single_frame_depth(262144) == 2 &&
          single_frame_depth(262145) == 1);
}

int main() {
    check_tables();
    check_searches();
    check_plans();
    printf("rateplan_selftest ok: %d tables, %d searches, %d plans\n", tables, searches, plans);
    return 0;
}
