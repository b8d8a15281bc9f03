// requant_plan_selftest - the host plan of requantisation (tinyimgcodec_amd/csrc/tic_requant_plan.h: the functions the library itself calls)
// on the CPU.  The job table is walked the way requant_kernel_v walks it - a workgroup finds its job by counting the entries of
// first_group[] that are <= its index, its four waves take chunks of 8 blocks, four in flight, with the job's own wave stride - and every
// block a lane would load or store is checked against the buffers: each destination block of each job is written exactly once, nothing is
// read or written outside, no workgroup is without a job.  Host only: no HIP header, no device.  Built alone, under the address and
// undefined-behaviour sanitizers.
//
//   requant_plan_selftest                 the header's functions                                   -> "requant_plan_selftest ok N cases", exit 0
//   requant_plan_selftest --break-stride  the walk with the GRID's wave stride instead of the job's -> counts its counterexamples, exit 1
//
// The second form is what shows that the sweep can fail.
#include "../../tinyimgcodec_amd/csrc/tic_requant_plan.h"

#include <stdio.h>
#include <string.h>

#include <vector>

using namespace tic;

namespace {

struct Rng { // xorshift64*: the same cases on every run
    unsigned long long s;
    unsigned long long next() {
        s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
        return s * 2685821657736338717ull;
    }
    size_t in(size_t lo, size_t hi) { return lo + (size_t)(next() % (unsigned long long)(hi - lo + 1)); } // [lo, hi]
};

long g_checks = 0, g_bad = 0;
bool g_break_stride = false;
#define CHECK(c)                                                              \
    do {                                                                      \
        g_checks++;                                                           \
        if (!(c)) {                                                           \
            if (g_bad++ < 10) fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
        }                                                                     \
    } while (0)

// The kernel's walk over a filled table: written[b] counts the stores to destination block b, job_of[b] names the job that stored there last;
// every load and store is checked against the buffers' block counts.
void walk(const RequantJobTable &t, size_t ngroups, size_t src_cap, size_t dst_cap, std::vector<int> &written, std::vector<int> &job_of) {
    for (size_t g = 0; g < ngroups; g++) {
        int job = -1;
        for (int l = 0; l < kSizeMaxProbes; l++) job += t.first_group[l] <= (uint32_t)g; // the ballot's count - 1
        CHECK(job >= 0 && job < kSizeMaxProbes);
        if (job < 0) continue;
        const RequantJobRec &r = t.rec[job];
        CHECK(g >= r.first_group && g < (size_t)r.first_group + r.ngroups);
        // the kernel's own arithmetic (requant_walk, requant_round_stride, requant_lane_block), wave by wave, lane group by lane group
        for (int wave = 0; wave < kRequantWaves; wave++) {
            RequantWalk wk = requant_walk(r.nblocks, g - r.first_group, r.ngroups, wave);
            if (g_break_stride) wk.nwaves = (unsigned long long)ngroups * kRequantWaves;
            for (unsigned long long base = wk.first_chunk; base < wk.nchunks; base += requant_round_stride(wk))
                for (int u = 0; u < kRequantUnroll; u++)
                    for (int lane = 0; lane < 64; lane += 8) {
                        unsigned long long ch, blk;
                        if (!requant_lane_block(wk, base, u, lane, &ch, &blk)) continue;
                        CHECK(r.src_block + blk < src_cap);
                        CHECK(r.dst_block + blk < dst_cap);
                        if (r.dst_block + blk < dst_cap) {
                            written[(size_t)(r.dst_block + blk)]++;
                            job_of[(size_t)(r.dst_block + blk)] = job;
                        }
                    }
        }
    }
}

void one_case(Rng &rng, long *cases) {
    static const size_t kBlocks[] = {1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 130, 255, 256, 257, 2047, 2051, 16384, 131071, 131073, 140000};
    const int n = (int)rng.in(1, kSizeMaxProbes);
    std::vector<RequantJobIn> in((size_t)n);
    const bool shared = rng.in(0, 1) == 1; // every job reads the same frame (a size table), or each its own
    size_t dst = 0, src = 0, big = 0;
    for (int k = 0; k < n; k++) {
        size_t nb = kBlocks[rng.in(0, sizeof kBlocks / sizeof kBlocks[0] - 1)];
        if (nb > 3000 && ++big > 2) nb = 65; // (two large jobs per case keep the sweep short)
        if (shared && k) nb = in[0].nblocks;
        const size_t gap = rng.in(0, 3) == 0 ? rng.in(1, 9) : 0; // destinations need not be back to back
        in[(size_t)k] = RequantJobIn{shared ? 0 : src, dst + gap, nb, (int)rng.in(1, 99), (int)rng.in(1, 99), (uint32_t)k};
        dst += gap + nb;
        if (!shared) src += nb;
    }
    const size_t src_cap = shared ? in[0].nblocks : src, dst_cap = dst + rng.in(0, 5);
    RequantJobTable t;
    size_t ngroups = 0;
    CHECK(fill_requant_job_table(&t, n, in.data(), src_cap, dst_cap, &ngroups));
    size_t want_groups = 0;
    for (int k = 0; k < n; k++) want_groups += size_probe_groups(in[(size_t)k].nblocks);
    CHECK(ngroups == want_groups && ngroups <= (size_t)kSizeMaxProbes * kSizeMaxGroups);
    std::vector<int> written(dst_cap, 0), job_of(dst_cap, -1);
    walk(t, ngroups, src_cap, dst_cap, written, job_of);
    std::vector<int> want(dst_cap, 0);
    for (int k = 0; k < n; k++)
        for (size_t b = 0; b < in[(size_t)k].nblocks; b++) {
            want[in[(size_t)k].dst_block + b] = 1;
            CHECK(job_of[in[(size_t)k].dst_block + b] == k);
        }
    CHECK(written == want);
    for (int k = 0; k < n; k++) CHECK(t.rec[k].q_from == (uint32_t)in[(size_t)k].q_from && t.rec[k].q_to == (uint32_t)in[(size_t)k].q_to && t.rec[k].flag == (uint32_t)k);
    for (int k = n; k < kSizeMaxProbes; k++) CHECK(t.first_group[k] == 0xffffffffu);
    // refusals: one field of one job spoilt at a time
    {
        std::vector<RequantJobIn> bad = in;
        const size_t k = rng.in(0, (size_t)n - 1);
        switch (rng.in(0, 6)) {
        case 0: bad[k].nblocks = 0; break;
        case 1: bad[k].q_from = rng.in(0, 1) ? 0 : 100; break;
        case 2: bad[k].q_to = rng.in(0, 1) ? -3 : 100; break;
        case 3: bad[k].flag = kSizeMaxProbes; break;
        case 4: bad[k].src_block = src_cap - bad[k].nblocks + 1; break;
        case 5: bad[k].dst_block = dst_cap - bad[k].nblocks + 1; break;
        default:
            if (n < 2) bad[k].nblocks = 0;
            else bad[k].dst_block = bad[k ? k - 1 : 1].dst_block + bad[k ? k - 1 : 1].nblocks - 1; // overlaps its neighbour's last block
        }
        size_t ng = 0;
        CHECK(!fill_requant_job_table(&t, n, bad.data(), src_cap, dst_cap, &ng));
    }
    CHECK(!fill_requant_job_table(&t, 0, in.data(), src_cap, dst_cap, &ngroups) && !fill_requant_job_table(&t, kSizeMaxProbes + 1, in.data(), src_cap, dst_cap, &ngroups));
    (*cases)++;
}

void splits(long *cases) {
    static const size_t kN[] = {1, 64, 2047, 4096, 16384, 131071, 131072, 131073, 262144, 4194304};
    for (size_t n : kN)
        for (size_t nq = 1; nq <= (size_t)kSizeMaxProbes; nq++) {
            const size_t g = size_probe_groups(n), sp = requant_size_split(n, nq);
            CHECK(sp >= 1 && sp <= nq);
            CHECK(g < kRequantFillGroups || sp == 1);                    // a frame that fills the device is read once
            CHECK(sp == nq || sp * g >= kRequantFillGroups);             // otherwise the grid reaches the fill, or every quality has a workgroup
            size_t seen = 0;                                             // the kernel's own division: quality i = y + li * split
            for (size_t y = 0; y < sp; y++) seen += (nq - y + sp - 1) / sp;
            CHECK(seen == nq);
            (*cases)++;
        }
}

} // namespace

int main(int argc, char **argv) {
    g_break_stride = argc > 1 && !strcmp(argv[1], "--break-stride");
    Rng rng{0x9e3779b97f4a7c15ull};
    long cases = 0;
    for (int i = 0; i < 100; i++) one_case(rng, &cases);
    splits(&cases);
    if (g_bad) {
        printf("requant_plan_selftest FAILED: %ld of %ld checks\n", g_bad, g_checks);
        return 1;
    }
    printf("requant_plan_selftest ok %ld cases, %ld checks\n", cases, g_checks);
    return 0;
}
