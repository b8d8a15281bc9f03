// tic_rate_plan.h - the host plan of rate control, free of HIP and of the context: the chunks of a batch call, the table the size kernel's
// descriptor form reads (stream_size_kernel_v, tic_size_gpu.hip), the layout of one submission's probes in the coefficient workspace, and
// the bisection by size as a state machine (RateSearch) that EVERY search by size drives - the single-frame ones (tic_compress_to_size,
// tic_compress_adaptive_to_size) one frame at a time, tic_compress_batch_to_size every frame of a chunk in lockstep (round_probes, which
// the search by distortion of tic_rd_plan.h shares).
// tests/native/rateplan_selftest.cpp compiles it alone and sweeps it under the address and undefined-behaviour sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "tic_host_pipeline.h"

namespace tic {

// ---- the size kernel's descriptor form ------------------------------------------------------------------------------------------------------
// A PROBE is one frame's coefficients at one quality.  A launch takes up to kSizeMaxProbes of them (one table entry per lane of a wave),
// their coefficients back to back; a probe gets a workgroup per kSizeGroupChunks chunks of 8 blocks - what a workgroup's four waves hold in
// flight in one round - and at most kSizeMaxGroups (4 per CU: each ends in ONE atomic on the probe's result; beyond that the waves stride).
constexpr int kSizeMaxProbes = 64;
constexpr size_t kSizeMaxGroups = 1024;
constexpr size_t kSizeGroupChunks = 16;
inline size_t size_probe_groups(size_t nblocks) {
    const size_t chunks = (nblocks + 7) / 8, groups = (chunks + kSizeGroupChunks - 1) / kSizeGroupChunks;
    return groups > kSizeMaxGroups ? kSizeMaxGroups : groups;
}

struct SizeProbeRec {
    unsigned long long first_block; // in the launch's coefficients, 64 each
    unsigned long long nblocks;
    uint32_t first_group, ngroups;  // its workgroups: [first_group, first_group + ngroups) of the grid
    uint32_t result;                // the SizeResult entry it adds into
    uint32_t pad;
};
static_assert(sizeof(SizeProbeRec) == 32, "a record is 32 bytes");
// A workgroup finds its probe by ONE load per lane and a ballot: lane l compares first_group[l] with the workgroup's index; entries behind
// the last probe are 0xffffffff.
struct SizeProbeTable {
    uint32_t first_group[kSizeMaxProbes];
    SizeProbeRec rec[kSizeMaxProbes];
};

// Fills `t` for n probes (1..kSizeMaxProbes) of nblocks[k] >= 1 blocks, coefficients back to back, probe k adding into entry result[k].
// *ngroups: the launch's grid; *nblk: the blocks it reads.  False when n or a block count is out of range.
inline bool fill_size_probe_table(SizeProbeTable *t, int n, const size_t *nblocks, const uint32_t *result, size_t *ngroups, size_t *nblk) {
    if (n < 1 || n > kSizeMaxProbes) return false;
    for (int k = 0; k < kSizeMaxProbes; k++) {
        t->first_group[k] = 0xffffffffu;
        t->rec[k] = SizeProbeRec();
    }
    size_t blk = 0, grp = 0;
    for (int k = 0; k < n; k++) {
        if (nblocks[k] == 0) return false;
        const size_t groups = size_probe_groups(nblocks[k]);
        SizeProbeRec &r = t->rec[k];
        r.first_block = blk, r.nblocks = nblocks[k];
        r.first_group = (uint32_t)grp, r.ngroups = (uint32_t)groups, r.result = result[k];
        t->first_group[k] = (uint32_t)grp;
        blk += nblocks[k], grp += groups;
    }
    *ngroups = grp, *nblk = blk;
    return true;
}

// ---- the chunks of a call --------------------------------------------------------------------------------------------------------------------
// The mixed batch's plan with every frame at one "quality": frames ordered by (width, height), chunks of at most 64 frames and 32 MB of
// staged pixels, block-less frames and frames the batch does not take (more than kEntropyMaxGroups entropy groups, or more pixels than a
// chunk) set aside - the SAME frames the mixed route sets aside, so that what phase 2 of tic_compress_batch_to_size hands to that route
// all goes through its batch kernels.  A chunk's transform runs (neighbours of equal width whose heights are multiples of 8) are the
// mixed plan's; run_of[f] names the run of frame f (plan order), numbered through the whole plan.
//
// kRateWorkspaceBytes bounds the coefficients one submission of a search leaves between the transforms that write them and the size launch
// that reads them: what is written and read back within about 256 MiB of traffic is still in the Infinity Cache (256 MiB), and a
// transform moves half as many pixel bytes as coefficient bytes beside them - 128 MiB of coefficients keep a submission inside it.  The
// look-ahead of a chunk's search is the deepest of 3, 2, 1 at which its blocks x 128 B x 2^depth probes per frame (the first round's count:
// qmin and 2^depth - 1 middles) stay within it.
constexpr size_t kRateWorkspaceBytes = (size_t)128 << 20;
inline int rate_depth(size_t chunk_blocks) {
    for (int d = 3; d > 1; d--)
        if ((chunk_blocks * 128) << d <= kRateWorkspaceBytes) return d;
    return 1;
}

// The look-ahead of a SINGLE-FRAME search of a frame of n blocks.  Not rate_depth: a probe of such a search takes the whole coefficient
// workspace in its turn (the stream orders the probes), so no workspace bounds the look-ahead; what does is a host wait against a probe -
// a wait costs about what a probe of a 4096^2 frame does (262144 blocks, some 15 us), a probe of a small frame a fraction of that: deep
// look-ahead for small frames, none beyond 4096^2.
inline int single_frame_depth(size_t n) { return n <= 16384 ? 3 : n <= 262144 ? 2 : 1; }

struct RatePlan {
    MixedPlan mixed;
    std::vector<int> run_of; // per frame of mixed.frames
    std::vector<int> depth;  // per chunk
};
inline RatePlan plan_rate_batch(const int *hs, const int *ws, int n, int chunk_frames, size_t chunk_bytes) {
    RatePlan p;
    const std::vector<int> q0((size_t)(n > 0 ? n : 0), 0);
    p.mixed = plan_mixed_batch(hs, ws, q0.data(), n, chunk_frames, chunk_bytes);
    p.run_of.assign(p.mixed.frames.size(), 0);
    int run = 0;
    for (const MixedChunk &c : p.mixed.chunks) {
        for (const MixedRun &r : c.runs) {
            for (int k = 0; k < r.count; k++) p.run_of[(size_t)(r.first + k)] = run;
            run++;
        }
        p.depth.push_back(rate_depth(c.nblk));
    }
    return p;
}

// ---- one submission ------------------------------------------------------------------------------------------------------------------------
// The probes of one submission, in queue order.  They are cut into PASSES: the probes of a pass lie back to back in the workspace, from its
// start, and a pass holds at most `workspace_blocks` (one probe may exceed it alone).  The stream orders the passes, so the next one
// overwrites the workspace without a host wait.  Inside a pass the transforms come first, then one size launch per kSizeMaxProbes probes.
struct RateProbe {
    int frame;   // index into MixedPlan::frames
    int quality;
};
struct RateSubmission {
    std::vector<RateProbe> probes;
    std::vector<size_t> first_block; // per probe: where its coefficients start in the workspace
    std::vector<int> pass_first;     // pass i is probes [pass_first[i], pass_first[i + 1])
    size_t max_pass_blocks = 0;
};
inline void layout_rate_submission(const MixedPlan &p, RateSubmission &s, size_t workspace_blocks) {
    s.first_block.assign(s.probes.size(), 0);
    s.pass_first.clear();
    s.max_pass_blocks = 0;
    size_t blk = 0;
    for (size_t i = 0; i < s.probes.size(); i++) {
        const size_t nb = p.frames[(size_t)s.probes[i].frame].nblk;
        if (i == 0 || blk + nb > workspace_blocks) {
            s.pass_first.push_back((int)i);
            blk = 0;
        }
        s.first_block[i] = blk;
        blk += nb;
        s.max_pass_blocks = std::max(s.max_pass_blocks, blk);
    }
    s.pass_first.push_back((int)s.probes.size());
}
// How many probes from probe i on (inside [i, end)) ONE transform launch takes as one tall frame: neighbours in the queue that are
// neighbours of one transform run at the same quality.  *h_total: its rows.
inline int rate_transform_run(const RatePlan &p, const RateSubmission &s, int i, int end, int *h_total) {
    const MixedFrame &a = p.mixed.frames[(size_t)s.probes[(size_t)i].frame];
    int count = 1;
    *h_total = a.h;
    while (i + count < end) {
        const RateProbe &u = s.probes[(size_t)(i + count - 1)], &v = s.probes[(size_t)(i + count)];
        if (v.frame != u.frame + 1 || v.quality != u.quality || p.run_of[(size_t)v.frame] != p.run_of[(size_t)u.frame]) break;
        *h_total += p.mixed.frames[(size_t)v.frame].h;
        count++;
    }
    return count;
}

// ---- the search ------------------------------------------------------------------------------------------------------------------------------
// The one copy of the bisection by size.  Its contract is that of tic_compress_to_size_dev; what is free is WHEN a quality is probed.  One submission probes every middle
// the bisection can reach within `depth` further steps from where it stands (2^depth - 1 probes, the first one qmin as well), then the
// bisection is replayed over the known sizes as far as they carry.  Sizes: -1 = no code, kRateUnknown = not probed.
constexpr long long kRateUnknown = -2;
inline void rate_candidates(int lo, int hi, int depth, const long long *known, int *out, int *nout) {
    if (lo >= hi || depth == 0) return;
    const int mid = (lo + hi + 1) / 2;
    if (known[mid] == kRateUnknown) out[(*nout)++] = mid;
    rate_candidates(mid, hi, depth - 1, known, out, nout);
    rate_candidates(lo, mid - 1, depth - 1, known, out, nout);
}

// One frame of a lockstep search.  state: still searching, or how it ended - at quality lo (known[lo] is its length), qmin larger than the
// budget (known[qmin] is its length), qmin without a code.
enum { kRateSearching = 0, kRateFits = 1, kRateTooLarge = 2, kRateNoCode = 3 };
constexpr int kRateMaxCandidates = 8; // qmin and the 7 middles of depth 3
struct RateSearch {
    long long known[100];
    unsigned long long budget;
    int qmin, lo, hi, state;
};
inline void rate_search_begin(RateSearch &s, int qmin, int qmax, unsigned long long budget) {
    for (auto &k : s.known) k = kRateUnknown;
    s.budget = budget;
    s.qmin = s.lo = qmin, s.hi = qmax, s.state = kRateSearching;
}
inline bool rate_fits(const RateSearch &s, int q) { return s.known[q] >= 0 && (unsigned long long)s.known[q] <= s.budget; }
// The qualities the frame wants probed in the next submission (into cand[kRateMaxCandidates]); 0: it is settled.
inline int rate_search_round(const RateSearch &s, int depth, int *cand) {
    int nc = 0;
    if (s.state != kRateSearching) return 0;
    if (s.known[s.qmin] == kRateUnknown) cand[nc++] = s.qmin;
    rate_candidates(s.lo, s.hi, depth, s.known, cand, &nc);
    return nc;
}
// ... and, once their sizes are in known[], the bisection as far as the known sizes carry it.
inline void rate_search_replay(RateSearch &s) {
    if (s.state != kRateSearching) return;
    if (!rate_fits(s, s.qmin)) {
        s.state = s.known[s.qmin] < 0 ? kRateNoCode : kRateTooLarge;
        return;
    }
    while (s.lo < s.hi) {
        const int mid = (s.lo + s.hi + 1) / 2;
        if (s.known[mid] == kRateUnknown) return;
        if (rate_fits(s, mid)) s.lo = mid; else s.hi = mid - 1;
    }
    s.state = kRateFits;
}

inline int search_round(const RateSearch &s, int depth, int *cand) { return rate_search_round(s, depth, cand); }
inline void search_replay(RateSearch &s) { rate_search_replay(s); }

// The probes every unsettled frame of chunk `c` wants - by size or by distortion: search_round / search_replay are overloaded for RateSearch
// and for PsnrSearch (tic_rd_plan.h) - queued candidate by candidate: the frames' first candidates in chunk order, then their second
// ones ... - in the first round every frame of a call asks for the same qualities, and neighbours of a transform run are neighbours in
// the queue.  search[f]: the state of plan frame f.
template <class Search> inline void round_probes(const MixedChunk &c, const Search *search, int depth, std::vector<RateProbe> &probes) {
    probes.clear();
    std::vector<int> cand((size_t)c.count * kRateMaxCandidates), nc((size_t)c.count);
    int most = 0;
    for (int k = 0; k < c.count; k++) {
        nc[(size_t)k] = search_round(search[c.first + k], depth, &cand[(size_t)k * kRateMaxCandidates]);
        most = std::max(most, nc[(size_t)k]);
    }
    for (int j = 0; j < most; j++)
        for (int k = 0; k < c.count; k++)
            if (j < nc[(size_t)k]) probes.push_back(RateProbe{c.first + k, cand[(size_t)k * kRateMaxCandidates + (size_t)j]});
}

} // namespace tic
