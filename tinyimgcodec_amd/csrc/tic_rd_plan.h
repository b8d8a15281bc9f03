// tic_rd_plan.h - the host plan of rate-distortion control, free of HIP and of the context: the table the measuring kernel's descriptor
// form reads (idct_sse_kernel_v, tic_kernels.hip) and the bisection by distortion as a state machine (PsnrSearch) that tic_compress_to_psnr
// drives for one frame and tic_compress_batch_to_psnr for every frame of a chunk in lockstep.  The chunks of a call, the layout of a
// submission's probes in the coefficient workspace, the look-ahead depths and the lockstep queue (round_probes) are the rate plan's
// (tic_rate_plan.h).
// tests/native/rdplan_selftest.cpp compiles it alone and sweeps it under the address and undefined-behaviour sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "tic_rate_plan.h"

namespace tic {

// ---- the measuring kernel's descriptor form ---------------------------------------------------------------------------------------------------
// A PROBE is one frame's coefficients at one quality, compared with that frame's pixels.  A launch takes up to kSseMaxProbes of them (one
// table entry per lane of a wave), any block counts.  A WORKGROUP-TILE is what one workgroup of the inverse transform holds at a time:
// kSseWavesPerWG tiles of 8 blocks, one per wave.  A probe gets a workgroup per workgroup-tile and at most `max_groups` (kSseMaxGroups in
// production, 4 per CU, the size kernel's cap): group g of a probe walks workgroup-tiles g, g + ngroups, ... of that probe only, sums in
// registers and ends in ONE atomic per sum on the probe's result.
constexpr int kSseMaxProbes = 64;
constexpr size_t kSseMaxGroups = 1024;
constexpr int kSseWavesPerWG = 4; // (== kWavesPerWG, tic_kernels.hip asserts it)
inline size_t sse_probe_groups(size_t ntiles, size_t max_groups) {
    const size_t wgt = (ntiles + kSseWavesPerWG - 1) / kSseWavesPerWG;
    return wgt > max_groups ? max_groups : wgt;
}

// What IdctArgs + SseArgs hold for a single launch, per probe, and its workgroups.  Device pointers, never followed on the host.
struct SseProbeRec {
    const int16_t *coeffs;          // its coefficients: int16 [N][64] zig-zag, DC integrated
    const uint8_t *img;             // its frame: uint8 [h][stride]
    const void *consts;             // DctqConsts of its quality
    long long stride;               // bytes between the frame's rows
    int h, w, bw, tiles_x, ntiles;
    int aligned8;                   // img and stride are multiples of 8 -> 8-byte row loads
    uint32_t first_group, ngroups;  // its workgroups: [first_group, first_group + ngroups) of the grid
    uint32_t result;                // the DistortionResult entry it adds into
    uint32_t scaled_exp1;           // 0: a probe of the float codec; e + 1: decode()'s scaled_dct branch at exponent e (consts of quality 50)
    uint32_t pad[2];
};
static_assert(sizeof(SseProbeRec) == 80, "a record is 80 bytes");
// A workgroup finds its probe by ONE load per lane and a ballot: lane l compares first_group[l] with the workgroup's index; entries behind
// the last probe are 0xffffffff.
struct SseProbeTable {
    uint32_t first_group[kSseMaxProbes];
    SseProbeRec rec[kSseMaxProbes];
};

struct SseProbeIn {
    const int16_t *coeffs;
    const uint8_t *img;
    const void *consts;
    long long stride;
    int h, w;        // at least one block: h, w >= 1
    uint32_t result;
    int scaled_exp = -1; // >= 0: a stream of the integer encoder at this exponent (its setting); consts must be those of quality 50
};
// Fills `t` for n probes (1..kSseMaxProbes) with at most max_groups (1..kSseMaxGroups) workgroups each.  *ngroups: the launch's grid.
// False when n, the cap or a frame size is out of range.
inline bool fill_sse_probe_table(SseProbeTable *t, int n, const SseProbeIn *in, size_t max_groups, size_t *ngroups) {
    if (n < 1 || n > kSseMaxProbes || max_groups < 1 || max_groups > kSseMaxGroups) return false;
    for (int k = 0; k < kSseMaxProbes; k++) {
        t->first_group[k] = 0xffffffffu;
        t->rec[k] = SseProbeRec();
    }
    size_t grp = 0;
    for (int k = 0; k < n; k++) {
        if (in[k].h < 1 || in[k].w < 1 || in[k].scaled_exp > 62) return false;
        SseProbeRec &r = t->rec[k];
        r.coeffs = in[k].coeffs, r.img = in[k].img, r.consts = in[k].consts, r.stride = in[k].stride;
        r.h = in[k].h, r.w = in[k].w;
        r.bw = (r.w + 7) / 8;
        r.tiles_x = (r.bw + 7) / 8;
        r.ntiles = ((r.h + 7) / 8) * r.tiles_x;
        r.aligned8 = ((((uintptr_t)in[k].img) | (uintptr_t)in[k].stride) & 7) == 0;
        const size_t groups = sse_probe_groups((size_t)r.ntiles, max_groups);
        r.first_group = (uint32_t)grp, r.ngroups = (uint32_t)groups, r.result = in[k].result;
        r.scaled_exp1 = in[k].scaled_exp >= 0 ? (uint32_t)in[k].scaled_exp + 1u : 0u;
        t->first_group[k] = (uint32_t)grp;
        grp += groups;
    }
    *ngroups = grp;
    return true;
}

// ---- the search by distortion -------------------------------------------------------------------------------------------------------------------
// The one copy of the bisection by distortion.  Its contract is that of tic_compress_to_psnr_dev: lo, hi = qmin, qmax; while lo < hi: mid = (lo + hi) / 2;
// meets(mid) ? hi = mid : lo = mid + 1, behind a first test of qmax.  What is free is WHEN a quality is probed: one submission probes every
// middle the bisection can reach within `depth` further steps (2^depth - 1 probes, the first one qmax as well), then the bisection is
// replayed over the known results as far as they carry.  known[]: stream lengths as the size search keeps them (-1 = no code,
// kRateUnknown = not probed); known_sse[]: the squared error beside each.
inline void psnr_candidates(int lo, int hi, int depth, const long long *known, int *out, int *nout) {
    if (lo >= hi || depth == 0) return;
    const int mid = (lo + hi) / 2;
    if (known[mid] == kRateUnknown) out[(*nout)++] = mid;
    psnr_candidates(lo, mid, depth - 1, known, out, nout);
    psnr_candidates(mid + 1, hi, depth - 1, known, out, nout);
}

// One frame of a lockstep search.  state: still searching, or how it ended - at quality lo (known[lo] its length, known_sse[lo] its error),
// qmax short of the bound, qmax without a code (both: known_sse[qmax] is its error).
enum { kPsnrSearching = 0, kPsnrMeets = 1, kPsnrOutOfReach = 2, kPsnrNoCode = 3 };
struct PsnrSearch {
    long long known[100];
    uint64_t known_sse[100];
    uint64_t max_sse;
    int qmin, qmax, lo, hi, state;
};
inline void psnr_search_begin(PsnrSearch &s, int qmin, int qmax, uint64_t max_sse) {
    for (auto &k : s.known) k = kRateUnknown;
    for (auto &k : s.known_sse) k = 0;
    s.max_sse = max_sse;
    s.qmin = s.lo = qmin, s.qmax = s.hi = qmax, s.state = kPsnrSearching;
}
inline bool psnr_meets(const PsnrSearch &s, int q) { return s.known[q] >= 0 && s.known_sse[q] <= s.max_sse; }
// The qualities the frame wants probed in the next submission (into cand[kRateMaxCandidates]: qmax and the 7 middles of depth 3 at most);
// 0: it is settled.
inline int psnr_search_round(const PsnrSearch &s, int depth, int *cand) {
    int nc = 0;
    if (s.state != kPsnrSearching) return 0;
    if (s.known[s.qmax] == kRateUnknown) cand[nc++] = s.qmax; // (never a middle: mid < hi <= qmax)
    psnr_candidates(s.lo, s.hi, depth, s.known, cand, &nc);
    return nc;
}
// ... and, once their results are in known[] and known_sse[], the bisection as far as they carry it.
inline void psnr_search_replay(PsnrSearch &s) {
    if (s.state != kPsnrSearching) return;
    if (!psnr_meets(s, s.qmax)) {
        s.state = s.known[s.qmax] < 0 ? kPsnrNoCode : kPsnrOutOfReach;
        return;
    }
    while (s.lo < s.hi) {
        const int mid = (s.lo + s.hi) / 2;
        if (s.known[mid] == kRateUnknown) return;
        if (psnr_meets(s, mid)) s.hi = mid; else s.lo = mid + 1;
    }
    s.state = kPsnrMeets;
}

inline int search_round(const PsnrSearch &s, int depth, int *cand) { return psnr_search_round(s, depth, cand); }
inline void search_replay(PsnrSearch &s) { psnr_search_replay(s); }

} // namespace tic
