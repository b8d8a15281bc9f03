// scaledplan_selftest - the table of the integer transform's descriptor form (tinyimgcodec_amd/csrc/tic_scaled_frames.h: fill_scaled_table)
// and a host model of the kernel's walk over it, on the CPU.  tests/test_scaled_batch_cpu.py builds it with the address and
// undefined-behaviour sanitizers and runs it.
//   scaledplan_selftest   -> "scaledplan_selftest ok: <n> tables, <m> walks", exit 0; the first failed check is printed, exit 1
// On random lists of 1..64 records of 1..70,000 blocks, widths of any number of blocks (a multiple of 8 or not), settings 0..3, output areas
// in any order with gaps between them, some records naming the pixels of the record in front:
//   - strips tile the launch without gap or overlap: first_strip is the prefix sum of (h / 8) * ceil(bw / 8), the total is returned;
//   - no strip belongs to two records: every strip index finds - by the kernel's rule, the number of entries <= index, minus one - the
//     record whose strips contain it; entries behind the last record are 0xffffffff;
//   - every record carries its offset, pitch, geometry, setting, output block and alignment;
//   - the walk of fdctq_scaled_kernel_v, modelled wave by wave at grids of 1, 3 and 8,192 waves - a wave keeps its record until a strip
//     lies behind the record's last one, looks up the NEXT strip's record while it works on the current one, and counts how often the
//     setting changes under it - writes every block of every record exactly once and nothing outside the records' areas, reads only
//     pixels inside the record's frame, and a wave's setting changes at most (records it meets - 1) times.
// What is refused: no record, more than 64, a size that is no positive multiple of 8, a setting outside 0..3, more than 2^31 - 1 strips.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../tinyimgcodec_amd/csrc/tic_scaled_frames.h"

using namespace tic;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            printf("scaledplan_selftest FAILED: %s (line %d)\n", #cond, __LINE__);      \
            exit(1);                                                                    \
        }                                                                               \
    } while (0)

static std::mt19937_64 rng(20261019);
static int tables = 0, walks = 0;
static int rnd(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }

struct Frame {
    int h, w, qf;
    unsigned long long img_off, first_block;
    long long pitch;
};

// A frame of about `blocks` blocks (1..70,000), bw anything from 1 to the whole count.
static Frame make_frame(int blocks) {
    Frame f;
    const int bw = rnd(1, blocks), bh = std::max(1, blocks / bw);
    f.h = bh * 8, f.w = bw * 8, f.qf = rnd(0, 3);
    f.pitch = f.w + (rnd(0, 3) == 0 ? rnd(1, 40) : 0); // strided now and then, aligned or not
    f.img_off = f.first_block = 0;
    return f;
}

static void check_table(std::vector<Frame> fr, unsigned long long img_base) {
    const int n = (int)fr.size();
    // output areas in a shuffled order with gaps; pixels back to back, a record now and then naming the frame in front again
    std::vector<int> order((size_t)n);
    for (int k = 0; k < n; k++) order[(size_t)k] = k;
    for (int k = n - 1; k > 0; k--) std::swap(order[(size_t)k], order[(size_t)rnd(0, k)]);
    unsigned long long out_blocks = 0, pix = (unsigned long long)rnd(0, 15);
    for (int k : order) {
        fr[(size_t)k].first_block = out_blocks + (unsigned long long)rnd(0, 5);
        out_blocks = fr[(size_t)k].first_block + (unsigned long long)(fr[(size_t)k].h / 8) * (unsigned long long)(fr[(size_t)k].w / 8);
    }
    for (int k = 0; k < n; k++) {
        if (k > 0 && rnd(0, 3) == 0) {
            const int qf = fr[(size_t)k].qf;
            const unsigned long long blk = fr[(size_t)k].first_block;
            const int bh = fr[(size_t)k].h / 8, bw = fr[(size_t)k].w / 8;
            if (bh * bw == (fr[(size_t)k - 1].h / 8) * (fr[(size_t)k - 1].w / 8)) { // the same pixels at another setting, into another area
                fr[(size_t)k] = fr[(size_t)k - 1];
                fr[(size_t)k].qf = qf, fr[(size_t)k].first_block = blk;
                continue;
            }
        }
        fr[(size_t)k].img_off = pix;
        pix += (unsigned long long)fr[(size_t)k].pitch * (unsigned long long)fr[(size_t)k].h + (unsigned long long)rnd(0, 9);
    }
    std::vector<unsigned long long> off((size_t)n), blk((size_t)n);
    std::vector<long long> pitch((size_t)n);
    std::vector<int> hs((size_t)n), ws((size_t)n), qfs((size_t)n);
    for (int k = 0; k < n; k++) {
        const Frame &f = fr[(size_t)k];
        off[(size_t)k] = f.img_off, blk[(size_t)k] = f.first_block, pitch[(size_t)k] = f.pitch, hs[(size_t)k] = f.h, ws[(size_t)k] = f.w, qfs[(size_t)k] = f.qf;
    }
    ScaledFrameTable t;
    uint32_t total = 0;
    CHECK(fill_scaled_table(&t, n, img_base, 4096ull, off.data(), pitch.data(), hs.data(), ws.data(), qfs.data(), blk.data(), &total));
    tables++;
    CHECK(t.img_base == img_base && t.out_base == 4096ull);
    uint32_t strip = 0;
    for (int k = 0; k < n; k++) {
        const ScaledFrameRec &r = t.rec[k];
        const Frame &f = fr[(size_t)k];
        const uint32_t bw = (uint32_t)f.w / 8, tiles_x = (bw + 7) / 8, strips = (uint32_t)(f.h / 8) * tiles_x;
        CHECK(r.bw == bw && r.tiles_x == tiles_x && r.nstrips == strips && strips >= 1 && (unsigned long long)strips * 8 >= (unsigned long long)bw * (f.h / 8));
        CHECK(r.first_strip == strip && t.first_strip[k] == strip); // no gap, no overlap
        CHECK(r.img_off == f.img_off && r.pitch == f.pitch && r.first_block == f.first_block && r.qf == f.qf);
        CHECK(r.aligned8 == (uint32_t)(((img_base + f.img_off) % 8 == 0) && (f.pitch % 8 == 0)));
        for (uint32_t g : {strip, strip + strips / 2, strip + strips - 1}) CHECK(scaled_record_of_strip(t, g) == k);
        if (k > 0) CHECK(scaled_record_of_strip(t, strip - 1) == k - 1);
        strip += strips;
    }
    CHECK(strip == total && scaled_record_of_strip(t, total - 1) == n - 1);
    for (int k = n; k < kScaledMaxFrames; k++) CHECK(t.first_strip[k] == 0xffffffffu && t.rec[k].nstrips == 0 && t.rec[k].bw == 0);

    // the walk, wave by wave
    std::vector<unsigned char> written((size_t)out_blocks);
    for (const uint32_t nwaves : {1u, 3u, 8192u}) {
        std::fill(written.begin(), written.end(), 0);
        for (uint32_t wave = 0; wave < nwaves && wave < total; wave++) {
            uint32_t g = wave;
            int rc = scaled_record_of_strip(t, g), met = 1, reloads = 0, tab_qf = -1;
            for (; g < total; g += nwaves) {
                const uint32_t gn = g + nwaves;
                int rn = rc;
                if (gn < total) {
                    if (gn >= t.rec[rn].first_strip + t.rec[rn].nstrips) rn = scaled_record_of_strip(t, gn), met++;
                    CHECK(rn >= 0 && rn < n && gn >= t.rec[rn].first_strip && gn < t.rec[rn].first_strip + t.rec[rn].nstrips); // the prefetch is the next strip's
                }
                const ScaledFrameRec &r = t.rec[rc];
                CHECK(g >= r.first_strip && g < r.first_strip + r.nstrips);
                if (r.qf != tab_qf) tab_qf = r.qf, reloads++;
                const uint32_t tile = g - r.first_strip, ty = tile / r.tiles_x, tx = tile - ty * r.tiles_x;
                for (uint32_t b = 0; b < 8; b++) {
                    const uint32_t bx = tx * 8 + b;
                    if (bx >= r.bw) continue;
                    // pixel rows ty * 8 .. + 7, bytes bx * 8 .. + 7 of each: inside the frame
                    CHECK((unsigned long long)(ty * 8 + 7) < (unsigned long long)hs[(size_t)rc] && (unsigned long long)bx * 8 + 7 < (unsigned long long)ws[(size_t)rc]);
                    const unsigned long long o = r.first_block + (unsigned long long)ty * r.bw + bx;
                    CHECK(o < out_blocks);
                    CHECK(written[(size_t)o] == 0);
                    written[(size_t)o] = 1;
                }
                rc = rn;
            }
            CHECK(reloads >= 1 && reloads <= met);
            walks++;
        }
        for (int k = 0; k < n; k++) {
            const unsigned long long nb = (unsigned long long)(fr[(size_t)k].h / 8) * (unsigned long long)(fr[(size_t)k].w / 8);
            for (unsigned long long o = 0; o < nb; o++) CHECK(written[(size_t)(fr[(size_t)k].first_block + o)] == 1);
        }
        size_t sum = 0, want = 0;
        for (unsigned char c : written) sum += c;
        for (int k = 0; k < n; k++) want += (size_t)(fr[(size_t)k].h / 8) * (size_t)(fr[(size_t)k].w / 8);
        CHECK(sum == want); // nothing in the gaps
    }
}

int main() {
    // every record count, small frames; then fewer tables of large frames
    for (int n = 1; n <= kScaledMaxFrames; n++) {
        std::vector<Frame> fr;
        for (int k = 0; k < n; k++) fr.push_back(make_frame(rnd(1, n % 7 == 0 ? 2000 : 40)));
        check_table(fr, (unsigned long long)(n % 3 == 0 ? 0 : 8 * rnd(1, 1000)));
    }
    for (int rep = 0; rep < 6; rep++) {
        std::vector<Frame> fr;
        const int n = rep == 0 ? 64 : rnd(1, 64);
        for (int k = 0; k < n; k++) fr.push_back(make_frame(k % 5 == 0 ? 70000 : rnd(1, 70000)));
        check_table(fr, 256);
    }
    { // one block; 8 x 72 (two strips per block row, the second with one block); 24 x 8
        std::vector<Frame> fr = {{8, 8, 0, 0, 0, 8}, {8, 72, 3, 0, 0, 72}, {24, 8, 1, 0, 0, 8}};
        check_table(fr, 0);
    }
    // refused
    ScaledFrameTable t;
    uint32_t total = 0;
    unsigned long long zero[65] = {0};
    long long pitch[65];
    int h8[65], w8[65], q0[65];
    for (int k = 0; k < 65; k++) pitch[k] = 8, h8[k] = w8[k] = 8, q0[k] = 0;
    CHECK(!fill_scaled_table(&t, 0, 0, 0, zero, pitch, h8, w8, q0, zero, &total));
    CHECK(!fill_scaled_table(&t, 65, 0, 0, zero, pitch, h8, w8, q0, zero, &total));
    CHECK(fill_scaled_table(&t, 64, 0, 0, zero, pitch, h8, w8, q0, zero, &total) && total == 64);
    for (int bad : {0, 4, 12, -8}) {
        h8[3] = bad;
        CHECK(!fill_scaled_table(&t, 8, 0, 0, zero, pitch, h8, w8, q0, zero, &total));
        h8[3] = 8, w8[5] = bad;
        CHECK(!fill_scaled_table(&t, 8, 0, 0, zero, pitch, h8, w8, q0, zero, &total));
        w8[5] = 8;
    }
    for (int bad : {-1, 4}) {
        q0[7] = bad;
        CHECK(!fill_scaled_table(&t, 8, 0, 0, zero, pitch, h8, w8, q0, zero, &total));
        q0[7] = 0;
    }
    for (int k = 0; k < 64; k++) h8[k] = 8 * (1 << 25), w8[k] = 8; // 2^25 strips each: 2^31 in all
    CHECK(!fill_scaled_table(&t, 64, 0, 0, zero, pitch, h8, w8, q0, zero, &total));
    CHECK(fill_scaled_table(&t, 63, 0, 0, zero, pitch, h8, w8, q0, zero, &total) && total == 63u << 25);
    printf("scaledplan_selftest ok: %d tables, %d walks\n", tables, walks);
    return 0;
}
