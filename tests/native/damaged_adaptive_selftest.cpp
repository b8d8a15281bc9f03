// damaged_adaptive_selftest.cpp - the corpus of damaged per-image-table streams (tests/damaged_adaptive.py) through the host half of
// their decoder (tic_adaptive.cpp: adaptive_parse_table, adaptive_decode, adaptive_dec_tab_buildable, adaptive_dec_tab_build) built as
// host code with AddressSanitizer + UBSan (CPU only; tests/test_damaged_adaptive_cpu.py writes the case file and runs it).  Every
// stream lies in an exact-size heap buffer, every output in an exact-size one.  Per entry:
//   (a) the result is the fixture's outcome: the table parser refuses exactly the entries of the table classes (header .. not_prefix),
//       adaptive_decode refuses those and the entries of the payload classes (no_code .. dc_range) and gives the stored coefficients
//       for every other one;
//   (b) the table parses again from an exact-size copy of the stream's first 16 + kAdaptMaxTableBytes bytes;
//   (c) a table that parses is a prefix code inside the limits, adaptive_dec_tab_buildable agrees with the build, and a built look-up
//       table names only entries of its table and has nlong within the arrays (adaptive_table_checks.h).
//
// File: "TICD", u32 entries; per entry: u32 name length + name, u32 stream length + stream, u8 outcome (0 a table class, 1 a payload
// class, 2 coefficients) [u32 blocks, int16 blocks x 64].  Little-endian.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../../tinyimgcodec_amd/csrc/tic_adaptive.h"
#include "../../tinyimgcodec_amd/csrc/tic_entropy.h"
#include "adaptive_table_checks.h"

static std::string g_case;
static int fail(const char *what, long a = 0, long b = 0) {
    fprintf(stderr, "FAIL %s: %s (%ld, %ld)\n", g_case.c_str(), what, a, b);
    return 1;
}

struct Reader {
    FILE *f;
    bool ok = true;
    void bytes(void *p, size_t n) {
        if (n && fread(p, 1, n, f) != n) ok = false;
    }
    uint8_t u8() { uint8_t v = 0; bytes(&v, 1); return v; }
    uint32_t u32() { uint8_t b[4] = {0, 0, 0, 0}; bytes(b, 4); return b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24); }
};

int main(int argc, char **argv) {
    if (argc != 2) return fail("usage: damaged_adaptive_selftest <case file>");
    Reader r{fopen(argv[1], "rb")};
    char magic[4] = {0, 0, 0, 0};
    if (!r.f) return fail("cannot open the case file");
    r.bytes(magic, 4);
    const uint32_t n = r.u32();
    if (!r.ok || memcmp(magic, "TICD", 4) != 0) return fail("not a case file");
    size_t by_outcome[3] = {0, 0, 0}, built = 0, unbuildable = 0, longs = 0;
    for (uint32_t c = 0; c < n; c++) {
        std::vector<char> name(r.u32());
        r.bytes(name.data(), name.size());
        g_case.assign(name.begin(), name.end());
        std::vector<uint8_t> stream(r.u32());
        r.bytes(stream.data(), stream.size());
        const int outcome = r.u8();
        std::vector<int16_t> want;
        if (outcome == 2) {
            want.resize((size_t)r.u32() * 64);
            r.bytes(want.data(), want.size() * 2); // (little-endian hosts only, as the library)
        }
        if (!r.ok || outcome > 2) return fail("short or malformed case file");
        by_outcome[outcome]++;

        const size_t len = stream.size();
        std::unique_ptr<uint8_t[]> s(new uint8_t[len ? len : 1]);
        memcpy(s.get(), stream.data(), len);
        int h = 0, w = 0;
        if (tic::parse_header(s.get(), len, &h, &w, nullptr, nullptr) != 0 || h < 0 || w < 0) return fail("no header");
        const size_t nb = tic::num_blocks(h, w);
        // (a)
        std::unique_ptr<AdaptTable> t(new AdaptTable);
        memset(t.get(), 0x7f, sizeof(AdaptTable));
        const char *why_p = nullptr, *why_d = nullptr;
        const int rc_p = tic::adaptive_parse_table(s.get(), len, t.get(), &why_p);
        if ((rc_p != 0) != (outcome == 0)) return fail(rc_p ? why_p : "the table parses where the fixture has a table class", rc_p, outcome);
        std::unique_ptr<int16_t[]> zz(new int16_t[nb * 64 ? nb * 64 : 1]);
        for (size_t i = 0; i < nb * 64; i++) zz[i] = 0x5A5A;
        const int rc_d = tic::adaptive_decode(s.get(), len, h, w, zz.get(), &why_d);
        if (!why_p || !why_d) return fail("no message pointer");
        if ((rc_d != 0) != (outcome != 2)) return fail(rc_d ? why_d : "adaptive_decode decodes where the fixture refuses", rc_d, outcome);
        if (rc_p != 0 && strcmp(why_p, why_d) != 0) return fail("the parser and the decoder give different table messages");
        if (outcome == 2) {
            if (want.size() != nb * 64) return fail("the fixture's block count is not the header's", (long)want.size() / 64, (long)nb);
            for (size_t i = 0; i < want.size(); i++)
                if (zz[i] != want[i]) return fail("a coefficient differs from the fixture's (block, scan position)", (long)(i / 64), (long)(i % 64));
        }
        if (rc_p != 0) continue;
        // (b)
        const size_t head = len < 16 + tic::kAdaptMaxTableBytes ? len : 16 + tic::kAdaptMaxTableBytes;
        std::unique_ptr<uint8_t[]> hs(new uint8_t[head]);
        memcpy(hs.get(), s.get(), head);
        std::unique_ptr<AdaptTable> t2(new AdaptTable);
        if (tic::adaptive_parse_table(hs.get(), head, t2.get(), nullptr) != 0 || t2->ndc != t->ndc || t2->nac != t->nac || t2->payload_bit != t->payload_bit)
            return fail("the table does not parse from the stream's first 16 + kAdaptMaxTableBytes bytes");
        // (c)
        if (const char *f = table_fault(*t, len)) return fail(f);
        std::unique_ptr<AdaptDecTab> d(new AdaptDecTab);
        const bool buildable = tic::adaptive_dec_tab_buildable(*t);
        if (tic::adaptive_dec_tab_build(*t, d.get()) != buildable) return fail("adaptive_dec_tab_buildable disagrees with the build");
        if (!buildable) {
            unbuildable++;
            continue;
        }
        if (const char *f = lut_fault(*t, *d)) return fail(f);
        built++;
        longs += d->nlong[0] + d->nlong[1];
    }
    fclose(r.f);
    if (n == 0) return fail("no entry checked");
    printf("damaged_adaptive_selftest ok %u entries: %zu table refusals, %zu payload refusals, %zu decoded; %zu look-up tables built (%zu long codes), %zu tables with a code of length zero\n",
           n, by_outcome[0], by_outcome[1], by_outcome[2], built, longs, unbuildable);
    return 0;
}
