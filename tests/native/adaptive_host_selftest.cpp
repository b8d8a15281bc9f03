// adaptive_host_selftest.cpp - the host half of the per-image-table decoder (tic_adaptive.cpp: adaptive_parse_table, adaptive_decode,
// adaptive_dec_tab_build) built as host code with AddressSanitizer + UBSan (CPU only; tests/test_adaptive_tables_cpu.py writes the case
// file and runs it).  That code parses a table from untrusted bytes and builds the look-up table device lanes index; the GPU tests reach
// it, a machine without a GPU never did.  Every stream lies in an exact-size heap buffer, every output in an exact-size one.
//   (a) adaptive_decode gives the coefficients of the bit-serial model (tests/adaptive_tables.py decode_model), or an error where the
//       model raises (and for the one table the product refuses by its documented limit of 64 bits per symbol);
//   (b) adaptive_parse_table + adaptive_dec_tab_build give exactly the tables of lut_model, adaptive_dec_tab_buildable agrees with the build;
//   (c) on the cases marked for it, every single-bit flip of the table region and every cut from 16 bytes to the payload's first byte:
//       the parser succeeds exactly when adaptive_decode does not fail with a table message (the same message); a table that parses is a
//       prefix code inside the limits (brute force over its entries); a built look-up table names only entries of the parsed table.
//
// File: "TICA", u32 cases; per case: u32 name length + name, u32 stream length + stream, u8 model (0 error, 1 coefficients) [u32 blocks,
// int16 blocks x 64], u8 tables (0 none, 1) [per table DC, AC: u16 x 2048 primary entries, u32 n, u64 x n codes, u16 x n (length << 8) |
// symbol], u8 mutate.  Little-endian.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../tinyimgcodec_amd/csrc/tic_adaptive.h"
#include "../../tinyimgcodec_amd/csrc/tic_entropy.h"
#include "adaptive_table_checks.h" // table_fault, lut_fault

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
    uint16_t u16() { uint8_t b[2] = {0, 0}; bytes(b, 2); return (uint16_t)(b[0] | (b[1] << 8)); }
    uint32_t u32() { uint32_t lo = u16(); return lo | ((uint32_t)u16() << 16); }
    uint64_t u64() { uint64_t lo = u32(); return lo | ((uint64_t)u32() << 32); }
};

struct ModelTab {
    std::vector<uint16_t> prim;
    std::vector<uint64_t> codes;
    std::vector<uint16_t> ls;
};

static bool is_table_message(const char *why) { return strstr(why, "table") != nullptr || strstr(why, "header") != nullptr; }

// One stream (an exact-size copy is made here): parser against decoder, and the properties of what parses.  -> 0, or 1 after a message.
static int consistent(const std::vector<uint8_t> &bytes, size_t *parsed, size_t *decoded) {
    std::unique_ptr<uint8_t[]> s(new uint8_t[bytes.size()]);
    memcpy(s.get(), bytes.data(), bytes.size());
    const size_t len = bytes.size();
    int h = 0, w = 0;
    if (tic::parse_header(s.get(), len, &h, &w, nullptr, nullptr) != 0) return fail("mutation: no header");
    const size_t nb = tic::num_blocks(h, w);
    std::unique_ptr<int16_t[]> zz(new int16_t[nb * 64]);
    std::unique_ptr<AdaptTable> t(new AdaptTable);
    memset(t.get(), 0x7f, sizeof(AdaptTable));
    const char *why_p = nullptr, *why_d = nullptr;
    const int rc_p = tic::adaptive_parse_table(s.get(), len, t.get(), &why_p);
    const int rc_d = tic::adaptive_decode(s.get(), len, h, w, zz.get(), &why_d);
    if (!why_p || !why_d) return fail("mutation: no message pointer");
    const bool table_failure = rc_d != 0 && is_table_message(why_d);
    if ((rc_p == 0) == table_failure) return fail("the parser and the decoder disagree about the table", rc_p, rc_d);
    if (rc_p != 0 && strcmp(why_p, why_d) != 0) return fail("the parser and the decoder give different table messages", rc_p, rc_d);
    if (rc_p != 0 && !is_table_message(why_p)) return fail("a parser failure without a table message", rc_p);
    if (rc_d == 0 && why_d[0]) return fail("a message beside success");
    *decoded += rc_d == 0;
    if (rc_p != 0) return 0;
    *parsed += 1;
    if (const char *f = table_fault(*t, len)) return fail(f);
    std::unique_ptr<AdaptDecTab> d(new AdaptDecTab);
    const bool buildable = tic::adaptive_dec_tab_buildable(*t);
    if (tic::adaptive_dec_tab_build(*t, d.get()) != buildable) return fail("adaptive_dec_tab_buildable disagrees with the build");
    if (buildable)
        if (const char *f = lut_fault(*t, *d)) return fail(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) return fail("usage: adaptive_host_selftest <case file>");
    Reader r{fopen(argv[1], "rb")};
    char magic[4] = {0, 0, 0, 0};
    if (!r.f) return fail("cannot open the case file");
    r.bytes(magic, 4);
    const uint32_t ncases = r.u32();
    if (!r.ok || memcmp(magic, "TICA", 4) != 0) return fail("not a case file");
    size_t checked = 0, mutations = 0, parsed = 0, decoded = 0;
    for (uint32_t c = 0; c < ncases; c++) {
        std::vector<char> name(r.u32());
        r.bytes(name.data(), name.size());
        g_case.assign(name.begin(), name.end());
        std::vector<uint8_t> stream(r.u32());
        r.bytes(stream.data(), stream.size());
        const bool model_ok = r.u8() != 0;
        std::vector<int16_t> want;
        if (model_ok) {
            want.resize((size_t)r.u32() * 64);
            for (int16_t &v : want) v = (int16_t)r.u16();
        }
        const bool have_tabs = r.u8() != 0;
        ModelTab mt[2];
        if (have_tabs)
            for (int k = 0; k < 2; k++) {
                mt[k].prim.resize(1u << kAdaptDecK);
                for (uint16_t &v : mt[k].prim) v = r.u16();
                const uint32_t n = r.u32();
                if (n > 256) return fail("case file: a long list of more than 256 codes", n);
                mt[k].codes.resize(n);
                mt[k].ls.resize(n);
                for (uint64_t &v : mt[k].codes) v = r.u64();
                for (uint16_t &v : mt[k].ls) v = r.u16();
            }
        const bool mutate = r.u8() != 0;
        if (!r.ok) return fail("short case file");

        const size_t len = stream.size();
        std::unique_ptr<uint8_t[]> s(new uint8_t[len ? len : 1]);
        memcpy(s.get(), stream.data(), len);
        int h = 0, w = 0;
        if (tic::parse_header(s.get(), len, &h, &w, nullptr, nullptr) != 0) return fail("no header");
        const size_t nb = tic::num_blocks(h, w);
        // (a)
        std::unique_ptr<int16_t[]> zz(new int16_t[nb * 64 ? nb * 64 : 1]);
        for (size_t i = 0; i < nb * 64; i++) zz[i] = 0x5A5A;
        const char *why = nullptr;
        const int rc = tic::adaptive_decode(s.get(), len, h, w, zz.get(), &why);
        if (model_ok) {
            if (rc != 0) return fail(why ? why : "adaptive_decode failed where the model decodes", rc);
            if (want.size() != nb * 64) return fail("the model's block count is not the header's", (long)want.size() / 64, (long)nb);
            for (size_t i = 0; i < want.size(); i++)
                if (zz[i] != want[i]) return fail("a coefficient differs from the model's (block, scan position)", (long)(i / 64), (long)(i % 64));
        } else if (rc == 0) {
            return fail("adaptive_decode decodes where the model raises");
        }
        // (b)
        std::unique_ptr<AdaptTable> t(new AdaptTable);
        const int rc_p = tic::adaptive_parse_table(s.get(), len, t.get(), &why);
        if ((rc_p == 0) != have_tabs) return fail("adaptive_parse_table and the model disagree about the table", rc_p);
        if (have_tabs) {
            // (the parser also promises to need no more than the first 16 + kAdaptMaxTableBytes bytes: an exact-size copy of those)
            const size_t head = len < 16 + tic::kAdaptMaxTableBytes ? len : 16 + tic::kAdaptMaxTableBytes;
            std::unique_ptr<uint8_t[]> hs(new uint8_t[head]);
            memcpy(hs.get(), s.get(), head);
            std::unique_ptr<AdaptTable> t2(new AdaptTable);
            if (tic::adaptive_parse_table(hs.get(), head, t2.get(), &why) != 0 || t2->ndc != t->ndc || t2->nac != t->nac || t2->payload_bit != t->payload_bit)
                return fail("the table does not parse from the stream's first 16 + kAdaptMaxTableBytes bytes");
            if (const char *f = table_fault(*t, len)) return fail(f);
            std::unique_ptr<AdaptDecTab> d(new AdaptDecTab);
            const bool buildable = tic::adaptive_dec_tab_buildable(*t);
            if (tic::adaptive_dec_tab_build(*t, d.get()) != buildable) return fail("adaptive_dec_tab_buildable disagrees with the build");
            if (!buildable) return fail("the look-up table of a case does not build"); // (no case of the fixture has a code of length zero)
            for (int k = 0; k < 2; k++) {
                for (unsigned i = 0; i < (1u << kAdaptDecK); i++)
                    if (d->prim[k][i] != mt[k].prim[i]) return fail("a primary entry differs from lut_model's (table, window)", k, (long)i);
                if (d->nlong[k] != mt[k].codes.size()) return fail("the long list's length differs from lut_model's", k, (long)d->nlong[k]);
                for (size_t i = 0; i < mt[k].codes.size(); i++)
                    if (d->long_code[k][i] != mt[k].codes[i] || d->long_ls[k][i] != mt[k].ls[i]) return fail("a long entry differs from lut_model's (table, index)", k, (long)i);
            }
            if (const char *f = lut_fault(*t, *d)) return fail(f);
        }
        checked++;
        // (c)
        if (mutate) {
            if (!have_tabs) return fail("a case to mutate without a table");
            // (flips first, then cuts; a few threads, each mutation on copies of its own - the calls under test share no state)
            const size_t payload_bit = t->payload_bit, flips = payload_bit - 128;
            const size_t last_cut = payload_bit / 8 + 1 < len ? payload_bit / 8 + 1 : len, total = flips + (last_cut - 16 + 1);
            const unsigned nthreads = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
            std::atomic<size_t> next{0}, n_parsed{0}, n_decoded{0};
            std::atomic<int> failed{0};
            auto work = [&]() {
                size_t p = 0, dcd = 0;
                for (size_t i = next++; i < total && !failed; i = next++) {
                    std::vector<uint8_t> m;
                    if (i < flips) {
                        m = stream;
                        m[(128 + i) >> 3] ^= (uint8_t)(0x80u >> ((128 + i) & 7));
                    } else {
                        m.assign(stream.begin(), stream.begin() + (long)(16 + (i - flips)));
                    }
                    if (consistent(m, &p, &dcd)) {
                        fail(i < flips ? "... at the flipped bit" : "... at the cut length", (long)(i < flips ? 128 + i : 16 + (i - flips)));
                        failed = 1;
                    }
                }
                n_parsed += p;
                n_decoded += dcd;
            };
            std::vector<std::thread> pool;
            for (unsigned k = 1; k < nthreads; k++) pool.emplace_back(work);
            work();
            for (std::thread &th : pool) th.join();
            if (failed) return 1;
            mutations += total;
            parsed += n_parsed;
            decoded += n_decoded;
        }
    }
    fclose(r.f);
    if (checked != ncases || checked == 0) return fail("no case checked");
    printf("adaptive_host_selftest ok %zu cases, %zu mutations (%zu tables parsed, %zu streams decoded)\n", checked, mutations, parsed, decoded);
    return 0;
}
