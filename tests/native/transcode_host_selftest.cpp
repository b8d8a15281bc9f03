// transcode_host_selftest.cpp - the host half of lossless re-tabling, as a stand-alone program for AddressSanitizer + UBSan
// (tests/test_entropy_decode_cpu.py compiles it with tic_entropy.cpp as HOST code and runs it; nothing of it is loaded into Python).
//
//   transcode_host_selftest cases.bin out.bin
//
// cases.bin: "TICT", uint32 count, then per case uint32 length + the stream's bytes (the damaged default-table corpus of
// tests/damaged_streams.py, scaled_dct entries left out).  Per case: parse_header, the host reader entropy_decode into the zz16 layout
// (absolute DC; a running DC outside int16 is reported, the layout cannot hold it), then the host writer entropy_encode, which takes the
// DC differences again - the glue of tic_retable_default / tic_retable_adaptive's host route without a GPU.  out.bin: per case uint32 length
// + the default-table re-write (length 0xffffffff: refused).  The test compares their sha256 with tests/golden/retable_damaged.json - the
// unmodified reference's reader followed by its writer.  Streams and outputs live in exact-size heap blocks: a read or write one byte
// outside is the sanitizer's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tinyimgcodec_hip.h"
#include "../../tinyimgcodec_amd/csrc/tic_entropy.h"

static bool read_u32(FILE *f, uint32_t *v) { return fread(v, 4, 1, f) == 1; }

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]);
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "cannot open the files\n");
        return 2;
    }
    char magic[4];
    uint32_t count = 0;
    if (fread(magic, 1, 4, in) != 4 || memcmp(magic, "TICT", 4) != 0 || !read_u32(in, &count)) {
        fprintf(stderr, "bad cases file\n");
        return 2;
    }
    unsigned refused = 0, twice = 0;
    for (uint32_t k = 0; k < count; k++) {
        uint32_t len = 0;
        if (!read_u32(in, &len)) return 2;
        std::unique_ptr<uint8_t[]> s(new uint8_t[len ? len : 1]); // exact size
        if (len && fread(s.get(), 1, len, in) != len) return 2;
        int h = 0, w = 0, q = 0;
        uint32_t flag = 0;
        uint32_t out_len = 0xffffffffu;
        std::unique_ptr<uint8_t[]> res;
        if (tic::parse_header(s.get(), len, &h, &w, &q, &flag) == TIC_OK && !(flag >> 30) && h >= 0 && w >= 0 && q >= 1 && q <= 99) {
            const size_t n = tic::num_blocks(h, w);
            std::unique_ptr<int16_t[]> zz(new int16_t[n * 64 ? n * 64 : 1]);
            std::vector<tic::DcWide> wide;
            tic::entropy_decode(s.get(), len, h, w, zz.get(), &wide);
            if (wide.empty()) {
                // the length first, from the size walk; then the writer into a block of exactly that size
                size_t need = 0;
                if (tic::entropy_size(zz.get(), h, w, &need) == TIC_OK) {
                    res.reset(new uint8_t[need]);
                    size_t got = 0;
                    const int rc = tic::entropy_encode(zz.get(), h, w, q, res.get(), need, &got);
                    if (rc != TIC_OK || got != need) {
                        fprintf(stderr, "case %u: entropy_encode returned %d, %zu bytes of %zu\n", k, rc, got, need);
                        return 1;
                    }
                    out_len = (uint32_t)got;
                    // canonical: the re-write read and written once more is itself
                    std::unique_ptr<int16_t[]> zz2(new int16_t[n * 64 ? n * 64 : 1]);
                    tic::entropy_decode(res.get(), got, h, w, zz2.get(), &wide);
                    std::unique_ptr<uint8_t[]> again(new uint8_t[need]);
                    size_t got2 = 0;
                    if (!wide.empty() || tic::entropy_encode(zz2.get(), h, w, q, again.get(), need, &got2) != TIC_OK || got2 != got ||
                        memcmp(again.get(), res.get(), got) != 0) {
                        fprintf(stderr, "case %u: the re-write is not a fixed point of reader + writer\n", k);
                        return 1;
                    }
                    twice++;
                }
            }
        }
        if (out_len == 0xffffffffu) refused++;
        fwrite(&out_len, 4, 1, out);
        if (out_len != 0xffffffffu) fwrite(res.get(), 1, out_len, out);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("transcode_host_selftest ok %u cases, %u refused, %u re-written twice\n", count, refused, twice);
    return 0;
}
