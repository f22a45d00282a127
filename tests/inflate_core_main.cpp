// The decoder of insilicoseq_amd/csrc/iss_inflate_core.h as a stand-alone program (tests/test_inflate_core_host.py builds it with the
// system compiler under the address and undefined-behaviour sanitizers and runs it): one lane, an empty sync.
//   inflate_core_main CASES OUT
// CASES: u32 count, then per case u32 payload bytes, u32 ISIZE, u32 CRC-32 and the payload.  Every case gets a payload buffer and an
// output buffer of exactly its sizes, so a read behind the payload or a write outside [0, ISIZE) is the sanitizer's report.  Prints
// "index status crc" per case; OUT receives the bytes of the cases that end OK or TRAILING, back to back.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "iss_inflate_core.h"

static bool read_u32(FILE *f, uint32_t *v) { return fread(v, 4, 1, f) == 1; }

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s CASES OUT\n", argv[0]);
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    uint32_t n = 0;
    if (!in || !out || !read_u32(in, &n)) {
        fprintf(stderr, "cannot open the case file or the output\n");
        return 2;
    }
    std::vector<uint32_t> tab(256), ops((size_t)iss_inf::N_OPS * 32);
    iss_inf::crc_tables(tab.data(), ops.data());
    std::unique_ptr<iss_inf::Work> work(new iss_inf::Work);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t pay_len = 0, isize = 0, crc = 0;
        if (!read_u32(in, &pay_len) || !read_u32(in, &isize) || !read_u32(in, &crc)) return 2;
        std::unique_ptr<uint8_t[]> pay(new uint8_t[pay_len]), data(new uint8_t[isize]);  // exact sizes: no slack for a stray access
        if (pay_len && fread(pay.get(), 1, pay_len, in) != pay_len) return 2;
        memset(work.get(), 0xA5, sizeof(iss_inf::Work));  // (nothing may depend on what the member before left behind)
        uint32_t got = 0;
        const int st = iss_inf::inflate_member(pay.get(), pay_len, data.get(), isize, crc, *work, tab.data(), ops.data(), 0, 1, iss_inf::NoSync{}, &got);
        printf("%u %d %08x\n", i, st, got);
        if ((st == iss_inf::ST_OK || st == iss_inf::ST_TRAILING) && isize && fwrite(data.get(), 1, isize, out) != isize) return 2;
    }
    fclose(in);
    fclose(out);
    return 0;
}
