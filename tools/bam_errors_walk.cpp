// bam_errors_walk.cpp -- the record view and the tag walk every BAM kernel reads through and the MD walk of `report --bam --errors`
// (insilicoseq_amd/csrc/iss_bam_record.h) -- the code lane 0 of k_be_records runs, the tag walk lane 0 of k_bam_tally too -- driven
// on the host, one record at a time, so that a sanitizer can watch them on damaged records:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I insilicoseq_amd/csrc -o bam_errors_walk tools/bam_errors_walk.cpp
//   ./bam_errors_walk records.bin
// records.bin: the raw alignment records (block_size first) back to back, as tests/test_bam_errors_walk_host.py writes them from the
// test cases.  Every record is copied into a heap block of exactly its own size, so that a read past either end is seen.
// One line per record: U not aligned | N no MD | 1 2 3 the ISS_BR_ALN_* code | T tallied, then its mismatches and deleted letters.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "iss_bam_record.h"

using namespace iss::be;
using namespace iss::brec;

static void one(const uint8_t *rec, int64_t size) {
    const RecHead h = rec_head(rec);
    const uint32_t n_cigar = h.n_cigar;
    const int64_t l_seq = h.l_seq;
    if (size != h.end() || !h.fits()) {
        puts("S");  // not a record the read tally takes: the walks never see it
        return;
    }
    if ((h.flag & 4u) || !n_cigar || !l_seq) {
        puts("U");
        return;
    }
    const uint8_t *const cig = rec + h.cigar_at();
    unsigned long long qsum = 0;
    bool bad_op = false;
    for (uint32_t i = 0; i < n_cigar; ++i) {
        const uint32_t c = u32(cig + 4 * i), op = c & 15u;
        bad_op |= op > OP_LAST;
        if (in(op, OPS_QUERY)) qsum += c >> 4;
    }
    if (bad_op || qsum != (unsigned long long)l_seq) {
        printf("%d\n", BE_ALN_CIGAR);
        return;
    }
    const uint8_t *const aux = rec + h.aux_at();
    int64_t md_at = 0;
    uint32_t md_len = 0;
    const int st = be_tag_walk(aux, (rec + size) - aux, &md_at, &md_len);
    if (st != BE_TAGS_MD) {
        puts(st == BE_TAGS_NO_MD ? "N" : "2");
        return;
    }
    std::vector<uint8_t> map((size_t)l_seq, 0);  // (exactly the read's length: a mismatch placed past it is seen)
    uint32_t n_mism = 0, n_del = 0;
    const bool ok = be_md_walk(cig, n_cigar, aux + md_at, md_len,
                               [&](uint32_t q, uint32_t ch) { map.at(q) = (uint8_t)(0x80u | be_letter_code(ch)); ++n_mism; },
                               [&](uint32_t q, uint32_t) { if ((int64_t)q > l_seq) abort(); ++n_del; });
    if (!ok) printf("%d\n", BE_ALN_MD);
    else printf("T %u %u\n", n_mism, n_del);
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s records.bin\n", argv[0]);
        return 2;
    }
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) {
        perror(argv[1]);
        return 2;
    }
    for (;;) {
        uint8_t head[4];
        if (fread(head, 1, 4, fh) != 4) break;
        const int64_t block_size = (int32_t)u32(head);
        if (block_size < 32 || block_size > (1 << 28)) {
            fprintf(stderr, "block_size %lld: not a record\n", (long long)block_size);
            return 2;
        }
        uint8_t *rec = (uint8_t *)malloc((size_t)(4 + block_size));
        memcpy(rec, head, 4);
        if (fread(rec + 4, 1, (size_t)block_size, fh) != (size_t)block_size) {
            fprintf(stderr, "the file ends inside a record\n");
            return 2;
        }
        one(rec, 4 + block_size);
        free(rec);
    }
    fclose(fh);
    return 0;
}
