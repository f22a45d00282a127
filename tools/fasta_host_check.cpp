// fasta_host_check.cpp -- a stand-alone driver of iss_fasta_host_index and of the table check of iss_genome_upload_fasta (the host
// build of iss_fasta_core.h, the grammar the k_fa_* kernels are compiled from) over the hand cases of DESIGN.md section 31, for a run
// under the host sanitizers.  It needs no GPU.  The library's source is compiled in, so the entries run instrumented:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I include -x hip tools/fasta_host_check.cpp -o fasta_host_check && ./fasta_host_check
// Every buffer is a std::vector of exactly the size the entry may touch, so a byte read or written outside it is reported.
#include "../insilicoseq_amd/csrc/iss_mi355x.hip"

#include <cstdio>
#include <string>
#include <vector>

namespace {

struct Row {
    int64_t header_off, header_len, body_off, body_len, letters;
    int32_t flags;
    bool operator==(const Row &o) const {
        return header_off == o.header_off && header_len == o.header_len && body_off == o.body_off && body_len == o.body_len &&
               letters == o.letters && flags == o.flags;
    }
};

// the grammar byte by byte, without the core header
std::vector<Row> naive(const std::string &t) {
    const int64_t n = (int64_t)t.size();
    std::vector<int64_t> heads;
    for (int64_t i = 0; i < n; ++i)
        if (t[(size_t)i] == '>' && (i == 0 || t[(size_t)i - 1] == '\n')) heads.push_back(i);
    std::vector<Row> rows;
    for (size_t r = 0; r < heads.size(); ++r) {
        const int64_t h = heads[r], end = r + 1 < heads.size() ? heads[r + 1] : n;
        int64_t eol = h;
        while (eol < end && t[(size_t)eol] != '\n') ++eol;
        Row row{h, eol - h - 1, eol < end ? eol + 1 : end, 0, 0, 0};
        row.body_len = end - row.body_off;
        for (int64_t i = row.body_off; i < end; ++i) {
            const unsigned char c = (unsigned char)t[(size_t)i];
            if (c == '\r' || c == '\n') continue;
            ++row.letters;
            if (c < 0x21 || c > 0x7E) row.flags = ISS_FA_ODD;
        }
        rows.push_back(row);
    }
    return rows;
}

int run_case(const char *name, const std::string &t) {
    const std::vector<Row> want = naive(t);
    std::vector<uint8_t> text(t.begin(), t.end());
    int64_t n = -1;
    int rc = iss_fasta_host_index(text.data(), (int64_t)text.size(), 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n);
    if (rc || n != (int64_t)want.size()) {
        fprintf(stderr, "%s: count: rc %d, %lld records, want %zu\n", name, rc, (long long)n, want.size());
        return 1;
    }
    const size_t m = want.size();
    std::vector<int64_t> ho(m), hl(m), bo(m), bl(m), le(m);
    std::vector<int32_t> fl(m);
    rc = iss_fasta_host_index(text.data(), (int64_t)text.size(), (int64_t)m, ho.data(), hl.data(), bo.data(), bl.data(), le.data(), fl.data(), &n);
    bool ok = rc == 0 && n == (int64_t)m;
    for (size_t r = 0; ok && r < m; ++r) ok = Row{ho[r], hl[r], bo[r], bl[r], le[r], fl[r]} == want[r];
    if (!ok) {
        fprintf(stderr, "%s: rows differ (rc %d)\n", name, rc);
        return 1;
    }
    // the table the upload would get passes its check, over the whole text and over the span of its bodies
    int rule = -1;
    if (iss::fa::fa_table_check((int64_t)text.size(), (int64_t)m, bo.data(), bl.data(), le.data(), &rule) != -1 || rule != 0) {
        fprintf(stderr, "%s: its own table was refused (rule %d)\n", name, rule);
        return 1;
    }
    // the 16-byte masks the kernels take, over every aligned piece, against the byte rules
    for (size_t at = 0; at < text.size(); at += 16) {
        uint32_t w[4] = {0, 0, 0, 0};
        const int nv = (int)std::min<size_t>(16, text.size() - at);
        memcpy(w, text.data() + at, (size_t)nv);
        const iss::fa::Masks16 mk = iss::fa::fa_masks16(w, nv, at ? text[at - 1] : 0x0Au);
        for (int j = 0; j < 16; ++j) {
            const bool in = j < nv;
            const uint32_t c = in ? text[at + (size_t)j] : 0u, prev = in && at + (size_t)j ? text[at + (size_t)j - 1] : 0x0Au;
            if (((mk.eol >> j) & 1u) != (in && iss::fa::fa_is_eol(c)) || ((mk.odd >> j) & 1u) != (in && iss::fa::fa_is_odd(c)) ||
                ((mk.head >> j) & 1u) != (in && iss::fa::fa_is_header(prev, c))) {
                fprintf(stderr, "%s: masks differ at byte %zu\n", name, at + (size_t)j);
                return 1;
            }
        }
    }
    printf("%s ok (%zu records)\n", name, m);
    return 0;
}

int refused(const char *name, int64_t n_bytes, std::vector<int64_t> bo, std::vector<int64_t> bl, std::vector<int64_t> le, int64_t row, int want_rule) {
    int rule = 0;
    const int64_t got = iss::fa::fa_table_check(n_bytes, (int64_t)bo.size(), bo.data(), bl.data(), le.data(), &rule);
    if (got != row || rule != want_rule) {
        fprintf(stderr, "%s: row %lld rule %d, want row %lld rule %d\n", name, (long long)got, rule, (long long)row, want_rule);
        return 1;
    }
    printf("%s refused\n", name);
    return 0;
}

}  // namespace

int main() {
    int bad = 0;
    bad += run_case("empty_file", "");
    bad += run_case("no_header_at_all", "ACGT\nACGT\n");
    bad += run_case("junk_in_front", "junk line\nmore junk\n>a first\nACGT\nAC\n>b\nGG\n");
    bad += run_case("gt_inside_a_line", ">a\nAC>GT\nA>\n>b x\nTT\n");
    bad += run_case("header_as_last_line", ">a\nACGT\n>b no newline");
    bad += run_case("empty_record_between_headers", ">a\n>b\nACGT\n>c\n");
    bad += run_case("header_is_gt_alone", ">\nACGT\n>\n>x\nA\n");
    bad += run_case("crlf", ">a desc\r\nACGT\r\nAC\r\n>b\r\nGG\r\n");
    bad += run_case("lone_cr_inside_a_line", ">a\nAC\rGT\nA\r\n");
    bad += run_case("blank_lines", "\n\n>a\n\nAC\n\n\nGT\n\n>b\n\n");
    bad += run_case("no_final_newline", ">a\nACGT\nACG");
    bad += run_case("body_with_a_space", ">a\nAC GT\n  AC\n>b\nGG\n");
    bad += run_case("body_with_a_tab", ">a\nAC\tGT\n>b\nGG\n");
    bad += run_case("body_with_a_vertical_tab", ">a\nAC\x0bGT\n>b\nGG\n");
    bad += run_case("body_with_a_form_feed", ">a\nAC\x0c" "GT\nAA\n>b\nGG\n");
    bad += run_case("body_with_a_high_byte", ">a\nAC\xc3\xa9GT\n>b\nGG\n");
    bad += run_case("body_with_a_del_byte", ">a\nAC\x7fGT\n>b\nGG\n");
    bad += run_case("lower_case_and_iupac", ">a\nacgtnRYKM\nswbdhvN\n>b\nNNNN\n");
    bad += run_case("four_tiny_records_in_16_bytes", ">\nAC\n>\nGT\n>\nTT\n>\nCA\n");
    bad += run_case("four_tiny_records_in_one_lane", "thirteen junk\n>\nAC\n>\nGT\n>\nTT\n>\nCA\n");
    bad += run_case("header_only_file", ">only");
    bad += run_case("cr_before_header_is_no_line_end", ">a\nAC\r>b\nGG\n");
    {   // a text over three tiles with a header at the second tile's first byte
        std::string big = ">a\n";
        while (big.size() + 61 < (size_t)iss::fa::FA_TILE) big += std::string(60, "ACGT"[big.size() & 3]) + "\n";
        big += std::string((size_t)iss::fa::FA_TILE - big.size() - 1, 'C') + "\n>b at the edge\n";
        for (int k = 0; k < 150; ++k) big += std::string(59, 'G') + "\r\n";
        bad += run_case("across_tiles", big);
    }
    // tables that break a rule are refused: nothing would be launched
    bad += refused("a range past the span", 20, {2, 12}, {4, 9}, {4, 9}, 1, 1);
    bad += refused("a negative offset", 20, {-1}, {4}, {4}, 0, 1);
    bad += refused("overlapping bodies", 20, {2, 5}, {4, 4}, {4, 4}, 1, 2);
    bad += refused("bodies out of order", 20, {10, 2}, {4, 4}, {4, 4}, 1, 2);
    bad += refused("letters too large", 20, {2, 8}, {4, 4}, {4, 5}, 1, 3);
    bad += refused("negative letters", 20, {2}, {4}, {-1}, 0, 3);
    {   // ... and through the entry itself: the check comes before the context is touched beyond its error text
        const int64_t bo[1] = {30}, bl[1] = {4}, le[1] = {4};
        int32_t id = 7;
        const uint8_t text[8] = {'>', 'a', '\n', 'A', 'C', 'G', 'T', '\n'};
        if (iss_genome_upload_fasta(nullptr, text, 8, 1, bo, bl, le, &id) != ISS_E_INVALID) {
            fprintf(stderr, "a NULL context was not refused\n");
            ++bad;
        }
    }
    if (bad) return 1;
    printf("all ok\n");
    return 0;
}
