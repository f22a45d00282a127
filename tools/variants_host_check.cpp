// variants_host_check.cpp -- a stand-alone driver of iss_variants_host_apply and iss_variants_host_lift (the host build of
// iss_variants_core.h, the mapping the splice and lift kernels are compiled from) over the hand cases of DESIGN.md section 30, for a
// run under the host sanitizers.  It needs no GPU.  The library's source is compiled in, so the entries run instrumented:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I include -x hip tools/variants_host_check.cpp -o variants_host_check && ./variants_host_check
// Every buffer is a std::vector of exactly the size the entry may touch, so a byte read or written outside it is reported.
#include "../insilicoseq_amd/csrc/iss_mi355x.hip"

#include <cstdio>
#include <string>
#include <vector>

namespace {

struct Variant {
    int64_t pos0;
    std::string ref, alt;
};

int run_case(const char *name, const std::string &seq, const std::vector<Variant> &vs) {
    const int64_t n = (int64_t)vs.size(), L = (int64_t)seq.size();
    std::vector<int64_t> pos0, alt_off, out_pos;
    std::vector<int32_t> ref_len, alt_len;
    std::string alt;
    int64_t delta = 0;
    for (const Variant &v : vs) {
        pos0.push_back(v.pos0);
        ref_len.push_back((int32_t)v.ref.size());
        alt_len.push_back((int32_t)v.alt.size());
        alt_off.push_back((int64_t)alt.size());
        out_pos.push_back(v.pos0 + delta);
        alt += v.alt;
        delta += (int64_t)v.alt.size() - (int64_t)v.ref.size();
    }
    out_pos.push_back(L + delta);
    // the naive splice, from the right to the left
    std::string want = seq;
    for (int64_t i = n - 1; i >= 0; --i) want.replace((size_t)vs[(size_t)i].pos0, vs[(size_t)i].ref.size(), vs[(size_t)i].alt);
    std::vector<uint8_t> src(seq.begin(), seq.end()), blob(alt.begin(), alt.end()), out((size_t)(L + delta));
    int rc = iss_variants_host_apply(src.data(), L, n, pos0.data(), ref_len.data(), alt_len.data(), alt_off.data(), blob.data(),
                                     (int64_t)blob.size(), out_pos.data(), out.data(), (int64_t)out.size());
    if (rc || std::string(out.begin(), out.end()) != want) {
        fprintf(stderr, "%s: apply: rc %d, got %.*s, want %s\n", name, rc, (int)out.size(), (const char *)out.data(), want.c_str());
        return 1;
    }
    std::vector<int64_t> h((size_t)(L + delta) + 1), lifted(h.size());
    for (size_t t = 0; t < h.size(); ++t) h[t] = (int64_t)t;
    rc = iss_variants_host_lift(n, pos0.data(), ref_len.data(), alt_len.data(), out_pos.data(), h.data(), (int64_t)h.size(), lifted.data());
    bool ok = rc == 0 && lifted.back() == L;
    for (size_t t = 1; ok && t < lifted.size(); ++t) ok = lifted[t] >= lifted[t - 1];
    for (int64_t i = 0; ok && i < n; ++i)  // an ALT run's letters: the replaced ones, then the end of what was replaced
        for (int64_t k = 0; ok && k < alt_len[(size_t)i]; ++k)
            ok = lifted[(size_t)(out_pos[(size_t)i] + k)] == pos0[(size_t)i] + std::min<int64_t>(k, ref_len[(size_t)i]);
    if (!ok) {
        fprintf(stderr, "%s: lift: rc %d\n", name, rc);
        return 1;
    }
    printf("%s ok\n", name);
    return 0;
}

}  // namespace

int main() {
    const std::string s = "ACGTTGCAAGGCTTAC";
    std::vector<Variant> every_other;
    for (size_t i = 0; i < s.size(); i += 2) every_other.push_back({(int64_t)i, s.substr(i, 1), s[i] == 'A' ? "C" : "A"});
    int bad = 0;
    bad += run_case("variant_at_pos_1", s, {{0, "A", "T"}});
    bad += run_case("deletion_of_the_last_base", s, {{(int64_t)s.size() - 1, "C", ""}});
    bad += run_case("insertion_after_the_last_base", s, {{(int64_t)s.size(), "", "GGA"}});
    bad += run_case("deletion_then_insertion", s, {{2, "GT", ""}, {4, "", "CCC"}});
    bad += run_case("insertion_at_the_start_of_a_substitution", s, {{5, "", "AA"}, {5, "GC", "TT"}});
    bad += run_case("every_other_base", s, every_other);
    bad += run_case("empty_table", s, {});
    bad += run_case("length_1_snv", "g", {{0, "G", "t"}});
    bad += run_case("length_1_insertions", "A", {{0, "", "CC"}, {1, "", "T"}});
    bad += run_case("deletion_at_the_start", s, {{0, "ACG", ""}});
    bad += run_case("adjacent_deletions", s, {{3, "T", ""}, {4, "T", ""}, {5, "GC", ""}});
    {   // a record longer than one tile of the splice, a variant on either side of the boundary and one across it
        std::string big((size_t)iss::VAR_APPLY_TILE * 2 + 3, 'A');
        for (size_t i = 0; i < big.size(); ++i) big[i] = "ACGT"[(i * 7 + i / 5) & 3];
        const int64_t T = iss::VAR_APPLY_TILE;
        bad += run_case("across_a_tile", big, {{T - 9, big.substr((size_t)T - 9, 4), ""}, {T - 2, big.substr((size_t)T - 2, 6), "TT"},
                                               {2 * T - 20, "", std::string(40, 'G')}});
    }
    // tables that break a rule are refused before anything is read through them
    {
        std::vector<uint8_t> src(s.begin(), s.end()), out(64);
        const int64_t pos0[1] = {15}, alt_off[1] = {0}, out_pos[2] = {15, 14};
        const int32_t ref_len[1] = {3}, alt_len[1] = {1};
        const uint8_t alt[1] = {'A'};
        if (iss_variants_host_apply(src.data(), 16, 1, pos0, ref_len, alt_len, alt_off, alt, 1, out_pos, out.data(), 64) != ISS_E_INVALID) {
            fprintf(stderr, "a variant past the record's end was not refused\n");
            ++bad;
        }
    }
    if (bad) return 1;
    printf("all ok\n");
    return 0;
}
