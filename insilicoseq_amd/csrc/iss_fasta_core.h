// iss_fasta_core.h -- `generate --device_fasta`: the grammar of a FASTA text as the kernels and the host read it.  Plain C++ that
// compiles for the device (iss_fasta.hip.h: k_fa_*) and for the host (iss_fasta_host_index, the table check of
// iss_genome_upload_fasta; tools/fasta_host_check.cpp drives both under a sanitizer).  DESIGN.md section 31.
//
// The text is n bytes.  A HEADER starts at a '>' that is byte 0 or directly follows '\n'; bytes in front of the first header are
// ignored.  Record r runs from its header's '>' (header_off) to the next header's '>' or the end of the text (`end`):
//     eol         the first '\n' in [header_off, end), or `end` when there is none (a header as the last line, no '\n')
//     header_len  eol - header_off - 1: the bytes between '>' and that '\n' (a '\r' in front of it included: the host strips it)
//     body_off    eol + 1, or `end` when there is no '\n';   body_len = end - body_off
//     letters     the body's bytes other than '\r' and '\n'
//     flags       FA_ODD when the body holds a byte outside 0x21 .. 0x7E other than '\r' and '\n': white space inside a line, a
//                 control byte, a byte of a multi-byte character -- everything for which the host's strip() / splitlines() / decode()
//                 could see another sequence than "the bytes that are no line ends".  Such a record takes the host parser.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ISS_FA_HD __host__ __device__ __forceinline__
#else
#define ISS_FA_HD inline
#endif

namespace iss {
namespace fa {

constexpr int32_t FA_ODD = 1;

ISS_FA_HD bool fa_is_eol(uint32_t c) { return c == 0x0Au || c == 0x0Du; }
ISS_FA_HD bool fa_is_odd(uint32_t c) { return !fa_is_eol(c) && (c < 0x21u || c > 0x7Eu); }
// `prev`: the byte in front (byte 0 of the text: '\n')
ISS_FA_HD bool fa_is_header(uint32_t prev, uint32_t c) { return c == (uint32_t)'>' && prev == 0x0Au; }

// byte j (0 .. 15) of 16 bytes held as four little-endian words
ISS_FA_HD uint32_t fa_byte16(const uint32_t w[4], int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xFFu; }

// bit j of each mask: what byte j of the 16 bytes in w is; the first `nv` of them are bytes of the text (0 .. 16), `prev` stands in
// front of byte 0
struct Masks16 {
    uint32_t eol, odd, head;
};
ISS_FA_HD Masks16 fa_masks16(const uint32_t w[4], int nv, uint32_t prev) {
    Masks16 m = {0u, 0u, 0u};
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
    for (int j = 0; j < 16; ++j) {
        const uint32_t c = fa_byte16(w, j);
        m.eol |= (fa_is_eol(c) ? 1u : 0u) << j;
        m.odd |= (fa_is_odd(c) ? 1u : 0u) << j;
        m.head |= (fa_is_header(prev, c) ? 1u : 0u) << j;
        prev = c;
    }
    const uint32_t keep = nv >= 16 ? 0xFFFFu : (1u << (nv < 0 ? 0 : nv)) - 1u;
    m.eol &= keep;
    m.odd &= keep;
    m.head &= keep;
    return m;
}

// The row of a record from its three offsets (see above).
ISS_FA_HD void fa_row(int64_t header_off, int64_t eol, int64_t end, int64_t *header_len, int64_t *body_off, int64_t *body_len) {
    *header_len = eol - header_off - 1;
    *body_off = eol < end ? eol + 1 : end;
    *body_len = end - *body_off;
}

// The table iss_genome_upload_fasta takes, over a span of n_bytes: every body inside the span, ascending, not overlapping, no more
// letters than bytes.  Returns the first row that breaks a rule (*rule: 1 a range outside the span, 2 out of order or overlapping,
// 3 more letters than the body has bytes), or -1.
ISS_FA_HD int64_t fa_table_check(int64_t n_bytes, int64_t n, const int64_t *body_off, const int64_t *body_len, const int64_t *letters,
                                 int *rule) {
    int64_t at = 0;
    for (int64_t k = 0; k < n; ++k) {
        if (body_off[k] < 0 || body_len[k] < 0 || body_off[k] > n_bytes || body_len[k] > n_bytes - body_off[k]) { *rule = 1; return k; }
        if (body_off[k] < at) { *rule = 2; return k; }
        if (letters[k] < 0 || letters[k] > body_len[k]) { *rule = 3; return k; }
        at = body_off[k] + body_len[k];
    }
    *rule = 0;
    return -1;
}

// The last k in [0, n) with off[k] <= p, or -1.
ISS_FA_HD int64_t fa_find(const int64_t *off, int64_t n, int64_t p) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

}  // namespace fa
}  // namespace iss
