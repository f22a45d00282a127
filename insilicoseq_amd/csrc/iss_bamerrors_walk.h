// iss_bamerrors_walk.h -- the two serial walks of `report --bam --errors` over one alignment record: the optional fields up to the
// first MD:Z, and the MD string against the CIGAR.  Plain C++ that compiles for the device (iss_bamerrors.hip.h: lane 0 of a record's
// wavefront runs them) and for the host (tools/bam_errors_walk.cpp drives them under a sanitizer).  Neither walk reads a byte
// outside the ranges it is handed, whatever those bytes hold; numbers saturate.  DESIGN.md section 29.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ISS_BE_HD __host__ __device__ __forceinline__
#else
#define ISS_BE_HD inline
#endif

namespace iss {
namespace be {

constexpr int BE_ALN_CIGAR = 1, BE_ALN_TAGS = 2, BE_ALN_MD = 3;  // (= ISS_BR_ALN_*)
constexpr int BE_TAGS_MD = 0, BE_TAGS_NO_MD = 1, BE_TAGS_BAD = 2;
constexpr uint32_t BE_NUM_SAT = 1u << 20;  // an MD number stops growing here: more columns than any read has (1 024 at most)

ISS_BE_HD uint32_t be_u32(const uint8_t *p) {  // (a record starts at any alignment)
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
ISS_BE_HD bool be_digit(uint32_t ch) { return ch - (uint32_t)'0' < 10u; }
ISS_BE_HD bool be_letter(uint32_t ch) { return (ch | 0x20u) - (uint32_t)'a' < 26u; }
ISS_BE_HD uint32_t be_letter_code(uint32_t ch) {  // A, C, G, T in either case 0 .. 3, every other byte 4
    ch |= 0x20u;
    return ch == 'a' ? 0u : ch == 'c' ? 1u : ch == 'g' ? 2u : ch == 't' ? 3u : 4u;
}
ISS_BE_HD uint32_t be_complement(uint32_t code) { return code < 4u ? 3u - code : 4u; }

// The optional fields a[0 .. n): stops at the first MD:Z (its text at *md_at, *md_len bytes without the NUL).  Fewer than three
// bytes left end the walk cleanly.  BE_TAGS_BAD: an unknown type byte, a value past the end, a Z / H without its NUL, a B with an
// unknown subtype or a negative count.
ISS_BE_HD int be_tag_walk(const uint8_t *a, int64_t n, int64_t *md_at, uint32_t *md_len) {
    int64_t at = 0;
    while (at + 3 <= n) {
        const uint8_t t0 = a[at], t1 = a[at + 1], ty = a[at + 2];
        at += 3;
        int64_t sz;
        if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1;
        else if (ty == 's' || ty == 'S') sz = 2;
        else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
        else if (ty == 'Z' || ty == 'H') {
            int64_t z = at;
            while (z < n && a[z]) ++z;
            if (z >= n) return BE_TAGS_BAD;
            if (t0 == 'M' && t1 == 'D' && ty == 'Z') {
                *md_at = at;
                *md_len = (uint32_t)(z - at);
                return BE_TAGS_MD;
            }
            sz = z - at + 1;
        } else if (ty == 'B') {
            if (at + 5 > n) return BE_TAGS_BAD;
            const uint8_t sub = a[at];
            const int64_t cnt = (int32_t)be_u32(a + at + 1);
            const int64_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
            if (!es || cnt < 0) return BE_TAGS_BAD;
            sz = 5 + cnt * es;
        } else {
            return BE_TAGS_BAD;
        }
        if (at + sz > n) return BE_TAGS_BAD;
        at += sz;
    }
    return BE_TAGS_NO_MD;
}

// The MD string md[0 .. md_len) against the n_cigar operations at cig (4 bytes each, op in the low four bits; the caller has seen
// every op <= 8).  M, = and X take their columns from numbers and letters: on_mismatch(q, letter) for a letter at SEQ index q; a
// number carries over I, N, S, H and P.  D of length n wants the running number used up (zeros may be skipped), then '^' and
// exactly n letters: on_deletion(q, letter) for each, q the query bases in front of the gap.  Behind the last operation nothing
// but zeros may stand.  False: the string does not fit (a callback may have run by then: the caller adds counts only behind a
// walk that returned true).
template <class Mismatch, class Deletion>
ISS_BE_HD bool be_md_walk(const uint8_t *cig, uint32_t n_cigar, const uint8_t *md, uint32_t md_len, Mismatch on_mismatch,
                          Deletion on_deletion) {
    uint32_t k = 0, num = 0, q = 0;
    for (uint32_t i = 0; i < n_cigar; ++i) {
        const uint32_t c = be_u32(cig + 4 * (size_t)i), op = c & 15u;
        uint32_t n = c >> 4;
        if (op == 0u || op == 7u || op == 8u) {
            while (n) {
                if (num) {
                    const uint32_t t = num < n ? num : n;
                    num -= t;
                    n -= t;
                    q += t;
                    continue;
                }
                if (k >= md_len) return false;  // too short
                const uint32_t ch = md[k];
                if (be_digit(ch)) {
                    while (k < md_len && be_digit(md[k])) {
                        const uint32_t v = num * 10u + (md[k] - (uint32_t)'0');  // (num <= 2^20: no overflow)
                        num = v < BE_NUM_SAT ? v : BE_NUM_SAT;
                        ++k;
                    }
                } else if (be_letter(ch)) {
                    on_mismatch(q, ch);
                    ++q;
                    --n;
                    ++k;
                } else {
                    return false;  // '^' inside aligned columns, or a stray byte
                }
            }
        } else if (op == 1u || op == 4u) {
            q += n;
        } else if (op == 2u) {
            if (num) return false;  // a number that runs into the gap
            while (k < md_len && md[k] == '0') ++k;
            if (k >= md_len || md[k] != '^') return false;
            ++k;
            uint32_t got = 0;
            while (k < md_len && be_letter(md[k])) {
                if (got < n) on_deletion(q, (uint32_t)md[k]);
                ++got;
                ++k;
            }
            if (got == 0u || got != n) return false;
        }
    }
    if (num) return false;  // too long
    while (k < md_len && md[k] == '0') ++k;
    return k == md_len;
}

}  // namespace be
}  // namespace iss
