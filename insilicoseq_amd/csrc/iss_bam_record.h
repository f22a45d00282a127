// iss_bam_record.h -- one BAM alignment record as its readers see it (k_bam_tally, k_br_*, k_be_*, k_bd_records): the unaligned
// load, the fixed fields and the offsets behind them, the packed bases, the CIGAR op classes, the walk over the optional fields up
// to MD:Z, and --errors' MD walk.  Only the READING: which records a kernel takes and which codes it raises are its own.  Plain C++ for the device and the
// host (tools/bam_errors_walk.cpp runs it under a sanitizer); nothing reads outside the range it is handed.  DESIGN.md section 33.
#pragma once
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ISS_REC_HD __host__ __device__ __forceinline__
#else
#define ISS_REC_HD inline
#endif

namespace iss {
namespace brec {
ISS_REC_HD uint32_t u32(const uint8_t *p) {  // little-endian (as the host and the device are); a record starts at any alignment
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

constexpr int FIXED = 36;  // block_size and the 32 fixed bytes of a record
// The fixed fields of the record at rec (FIXED readable bytes), and where the variable ones lie: byte offsets from rec.  They
// are inside the record -- rec + 4 + block_size its end -- only where fits() holds.
struct RecHead {
    int32_t block_size, ref_id, pos, l_seq, next_ref, tlen;
    uint32_t l_name, mapq, n_cigar, flag;
    ISS_REC_HD uint32_t var() const { return l_name + 4u * n_cigar; }  // (at most 255 + 4 * 65535)
    ISS_REC_HD bool fits() const { return l_seq >= 0 && 32ll + var() + ((int64_t)l_seq + 1) / 2 + l_seq <= (int64_t)block_size; }
    // (32 bits hold every offset of a record with l_seq >= 0: below 2^19 + 2^30 + 2^31)
    ISS_REC_HD uint32_t cigar_at() const { return (uint32_t)FIXED + l_name; }
    ISS_REC_HD uint32_t seq_at() const { return (uint32_t)FIXED + var(); }
    ISS_REC_HD uint32_t qual_at() const { return seq_at() + ((uint32_t)l_seq + 1u) / 2u; }
    ISS_REC_HD uint32_t aux_at() const { return qual_at() + (uint32_t)l_seq; }
    ISS_REC_HD int64_t end() const { return 4 + (int64_t)block_size; }
};
ISS_REC_HD RecHead rec_head(const uint8_t *rec) {
    const uint32_t w12 = u32(rec + 12), w16 = u32(rec + 16);  // l_read_name, mapq, bin | n_cigar_op, flag
    return RecHead{(int32_t)u32(rec), (int32_t)u32(rec + 4), (int32_t)u32(rec + 8), (int32_t)u32(rec + 20), (int32_t)u32(rec + 24),
                   (int32_t)u32(rec + 32), w12 & 0xFFu, (w12 >> 8) & 0xFFu, w16 & 0xFFFFu, w16 >> 16};
}

// base q of the SEQ at data + seq_at as its 4-bit code ("=ACMGRSVTWYHKDBN"): the high half of byte q / 2 for even q, else the low
ISS_REC_HD uint32_t seq_nibble(const uint8_t *data, uint32_t seq_at, uint32_t q) { return ((uint32_t)data[seq_at + (q >> 1)] >> ((q & 1u) ? 0u : 4u)) & 15u; }
ISS_REC_HD uint32_t nib_code(uint32_t nib) { return nib == 1u ? 0u : nib == 2u ? 1u : nib == 4u ? 2u : nib == 8u ? 3u : 4u; }  // A, C, G, T, else 4

// CIGAR ops "MIDNSHP=X" (0 .. 8) and their classes, as sets of op codes
enum : uint32_t { OP_M = 0, OP_I = 1, OP_D = 2, OP_N = 3, OP_S = 4, OP_H = 5, OP_P = 6, OP_EQ = 7, OP_X = 8, OP_LAST = OP_X };
constexpr uint32_t OPS_COLUMN = 1u << OP_M | 1u << OP_EQ | 1u << OP_X;  // aligned columns: what MD describes
constexpr uint32_t OPS_QUERY = OPS_COLUMN | 1u << OP_I | 1u << OP_S;    // consume the read
constexpr uint32_t OPS_REF = OPS_COLUMN | 1u << OP_D | 1u << OP_N;      // consume the reference
ISS_REC_HD bool in(uint32_t op, uint32_t set) { return ((set >> op) & 1u) != 0u; }  // (op: the low four bits of a CIGAR word)
constexpr int BE_TAGS_MD = 0, BE_TAGS_NO_MD = 1, BE_TAGS_BAD = 2;
// The optional fields a[0 .. n): stops at the first MD:Z (its text at *md_at, *md_len bytes without the NUL).  Fewer than three
// bytes left end the walk cleanly.  BE_TAGS_BAD: an unknown type byte, a value past the end, a Z / H without its NUL, a B with an
// unknown subtype or a negative count.
ISS_REC_HD int be_tag_walk(const uint8_t *a, int64_t n, int64_t *md_at, uint32_t *md_len) {
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
            const int64_t cnt = (int32_t)u32(a + at + 1);
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
}  // namespace brec

// The serial walk of `report --bam --errors` over a record's MD string against its CIGAR (lane 0 of k_be_records' wavefront runs
// it).  Numbers saturate.
namespace be {
using brec::u32, brec::in, brec::OP_D, brec::OP_LAST, brec::OPS_COLUMN, brec::OPS_QUERY;
constexpr int BE_ALN_CIGAR = 1, BE_ALN_TAGS = 2, BE_ALN_MD = 3;  // (= ISS_BR_ALN_*)
constexpr uint32_t BE_NUM_SAT = 1u << 20;  // an MD number stops growing here: more columns than any read has (1 024 at most)
ISS_REC_HD bool be_digit(uint32_t ch) { return ch - (uint32_t)'0' < 10u; }
ISS_REC_HD bool be_letter(uint32_t ch) { return (ch | 0x20u) - (uint32_t)'a' < 26u; }
ISS_REC_HD uint32_t be_letter_code(uint32_t ch) {  // A, C, G, T in either case 0 .. 3, every other byte 4
    ch |= 0x20u;
    return ch == 'a' ? 0u : ch == 'c' ? 1u : ch == 'g' ? 2u : ch == 't' ? 3u : 4u;
}
ISS_REC_HD uint32_t be_complement(uint32_t code) { return code < 4u ? 3u - code : 4u; }

// The MD string md[0 .. md_len) against the n_cigar operations at cig (4 bytes each, op in the low four bits; the caller has seen
// every op <= OP_LAST).  M, = and X take their columns from numbers and letters: on_mismatch(q, letter) for a letter at SEQ index
// q; a number carries over I, N, S, H and P.  D of length n wants the running number used up (zeros may be skipped), then '^' and
// exactly n letters: on_deletion(q, letter) for each, q the query bases in front of the gap.  Behind the last operation nothing
// but zeros may stand.  False: the string does not fit (a callback may have run by then: the caller adds counts only behind a
// walk that returned true).
template <class Mismatch, class Deletion>
ISS_REC_HD bool be_md_walk(const uint8_t *cig, uint32_t n_cigar, const uint8_t *md, uint32_t md_len, Mismatch on_mismatch,
                          Deletion on_deletion) {
    uint32_t k = 0, num = 0, q = 0;
    for (uint32_t i = 0; i < n_cigar; ++i) {
        const uint32_t c = u32(cig + 4 * (size_t)i), op = c & 15u;
        uint32_t n = c >> 4;
        if (in(op, OPS_COLUMN)) {
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
        } else if (in(op, OPS_QUERY)) {  // I, S
            q += n;
        } else if (op == OP_D) {
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
