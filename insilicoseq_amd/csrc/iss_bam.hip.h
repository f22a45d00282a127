// iss_bam.hip.h -- device side of `model` (the reference's `iss model`, iss/bam.py:103-227 + iss/modeller.py): integer tallies over
// BAM alignment records (k_bam_tally, k_bam_qhist) and the quality / insert-size kernel density estimates built from them (k_kde_cdf).
//
// Records arrive as the inflated bytes of a chunk of the file plus the byte offset of every record's block_size field (host scan,
// iss_bam_scan) and a selection byte per record (the subsample, iss/bam.py:14-46).  All counts are integers: the tallies are exact and
// independent of the order in which records are processed.  Per-workgroup tables live in LDS and are added to the global u64 tables
// once per workgroup; a wave processes one record with its lanes over read positions, so the LDS increments of one wave instruction
// never collide.  DESIGN.md section 11 has the parity contract and the measured numbers.
#pragma once
#include "iss_bam_record.h"

namespace iss {
namespace bam {

constexpr int MAX_LEN = 301;  // the reference's [301][16] / [301][9] matrices (iss/bam.py:118-121)
constexpr int NQ = 94;        // phred 0..93 (SAM specification: qualities are 0..93)
constexpr int NTLEN = 2000;   // template lengths 0 < |tlen| < 2000 (iss/modeller.py:25-29)
constexpr int N_SLICE = 8;    // (mate, mean-quality bin): mate * 4 + bin

// word offsets of the global u64 tally (ISS_BAM_TALLY_WORDS words in all; include/iss_mi355x.h lists the same layout)
constexpr int OFF_SUBST = 0;                                // [2][301][16]
constexpr int OFF_INDEL = OFF_SUBST + 2 * MAX_LEN * 16;     // [2][301][9]
constexpr int OFF_QHIST = OFF_INDEL + 2 * MAX_LEN * 9;      // [8][301][94]
constexpr int OFF_TLEN = OFF_QHIST + N_SLICE * MAX_LEN * NQ;  // [2000]
constexpr int OFF_NREAD = OFF_TLEN + NTLEN;                 // [8] reads per (mate, bin)
constexpr int OFF_MINLEN = OFF_NREAD + N_SLICE;             // [8] shortest read per (mate, bin) (~0: none)
constexpr int OFF_TAKEN = OFF_MINLEN + N_SLICE;             // [8] [0] = records tallied
constexpr int TALLY_WORDS = OFF_TAKEN + 8;

// error codes of a record (the first one in file order is reported: ((record index) << 8) | code, atomicMin)
enum : uint32_t { E_REC_MALFORMED = 1, E_REC_TOO_LONG = 2, E_REC_NO_QUAL = 3, E_REC_CIGAR_OP = 4, E_REC_NO_MD = 5, E_REC_BAD_MD = 6,
                  E_REC_INDEL_INDEX = 7, E_REC_QUAL_RANGE = 8, E_REC_CIGAR_LEN = 9 };

constexpr int TALLY_THREADS = 256;
constexpr int TALLY_WAVES = TALLY_THREADS / 64;
constexpr int REFC_PITCH = 304;
struct TallyLds {
    uint32_t subst[2 * MAX_LEN * 16];
    uint32_t indel[2 * MAX_LEN * 9];
    uint32_t tlen[NTLEN];
    uint32_t nread[N_SLICE];
    uint32_t minlen[N_SLICE];
    uint32_t taken[4];
    uint8_t refc[TALLY_WAVES][REFC_PITCH];  // per query position: 0 not aligned, 1 match, 0x80 | letter a mismatch (MD)
};
constexpr size_t TALLY_LDS = sizeof(TallyLds);
constexpr size_t QHIST_LDS = sizeof(uint32_t) * MAX_LEN * NQ;

using brec::OP_D, brec::OP_H, brec::OP_I, brec::OP_M, brec::OP_S;
constexpr uint32_t OPS_MODEL_QUERY = 1u << OP_M | 1u << OP_I | 1u << OP_S, OPS_MODEL = OPS_MODEL_QUERY | 1u << OP_D | 1u << OP_H;  // of a tallied record
// 4-bit base code ("=ACMGRSVTWYHKDBN") -> index in A, T, C, G order; -1 for every other letter
__device__ __forceinline__ int nib_base(uint32_t nib) { return nib == 1 ? 0 : nib == 8 ? 1 : nib == 2 ? 2 : nib == 4 ? 3 : -1; }
__device__ __forceinline__ int md_base(uint32_t ch) {  // an MD letter, either case
    ch |= 0x20;
    return ch == 'a' ? 0 : ch == 't' ? 1 : ch == 'c' ? 2 : ch == 'g' ? 3 : 4;
}
// dispatch_dict of iss/modeller.py:162-179: [reference][query], both in A, T, C, G order
__device__ __forceinline__ int subst_col(int ref, int qry) {
    constexpr uint64_t T = 0xCFEDB8A967452310ull;  // 16 nibbles: A: 0 1 3 2, T: 5 4 7 6, C: 9 10 8 11, G: 13 14 15 12
    return (int)((T >> (4 * (ref * 4 + qry))) & 15);
}

__device__ __forceinline__ void report(unsigned long long *err, int64_t rec, uint32_t code) {
    atomicMin(err, ((unsigned long long)rec << 8) | code);
}

// One wave per record (lanes over read positions); every wave of a workgroup runs the same number of iterations (n_iter) so the phases
// can be separated by workgroup barriers.  meta[r] = {byte offset of the qualities, slice | reverse << 8 | length << 16} for k_bam_qhist
// (slice 0xFF: the record adds no qualities).
__global__ void __launch_bounds__(TALLY_THREADS) k_bam_tally(const uint8_t *__restrict__ data, const uint32_t *__restrict__ offs,
                                                             const uint8_t *__restrict__ select, int64_t n_rec, int64_t n_iter, int64_t rec_base,
                                                             uint2 *__restrict__ meta, unsigned long long *__restrict__ tally,
                                                             unsigned long long *__restrict__ err) {
    extern __shared__ __align__(16) uint8_t lds_raw[];
    TallyLds &L = *reinterpret_cast<TallyLds *>(lds_raw);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int i = tid; i < 2 * MAX_LEN * 16; i += TALLY_THREADS) L.subst[i] = 0;
    for (int i = tid; i < 2 * MAX_LEN * 9; i += TALLY_THREADS) L.indel[i] = 0;
    for (int i = tid; i < NTLEN; i += TALLY_THREADS) L.tlen[i] = 0;
    if (tid < N_SLICE) { L.nread[tid] = 0; L.minlen[tid] = 0xFFFFFFFFu; }
    if (tid < 4) L.taken[tid] = 0;
    uint8_t *refc = L.refc[w];
    __syncthreads();

    const int64_t stride = (int64_t)gridDim.x * TALLY_WAVES;  // n_iter = ceil(n_rec / stride), from the host
    for (int64_t it = 0; it < n_iter; ++it) {
        const int64_t r = it * stride + (int64_t)blockIdx.x * TALLY_WAVES + w;
        // ---- phase A: header, template length, qualities, CIGAR check, MD tag lookup
        bool live = r < n_rec && select[r] != 0;
        int mate = -1, l_seq = 0, n_cig = 0, md_off = 0, md_len = 0, m_total = 0;
        const uint8_t *p = nullptr, *cig = nullptr, *seq = nullptr;
        uint2 my_meta = make_uint2(0, 0xFFu);
        if (live) {
            const uint8_t *rec = data + offs[r];
            const brec::RecHead h = brec::rec_head(rec);
            const uint32_t flag = h.flag;
            const int32_t tlen = h.tlen;
            p = rec + 4;
            n_cig = (int)h.n_cigar;
            l_seq = h.l_seq;
            if (!h.fits()) {
                if (lane == 0) report(err, rec_base + r, E_REC_MALFORMED);
                live = false;
            } else if (l_seq > MAX_LEN) {
                if (lane == 0) report(err, rec_base + r, E_REC_TOO_LONG);
                live = false;
            }
            if (live) {
                if (lane == 0) atomicAdd(&L.taken[0], 1u);
                if (flag & 1) {  // is_paired: abs(template_length), kept when 0 < t < 2000 (iss/bam.py:126-129, modeller.py:25-29)
                    const int64_t t = tlen < 0 ? -(int64_t)tlen : (int64_t)tlen;
                    if (t > 0 && t < NTLEN && lane == 0) atomicAdd(&L.tlen[t], 1u);
                }
                mate = (flag & 64) ? 0 : (flag & 128) ? 1 : -1;
                cig = rec + h.cigar_at();
                seq = rec + h.seq_at();
                const uint8_t *qual = rec + h.qual_at();
                if (mate >= 0) {  // query_qualities, np.mean -> int (iss/bam.py:132-152, modeller.py:56-59)
                    if (l_seq == 0 || qual[0] == 0xFF) {
                        if (lane == 0) report(err, rec_base + r, E_REC_NO_QUAL);
                        live = false;
                    } else {
                        uint32_t s = 0;
                        bool bad = false;
                        for (int i = lane; i < l_seq; i += 64) {
                            const uint32_t q = qual[i];
                            s += q;
                            bad |= q >= NQ;
                        }
                        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
                        if (__any(bad)) {
                            if (lane == 0) report(err, rec_base + r, E_REC_QUAL_RANGE);
                            live = false;
                        } else {
                            const uint32_t mean = s / (uint32_t)l_seq;  // int(np.mean(q)): exact
                            if (mean < 40) {                           // np.split(range(40), 4); 40 and above: no bin
                                const uint32_t slice = (uint32_t)mate * 4 + mean / 10;
                                my_meta = make_uint2((uint32_t)(qual - data), slice | (((flag >> 4) & 1u) << 8) | ((uint32_t)l_seq << 16));
                                if (lane == 0) {
                                    atomicAdd(&L.nread[slice], 1u);
                                    atomicMin(&L.minlen[slice], (uint32_t)l_seq);
                                }
                            }
                        }
                    }
                }
            }
            if (live) {  // CIGAR: M / I / D / S / H only, query-consuming operations cover the read
                bool bad_op = false;
                int qsum = 0, msum = 0;
                for (int i = lane; i < n_cig; i += 64) {
                    const uint32_t c = brec::u32(cig + 4 * i), op = c & 15, ln = c >> 4;
                    bad_op |= !brec::in(op, OPS_MODEL);
                    if (brec::in(op, OPS_MODEL_QUERY)) qsum += (int)min(ln, 1u << 20);
                    if (op == OP_M) msum += (int)min(ln, 1u << 20);
                }
                for (int o = 32; o > 0; o >>= 1) { qsum += __shfl_xor(qsum, o); msum += __shfl_xor(msum, o); }
                if (__any(bad_op)) {
                    if (lane == 0) report(err, rec_base + r, E_REC_CIGAR_OP);
                    live = false;
                } else if (qsum != l_seq) {
                    if (lane == 0) report(err, rec_base + r, E_REC_CIGAR_LEN);
                    live = false;
                }
                m_total = msum;
            }
            if (live) {  // the MD:Z tag (lane 0 walks the optional fields)
                int found = 0, off = 0, len = 0;
                if (lane == 0) {
                    const uint8_t *const aux = rec + h.aux_at();
                    int64_t md_at = 0;
                    uint32_t n = 0;
                    const int st = brec::be_tag_walk(aux, (rec + h.end()) - aux, &md_at, &n);
                    found = st == brec::BE_TAGS_MD;
                    off = (int)((aux - p) + md_at);
                    len = (int)n;
                    if (!found) report(err, rec_base + r, st == brec::BE_TAGS_BAD ? E_REC_MALFORMED : E_REC_NO_MD);
                }
                found = __shfl(found, 0);
                md_off = __shfl(off, 0);
                md_len = __shfl(len, 0);
                if (!found) live = false;
            }
        }
        if (r < n_rec && lane == 0) meta[r] = my_meta;
        for (int i = lane; i < REFC_PITCH; i += 64) refc[i] = 0;
        __syncthreads();
        // ---- phase B: the aligned (M) query positions
        if (live) {
            int q = 0;
            for (int k = 0; k < n_cig; ++k) {
                const uint32_t c = brec::u32(cig + 4 * k), op = c & 15, ln = c >> 4;
                if (op == OP_M)
                    for (int i = lane; i < (int)ln; i += 64) refc[q + i] = 1;
                if (brec::in(op, OPS_MODEL_QUERY)) q += (int)ln;
            }
        }
        __syncthreads();
        // ---- phase C: the mismatches of the MD tag (lane 0), placed at their query positions
        if (live && lane == 0) {
            const uint8_t *md = p + md_off;
            int col = 0, ci = 0, q0 = 0, cb = 0;  // cursor: CIGAR op ci starts at query position q0 after cb aligned columns
            bool bad = false;
            for (int k = 0; k < md_len && !bad;) {
                const uint8_t ch = md[k];
                if (ch >= '0' && ch <= '9') {
                    int64_t v = 0;
                    while (k < md_len && md[k] >= '0' && md[k] <= '9' && v <= MAX_LEN) v = v * 10 + (md[k++] - '0');
                    col += (int)min(v, (int64_t)MAX_LEN + 1);
                    bad = col > m_total;
                } else if (ch == '^') {
                    ++k;
                    while (k < md_len && ((md[k] | 0x20) >= 'a' && (md[k] | 0x20) <= 'z')) ++k;
                } else {
                    int qpos = -1;
                    while (ci < n_cig) {
                        const uint32_t c = brec::u32(cig + 4 * ci), op = c & 15, ln = c >> 4;
                        if (op == OP_M) {
                            if (col < cb + (int)ln) { qpos = q0 + (col - cb); break; }
                            cb += (int)ln;
                            q0 += (int)ln;
                        } else if (op == OP_I || op == OP_S) {
                            q0 += (int)ln;
                        }
                        ++ci;
                    }
                    if (qpos < 0) { bad = true; break; }
                    refc[qpos] = (uint8_t)(0x80 | md_base(ch));
                    ++col;
                    ++k;
                }
            }
            if (bad || col != m_total) {
                report(err, rec_base + r, E_REC_BAD_MD);
                refc[REFC_PITCH - 1] = 0xFF;  // tells the wave
            }
        }
        __syncthreads();
        if (live && refc[REFC_PITCH - 1] == 0xFF) live = false;
        // ---- phase D: substitutions (dispatch_subst over get_aligned_pairs(matches_only=True, with_seq=True), iss/bam.py:155-162)
        bool has_indels = false;
        if (live) {
            bool odd = false;
            for (int q = lane; q < l_seq; q += 64) {
                const uint32_t c = refc[q];
                if (!c) continue;
                const int qb = nib_base(brec::seq_nibble(seq, 0u, (uint32_t)q));
                const int rb = c == 1 ? qb : (int)(c & 7);
                const bool ok = qb >= 0 && (c == 1 || (rb < 4 && rb != qb));
                if (!ok) { odd = true; continue; }
                if (mate >= 0) atomicAdd(&L.subst[(mate * MAX_LEN + q) * 16 + subst_col(rb, qb)], 1u);
            }
            has_indels = __any(odd);
        }
        // ---- phase E: dispatch_indels (iss/modeller.py:262-315) for a flagged read1 / read2, lane 0
        if (live && has_indels && mate >= 0 && lane == 0) {
            int lo = 0, hi = 0;  // query_alignment_start / end: soft clips behind any hard clip at either end
            for (int k = 0; k < n_cig; ++k) {
                const uint32_t c = brec::u32(cig + 4 * k), op = c & 15;
                if (op == OP_S) lo += (int)(c >> 4);
                else if (op != OP_H) break;
            }
            for (int k = n_cig - 1; k >= 0; --k) {
                const uint32_t c = brec::u32(cig + 4 * k), op = c & 15;
                if (op == OP_S) hi += (int)(c >> 4);
                else if (op != OP_H) break;
            }
            if (lo + hi > l_seq) hi = l_seq - lo;  // an all-clipped read: an empty alignment sequence
            const int la = l_seq - lo - hi;
            int64_t pos = 0;
            for (int k = 0; k < n_cig; ++k) {
                const uint32_t c = brec::u32(cig + 4 * k), op = c & 15, ln = c >> 4;
                if (op == OP_M) {
                    pos += ln;
                } else if (op == OP_I || op == OP_D) {
                    const int lim = op == OP_I ? l_seq : la;  // query_sequence[position] / query_alignment_sequence[position]
                    if (pos < -lim || pos >= lim) { report(err, rec_base + r, E_REC_INDEL_INDEX); break; }
                    const int qi = (op == OP_I ? 0 : lo) + (int)(pos < 0 ? pos + lim : pos);
                    const int b = nib_base(brec::seq_nibble(seq, 0u, (uint32_t)qi));
                    if (b >= 0) {
                        const int row = (int)(pos < 0 ? pos + MAX_LEN : pos);  // Python's negative index into the 301 rows
                        atomicAdd(&L.indel[(mate * MAX_LEN + row) * 9 + (op == OP_I ? 1 : 5) + b], 1u);
                    }
                    pos = op == OP_I ? pos + ln : pos - ln;
                }
            }
        }
        __syncthreads();
    }
    // ---- flush: once per workgroup
    for (int i = tid; i < 2 * MAX_LEN * 16; i += TALLY_THREADS)
        if (L.subst[i]) atomicAdd(&tally[OFF_SUBST + i], (unsigned long long)L.subst[i]);
    for (int i = tid; i < 2 * MAX_LEN * 9; i += TALLY_THREADS)
        if (L.indel[i]) atomicAdd(&tally[OFF_INDEL + i], (unsigned long long)L.indel[i]);
    for (int i = tid; i < NTLEN; i += TALLY_THREADS)
        if (L.tlen[i]) atomicAdd(&tally[OFF_TLEN + i], (unsigned long long)L.tlen[i]);
    if (tid < N_SLICE && L.nread[tid]) {
        atomicAdd(&tally[OFF_NREAD + tid], (unsigned long long)L.nread[tid]);
        atomicMin(&tally[OFF_MINLEN + tid], (unsigned long long)L.minlen[tid]);
    }
    if (tid == 0 && L.taken[0]) atomicAdd(&tally[OFF_TAKEN], (unsigned long long)L.taken[0]);
}

// Quality histograms per (mate, bin, position): blockIdx.y is the slice, its [301][94] u32 table fills the workgroup's LDS.
__global__ void __launch_bounds__(TALLY_THREADS) k_bam_qhist(const uint8_t *__restrict__ data, const uint2 *__restrict__ meta, int64_t n_rec,
                                                             unsigned long long *__restrict__ tally) {
    extern __shared__ __align__(16) uint8_t lds_raw[];
    uint32_t *h = reinterpret_cast<uint32_t *>(lds_raw);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t slice = blockIdx.y;
    for (int i = tid; i < MAX_LEN * NQ; i += TALLY_THREADS) h[i] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * TALLY_WAVES;
    for (int64_t r = (int64_t)blockIdx.x * TALLY_WAVES + w; r < n_rec; r += stride) {
        const uint2 m = meta[r];
        if ((m.y & 0xFF) != slice) continue;
        const int len = (int)(m.y >> 16);
        const bool rev = (m.y >> 8) & 1;
        const uint8_t *q = data + m.x;
        for (int i = lane; i < len; i += 64) atomicAdd(&h[i * NQ + q[rev ? len - 1 - i : i]], 1u);  // read_quality[::-1] if is_reverse
    }
    __syncthreads();
    unsigned long long *g = tally + OFF_QHIST + (size_t)slice * MAX_LEN * NQ;
    for (int i = tid; i < MAX_LEN * NQ; i += TALLY_THREADS)
        if (h[i]) atomicAdd(&g[i], (unsigned long long)h[i]);
}

// scipy 1.15 gaussian_kde(q, bw_method=0.2 / np.std(q, ddof=1)).evaluate(grid) for data given as (value, count): the weighted np.cov
// (aweights 1/n, ddof 1) times factor**2, its Cholesky root s, points and data multiplied by 1/s, exp(-r**2/2) * norm summed over the
// distinct values in ascending order.  No contraction: every product and sum rounds like numpy's.
struct KdeFit {
    double s, inv, w, norm;
};
template <class Count>
__device__ KdeFit kde_fit(Count count, int n_val, int64_t x0) {
#pragma clang fp contract(off)
    double n = 0, sx = 0;
    for (int v = 0; v < n_val; ++v) {
        const double c = (double)count(v);
        n += c;
        sx += c * (double)(x0 + v);
    }
    const double mean = sx / n;
    double ss = 0;
    for (int v = 0; v < n_val; ++v) {
        const double c = (double)count(v);
        if (c != 0) { const double d = (double)(x0 + v) - mean; ss += c * (d * d); }
    }
    const double std1 = sqrt(ss / (n - 1.0));
    const double factor = 0.2 / std1;
    const double w = 1.0 / n, wsum = n * w;
    const double avg = (sx * w) / wsum;
    const double fact = wsum - (n * (w * w)) / wsum;
    double cs = 0;
    for (int v = 0; v < n_val; ++v) {
        const double c = (double)count(v);
        if (c != 0) { const double d = (double)(x0 + v) - avg; cs += c * ((d * w) * d); }
    }
    const double cov = cs / fact;
    KdeFit f;
    f.s = sqrt(cov) * factor;
    f.inv = 1.0 / f.s;  // the triangular solve by the 1x1 Cholesky factor: a multiplication by its inverse
    f.w = w;
    f.norm = 0.3989422804014327 / f.s;  // (2 pi)**-0.5 / s
    return f;
}
template <class Count>
__device__ double kde_at(Count count, int n_val, int64_t x0, const KdeFit &f, double y) {
#pragma clang fp contract(off)
    const double ys = y * f.inv;
    double est = 0;
    for (int v = 0; v < n_val; ++v) {
        const double c = (double)count(v);
        if (c == 0) continue;
        const double r = (double)(x0 + v) * f.inv - ys;
        const double arg = exp(-(r * r) / 2.0) * f.norm;
        est += c * (f.w * arg);
    }
    return est;
}

constexpr int KDE_THREADS = 256;
constexpr int KDE_Q_POINTS = 41;  // kde.evaluate(range(41)), iss/modeller.py:129
// blocks [0, n_q_blocks): one thread per (slice, position): the 41-point CDF of raw_qualities_to_histogram (iss/modeller.py:99-134)
// -- rows of slices with fewer than two reads and positions at or past the slice's shortest read are NaN; the last block, when
// with_isize: the insert-size CDF (iss/modeller.py:12-38) on its 2000-point linspace grid.
__global__ void __launch_bounds__(KDE_THREADS) k_kde_cdf(const unsigned long long *__restrict__ tally, double *__restrict__ qcdf,
                                                         double *__restrict__ isize_cdf, int read_length, int n_q_blocks) {
#pragma clang fp contract(off)
    __shared__ double est[NTLEN];
    if ((int)blockIdx.x < n_q_blocks) {
        const int t = blockIdx.x * KDE_THREADS + threadIdx.x;
        if (t >= N_SLICE * MAX_LEN) return;
        const int slice = t / MAX_LEN, pos = t % MAX_LEN;
        double *out = qcdf + (size_t)t * KDE_Q_POINTS;
        const unsigned long long nr = tally[OFF_NREAD + slice], ml = tally[OFF_MINLEN + slice];
        if (nr < 2 || (unsigned long long)pos >= ml) {
            for (int j = 0; j < KDE_Q_POINTS; ++j) out[j] = __longlong_as_double(0x7FF8000000000000ll);
            return;
        }
        const unsigned long long *h = tally + OFF_QHIST + ((size_t)slice * MAX_LEN + pos) * NQ;
        int first = -1, last = -1;
        for (int v = 0; v < NQ; ++v)
            if (h[v]) { if (first < 0) first = v; last = v; }
        // np.std(q) == 0: the reference's LinAlgError branch adds 1 to the last value -- one count moves from v to v + 1
        const bool moved = first == last;
        auto count = [&](int v) -> unsigned long long {
            unsigned long long c = v < NQ ? h[v] : 0;
            if (moved && v == first) c -= 1;
            if (moved && v == first + 1) c += 1;
            return c;
        };
        const int n_val = NQ + 1;
        const KdeFit f = kde_fit(count, n_val, 0);
        double cum = 0;
        for (int j = 0; j < KDE_Q_POINTS; ++j) {
            cum += kde_at(count, n_val, 0, f, (double)j);
            out[j] = cum;
        }
        const double tot = out[KDE_Q_POINTS - 1];
        for (int j = 0; j < KDE_Q_POINTS; ++j) out[j] = out[j] / tot;
        return;
    }
    // insert sizes: isd = tlen - 2 * read_length over the template-length histogram (the host checked n >= 2 and a non-zero spread)
    const unsigned long long *h = tally + OFF_TLEN;
    auto count = [&](int v) -> unsigned long long { return h[v]; };
    const int64_t x0 = -2 * (int64_t)read_length;
    int lo = NTLEN, hi = -1;
    for (int v = 1; v < NTLEN; ++v)
        if (h[v]) { lo = min(lo, v); hi = v; }
    const KdeFit f = kde_fit(count, NTLEN, x0);
    const double start = (double)(x0 + lo), stop = (double)(x0 + hi);
    const double step = (stop - start) / (double)(NTLEN - 1);  // np.linspace(min(isd), max(isd), 2000)
    for (int j = threadIdx.x; j < NTLEN; j += KDE_THREADS) {
        const double y = j == NTLEN - 1 ? stop : (double)j * step + start;
        est[j] = kde_at(count, NTLEN, x0, f, y);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double cum = 0;
        for (int j = 0; j < NTLEN; ++j) { cum += est[j]; est[j] = cum; }
        for (int j = 0; j < NTLEN; ++j) isize_cdf[j] = est[j] / cum;
    }
}

}  // namespace bam
}  // namespace iss
