// iss_fqtally.hip.h -- k_fq_*: the tallies of iss_tally.hip.h over FASTQ TEXT instead of output rows (iss_fq_feed): what a read set
// from a sequencer, or a file this project wrote last week, looks like -- to put beside `generate --report`'s tally of a run.
// Input: a chunk of FASTQ text in device memory that holds whole four-line records ('\n' ends a line, one '\r' directly before it
// belongs to the terminator).  One flat u64 array of the context, added to (include/iss_mi355x.h has the layout), for L = max_len:
//   pairs [1] | qual [2][L][94] | base [2][L][5] | gc [2][L + 1] | meanq [2][94] | insert [2048] | length [2][L + 1]
// -- iss_tally.hip.h's layout and one field behind it; `insert` stays zero (a FASTQ file does not say it).  One feed is one mate.
//   a  k_fq_count       '\n' bytes of every FQ_TILE bytes
//      k_fq_head        exclusive scan of the tile counts (one workgroup); the feed's head: lines, the index of its first record
//                       over all feeds of the mate, the TRUNCATED check
//      k_fq_lines       byte offset of every line start (u32: a chunk is below 2^31 bytes)
//   b  k_fq_records     record r = lines 4r .. 4r + 3 (by line number, never by looking for '@': a quality line may start with it):
//                       validated, the first bad one over all feeds kept by an atomic minimum; the per-read fields (gc, meanq,
//                       length, pairs); every record's length, or FQ_BAD, for stage c
//   c  k_fq_positions   the per-position fields (qual, base) of the good records, one tile of 64 positions per workgroup
// Every count is an exact integer sum: the words depend neither on the launch geometry nor on the order of arrival.  Counts are
// gathered in LDS (u32) and added to the u64 words once per workgroup, one global atomic per non-zero counter (iss_tally.hip.h).
// Plain vector code.  DESIGN.md section 24.  Included by iss_mi355x.hip.
#pragma once

namespace iss {
namespace fq {

constexpr int FQ_THREADS = 256;
constexpr int FQ_TILE = FQ_THREADS * 16;  // bytes of a newline tile: one uint4 per lane
constexpr int FQ_HEAD_PER = 8;            // tile counts per lane and pass of k_fq_head
constexpr int FQ_MAX_LEN = 1024;          // (= ISS_FQ_MAX_LEN)
constexpr int FQ_GROUP = 16;              // lanes of a record in k_fq_records: 4 bytes a lane, 64 bytes a step
constexpr int FQ_POS_TILE = 64;           // positions of a workgroup's tables in k_fq_positions: a wave's lanes
static_assert(FQ_THREADS == TALLY_THREADS && FQ_POS_TILE == TALLY_TILE, "k_fq_positions uses iss_tally.hip.h's phred tile");
constexpr int FQ_TARGET_WGS = 2048;       // workgroups of a launch, about: 8 per compute unit
constexpr uint32_t FQ_BAD = 0xFFFFFFFFu;  // rec_len of a record that is not tallied

constexpr int FQ_REC_NO_AT = 1, FQ_REC_NO_PLUS = 2, FQ_REC_LENGTHS = 3, FQ_REC_TOO_LONG = 4, FQ_REC_QUAL_RANGE = 5, FQ_REC_TRUNCATED = 6;

struct FqLayout {  // word offsets of the fields for max_len L: tally_layout(L) and the length field behind it
    TallyLayout t;
    int64_t length, words;
};
__host__ __device__ inline FqLayout fq_layout(int L) {
    FqLayout f;
    f.t = tally_layout(L);
    f.length = f.t.words;
    f.words = f.length + 2 * ((int64_t)L + 1);
    return f;
}

struct FqHead {  // of the feed in flight (k_fq_head writes it)
    uint32_t n_lines;     // '\n' bytes of the chunk
    uint32_t longest;     // longest good read of the chunk (k_fq_records: atomic maximum)
    uint64_t first_rec;   // index of the chunk's record 0 over all records fed for the mate
};

struct FqState {  // of the context, behind the tally words
    unsigned long long records[2];  // whole records fed per mate
    unsigned long long bad[2];      // ((record << 8) | code) of the first bad record per mate, the smallest wins; ~0: none
};

struct FqArgs {
    const uint8_t *text;  // the chunk, 16-byte aligned; readable up to the next multiple of FQ_TILE and 16 bytes beyond
    uint32_t n_bytes;     // 1 .. 2^31 - 1
    uint32_t n_tiles;     // ceil(n_bytes / FQ_TILE)
    uint32_t *tile_cnt;   // [n_tiles]: '\n' count of the tile, then (k_fq_head) of the tiles before it
    uint32_t *line_start; // [n_bytes + 1]: line k starts at line_start[k]; line_start[n_lines] = one past the last '\n'
    uint32_t *rec_len;    // [n_bytes / 4]: the record's read length or FQ_BAD
    FqHead *head;
    FqState *state;
    unsigned long long *tally;
    int32_t mate, L;      // L: the context's max_len
};

// bit j: byte j of the lane's 16 is '\n'; bytes at or past the chunk's end are no bytes
__device__ __forceinline__ uint32_t fq_newlines(const FqArgs &A, uint32_t at) {
    if (at >= A.n_bytes) return 0u;
    const uint4 v = *reinterpret_cast<const uint4 *>(A.text + at);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t t = w[k] ^ 0x0A0A0A0Au;  // a '\n' -> a zero byte
        const uint32_t z = ~((((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t)) & 0x80808080u;
        m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * k);
    }
    const uint32_t nv = A.n_bytes - at;
    return nv >= 16u ? m : m & ((1u << nv) - 1u);
}

// exclusive scan over the workgroup's FQ_THREADS values; *total: their sum.  `sh`: FQ_THREADS words of LDS (vcf_block_scan's shape)
__device__ __forceinline__ uint32_t fq_block_scan(uint32_t v, uint32_t *sh, uint32_t *total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < FQ_THREADS; d <<= 1) {
        const uint32_t x = t >= d ? sh[t - d] : 0u;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const uint32_t incl = sh[t];
    *total = sh[FQ_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// grid = n_tiles
__global__ __launch_bounds__(FQ_THREADS) void k_fq_count(const FqArgs A) {
    __shared__ uint32_t sh[FQ_THREADS];
    uint32_t total;
    (void)fq_block_scan((uint32_t)__popc(fq_newlines(A, blockIdx.x * (uint32_t)FQ_TILE + threadIdx.x * 16u)), sh, &total);
    if (threadIdx.x == 0) A.tile_cnt[blockIdx.x] = total;
}

// one workgroup: tile_cnt[b] -> '\n' bytes of the tiles before b; the feed's head; the chunk-level check
__global__ __launch_bounds__(FQ_THREADS) void k_fq_head(const FqArgs A) {
    __shared__ uint32_t sh[FQ_THREADS];
    uint32_t carry = 0u;
    for (uint32_t base = 0; base < A.n_tiles; base += FQ_THREADS * FQ_HEAD_PER) {
        const uint32_t at = base + threadIdx.x * FQ_HEAD_PER;
        uint32_t v[FQ_HEAD_PER], s = 0u;
        for (int k = 0; k < FQ_HEAD_PER; ++k) {
            v[k] = at + k < A.n_tiles ? A.tile_cnt[at + k] : 0u;
            s += v[k];
        }
        uint32_t total;
        uint32_t run = carry + fq_block_scan(s, sh, &total);
        for (int k = 0; k < FQ_HEAD_PER; ++k) {
            if (at + k < A.n_tiles) A.tile_cnt[at + k] = run;
            run += v[k];
        }
        carry += total;
    }
    if (threadIdx.x == 0) {
        const unsigned long long first = A.state->records[A.mate], n_rec = carry >> 2;
        A.head->n_lines = carry;
        A.head->longest = 0u;
        A.head->first_rec = first;
        A.state->records[A.mate] = first + n_rec;
        A.line_start[0] = 0u;
        // lines beyond the last whole record, or bytes beyond the last '\n': a record that is not all there
        if ((carry & 3u) || A.text[A.n_bytes - 1u] != (uint8_t)'\n')
            atomicMin(&A.state->bad[A.mate], ((first + n_rec) << 8) | (unsigned long long)FQ_REC_TRUNCATED);
    }
}

// grid = n_tiles: the '\n' number k of the chunk, at byte p, makes line_start[k + 1] = p + 1
__global__ __launch_bounds__(FQ_THREADS) void k_fq_lines(const FqArgs A) {
    __shared__ uint32_t sh[FQ_THREADS];
    const uint32_t at = blockIdx.x * (uint32_t)FQ_TILE + threadIdx.x * 16u;
    uint32_t m = fq_newlines(A, at), total;
    uint32_t k = A.tile_cnt[blockIdx.x] + fq_block_scan((uint32_t)__popc(m), sh, &total);
    while (m) {
        const uint32_t j = (uint32_t)__ffs((int)m) - 1u;
        if (k < A.n_bytes) A.line_start[k + 1u] = at + j + 1u;  // (always: a chunk has n_bytes '\n' bytes at most)
        ++k;
        m &= m - 1u;
    }
}

// the line [s, e) without its terminator, for line_start s and next line_start nx ('\n' at nx - 1, one '\r' before it dropped)
__device__ __forceinline__ uint32_t fq_line_end(const uint8_t *text, uint32_t s, uint32_t nx) {
    uint32_t e = nx - 1u;
    if (e > s && text[e - 1u] == (uint8_t)'\r') --e;
    return e;
}

inline size_t fq_records_lds(int L) { return sizeof(uint32_t) * (size_t)(2 * (L + 1) + TALLY_NQ + 2); }

// Stage b.  FQ_GROUP lanes a record, 16 records a workgroup and pass, record r of pass i = (i * gridDim.x + blockIdx.x) * 16 + group.
// The lanes of a group read the two lines 4 bytes each, 64 bytes a step (unaligned: a line starts anywhere; bytes past the line's
// end, three at most, are read -- the buffer reaches 16 bytes past its last tile -- and not counted), and sum over the group by shuffles.
__global__ __launch_bounds__(FQ_THREADS) void k_fq_records(const FqArgs A) {
    extern __shared__ uint32_t fq_records_lds_[];
    const uint32_t tid = threadIdx.x, L = (uint32_t)A.L;
    uint32_t *const s_len = fq_records_lds_, *const s_gc = s_len + (L + 1u), *const s_mq = s_gc + (L + 1u), *const s_misc = s_mq + TALLY_NQ;
    const uint32_t n_lds = 2u * (L + 1u) + TALLY_NQ + 2u;  // s_misc: good records, longest good read
    for (uint32_t i = tid; i < n_lds; i += FQ_THREADS) s_len[i] = 0u;
    __syncthreads();
    const uint32_t lane = tid & (FQ_GROUP - 1), per_pass = FQ_THREADS / FQ_GROUP;
    const uint32_t n_rec = A.head->n_lines >> 2;
    const uint64_t first_rec = A.head->first_rec;
    const uint8_t *const text = A.text;
    // (the trip count is the same for all lanes of a group, and the shuffles stay inside it)
    for (uint64_t r64 = (uint64_t)blockIdx.x * per_pass + (tid / FQ_GROUP); r64 < n_rec; r64 += (uint64_t)gridDim.x * per_pass) {
        const uint32_t r = (uint32_t)r64;
        const uint32_t s0 = A.line_start[4u * r], s1 = A.line_start[4u * r + 1u], s2 = A.line_start[4u * r + 2u],
                       s3 = A.line_start[4u * r + 3u], s4 = A.line_start[4u * r + 4u];
        const uint32_t e0 = fq_line_end(text, s0, s1), e1 = fq_line_end(text, s1, s2), e2 = fq_line_end(text, s2, s3),
                       e3 = fq_line_end(text, s3, s4);
        const uint32_t len = e1 - s1;
        uint32_t code = 0u;
        if (e0 == s0 || text[s0] != (uint8_t)'@') code = FQ_REC_NO_AT;
        else if (e2 == s2 || text[s2] != (uint8_t)'+') code = FQ_REC_NO_PLUS;
        else if (e3 - s3 != len) code = FQ_REC_LENGTHS;
        else if (len > L) code = FQ_REC_TOO_LONG;
        uint32_t gc = 0u, qs = 0u, out_of_range = 0u;
        if (!code) {
            for (uint32_t at = lane * 4u; at < len; at += FQ_GROUP * 4u) {
                uint32_t bw, qw;
                __builtin_memcpy(&bw, text + s1 + at, 4);
                __builtin_memcpy(&qw, text + s3 + at, 4);
                const uint32_t nv = min(4u, len - at);
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j) {
                    if (j < nv) {
                        const uint32_t b = (bw >> (8u * j)) & 0xFFu, q = (qw >> (8u * j)) & 0xFFu;
                        gc += ((b & 0xDBu) == 0x43u) ? 1u : 0u;  // 'C' 0x43, 'G' 0x47, 'c' 0x63, 'g' 0x67 (k_tally_reads' test)
                        out_of_range |= (q < 33u || q > 126u) ? 1u : 0u;
                        qs += q - 33u;
                    }
                }
            }
#pragma unroll
            for (int d = 1; d < FQ_GROUP; d <<= 1) {
                gc += __shfl_xor(gc, d);
                qs += __shfl_xor(qs, d);
                out_of_range |= __shfl_xor(out_of_range, d);
            }
            if (out_of_range) code = FQ_REC_QUAL_RANGE;
        }
        if (lane == 0u) {
            A.rec_len[r] = code ? FQ_BAD : len;
            if (code) {
                atomicMin(&A.state->bad[A.mate], ((first_rec + r) << 8) | (unsigned long long)code);
            } else {
                atomicAdd(&s_len[len], 1u);
                atomicAdd(&s_gc[gc], 1u);
                if (len) atomicAdd(&s_mq[min(qs / len, (uint32_t)TALLY_NQ - 1u)], 1u);  // (a read of length 0 has no mean)
                atomicAdd(&s_misc[0], 1u);
                atomicMax(&s_misc[1], len);
            }
        }
    }
    __syncthreads();
    const FqLayout lay = fq_layout((int)L);
    const int64_t m = A.mate;
    for (uint32_t i = tid; i < L + 1u; i += FQ_THREADS) {
        if (s_len[i]) atomicAdd(&A.tally[lay.length + m * (L + 1) + i], (unsigned long long)s_len[i]);
        if (s_gc[i]) atomicAdd(&A.tally[lay.t.gc + m * (L + 1) + i], (unsigned long long)s_gc[i]);
    }
    for (uint32_t i = tid; i < (uint32_t)TALLY_NQ; i += FQ_THREADS)
        if (s_mq[i]) atomicAdd(&A.tally[lay.t.meanq + m * TALLY_NQ + i], (unsigned long long)s_mq[i]);
    if (tid == 0u && s_misc[0]) {
        if (A.mate == 0) atomicAdd(&A.tally[0], (unsigned long long)s_misc[0]);
        atomicMax(&A.head->longest, s_misc[1]);
    }
}

// Stage c.  Workgroup (t, c): positions [64 t, 64 t + 64) of the records c * 4 + wave, then every gridDim.y * 4 further; its tables
// are those of one tile, 64 positions x (94 phreds + 5 base codes) -- at max_len 1024 the whole table does not fit a workgroup's
// LDS (k_tally_lines tiles its rows likewise).  A wave takes a record, a lane a position: the 64 lanes of a wave instruction stand
// at 64 different positions, hence -- the pitch is odd -- at 64 different LDS words of different banks at equal phreds.
// A tile past the chunk's longest read has nothing to count and leaves at once.
__global__ __launch_bounds__(FQ_THREADS) void k_fq_positions(const FqArgs A) {
    __shared__ uint32_t s_qual[FQ_POS_TILE * TALLY_QPITCH];
    __shared__ uint32_t s_base[FQ_POS_TILE * 5];
    const uint32_t tid = threadIdx.x, pos0 = blockIdx.x * (uint32_t)FQ_POS_TILE;
    if (pos0 >= A.head->longest) return;  // (the same word for every lane of the workgroup: nobody waits at a barrier below)
    tile_qual_zero<1>(s_qual, tid);
    for (uint32_t i = tid; i < (uint32_t)FQ_POS_TILE * 5u; i += FQ_THREADS) s_base[i] = 0u;
    __syncthreads();
    const uint32_t lane = tid & 63u, waves = FQ_THREADS / 64, L = (uint32_t)A.L;
    const uint32_t n_rec = A.head->n_lines >> 2;
    const uint32_t pos = pos0 + lane;
    for (uint64_t r64 = (uint64_t)blockIdx.y * waves + (tid >> 6); r64 < n_rec; r64 += (uint64_t)gridDim.y * waves) {
        const uint32_t r = (uint32_t)r64, len = A.rec_len[r];
        if (len == FQ_BAD || pos >= len) continue;  // (len <= L)
        const uint32_t b = A.text[A.line_start[4u * r + 1u] + pos], q = A.text[A.line_start[4u * r + 3u] + pos];
        atomicAdd(&s_qual[lane * TALLY_QPITCH + (q - 33u)], 1u);  // (k_fq_records saw 33 <= q <= 126)
        atomicAdd(&s_base[lane * 5u + export_code(b)], 1u);
    }
    __syncthreads();
    const FqLayout lay = fq_layout((int)L);
    const int64_t m = A.mate;
    tile_qual_flush<1>(s_qual, tid, pos0, L, A.tally + lay.t.qual + m * L * TALLY_NQ);
    tile_base_flush<1>(s_base, tid, pos0, L, A.tally + lay.t.base + m * L * 5);
}

// The launch geometry of stages b and c (host): wgs workgroups aimed at (0: FQ_TARGET_WGS) by k_fq_records and by every tile
// column of k_fq_positions, no more than the text can keep busy.
struct FqPlan {
    uint32_t n_tiles, rec_wgs, pos_tiles, pos_chunks;
};
inline FqPlan fq_plan(int64_t n_bytes, int L, int wgs) {
    const int64_t target = wgs > 0 ? wgs : FQ_TARGET_WGS;
    FqPlan p;
    p.n_tiles = (uint32_t)((n_bytes + FQ_TILE - 1) / FQ_TILE);
    p.rec_wgs = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(target, p.n_tiles));  // (a tile holds about a pass of records)
    p.pos_tiles = (uint32_t)((L + FQ_POS_TILE - 1) / FQ_POS_TILE);
    // (per tile column, not in all: the host does not know the longest read, and the columns beyond it -- 13 of 16 for 151-base
    //  reads at max_len 1024 -- leave at their first instruction)
    p.pos_chunks = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(target, p.n_tiles), 65535));
    return p;
}

}  // namespace fq
}  // namespace iss
