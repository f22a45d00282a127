// iss_api_fasta.hip.h -- C ABI of `generate --device_fasta` (kernels: iss_fasta.hip.h, grammar: iss_fasta_core.h):
// iss_fa_* -- a session (iss_host_session.hip.h, no model) that indexes a FASTA text on the device: records, header and body ranges,
// letters, flags --, iss_fasta_host_index -- the same table from the core header on the host, no GPU --, and iss_genome_upload_fasta --
// the bodies of a span of the file as it stands, their line ends removed on the device, in front of k_pack_group / k_pack_genome.
#pragma once

struct iss_fa : iss_session {
    Stream stream;
    Grown<DevMem<uint8_t>> text;             // the text, readable up to the next multiple of the tile
    Grown<DevMem<unsigned long long>> pre;   // FaText::pre
    Grown<DevMem<int64_t>> rows;             // FaRows: five int64 arrays, then the flags
};

static_assert(iss::fa::FA_ODD == ISS_FA_ODD, "include/iss_mi355x.h: ISS_FA_ODD");

namespace {

const char *const FA_TABLE_RULES[] = {"", "a body outside the span", "bodies out of order or overlapping", "more letters than the body has bytes"};

size_t fa_text_bytes(int64_t n_bytes) { return (size_t)((n_bytes + iss::fa::FA_TILE - 1) / iss::fa::FA_TILE) * iss::fa::FA_TILE + 16; }

// a and b of iss_fasta.hip.h over a text that stands on the device
hipError_t fa_prefix_launch(const iss::fa::FaText &A, hipStream_t st) {
    hipLaunchKernelGGL(iss::fa::k_fa_count, dim3((unsigned)A.n_tiles), dim3(iss::fa::FA_THREADS), 0, st, A);
    hipLaunchKernelGGL(iss::fa::k_fa_scan, dim3(1), dim3(iss::fa::FA_THREADS), 0, st, A);
    return hipGetLastError();
}

}  // namespace

extern "C" {

int iss_fasta_tile(void) { return iss::fa::FA_TILE; }
int iss_fasta_scan_span(void) { return iss::fa::FA_SCAN_SPAN; }

int iss_fasta_host_index(const uint8_t *text, int64_t n_bytes, int64_t capacity, int64_t *header_off, int64_t *header_len, int64_t *body_off,
                         int64_t *body_len, int64_t *letters, int32_t *flags, int64_t *n_records) {
    if (n_bytes < 0 || capacity < 0 || !n_records || (n_bytes && !text) ||
        (capacity && (!header_off || !header_len || !body_off || !body_len || !letters || !flags)))
        return fail(nullptr, ISS_E_INVALID, "iss_fasta_host_index: bad argument");
    using namespace iss::fa;
    int64_t n = 0;
    uint32_t prev = 0x0Au;
    for (int64_t i = 0; i < n_bytes; ++i) {
        n += fa_is_header(prev, text[i]) ? 1 : 0;
        prev = text[i];
    }
    *n_records = n;
    if (capacity < n || !n) return 0;
    int64_t r = -1, eol = -1, n_eol = 0;  // the open record; its header's '\n' (-1: not seen yet); line-end bytes of its body so far
    int32_t odd = 0;
    auto close = [&](int64_t end) {
        fa_row(header_off[r], eol < 0 ? end : eol, end, &header_len[r], &body_off[r], &body_len[r]);
        letters[r] = body_len[r] - n_eol;
        flags[r] = odd;
    };
    prev = 0x0Au;
    for (int64_t i = 0; i < n_bytes; ++i) {
        const uint32_t c = text[i];
        if (fa_is_header(prev, c)) {
            if (r >= 0) close(i);
            header_off[++r] = i;
            eol = -1, n_eol = 0, odd = 0;
        } else if (r >= 0 && eol < 0) {
            if (c == 0x0Au) eol = i;
        } else if (r >= 0) {
            n_eol += fa_is_eol(c) ? 1 : 0;
            odd |= fa_is_odd(c) ? FA_ODD : 0;
        }
        prev = c;
    }
    close(n_bytes);
    return 0;
}

int iss_fa_create(int device_ordinal, iss_fa **out) {
    if (!out) return fail(nullptr, ISS_E_INVALID, "iss_fa_create: out is NULL");
    *out = nullptr;
    ISS_TRY(session_open(device_ordinal, out));
    return stream_create(*out, (*out)->stream, hipStreamNonBlocking);
}

void iss_fa_destroy(iss_fa *fa) {
    if (!fa) return;
    session_close(fa, {fa->stream});
    delete fa;
}

const char *iss_fa_last_error(const iss_fa *fa) { return session_last_error(fa); }

int iss_fa_index(iss_fa *fa, const uint8_t *text, int64_t n_bytes, int64_t capacity, int64_t *header_off, int64_t *header_len,
                 int64_t *body_off, int64_t *body_len, int64_t *letters, int32_t *flags, int64_t *n_records) {
    if (!fa || n_bytes < 0 || capacity < 0 || !n_records || (n_bytes && !text) ||
        (capacity && (!header_off || !header_len || !body_off || !body_len || !letters || !flags)))
        return fail(fa, ISS_E_INVALID, "iss_fa_index: bad argument");
    *n_records = 0;
    if (!n_bytes) return 0;
    using namespace iss::fa;
    HIP_TRY(fa, hipSetDevice(fa->device));
    FaText A{};
    A.n_bytes = n_bytes;
    A.n_tiles = (n_bytes + FA_TILE - 1) / FA_TILE;
    if (A.n_tiles > 0x7FFFFFFFll) return fail(fa, ISS_E_INVALID, "iss_fa_index: a text holds less than 2^43 bytes");
    ISS_TRY(reserve(fa, fa->text, fa_text_bytes(n_bytes), (size_t)1 << 20, "the text"));
    ISS_TRY(reserve(fa, fa->pre, 3 * ((size_t)A.n_tiles + 1), (size_t)1 << 12, "the tile prefixes"));
    A.text = fa->text.p;
    A.pre = fa->pre.p;
    HIP_TRY(fa, hipMemcpyAsync(fa->text.p, text, (size_t)n_bytes, hipMemcpyHostToDevice, fa->stream));
    HIP_TRY(fa, fa_prefix_launch(A, fa->stream));
    unsigned long long total = 0;
    HIP_TRY(fa, hipMemcpyAsync(&total, fa->pre.p + A.n_tiles, sizeof total, hipMemcpyDeviceToHost, fa->stream));
    HIP_TRY(fa, hipStreamSynchronize(fa->stream));
    const int64_t n = (int64_t)total;
    *n_records = n;
    if (capacity < n || !n) return 0;  // (the count alone: the caller comes again with room for it)
    ISS_TRY(reserve(fa, fa->rows, 6 * (size_t)n, (size_t)1 << 12, "the rows"));
    FaRows R{};
    R.n_rec = n;
    R.header_off = fa->rows.p;
    R.header_len = R.header_off + n;
    R.body_off = R.header_len + n;
    R.body_len = R.body_off + n;
    R.letters = R.body_len + n;
    R.flags = reinterpret_cast<int32_t *>(R.letters + n);
    hipLaunchKernelGGL(k_fa_heads, dim3((unsigned)A.n_tiles), dim3(FA_THREADS), 0, fa->stream, A, R);
    hipLaunchKernelGGL(k_fa_rows, dim3((unsigned)((n + FA_THREADS - 1) / FA_THREADS)), dim3(FA_THREADS), 0, fa->stream, A, R);
    HIP_TRY(fa, hipGetLastError());
    int64_t *const host[5] = {header_off, header_len, body_off, body_len, letters};
    for (int k = 0; k < 5; ++k)
        HIP_TRY(fa, hipMemcpyAsync(host[k], fa->rows.p + (size_t)k * (size_t)n, (size_t)n * 8, hipMemcpyDeviceToHost, fa->stream));
    HIP_TRY(fa, hipMemcpyAsync(flags, R.flags, (size_t)n * 4, hipMemcpyDeviceToHost, fa->stream));
    HIP_TRY(fa, hipStreamSynchronize(fa->stream));
    return 0;
}

int iss_genome_upload_fasta(iss_ctx *ctx, const uint8_t *text, int64_t n_bytes, int32_t n, const int64_t *body_off, const int64_t *body_len,
                            const int64_t *letters, int32_t *genome_ids) {
    if (!ctx || n < 0 || n_bytes < 0 || (n_bytes && !text) || (n && (!body_off || !body_len || !letters || !genome_ids)))
        return fail(ctx, ISS_E_INVALID, "iss_genome_upload_fasta: bad argument");
    using namespace iss::fa;
    for (int32_t k = 0; k < n; ++k) genome_ids[k] = -1;
    // the table first: one that fails launches nothing
    int rule = 0;
    const int64_t bad_row = fa_table_check(n_bytes, n, body_off, body_len, letters, &rule);
    if (bad_row >= 0)
        return fail(ctx, ISS_E_INVALID, "iss_genome_upload_fasta: row " + std::to_string(bad_row) + ": " + FA_TABLE_RULES[rule]);
    bool large = false;
    for (int32_t k = 0; k < n; ++k) large |= letters[k] > SMALL_RECORD && letters[k] <= iss::MAX_RECORD;
    if (large && n != 1)
        return fail(ctx, ISS_E_INVALID, "iss_genome_upload_fasta: a record of more than " + std::to_string(SMALL_RECORD) + " letters comes alone");
    GroupPlan P;
    if (large) {  // (alone, in memory of its own: no arena)
        P.which.push_back(0);
        P.starts.push_back(0);
    } else {
        ISS_TRY(group_plan(ctx, "iss_genome_upload_fasta", n, letters, nullptr, P));
    }
    const int32_t m = (int32_t)P.which.size();
    if (!m) return 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    FaText A{};
    A.n_bytes = n_bytes;  // (>= 1: a placed record has a letter)
    A.n_tiles = (n_bytes + FA_TILE - 1) / FA_TILE;
    if (A.n_tiles > 0x7FFFFFFFll) return fail(ctx, ISS_E_INVALID, "iss_genome_upload_fasta: a span holds less than 2^43 bytes");
    // what the call needs beside the records' own memory, freed when it returns: the span, its tile prefixes, the table
    DevMem<uint8_t> d_text;
    DevMem<unsigned long long> d_pre;
    DevMem<int64_t> d_tab;  // body_off | body_len | letters | dest | e0 of the placed records, then the bad-letter counter
    DEV_ALLOC(ctx, d_text, fa_text_bytes(n_bytes));
    DEV_ALLOC(ctx, d_pre, 3 * ((size_t)A.n_tiles + 1));
    DEV_ALLOC(ctx, d_tab, 5 * (size_t)m + 1);
    A.text = d_text;
    A.pre = d_pre;
    // (pinned: the table's four arrays, then the counter on its way back, then the group's start coordinates and status rows)
    const size_t tab_b = ((size_t)m * 32 + 8 + 255) & ~(size_t)255;
    ISS_TRY(group_stage_reserve(ctx, tab_b + P.st_b + P.stat_b));
    int64_t *h_tab = reinterpret_cast<int64_t *>(ctx->group_stage.h.get());
    unsigned long long *h_bad = reinterpret_cast<unsigned long long *>(h_tab + 4 * (size_t)m);
    for (int32_t i = 0; i < m; ++i) {
        const int32_t k = P.which[(size_t)i];
        h_tab[i] = body_off[k];
        h_tab[(size_t)m + i] = body_len[k];
        h_tab[2 * (size_t)m + i] = letters[k];
        h_tab[3 * (size_t)m + i] = large ? 0 : P.starts[(size_t)i];
    }
    *h_bad = 0ull;
    FaStrip S{};
    S.n_rec = m;
    S.body_off = d_tab;
    S.body_len = d_tab + m;
    S.letters = d_tab + 2 * (size_t)m;
    S.dest = d_tab + 3 * (size_t)m;
    S.e0 = reinterpret_cast<unsigned long long *>(d_tab + 4 * (size_t)m);
    S.bad = reinterpret_cast<unsigned long long *>(d_tab + 5 * (size_t)m);
    Genome G;        // the large record
    GenomeGroup grp;  // the others (a return below frees what either owns so far)
    if (large) {
        ISS_TRY(genome_alloc_owned(ctx, G, letters[P.which[0]]));
        S.out = G.ascii;
    } else {
        ISS_TRY(group_block(ctx, P, grp));
        S.out = grp.ascii;
    }
    hipStream_t st = ctx->stream;
    // from here on a failure waits for the stream before it returns: what is queued reads the memory above
    hipError_t he = hipMemcpyAsync(d_text, text, (size_t)n_bytes, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(d_tab, h_tab, (size_t)m * 32, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemsetAsync(S.bad, 0, sizeof(unsigned long long), st);
    if (he == hipSuccess && !large) {  // the padding: every letter of the arena 'A', the records' letters come from k_fa_strip
        memcpy(ctx->group_stage.h + tab_b, P.starts.data(), (size_t)m * 8);
        he = hipMemsetAsync(grp.block, 'A', P.asc_b, st);
        if (he == hipSuccess) he = hipMemcpyAsync(grp.block + P.asc_b, ctx->group_stage.h + tab_b, (size_t)m * 8, hipMemcpyHostToDevice, st);
    }
    if (he == hipSuccess) he = fa_prefix_launch(A, st);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(k_fa_bases, dim3((unsigned)((m + FA_THREADS - 1) / FA_THREADS)), dim3(FA_THREADS), 0, st, A, S);
        hipLaunchKernelGGL(k_fa_strip, dim3((unsigned)A.n_tiles), dim3(FA_THREADS), 0, st, A, S);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(h_bad, S.bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
    if (he != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return fail(ctx, ISS_E_HIP, std::string("iss_genome_upload_fasta: ") + hipGetErrorString(he));
    }
    const char *stale = "iss_genome_upload_fasta: the table does not fit the text (letters outside their record's place were not written)";
    if (large) {
        unsigned long long res[3];
        ISS_TRY(genome_pack_owned(ctx, G, res));  // (waits for the stream)
        if (*h_bad) return fail(ctx, ISS_E_INVALID, stale);
        if (res[0]) {
            uint8_t c = 0;
            (void)hipMemcpy(&c, G.ascii + res[1], 1, hipMemcpyDeviceToHost);
            char buf[200];
            snprintf(buf, sizeof buf, "genome letter 0x%02x at offset %llu is outside the rev_comp alphabet (%llu such letters; "
                     "the reference raises KeyError, iss/util.py:90)", c, res[1], res[0]);
            return fail(ctx, ISS_E_INVALID, buf);
        }
        G.has_exceptions = res[2] != 0;
        HIP_TRY(ctx, hipEventRecord(ctx->ev_inputs, ctx->stream));
        ctx->inputs_pending = true;
        ctx->genomes.push_back(std::move(G));
        genome_ids[P.which[0]] = (int32_t)ctx->genomes.size() - 1;
        return 0;
    }
    unsigned long long *res = reinterpret_cast<unsigned long long *>(ctx->group_stage.h + tab_b + P.st_b);
    ISS_TRY(group_pack(ctx, P, grp, res));  // (waits for the stream)
    if (*h_bad) return fail(ctx, ISS_E_INVALID, stale);
    return group_adopt(ctx, P, std::move(grp), letters, res, genome_ids);
}

}  // extern "C"
