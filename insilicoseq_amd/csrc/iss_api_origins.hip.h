// iss_api_origins.hip.h -- C ABI: every pair's source intervals as BEDPE text built on the device (iss_origins_emit_batch,
// iss_origins_flush, iss_origins_compress; the kernels of iss_origins.hip.h, iss_bgzf_text.hip.h) and the host formatter of the same lines (iss_origins_host_text).
//
// The line (one per pair, tab separated, no header):
//     {id} s1 e1 {id} s2 e2 {id}_{i}_{cpu} . + - isz \n
// (fs, rs, re, isz) as iss_output_download_coords returns them: [s1, e1) = [fs, fs + RL) is the template interval of read 1
// (iss/generator.py:135-147), [s2, e2) = [rs, re) that of read 2 (generator.py:165-177), each clamped against the record's length
// len: s' = min(max(s, 0), len), e' = max(min(max(e, 0), len), s') -- an interval that is empty after the clamp reads "s' s'".
// Read 1 is '+', read 2 '-' (generator.py:149, 180); the name is the FASTQ read name without /1, /2; isz is the insert size as
// drawn.  Plain decimals, no padding.
#pragma once

extern "C" {

int iss_origins_emit_batch(iss_ctx *ctx, int fd, int32_t n_items, const char *const *record_ids, const int64_t *first_i,
                           const int64_t *first_pair, const int64_t *n_pairs, const int64_t *record_len, int32_t cpu_number) {
    if (!ctx || !ctx->have_model || n_items < 0 || cpu_number < 0 || fd < 0 ||
        (n_items && (!record_ids || !first_i || !first_pair || !n_pairs || !record_len)))
        return fail(ctx, ISS_E_INVALID, "iss_origins_emit_batch: bad argument");
    const iss::DevModel &M = ctx->M;
    std::vector<iss::OriginsItem> items;
    std::string ids;
    size_t bytes = 0;       // a bound of the text's: every item's pairs at the longest line the item can have
    uint64_t max_line = 0;  // the call's longest line, likewise
    int64_t pairs = 0, row_end = 0;
    for (int32_t k = 0; k < n_items; ++k) {
        if (!record_ids[k] || first_i[k] < 0 || first_pair[k] < 0 || n_pairs[k] < 0)
            return fail(ctx, ISS_E_INVALID, "iss_origins_emit_batch: bad argument");
        if (first_pair[k] + n_pairs[k] > ctx->os.capacity) return fail(ctx, ISS_E_INVALID, "iss_origins_emit_batch: rows out of range");
        if (record_len[k] < 1 || record_len[k] > iss::MAX_RECORD) return fail(ctx, ISS_E_INVALID, "iss_origins_emit_batch: record_len out of range");
        const size_t idlen = strlen(record_ids[k]);
        if (idlen > FASTQ_ID_MAX) return fail(ctx, ISS_E_INVALID, "iss_origins_emit_batch: record id longer than 4096 bytes");
        if (n_pairs[k] == 0) continue;
        if (first_pair[k] < row_end) return fail(ctx, ISS_E_INVALID, "iss_origins_emit_batch: items out of order or overlapping");
        row_end = first_pair[k] + n_pairs[k];
        iss::OriginsItem it{};
        it.cpu_len = (int32_t)snprintf(it.cpu, sizeof it.cpu, "%d", cpu_number);
        it.first_i = (uint64_t)first_i[k];
        it.first_pair = first_pair[k];
        it.rec_first = pairs;
        it.rec_len = record_len[k];
        it.id_off = (uint32_t)ids.size();
        it.id_len = (int32_t)idlen;
        ids.append(record_ids[k], idlen);
        const uint64_t line = iss::origins_line_bound(idlen, (uint64_t)it.cpu_len, record_len[k], it.first_i + (uint64_t)n_pairs[k] - 1);
        max_line = std::max(max_line, line);
        bytes += (size_t)n_pairs[k] * (size_t)line;
        pairs += n_pairs[k];
        items.push_back(it);
    }
    if (items.empty()) return 0;
    int asked = 0;
    if (const char *e = getenv("ISS_ORIGINS_TILE")) asked = std::max(1, atoi(e));  // pairs per workgroup (tests: other tilings; read per call)
    const int tile = iss::origins_tile_pairs(max_line, asked);
    const int64_t n_tiles = (pairs + tile - 1) / tile;
    if (n_tiles > (int64_t)0x7fffffff) return fail(ctx, ISS_E_INVALID, "iss_origins_emit_batch: too many rows for one call");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    OriginsPipe &q = ctx->oq;
    if (!q.ready) {
        for (auto &p : q.d_total) DEV_ALLOC(ctx, p, 64 / sizeof(uint64_t));
        ISS_TRY(append_start(ctx, q, true, origins_write, "origins text"));
    }
    ISS_TRY(append_attach(ctx, q, fd));
    if (bytes > q.cap) {
        ISS_TRY(append_flush(ctx, q, true));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the kernels of the last call write the buffers)
        reset_part<OriginsText>(q);
        const size_t cap = bytes + bytes / 8 + (1u << 16);
        for (int sl = 0; sl < 2; ++sl) {
            DEV_ALLOC(ctx, q.d_text[sl], cap + 16);
            PIN_ALLOC(ctx, q.h_text[sl], cap);
        }
        q.cap = cap;
    }
    const size_t scan_tiles = ((size_t)pairs + iss::VSCAN_TILE - 1) / iss::VSCAN_TILE;
    if ((size_t)pairs > q.pairs_cap || scan_tiles > q.tiles_cap) {  // the work arrays: only kernels of the context's stream touch them
        if (q.pairs_cap) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        reset_part<OriginsWork>(q);
        const size_t pc = (size_t)pairs + (size_t)pairs / 8 + 4096, tc = (pc + iss::VSCAN_TILE - 1) / iss::VSCAN_TILE + 1;
        DEV_ALLOC(ctx, q.d_len, pc);
        DEV_ALLOC(ctx, q.d_off, pc);
        DEV_ALLOC(ctx, q.d_tiles, tc);
        q.pairs_cap = pc;
        q.tiles_cap = tc;
    }
    if (q.z.mode) ISS_TRY(bgzt_reserve(ctx, q, q.z, q.cap));
    const int slot = q.next;
    ISS_TRY(writer_wait_slot(ctx, q, slot));
    hipStream_t st = ctx->stream;
    ISS_TRY(q.tab.stage(ctx, slot, items, ids, st));
    iss::OriginsArgs A{};
    A.desc = ctx->os.desc;
    A.n_pairs = pairs;
    A.RL = M.RL;
    A.n_items = (int32_t)items.size();
    A.items = q.tab.slot[slot].d_items;
    A.ids = q.tab.slot[slot].d_ids;
    A.len = q.d_len;
    A.off = q.d_off;
    A.total = q.d_total[slot];
    A.text = q.d_text[slot];
    A.text_cap = q.cap;
    A.tile = tile;
    A.region = iss::origins_region_bytes((uint64_t)tile, max_line);
    // the item table of the last iss_generate_batch call is resident (iss_output_export): its rows carry arena coordinates
    int set = -1;
    if (!ctx->last_first.empty() && ctx->batch_seq > 0) {
        set = (int)((ctx->batch_seq - 1) & 1u);
        A.batch = ctx->it.d_items[set];
        A.item_first = ctx->it.d_item_first[set];
        A.n_batch = (int32_t)ctx->last_first.size() - 1;
        A.row0 = ctx->last_row0;
        A.call_pairs = ctx->last_n;
    }
    const unsigned len_grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(iss::ORIGINS_TARGET_WGS, (pairs + iss::ORIGINS_THREADS - 1) / iss::ORIGINS_THREADS));
    hipLaunchKernelGGL(iss::k_origins_len, dim3(len_grid), dim3(iss::ORIGINS_THREADS), 0, st, A);
    hipLaunchKernelGGL(iss::k_vcf_scan_sums, dim3((unsigned)scan_tiles), dim3(iss::VSCAN_THREADS), 0, st, (const uint32_t *)q.d_len, (uint64_t)pairs, q.d_tiles);
    hipLaunchKernelGGL(iss::k_vcf_scan_tiles, dim3(1), dim3(iss::VSCAN_THREADS), 0, st, q.d_tiles, (uint64_t)scan_tiles, q.d_total[slot]);
    hipLaunchKernelGGL(iss::k_vcf_scan_apply, dim3((unsigned)scan_tiles), dim3(iss::VSCAN_THREADS), 0, st, (const uint32_t *)q.d_len, (uint64_t)pairs,
                       (const uint64_t *)q.d_tiles, q.d_off);
    hipLaunchKernelGGL(iss::k_origins_format, dim3((unsigned)n_tiles), dim3(iss::ORIGINS_THREADS), (size_t)A.region, st, A);
    HIP_TRY(ctx, hipGetLastError());
    // (iss_generate_batch refills a set of tables once the event of its last reader has passed, and k_setup of the call after the
    //  next rewrites the descriptors' set once this one has: these launches are the last readers now)
    if (set >= 0) HIP_TRY(ctx, hipEventRecord(ctx->it.ev_items[set], st));
    if (ctx->call_seq) HIP_TRY(ctx, hipEventRecord(ctx->ev_call_done[(int)((ctx->call_seq - 1) & 1u)], st));
    const uint64_t *d_total = q.d_total[slot];
    if (q.z.mode) {  // the text stays on the device: its members are what the writer fetches (the line offsets are still resident)
        ISS_TRY(bgzt_launch(ctx, q, q.z, slot, q.d_text[slot], bytes, q.d_off, (uint64_t)pairs, q.d_total[slot], st, &d_total));
    }
    return append_enqueue(ctx, q, slot, q.fd, d_total);
}

int iss_origins_compress(iss_ctx *ctx, int32_t mode) {
    if (!ctx) return fail(nullptr, ISS_E_INVALID, "ctx is NULL");
    return bgzt_set_mode(ctx, ctx->oq, ctx->oq.z, mode, "iss_origins_compress");
}

int iss_bgzf_text_code_build(const uint32_t *hist, uint32_t *entry, uint32_t *dentry, uint32_t *hdr_bits, uint32_t *hdr_words) {
    if (!hist || !entry || !dentry || !hdr_bits || !hdr_words) return ISS_E_INVALID;
    static iss::BgzfTextWork ws;  // (large for a stack frame; the function is a test hook, not re-entrant)
    iss::bgzf_text_build_code(hist, &ws, 0, 1, iss::DeflateNoSync());
    for (int s = 0; s < iss::DEFLATE_SYMS; ++s) entry[s] = ws.w.entry[s];
    for (int d = 0; d < iss::BGZT_DSYMS; ++d) dentry[d] = ws.dentry[d];
    for (int i = 0; i < iss::BGZT_HDR_WORDS; ++i) hdr_words[i] = ws.hdr[i];
    *hdr_bits = ws.hdr_bits;
    return 0;
}

int iss_origins_flush(iss_ctx *ctx) {
    if (!ctx) return fail(nullptr, ISS_E_INVALID, "ctx is NULL");
    return append_flush(ctx, ctx->oq);
}

int iss_origins_host_text(int fd, const char *record_id, int64_t first_i, int32_t cpu_number, int64_t n_pairs, int32_t read_length,
                          int64_t record_len, const int64_t *coords) {
    if (fd < 0 || !record_id || n_pairs < 0 || read_length < 1 || record_len < 1 || record_len > iss::MAX_RECORD || cpu_number < 0 || first_i < 0 ||
        (n_pairs && !coords))
        return fail(nullptr, ISS_E_INVALID, "iss_origins_host_text: bad argument");
    if (n_pairs == 0) return 0;
    const size_t idlen = strlen(record_id);
    char cpu_txt[16];
    const size_t cpu_len = fmt_u64(cpu_txt, (uint64_t)cpu_number);
    const int64_t chunk = 1 << 12;
    std::vector<uint8_t> buf;
    for (int64_t base = 0; base < n_pairs; base += chunk) {
        const int64_t hi = std::min(n_pairs, base + chunk);
        size_t need = 0;
        for (int64_t i = base; i < hi; ++i) {
            const int64_t *c = coords + 4 * i;
            need += iss::origins_line_len((uint32_t)idlen, (uint32_t)cpu_len, (uint64_t)(first_i + i),
                                          iss::origins_span(c[0], c[1], c[2], read_length, record_len), c[3]);
        }
        buf.resize(need);
        uint8_t *w = buf.data();
        for (int64_t i = base; i < hi; ++i) {
            const int64_t *c = coords + 4 * i;
            w = iss::origins_put_line(w, record_id, (uint32_t)idlen, cpu_txt, (uint32_t)cpu_len, (uint64_t)(first_i + i),
                                      iss::origins_span(c[0], c[1], c[2], read_length, record_len), c[3]);
        }
        if (write_all(fd, reinterpret_cast<const char *>(buf.data()), (size_t)(w - buf.data())))
            return fail(nullptr, ISS_E_IO, std::string("write failed: ") + strerror(errno));
    }
    return 0;
}

}  // extern "C"
