// iss_api_ubam.hip.h -- C ABI: unaligned BAM built on the device (iss_ubam_emit_batch, iss_ubam_flush) and the host formatter of
// the same record bytes (iss_ubam_host_records).
#pragma once

namespace {

int ubam_digits(uint64_t v) {
    int dg = 1;
    for (; v >= 10; v /= 10) ++dg;
    return dg;
}

}  // namespace

extern "C" {

int iss_ubam_emit_batch(iss_ctx *ctx, int fd, int32_t n_items, const char *const *record_ids, const int64_t *first_i,
                        const int64_t *first_pair, const int64_t *n_pairs, int32_t cpu_number) {
    if (!ctx || !ctx->have_model || n_items < 0 || cpu_number < 0 || fd < 0 || (n_items && (!record_ids || !first_i || !first_pair || !n_pairs)))
        return fail(ctx, ISS_E_INVALID, "iss_ubam_emit_batch: bad argument");
    const iss::DevModel &M = ctx->M;
    std::vector<iss::FastqItem> items;
    std::string ids;
    size_t bytes = 0, rec_len = 0;  // rec_len: record length of the item with the most pairs (the distance of its "previous record")
    int64_t pairs = 0, most = 0;
    for (int32_t k = 0; k < n_items; ++k) {
        if (!record_ids[k] || first_i[k] < 0 || first_pair[k] < 0 || n_pairs[k] < 0 || first_pair[k] + n_pairs[k] > ctx->os.capacity)
            return fail(ctx, ISS_E_INVALID, "iss_ubam_emit_batch: bad argument");
        if (n_pairs[k] == 0) continue;
        const size_t idlen = strlen(record_ids[k]);
        iss::FastqItem it{};
        it.cpu_len = (int32_t)snprintf(it.cpu, sizeof it.cpu, "%d", cpu_number);
        const int dg_last = ubam_digits((uint64_t)first_i[k] + (uint64_t)n_pairs[k] - 1);
        if (idlen + 1 + (size_t)dg_last + 1 + (size_t)it.cpu_len > (size_t)iss::UBAM_NAME_MAX)
            return fail(ctx, ISS_E_INVALID, std::string("iss_ubam_emit_batch: the read names of record '") + record_ids[k] +
                                                "' are longer than the 254 characters a BAM record holds");
        it.first_i = (uint64_t)first_i[k];
        it.before_first = iss::digits_before(it.first_i);
        it.text_off = bytes;
        it.first_pair = first_pair[k];
        it.rec_first = pairs;
        it.id_off = (uint32_t)ids.size();
        it.id_len = (int32_t)idlen;
        ids.append(record_ids[k], idlen);
        const size_t C = (size_t)iss::ubam_record_const(idlen, (uint64_t)it.cpu_len, (uint64_t)M.RL);
        bytes += 2 * ((size_t)n_pairs[k] * C + (size_t)(iss::digits_before(it.first_i + (uint64_t)n_pairs[k]) - it.before_first));
        pairs += n_pairs[k];
        if (n_pairs[k] > most) {
            most = n_pairs[k];
            rec_len = C + (size_t)dg_last;
        }
        items.push_back(it);
    }
    if (items.empty()) return 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    UbamPipe &q = ctx->uq;
    if (!q.ready) {
        iss::DeflateCode init{};
        for (int k = 0; k < 8; ++k) iss::crc_shift_operator((uint64_t)128 << k, init.crc_shift[k]);
        for (int sl = 0; sl < 2; ++sl) {  // (a call that fails before the pipe is ready makes them again: the handles release first)
            DEV_ALLOC(ctx, q.d_hist[sl], iss::DEFLATE_SYMS + 7);
            DEV_ALLOC(ctx, q.d_code[sl], 1);
            HIP_TRY(ctx, hipMemcpy(q.d_code[sl], &init, sizeof init, hipMemcpyHostToDevice));
        }
        ISS_TRY(append_start(ctx, q, true, ubam_write, "unaligned BAM"));
    }
    ISS_TRY(append_attach(ctx, q, fd));
    const uint32_t n_blocks = (uint32_t)((bytes + iss::DEFLATE_BLOCK - 1) / iss::DEFLATE_BLOCK);
    // members of a call: its own Huffman code never needs more than 8 bits per byte plus rounding; the smoothing of the counts,
    // the block headers and the members' frames are covered by the margin (a call that needs more fails, it is never cut)
    auto comp_bytes = [](size_t text, size_t blocks) { return text + text / 8 + blocks * (320 + iss::BGZF_FRAME) + 64; };
    if (bytes > q.cap || comp_bytes(bytes, n_blocks) > q.comp_cap || n_blocks > q.blocks_cap) {
        ISS_TRY(append_flush(ctx, q, true));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the kernels of the last call read the buffers)
        reset_part<UbamBuffers>(q);
        const size_t cap = bytes + bytes / 8 + (1u << 20);
        const size_t cap_blocks = (cap + iss::DEFLATE_BLOCK - 1) / iss::DEFLATE_BLOCK;
        const size_t comp_cap = comp_bytes(cap, cap_blocks);
        for (int sl = 0; sl < 2; ++sl) {
            DEV_ALLOC(ctx, q.d_text[sl], cap + 16);
            DEV_ALLOC(ctx, q.d_comp[sl], comp_cap + 8);
            PIN_ALLOC(ctx, q.h_comp[sl], comp_cap);
            DEV_ALLOC(ctx, q.d_bbytes[sl], cap_blocks);
            DEV_ALLOC(ctx, q.d_bcrc[sl], cap_blocks);
            DEV_ALLOC(ctx, q.d_boff[sl], cap_blocks + 1);
        }
        q.cap = cap;
        q.comp_cap = comp_cap;
        q.blocks_cap = (uint32_t)cap_blocks;
    }
    const int slot = q.next;
    ISS_TRY(writer_wait_slot(ctx, q, slot));
    ISS_TRY(q.tab.stage(ctx, slot, items, ids, ctx->stream));
    iss::UbamArgs A{};
    A.row = M.row;
    A.RL = M.RL;
    A.n_items = (int32_t)items.size();
    A.n_pairs = pairs;
    A.items = q.tab.slot[slot].d_items;
    A.ids = q.tab.slot[slot].d_ids;
    A.text = q.d_text[slot];
    for (int m = 0; m < 2; ++m) {
        A.base[m] = ctx->out[2 * m];
        A.qual[m] = ctx->out[2 * m + 1];
    }
    hipLaunchKernelGGL(iss::k_ubam_format, dim3((unsigned)((2 * pairs + iss::FASTQ_WAVES - 1) / iss::FASTQ_WAVES)), dim3(64 * iss::FASTQ_WAVES), 0,
                       ctx->stream, A);
    // the records stay on the device: histogram -> code -> member sizes + CRCs -> offsets -> bits (iss_ubam.hip.h)
    iss::DeflateArgs D{};
    D.n_bytes = bytes;
    D.n_blocks = n_blocks;
    D.out_cap = q.comp_cap;
    if (rec_len >= 8 && rec_len <= 32768 && !getenv("ISS_DEFLATE_RUNS_ONLY")) {
        D.dist = (uint32_t)rec_len;
        iss::deflate_dist_code(D.dist, &D.dist_sym, &D.dist_ebits, &D.dist_eval);
    }
    D.text[0] = q.d_text[slot];
    D.hist[0] = q.d_hist[slot];
    D.code[0] = q.d_code[slot];
    D.block_bytes[0] = q.d_bbytes[slot];
    D.block_crc[0] = q.d_bcrc[slot];
    D.block_off[0] = q.d_boff[slot];
    D.out[0] = q.d_comp[slot];
    HIP_TRY(ctx, hipMemsetAsync(q.d_hist[slot], 0, iss::DEFLATE_SYMS * 4, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(q.d_comp[slot], 0, std::min(q.comp_cap, comp_bytes(bytes, n_blocks)) + 8, ctx->stream));
    const unsigned hist_grid = (unsigned)std::min<uint64_t>(2048, (bytes / 16 + iss::DEFLATE_THREADS - 1) / iss::DEFLATE_THREADS + 1);
    hipLaunchKernelGGL(iss::k_bgzf_hist, dim3(hist_grid), dim3(iss::DEFLATE_THREADS), 0, ctx->stream, D);
    hipLaunchKernelGGL(iss::k_deflate_build, dim3(1), dim3(64), 0, ctx->stream, D);
    hipLaunchKernelGGL(iss::k_bgzf_len, dim3(n_blocks), dim3(iss::DEFLATE_THREADS), 0, ctx->stream, D);
    hipLaunchKernelGGL(iss::k_deflate_scan, dim3(1), dim3(1024), 0, ctx->stream, D);
    hipLaunchKernelGGL(iss::k_bgzf_encode, dim3(n_blocks), dim3(iss::DEFLATE_THREADS), 0, ctx->stream, D);
    HIP_TRY(ctx, hipGetLastError());
    q.job_blocks[slot] = n_blocks;
    return append_enqueue(ctx, q, slot, q.fd, q.d_boff[slot] + n_blocks);
}

int iss_ubam_flush(iss_ctx *ctx) {
    if (!ctx) return fail(nullptr, ISS_E_INVALID, "ctx is NULL");
    return append_flush(ctx, ctx->uq);
}

int iss_ubam_host_records(int fd, const char *record_id, int64_t first_i, int32_t cpu_number, int64_t n_pairs, int32_t read_length,
                          int32_t pitch, const uint8_t *r1_base, const uint8_t *r1_qual, const uint8_t *r2_base, const uint8_t *r2_qual) {
    if (fd < 0 || !record_id || n_pairs < 0 || read_length < 1 || pitch < read_length || cpu_number < 0 || first_i < 0 ||
        (n_pairs && (!r1_base || !r1_qual || !r2_base || !r2_qual)))
        return fail(nullptr, ISS_E_INVALID, "iss_ubam_host_records: bad argument");
    if (n_pairs == 0) return 0;
    const size_t idlen = strlen(record_id);
    char cpu_txt[16];
    const size_t cpu_len = fmt_u64(cpu_txt, (uint64_t)cpu_number);
    if (idlen + 1 + (size_t)ubam_digits((uint64_t)first_i + (uint64_t)n_pairs - 1) + 1 + cpu_len > (size_t)iss::UBAM_NAME_MAX)
        return fail(nullptr, ISS_E_INVALID, std::string("iss_ubam_host_records: the read names of record '") + record_id +
                                                "' are longer than the 254 characters a BAM record holds");
    const size_t C = (size_t)iss::ubam_record_const(idlen, cpu_len, (uint64_t)read_length), half = ((size_t)read_length + 1) / 2;
    const int64_t chunk = 1 << 12;
    std::vector<uint8_t> buf;
    for (int64_t base = 0; base < n_pairs; base += chunk) {
        const int64_t hi = std::min(n_pairs, base + chunk);
        buf.resize((size_t)(hi - base) * 2 * (C + 20));
        uint8_t *w = buf.data();
        for (int64_t i = base; i < hi; ++i)
            for (int mate = 0; mate < 2; ++mate) {
                char num[24];
                const size_t dg = fmt_u64(num, (uint64_t)(first_i + i));
                const size_t nlen = idlen + 1 + dg + 1 + cpu_len;
                for (int k = 0; k < iss::UBAM_FIXED; ++k)
                    *w++ = iss::ubam_fixed_byte(k, (uint32_t)(C + dg) - 4u, (uint32_t)nlen + 1u, iss::ubam_flag(mate), (uint32_t)read_length);
                memcpy(w, record_id, idlen); w += idlen;
                *w++ = '_';
                memcpy(w, num, dg); w += dg;
                *w++ = '_';
                memcpy(w, cpu_txt, cpu_len); w += cpu_len;
                *w++ = 0;
                const uint8_t *b = (mate ? r2_base : r1_base) + (size_t)i * pitch, *ql = (mate ? r2_qual : r1_qual) + (size_t)i * pitch;
                for (size_t k = 0; k < half; ++k)
                    *w++ = (uint8_t)((iss::ubam_code(b[2 * k]) << 4) | (2 * k + 1 < (size_t)read_length ? iss::ubam_code(b[2 * k + 1]) : 0u));
                memcpy(w, ql, (size_t)read_length); w += read_length;
            }
        if (write_all(fd, reinterpret_cast<const char *>(buf.data()), (size_t)(w - buf.data())))
            return fail(nullptr, ISS_E_IO, std::string("write failed: ") + strerror(errno));
    }
    return 0;
}

}  // extern "C"
