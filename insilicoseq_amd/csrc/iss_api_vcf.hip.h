// iss_api_vcf.hip.h -- C ABI: the --store_mutations VCF text built on the device (iss_vcf_emit, iss_vcf_flush, iss_vcf_compress).
#pragma once

namespace {

// one text job: the rows, their items, where the text goes
struct VcfJob {
    int fd = -1;                   // one file ...
    std::vector<int> wfds;         // ... or one per item: a worker set (wbase below)
    bool philox = false;
    const iss::MutRecord *mut = nullptr;
    int64_t n_slots = 0, call_pairs = 0;
    std::vector<iss::VcfItem> items;
    std::string ids;
    size_t longest = 0;            // of "{id}_{i}_" over the items
    std::vector<uint64_t> wbase;   // a worker set: [n_items + 1] first row of item k's worker in the text
    uint64_t wstride = 0;          // ... whose rows stand at mut + k * wstride
};

int vcf_pipe_init(iss_ctx *ctx) {
    VcfPipe &q = ctx->vq;
    if (q.ready) return 0;
    PIN_ALLOC(ctx, q.h_count, 64 / sizeof(uint32_t));
    DEV_ALLOC(ctx, q.d_stats, 2);
    return append_start(ctx, q, false, vcf_write, "VCF text");  // (no copy stream: the size rides the context's stream)
}

// an item of the table: the id's place in `ids`, the worker's number, the longest "{id}_{i}_" so far
int vcf_add_item(iss_ctx *ctx, VcfJob &J, const char *record_id, int64_t first_i, int64_t pair0, int64_t n_pairs, int32_t cpu_number) {
    const size_t idlen = strlen(record_id);
    if (idlen > FASTQ_ID_MAX) return fail(ctx, ISS_E_INVALID, "iss_vcf_emit: record id longer than 4096 bytes");
    iss::VcfItem it{};
    it.first_i = (uint64_t)first_i;
    it.pair0 = pair0;
    it.n_pairs = n_pairs;
    it.id_off = (uint32_t)J.ids.size();
    it.id_len = (int32_t)idlen;
    it.cpu_len = (int32_t)snprintf(it.cpu, sizeof it.cpu, "%d", cpu_number);
    J.ids.append(record_id, idlen);
    int dg = 1;
    for (uint64_t v = it.first_i + (uint64_t)std::max<int64_t>(it.n_pairs, 1) - 1; v >= 10; v /= 10) ++dg;
    J.longest = std::max(J.longest, idlen + (size_t)dg);
    J.items.push_back(it);
    return 0;
}

// the kernels of DESIGN.md section 14 for one job, on the context's stream; the job queued for the writer thread
int vcf_queue(iss_ctx *ctx, const VcfJob &J) {
    VcfPipe &q = ctx->vq;
    const bool philox = J.philox;
    const int64_t n_slots = J.n_slots, call_pairs = J.call_pairs;
    const std::vector<iss::VcfItem> &items = J.items;
    const std::string &ids = J.ids;
    const size_t longest = J.longest;
    iss::VcfArgs A{};
    // bytes of a row at most: 14 fixed characters, position + 1 and the phred with up to 6 each, two letters of an insertion
    const size_t row_max = longest + 12 /* the worker's number */ + 14 + 6 + 6 + 2;
    const size_t bound = (size_t)n_slots * row_max;
    // work arrays (one set: every kernel that touches them is on the context's stream)
    const size_t n_tiles = std::max<size_t>(1, ((size_t)std::max<int64_t>(n_slots, call_pairs) + iss::VSCAN_TILE - 1) / iss::VSCAN_TILE);
    if ((size_t)n_slots > q.slots_cap || (size_t)call_pairs > q.pairs_cap || n_tiles > q.tiles_cap) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the kernels of the emit before may still read them)
        const size_t sc = std::max(q.slots_cap, (size_t)n_slots + (size_t)n_slots / 4 + 4096);
        const size_t pc = std::max(q.pairs_cap, (size_t)call_pairs + (size_t)call_pairs / 4 + 4096);
        const size_t tc = (std::max(sc, pc) + iss::VSCAN_TILE - 1) / iss::VSCAN_TILE + 1;
        reset_part<VcfWork>(q);
        DEV_ALLOC(ctx, q.d_key, sc);
        DEV_ALLOC(ctx, q.d_slot, sc);
        DEV_ALLOC(ctx, q.d_order, sc);
        DEV_ALLOC(ctx, q.d_len, sc);
        DEV_ALLOC(ctx, q.d_off, sc + 1);
        DEV_ALLOC(ctx, q.d_cnt, pc);
        DEV_ALLOC(ctx, q.d_seg, pc + 1);
        DEV_ALLOC(ctx, q.d_tiles, tc);
        q.slots_cap = sc; q.pairs_cap = pc; q.tiles_cap = tc;
    }
    if (q.z.mode) ISS_TRY(bgzt_reserve(ctx, q, q.z, bound));
    const int slot = q.next;
    ISS_TRY(writer_wait_slot(ctx, q, slot));
    // (the slot is free: nothing reads its text or its tables)
    if (bound > q.text[slot].cap) {
        q.text[slot] = {};
        const size_t cap = bound + bound / 8 + (1u << 20);
        if (own_alloc_quiet(q.text[slot].d, cap)) return fail(ctx, ISS_E_NOMEM, "iss_vcf_emit: no device memory for the text");
        q.text[slot].cap = cap;
    }
    hipStream_t st = ctx->stream;
    ISS_TRY(q.tab.stage(ctx, slot, items, ids, st));
    A.mut = J.mut;
    A.n_slots = (uint32_t)n_slots;
    A.n_pairs = call_pairs;
    A.cnt = q.d_cnt;
    A.seg = q.d_seg;
    A.key = q.d_key;
    A.slot = q.d_slot;
    A.len = q.d_len;
    A.off = q.d_off;
    A.text = q.text[slot].d;
    A.text_cap = q.text[slot].cap;
    A.items = q.tab.slot[slot].d_items;
    A.ids = q.tab.slot[slot].d_ids;
    A.n_items = (int32_t)items.size();
    const bool set = !J.wbase.empty();  // a worker set: item k = worker k, its rows from wbase[k] (the table behind the items' copy)
    if (set) {
        const size_t nw = J.wbase.size();  // n_items + 1
        if (2 * nw > q.wb[slot].cap) {
            q.wb[slot] = {};
            PIN_ALLOC(ctx, q.wb[slot].h, 4 * nw);
            DEV_ALLOC(ctx, q.wb[slot].d, 4 * nw);
            q.wb[slot].cap = 4 * nw;
        }
        memcpy(q.wb[slot].h, J.wbase.data(), nw * sizeof(uint64_t));
        HIP_TRY(ctx, hipMemcpyAsync(q.wb[slot].d, q.wb[slot].h, nw * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        A.wbase = q.wb[slot].d;
        A.wstride = J.wstride;
        A.wbytes = q.wb[slot].d + nw;
    }
    auto grid_for = [](uint64_t n) { return dim3((unsigned)std::min<uint64_t>(2048, (n + iss::VCF_THREADS - 1) / iss::VCF_THREADS)); };
    auto scan = [&](const uint32_t *in, uint64_t n, uint64_t *out) {
        const unsigned tiles = (unsigned)((n + iss::VSCAN_TILE - 1) / iss::VSCAN_TILE);
        hipLaunchKernelGGL(iss::k_vcf_scan_sums, dim3(tiles), dim3(iss::VSCAN_THREADS), 0, st, in, n, q.d_tiles);
        hipLaunchKernelGGL(iss::k_vcf_scan_tiles, dim3(1), dim3(iss::VSCAN_THREADS), 0, st, q.d_tiles, (uint64_t)tiles, out + n);
        hipLaunchKernelGGL(iss::k_vcf_scan_apply, dim3(tiles), dim3(iss::VSCAN_THREADS), 0, st, in, n, (const uint64_t *)q.d_tiles, out);
    };
    const dim3 grid = grid_for((uint64_t)n_slots), block(iss::VCF_THREADS);
    q.job_debug[slot] = false;
    if (philox) {  // a, b: the slots that stay, in the order of iss_mutations_download
        A.flags = ctx->flags + ctx->last_row0;
        A.order = q.d_order;
        A.n_rows = q.d_seg + call_pairs;
        HIP_TRY(ctx, hipMemsetAsync(q.d_cnt, 0, (size_t)call_pairs * 4, st));
        HIP_TRY(ctx, hipMemsetAsync(q.d_order, 0, (size_t)n_slots * 4, st));
        // ISS_VCF_DEBUG: the writer thread reports how many slots held a row and how many of those stayed (the rest are stale)
        const bool debug = getenv("ISS_VCF_DEBUG") != nullptr;
        q.job_debug[slot] = debug;
        if (debug) {
            A.stats = q.d_stats;
            HIP_TRY(ctx, hipMemsetAsync(q.d_stats, 0, 2 * sizeof(uint32_t), st));
        }
        hipLaunchKernelGGL(iss::k_vcf_count, grid, block, 0, st, A);
        if (debug) HIP_TRY(ctx, hipMemcpyAsync(q.h_total[slot] + 1, q.d_stats, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        scan(q.d_cnt, (uint64_t)call_pairs, q.d_seg);
        hipLaunchKernelGGL(iss::k_vcf_scatter, grid, block, 0, st, A);
        hipLaunchKernelGGL(iss::k_vcf_rank, grid, block, 0, st, A);
        // the flag words are this call's set: k_setup of the call after the next rewrites it once this event has passed
        if (ctx->call_seq) {
            const int par = (int)((ctx->call_seq - 1) & 1u);
            HIP_TRY(ctx, hipEventRecord(ctx->ev_call_done[par], st));
        }
    }
    hipLaunchKernelGGL(iss::k_vcf_len, grid, block, 0, st, A);  // c
    scan(q.d_len, (uint64_t)n_slots, q.d_off);
    hipLaunchKernelGGL(iss::k_vcf_format, grid, block, 0, st, A);  // d
    HIP_TRY(ctx, hipGetLastError());
    if (set) {
        hipLaunchKernelGGL(iss::k_vcf_worker_bytes, dim3((unsigned)(J.wbase.size() + iss::VCF_THREADS - 1) / iss::VCF_THREADS), block, 0, st, A);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(q.wb[slot].h + J.wbase.size(), A.wbytes, J.wbase.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    }
    q.job_wfds[slot] = J.wfds;
    const uint64_t *d_total = q.d_off + n_slots;
    if (q.z.mode) {  // the rows' offsets are the line offsets (a slot without a row: an empty line)
        ISS_TRY(bgzt_launch(ctx, q, q.z, slot, q.text[slot].d, bound, q.d_off, (uint64_t)n_slots, q.d_off + n_slots, st, &d_total));
    }
    return append_enqueue(ctx, q, slot, J.fd, d_total);
}

}  // namespace

extern "C" {

int iss_vcf_emit(iss_ctx *ctx, int fd, int32_t source, int32_t n_items, const char *const *record_ids, const int64_t *first_i,
                 const int64_t *first_pair, const int64_t *n_pairs, int32_t cpu_number, int64_t *slots_needed) {
    if (slots_needed) *slots_needed = 0;
    if (!ctx || !ctx->have_model || fd < 0 || n_items < 0 || cpu_number < 0 || (source != 0 && source != 1) ||
        (n_items && (!record_ids || !first_i || !first_pair || !n_pairs)))
        return fail(ctx, ISS_E_INVALID, "iss_vcf_emit: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    VcfPipe &q = ctx->vq;
    ISS_TRY(vcf_pipe_init(ctx));
    // the rows: how many slots to look at, and which output row pair 0 of the call is
    const bool philox = source == 0;
    int64_t n_slots = 0, row0 = 0, call_pairs = 0;
    if (philox) {
        if (!ctx->pmut.d || !ctx->d_pmut_count) return 0;  // (no rows are captured: like iss_mutations_download)
        // the one value that comes back per call: the slots it reserved (this waits for the generation, not for the text)
        HIP_TRY(ctx, hipMemcpyAsync(q.h_count, ctx->d_pmut_count, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        n_slots = (int64_t)*q.h_count;
        if (n_slots > ctx->pmut.cap) {
            if (slots_needed) *slots_needed = n_slots;  // (the slots the call asked for: what a retry has to reserve)
            return fail(ctx, ISS_E_NOMEM, "mutation buffer too small for this call (reserve more with iss_mutations_reserve)");
        }
        row0 = ctx->last_row0;
        call_pairs = ctx->last_n;
    } else {
        const auto &m = ctx->mt;
        if (!m.d_mut) return 0;
        if (m.mut_n > m.mut_cap) return fail(ctx, ISS_E_INVALID, "iss_vcf_emit: more rows than iss_mt_mutations_reserve holds");
        n_slots = m.mut_n;
        row0 = m.mut_row0;
    }
    // the items that hold pairs, as pairs of the call: ascending, apart
    VcfJob J;
    for (int32_t k = 0; k < n_items; ++k) {
        if (!record_ids[k] || first_i[k] < 0 || first_pair[k] < 0 || n_pairs[k] < 0) return fail(ctx, ISS_E_INVALID, "iss_vcf_emit: bad argument");
        if (strlen(record_ids[k]) > FASTQ_ID_MAX) return fail(ctx, ISS_E_INVALID, "iss_vcf_emit: record id longer than 4096 bytes");
        if (n_pairs[k] == 0) continue;
        const int64_t pair0 = first_pair[k] - row0;
        if (pair0 < 0 || (philox && pair0 + n_pairs[k] > call_pairs))
            return fail(ctx, ISS_E_INVALID, "iss_vcf_emit: an item lies outside the rows of the last generate call");
        if (!J.items.empty() && pair0 < J.items.back().pair0 + J.items.back().n_pairs)
            return fail(ctx, ISS_E_INVALID, "iss_vcf_emit: items must stand in ascending row order and not overlap");
        ISS_TRY(vcf_add_item(ctx, J, record_ids[k], first_i[k], pair0, n_pairs[k], cpu_number));
    }
    if (J.items.empty() || n_slots == 0) return 0;
    if (n_slots > 0x7fffffff) return fail(ctx, ISS_E_INVALID, "iss_vcf_emit: too many rows");
    ISS_TRY(append_attach(ctx, q, fd));
    J.fd = fd;
    J.philox = philox;
    J.mut = philox ? ctx->pmut.d : ctx->mt.d_mut;
    J.n_slots = n_slots;
    J.call_pairs = call_pairs;
    return vcf_queue(ctx, J);
}

int iss_vcf_emit_workers(iss_ctx *ctx, int32_t n_workers, const int *fds, const char *const *record_ids, const int64_t *first_i,
                         const int64_t *first_pair, const int64_t *n_pairs, const int32_t *cpu_numbers) {
    if (!ctx || !ctx->have_model || n_workers < 1 || !fds || !record_ids || !first_i || !first_pair || !n_pairs || !cpu_numbers)
        return fail(ctx, ISS_E_INVALID, "iss_vcf_emit_workers: bad argument");
    if (ctx->vq.z.mode) return fail(ctx, ISS_E_INVALID, "iss_vcf_emit_workers: the worker set's text is not compressed (iss_vcf_compress is 1)");
    const auto &t = ctx->mts;
    if (n_workers != t.W) return fail(ctx, ISS_E_INVALID, "iss_vcf_emit_workers: one entry per worker of the seeded set");
    if (t.poisoned) return fail(ctx, ISS_E_INVALID, "iss_vcf_emit_workers: the last iss_generate_mt_workers call failed (its rows are undefined)");
    if (!t.d_mut) return 0;  // (no rows are captured: like iss_vcf_emit)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ISS_TRY(vcf_pipe_init(ctx));
    VcfPipe &q = ctx->vq;
    // item k = worker k (a worker that sits the round out, or made no row, has an empty range); the text's rows are the workers' rows
    // one worker after the other
    VcfJob J;
    uint64_t rows = 0;
    for (int32_t k = 0; k < n_workers; ++k) {
        if (!record_ids[k] || first_i[k] < 0 || n_pairs[k] < 0 || cpu_numbers[k] < 0 || (n_pairs[k] > 0 && fds[k] < 0))
            return fail(ctx, ISS_E_INVALID, "iss_vcf_emit_workers: bad argument");
        if (n_pairs[k] > 0 && (first_pair[k] != t.mut_row0[(size_t)k] || n_pairs[k] > t.mut_pairs[(size_t)k]))
            return fail(ctx, ISS_E_INVALID, "iss_vcf_emit_workers: a worker's item is not its rows of the last iss_generate_mt_workers call");
        if (t.mut_n[(size_t)k] > t.mut_rows) return fail(ctx, ISS_E_INVALID, "iss_vcf_emit_workers: more rows than iss_mt_workers_mutations_reserve holds");
        ISS_TRY(vcf_add_item(ctx, J, record_ids[k], first_i[k], 0, n_pairs[k], cpu_numbers[k]));
        J.wbase.push_back(rows);
        J.wfds.push_back(fds[k]);
        if (n_pairs[k] > 0) rows += (uint64_t)t.mut_n[(size_t)k];
    }
    J.wbase.push_back(rows);
    if (rows == 0) return 0;
    if (rows > 0x7fffffff) return fail(ctx, ISS_E_INVALID, "iss_vcf_emit_workers: too many rows");
    if (q.fd >= 0) ISS_TRY(append_flush(ctx, q));  // (a single file's running offset ends here)
    J.mut = t.d_mut;
    J.wstride = (uint64_t)t.mut_rows;
    J.n_slots = (int64_t)rows;
    return vcf_queue(ctx, J);
}

int iss_vcf_compress(iss_ctx *ctx, int32_t mode) {
    if (!ctx) return fail(nullptr, ISS_E_INVALID, "ctx is NULL");
    return bgzt_set_mode(ctx, ctx->vq, ctx->vq.z, mode, "iss_vcf_compress");
}

int iss_vcf_flush(iss_ctx *ctx) {
    if (!ctx) return fail(nullptr, ISS_E_INVALID, "ctx is NULL");
    return append_flush(ctx, ctx->vq);
}

}  // extern "C"
