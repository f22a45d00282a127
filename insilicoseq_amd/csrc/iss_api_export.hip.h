// iss_api_export.hip.h -- C ABI: the output rows as dense arrays in the caller's device memory (iss_output_export, k_rows_export)
// their mutation rows likewise (iss_mutations_export, iss_truth.hip.h), and the hand-over of the context to another stream without
// a wait on the host (iss_ctx_set_stream_ordered).
#pragma once

extern "C" {

int iss_output_export(iss_ctx *ctx, int64_t first_pair, int64_t n_pairs, int32_t encoding, void *d_bases, void *d_qual,
                      int64_t *d_coords, int32_t *d_item) {
    if (!ctx || !ctx->have_model) return fail(ctx, ISS_E_INVALID, "iss_output_export: upload a model first");
    if (encoding != ISS_EXPORT_ASCII && encoding != ISS_EXPORT_CODES) return fail(ctx, ISS_E_INVALID, "iss_output_export: unknown encoding");
    if (first_pair < 0 || n_pairs < 0 || first_pair + n_pairs > ctx->os.capacity)
        return fail(ctx, ISS_E_INVALID, "iss_output_export: rows out of range");
    if (!n_pairs || (!d_bases && !d_qual && !d_coords && !d_item)) return 0;
    const iss::DevModel &M = ctx->M;
    const int tile = iss::export_tile_pairs(M.RL);
    if (tile < 1) return fail(ctx, ISS_E_INVALID, "iss_output_export: read length beyond the export kernel's tile");
    const int64_t n_tiles = (n_pairs + tile - 1) / tile;
    if (n_tiles > (int64_t)0x7fffffff) return fail(ctx, ISS_E_INVALID, "iss_output_export: too many rows for one call");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    iss::ExportArgs E{};
    E.rows = ctx->out[0] + (size_t)first_pair * (size_t)M.row;
    E.desc = ctx->os.desc + first_pair;
    E.n_pairs = n_pairs;
    E.RL = M.RL;
    E.row = M.row;
    E.tile = tile;
    E.region = iss::export_region_bytes(tile, M.RL);
    E.encoding = encoding;
    E.bases = static_cast<uint8_t *>(d_bases);
    E.qual = static_cast<uint8_t *>(d_qual);
    E.coords = d_coords;
    E.item = d_item;
    // the item table of the last iss_generate_batch call is resident: the set of device tables that call's k_setup read
    int set = -1;
    if (!ctx->last_first.empty() && ctx->batch_seq > 0 && first_pair < ctx->last_row0 + ctx->last_n && first_pair + n_pairs > ctx->last_row0) {
        set = (int)((ctx->batch_seq - 1) & 1u);
        E.items = ctx->it.d_items[set];
        E.item_first = ctx->it.d_item_first[set];
        E.n_items = (int32_t)ctx->last_first.size() - 1;
        E.rel0 = first_pair - ctx->last_row0;
        E.call_pairs = ctx->last_n;
    }
    hipLaunchKernelGGL(iss::k_rows_export, dim3((unsigned)n_tiles), dim3(iss::EXPORT_THREADS), 2 * (size_t)E.region, ctx->stream, E);
    HIP_TRY(ctx, hipGetLastError());
    // (iss_generate_batch refills a set of tables once the event of its last reader has passed: this launch is that reader now)
    if (set >= 0) HIP_TRY(ctx, hipEventRecord(ctx->it.ev_items[set], ctx->stream));
    return 0;
}

int iss_mutations_export(iss_ctx *ctx, int64_t first_pair, int64_t n_pairs, int32_t encoding, uint8_t *truth, int32_t *events,
                         int64_t capacity, int64_t *n_events) {
    if (!ctx || !ctx->have_model) return fail(ctx, ISS_E_INVALID, "iss_mutations_export: upload a model first");
    if (encoding != ISS_EXPORT_ASCII && encoding != ISS_EXPORT_CODES) return fail(ctx, ISS_E_INVALID, "iss_mutations_export: unknown encoding");
    if ((events != nullptr) != (n_events != nullptr) || capacity < 0 || capacity > ((int64_t)1 << 40))
        return fail(ctx, ISS_E_INVALID, "iss_mutations_export: events and n_events go together, with a capacity of 0 or more");
    if (!ctx->pmut.d || ctx->pmut.cap < 1) return fail(ctx, ISS_E_INVALID, "iss_mutations_export: no rows are reserved (iss_mutations_reserve)");
    if (!ctx->pmut_call || !ctx->d_pmut_count)
        return fail(ctx, ISS_E_INVALID, "iss_mutations_export: no iss_generate / iss_generate_batch call since the rows were reserved");
    if (first_pair < 0 || n_pairs < 0 || first_pair + n_pairs > ctx->os.capacity)
        return fail(ctx, ISS_E_INVALID, "iss_mutations_export: rows out of range");
    const iss::DevModel &M = ctx->M;
    const bool want_truth = truth && n_pairs;
    if (want_truth) {  // (what iss_output_export would refuse, said before anything is launched)
        const int tile = iss::export_tile_pairs(M.RL);
        if (tile < 1) return fail(ctx, ISS_E_INVALID, "iss_mutations_export: read length beyond the export kernel's tile");
        if ((n_pairs + tile - 1) / tile > (int64_t)0x7fffffff) return fail(ctx, ISS_E_INVALID, "iss_mutations_export: too many rows for one call");
    }
    if (!want_truth && !events) return 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t call_pairs = ctx->last_n;
    iss::TruthArgs T{};
    T.mut = ctx->pmut.d;
    T.count = ctx->d_pmut_count;
    T.cap = (uint32_t)ctx->pmut.cap;
    T.flags = ctx->flags + ctx->last_row0;
    T.call_pairs = call_pairs;
    T.rel0 = first_pair - ctx->last_row0;
    T.n_pairs = n_pairs;
    T.RL = M.RL;
    T.encoding = encoding;
    T.w0 = std::min(std::max<int64_t>(T.rel0, 0), call_pairs);
    T.w1 = std::min(std::max<int64_t>(T.rel0 + n_pairs, T.w0), call_pairs);
    auto grid_for = [](uint64_t n, int threads) { return dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(2048, (n + threads - 1) / threads))); };
    if (events && T.w0 < T.w1) {  // the work arrays: sized once per reservation (a larger one waits for the kernels that read the old set)
        auto &w = ctx->tw;
        const size_t n_slots = (size_t)ctx->pmut.cap;
        const size_t n_tiles = ((size_t)call_pairs + iss::VSCAN_TILE - 1) / iss::VSCAN_TILE;
        if (n_slots > w.slots_cap || (size_t)call_pairs > w.pairs_cap || n_tiles > w.tiles_cap) {
            if (w.slots_cap || w.pairs_cap) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            const size_t sc = std::max(w.slots_cap, n_slots);
            const size_t pc = std::max(w.pairs_cap, std::max((size_t)call_pairs, (size_t)ctx->os.capacity));
            const size_t tc = (pc + iss::VSCAN_TILE - 1) / iss::VSCAN_TILE + 1;
            w = {};
            DEV_ALLOC(ctx, w.d_key, sc);
            DEV_ALLOC(ctx, w.d_slot, sc);
            DEV_ALLOC(ctx, w.d_order, sc);
            DEV_ALLOC(ctx, w.d_cnt, pc);
            DEV_ALLOC(ctx, w.d_seg, pc + 1);
            DEV_ALLOC(ctx, w.d_tiles, tc);
            w.slots_cap = sc; w.pairs_cap = pc; w.tiles_cap = tc;
        }
    }
    hipStream_t st = ctx->stream;
    if (want_truth) {
        // the bases a second time, then the substitutions' ref letters over them -- behind the copy, on the same stream
        ISS_TRY(iss_output_export(ctx, first_pair, n_pairs, encoding, truth, nullptr, nullptr, nullptr));
        T.truth = truth;
        hipLaunchKernelGGL(iss::k_truth_scatter, grid_for((uint64_t)ctx->pmut.cap, iss::TRUTH_THREADS), dim3(iss::TRUTH_THREADS), 0, st, T);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (events) {
        T.events = events;
        T.capacity = capacity;
        T.n_events = n_events;
        uint64_t rows_max = 0;
        if (T.w0 < T.w1) {  // stages a and b of the VCF text (iss_vcf.hip.h) over every reserved slot: unused ones hold pair -1
            auto &w = ctx->tw;
            iss::VcfArgs A{};
            A.mut = ctx->pmut.d;
            A.n_slots = (uint32_t)ctx->pmut.cap;
            A.n_pairs = call_pairs;
            A.flags = T.flags;
            A.cnt = w.d_cnt;
            A.seg = w.d_seg;
            A.key = w.d_key;
            A.slot = w.d_slot;
            A.order = w.d_order;
            A.n_rows = w.d_seg + call_pairs;
            HIP_TRY(ctx, hipMemsetAsync(w.d_cnt, 0, (size_t)call_pairs * 4, st));
            HIP_TRY(ctx, hipMemsetAsync(w.d_order, 0, (size_t)ctx->pmut.cap * 4, st));
            const dim3 grid = grid_for((uint64_t)ctx->pmut.cap, iss::VCF_THREADS), block(iss::VCF_THREADS);
            const unsigned tiles = (unsigned)(((uint64_t)call_pairs + iss::VSCAN_TILE - 1) / iss::VSCAN_TILE);
            hipLaunchKernelGGL(iss::k_vcf_count, grid, block, 0, st, A);
            hipLaunchKernelGGL(iss::k_vcf_scan_sums, dim3(tiles), dim3(iss::VSCAN_THREADS), 0, st, (const uint32_t *)w.d_cnt, (uint64_t)call_pairs, w.d_tiles);
            hipLaunchKernelGGL(iss::k_vcf_scan_tiles, dim3(1), dim3(iss::VSCAN_THREADS), 0, st, w.d_tiles, (uint64_t)tiles, w.d_seg + call_pairs);
            hipLaunchKernelGGL(iss::k_vcf_scan_apply, dim3(tiles), dim3(iss::VSCAN_THREADS), 0, st, (const uint32_t *)w.d_cnt, (uint64_t)call_pairs,
                               (const uint64_t *)w.d_tiles, w.d_seg);
            hipLaunchKernelGGL(iss::k_vcf_scatter, grid, block, 0, st, A);
            hipLaunchKernelGGL(iss::k_vcf_rank, grid, block, 0, st, A);
            HIP_TRY(ctx, hipGetLastError());
            T.seg = w.d_seg;
            T.order = w.d_order;
            rows_max = (uint64_t)std::min<int64_t>(ctx->pmut.cap, capacity);
        }
        hipLaunchKernelGGL(iss::k_truth_events, grid_for(rows_max, iss::TRUTH_THREADS), dim3(iss::TRUTH_THREADS), 0, st, T);
        HIP_TRY(ctx, hipGetLastError());
    }
    // the flag words are this call's set: k_setup of the call after the next rewrites it once this event has passed (iss_vcf_emit)
    if (ctx->call_seq) HIP_TRY(ctx, hipEventRecord(ctx->ev_call_done[(int)((ctx->call_seq - 1) & 1u)], st));
    return 0;
}

int iss_ctx_set_stream_ordered(iss_ctx *ctx, void *hip_stream) {
    if (!ctx) return fail(nullptr, ISS_E_INVALID, "ctx is NULL");
    hipStream_t next = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    if (next == ctx->stream) return 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t queued[5] = {ctx->stream, ctx->setup_stream, ctx->indel_stream, ctx->fill_stream, ctx->emit_stream};
    for (int k = 0; k < 5; ++k) {
        if (!queued[k]) continue;
        if (!ctx->ev_handover[k]) ISS_TRY(event_create(ctx, ctx->ev_handover[k], hipEventDisableTiming));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_handover[k], queued[k]));
        HIP_TRY(ctx, hipStreamWaitEvent(next, ctx->ev_handover[k], 0));
    }
    ctx->stream = next;
    return 0;
}

}  // extern "C"
