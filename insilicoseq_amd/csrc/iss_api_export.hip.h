// iss_api_export.hip.h -- C ABI: the output rows as dense arrays in the caller's device memory (iss_output_export, k_rows_export)
// and the hand-over of the context to another stream without a wait on the host (iss_ctx_set_stream_ordered).
#pragma once

extern "C" {

int iss_output_export(iss_ctx *ctx, int64_t first_pair, int64_t n_pairs, int32_t encoding, void *d_bases, void *d_qual,
                      int64_t *d_coords, int32_t *d_item) {
    if (!ctx || !ctx->have_model) return fail(ctx, ISS_E_INVALID, "iss_output_export: upload a model first");
    if (encoding != ISS_EXPORT_ASCII && encoding != ISS_EXPORT_CODES) return fail(ctx, ISS_E_INVALID, "iss_output_export: unknown encoding");
    if (first_pair < 0 || n_pairs < 0 || first_pair + n_pairs > ctx->capacity)
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
    E.desc = ctx->desc + first_pair;
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
        E.items = ctx->d_items[set];
        E.item_first = ctx->d_item_first[set];
        E.n_items = (int32_t)ctx->last_first.size() - 1;
        E.rel0 = first_pair - ctx->last_row0;
        E.call_pairs = ctx->last_n;
    }
    hipLaunchKernelGGL(iss::k_rows_export, dim3((unsigned)n_tiles), dim3(iss::EXPORT_THREADS), 2 * (size_t)E.region, ctx->stream, E);
    HIP_TRY(ctx, hipGetLastError());
    // (iss_generate_batch refills a set of tables once the event of its last reader has passed: this launch is that reader now)
    if (set >= 0) HIP_TRY(ctx, hipEventRecord(ctx->ev_items[set], ctx->stream));
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
        if (!ctx->ev_handover[k]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_handover[k], hipEventDisableTiming));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_handover[k], queued[k]));
        HIP_TRY(ctx, hipStreamWaitEvent(next, ctx->ev_handover[k], 0));
    }
    ctx->stream = next;
    return 0;
}

}  // extern "C"
