// iss_api_depth.hip.h -- C ABI: per-base coverage depth of the generated reads, built on the device in the caller's device
// words (iss_depth_mark, iss_depth_finish; the kernels of iss_depth.hip.h).
#pragma once

static_assert(iss::DEPTH_TILE == ISS_DEPTH_TILE_WORDS, "the header's tile size is the kernels'");

extern "C" {

int iss_depth_mark(iss_ctx *ctx, int64_t first_pair, int64_t n_pairs, const int64_t *d_table, int32_t n_table, int32_t *d_diff) {
    if (!ctx || !ctx->have_model) return fail(ctx, ISS_E_INVALID, "iss_depth_mark: upload a model first");
    if (first_pair < 0 || n_pairs < 0 || first_pair + n_pairs > ctx->os.capacity)
        return fail(ctx, ISS_E_INVALID, "iss_depth_mark: rows out of range");
    if (!n_pairs) return 0;
    if (!d_table || !d_diff) return fail(ctx, ISS_E_INVALID, "iss_depth_mark: d_table or d_diff is NULL");
    iss::DepthMarkArgs A{};
    // the item table of the last iss_generate_batch call, found as iss_output_export finds it
    int set = -1;
    if (!ctx->last_first.empty() && ctx->batch_seq > 0 && first_pair < ctx->last_row0 + ctx->last_n && first_pair + n_pairs > ctx->last_row0) {
        set = (int)((ctx->batch_seq - 1) & 1u);
        A.items = ctx->it.d_items[set];
        A.item_first = ctx->it.d_item_first[set];
        A.n_items = (int32_t)ctx->last_first.size() - 1;
        A.rel0 = first_pair - ctx->last_row0;
        A.call_pairs = ctx->last_n;
    }
    if (n_table < (set >= 0 ? std::max(A.n_items, 1) : 1))
        return fail(ctx, ISS_E_INVALID, "iss_depth_mark: n_table is smaller than the item count of the rows' generate call");
    int wgs = 0;
    if (const char *e = getenv("ISS_DEPTH_WGS")) wgs = std::max(1, atoi(e));  // workgroups aimed at (tests: other launch geometries)
    const int64_t target = wgs > 0 ? wgs : iss::DEPTH_TARGET_WGS;
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(target, (n_pairs + iss::DEPTH_THREADS - 1) / iss::DEPTH_THREADS));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    A.desc = ctx->os.desc + first_pair;
    A.n_pairs = n_pairs;
    A.RL = ctx->M.RL;
    A.table = d_table;
    A.n_table = n_table;
    A.diff = d_diff;
    hipLaunchKernelGGL(iss::k_depth_mark, dim3((unsigned)std::min<int64_t>(grid, 0x7fffffff)), dim3(iss::DEPTH_THREADS), 0, ctx->stream, A);
    HIP_TRY(ctx, hipGetLastError());
    // (iss_generate_batch refills a set of tables once the event of its last reader has passed: this launch is that reader now)
    if (set >= 0) HIP_TRY(ctx, hipEventRecord(ctx->it.ev_items[set], ctx->stream));
    return 0;
}

int iss_depth_finish(iss_ctx *ctx, const int32_t *d_diff, int64_t n_words, uint32_t *d_depth, const int64_t *d_table, int32_t n_table,
                     int32_t bin, uint64_t *d_stats, uint64_t *d_bins) {
    if (!ctx) return fail(nullptr, ISS_E_INVALID, "ctx is NULL");
    if (n_words < 0 || n_table < 0 || bin < 0) return fail(ctx, ISS_E_INVALID, "iss_depth_finish: negative n_words, n_table or bin");
    if (bin == 0) d_bins = nullptr;
    if (n_table == 0) d_stats = nullptr, d_bins = nullptr;
    if (n_words > 0 && !d_diff) return fail(ctx, ISS_E_INVALID, "iss_depth_finish: d_diff is NULL");
    if ((d_stats || d_bins) && !d_table) return fail(ctx, ISS_E_INVALID, "iss_depth_finish: statistics or windows without d_table");
    if (!d_depth && !d_stats && !d_bins) return 0;
    int wgs = 0;
    if (const char *e = getenv("ISS_DEPTH_WGS")) wgs = std::max(1, atoi(e));
    iss::DepthPlan plan;
    if (!iss::depth_plan(std::max<int64_t>(n_words, 1), n_table, bin, wgs, &plan)) return fail(ctx, ISS_E_INVALID, "iss_depth_finish: too many words for one call");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    auto &w = ctx->dw;
    if (plan.bytes > w.cap) {  // the work array: grown behind a wait for the kernels that may still read the old one
        if (w.d) HIP_TRY(ctx, hipStreamSynchronize(st));
        w = {};
        const size_t cap = plan.bytes + plan.bytes / 4 + 4096;
        DEV_ALLOC(ctx, w.d, cap);
        w.cap = cap;
    }
    iss::DepthFinishArgs A{};
    A.diff = d_diff;
    A.n_words = n_words;
    A.depth = d_depth;
    A.table = d_table;
    A.n_table = n_table;
    A.bin = bin;
    A.stats = reinterpret_cast<unsigned long long *>(d_stats);
    A.bins = reinterpret_cast<unsigned long long *>(d_bins);
    A.tiles = reinterpret_cast<uint32_t *>(w.d.get());
    A.n_tiles = n_words > 0 ? plan.n_tiles : 0;
    A.info = reinterpret_cast<int64_t *>(w.d + plan.off_info);
    A.first = reinterpret_cast<int64_t *>(w.d + plan.off_first);
    A.idx = reinterpret_cast<int32_t *>(w.d + plan.off_idx);
    A.bins_lds = d_bins ? plan.bins_lds : 0u;
    A.vec = ((reinterpret_cast<uintptr_t>(d_diff) | reinterpret_cast<uintptr_t>(d_depth)) & 15u) == 0;
    const dim3 block(iss::DEPTH_THREADS);
    if (d_stats || d_bins) {
        hipLaunchKernelGGL(iss::k_depth_table_prep, dim3(1), block, 0, st, A);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(iss::k_depth_clear, dim3(plan.grid), block, 0, st, A);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (n_words > 0) {
        hipLaunchKernelGGL(iss::k_depth_tile_sums, dim3(plan.grid), block, 0, st, A);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(iss::k_depth_scan_tiles, dim3(1), block, 0, st, A);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(iss::k_depth_apply, dim3(plan.grid), block, (size_t)A.bins_lds * 8, st, A);
        HIP_TRY(ctx, hipGetLastError());
    }
    return 0;
}

}  // extern "C"
