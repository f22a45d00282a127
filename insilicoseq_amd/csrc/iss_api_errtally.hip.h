// iss_api_errtally.hip.h -- C ABI: integer tallies of the mutation rows of the last generate call, built on the device and added
// to the caller's device words (iss_error_tally_words, iss_mutations_tally; k_errtally_rows, k_errtally_reads of
// iss_errtally.hip.h).
#pragma once

extern "C" {

int64_t iss_error_tally_words(const iss_ctx *ctx) {
    if (!ctx || !ctx->have_model) return -1;
    return iss::errtally_layout(ctx->M.RL).words;
}

int iss_mutations_tally(iss_ctx *ctx, int32_t source, int64_t first_pair, int64_t n_pairs, uint64_t *d_tally) {
    if (!ctx || !ctx->have_model) return fail(ctx, ISS_E_INVALID, "iss_mutations_tally: upload a model first");
    if (source != 0 && source != 1) return fail(ctx, ISS_E_INVALID, "iss_mutations_tally: unknown source");
    const bool philox = source == 0;
    if (philox) {
        if (!ctx->pmut.d || ctx->pmut.cap < 1) return fail(ctx, ISS_E_INVALID, "iss_mutations_tally: no rows are reserved (iss_mutations_reserve)");
        if (!ctx->pmut_call || !ctx->d_pmut_count)
            return fail(ctx, ISS_E_INVALID, "iss_mutations_tally: no iss_generate / iss_generate_batch call since the rows were reserved");
    } else {
        if (!ctx->mt.d_mut || ctx->mt.mut_cap < 1) return fail(ctx, ISS_E_INVALID, "iss_mutations_tally: no rows are reserved (iss_mt_mutations_reserve)");
        if (!ctx->mt.mut_call) return fail(ctx, ISS_E_INVALID, "iss_mutations_tally: no iss_generate_mt call since the rows were reserved");
    }
    if (first_pair < 0 || n_pairs < 0 || first_pair + n_pairs > ctx->os.capacity)
        return fail(ctx, ISS_E_INVALID, "iss_mutations_tally: rows out of range");
    if (!n_pairs) return 0;
    if (!d_tally) return fail(ctx, ISS_E_INVALID, "iss_mutations_tally: d_tally is NULL");
    if (!philox && ctx->mt.mut_n > ctx->mt.mut_cap)
        return fail(ctx, ISS_E_INVALID, "iss_mutations_tally: more rows than iss_mt_mutations_reserve holds");
    // the slots a workgroup may have to walk: every one of them adds to a u32 LDS counter at most once
    const int64_t n_slots = philox ? ctx->pmut.cap : ctx->mt.mut_n;
    if (n_slots > iss::ERRTALLY_MAX_SLOTS) return fail(ctx, ISS_E_INVALID, "iss_mutations_tally: too many rows for one call");
    const iss::DevModel &M = ctx->M;
    const int64_t n_tiles = (M.RL + iss::ERRTALLY_TILE - 1) / iss::ERRTALLY_TILE;
    // slot chunks: ISS_ERRTALLY_WGS (tests: other launch geometries), else enough to fill the device, none with too little to walk
    int64_t n_chunks = std::max<int64_t>(1, std::min<int64_t>(iss::ERRTALLY_TARGET_WGS / n_tiles, (n_slots + iss::ERRTALLY_WG_SLOTS - 1) / iss::ERRTALLY_WG_SLOTS));
    if (const char *e = getenv("ISS_ERRTALLY_WGS")) n_chunks = std::max(1, atoi(e));
    n_chunks = std::min<int64_t>(n_chunks, 65535);  // (gridDim.y)
    int64_t read_per = std::min<int64_t>((n_pairs + iss::ERRTALLY_TARGET_WGS - 1) / iss::ERRTALLY_TARGET_WGS, iss::ERRTALLY_MAX_WG_PAIRS);
    read_per = (read_per + iss::ERRTALLY_THREADS - 1) / iss::ERRTALLY_THREADS * iss::ERRTALLY_THREADS;
    const int64_t read_wgs = (n_pairs + read_per - 1) / read_per;
    if (read_per > iss::ERRTALLY_MAX_WG_PAIRS || read_wgs > (int64_t)0x7fffffff)
        return fail(ctx, ISS_E_INVALID, "iss_mutations_tally: too many rows for one call");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    auto &w = ctx->ew;  // the per-read work array: sized for the output rows (a larger one waits for the kernels that read the old one)
    if ((size_t)n_pairs > w.pairs_cap) {
        if (w.d) HIP_TRY(ctx, hipStreamSynchronize(st));
        w = {};
        const size_t pc = std::max((size_t)n_pairs, (size_t)ctx->os.capacity);
        DEV_ALLOC(ctx, w.d, pc * 2);
        w.pairs_cap = pc;
    }
    iss::ErrTallyArgs T{};
    if (philox) {
        T.mut = ctx->pmut.d;
        T.count = ctx->d_pmut_count;
        T.cap = (uint32_t)ctx->pmut.cap;
        T.flags = ctx->flags + ctx->last_row0;
        T.call_pairs = ctx->last_n;
        T.rel0 = first_pair - ctx->last_row0;
    } else {
        T.mut = ctx->mt.d_mut;
        T.cap = (uint32_t)ctx->mt.mut_n;
        T.used = (uint32_t)ctx->mt.mut_n;
        T.rel0 = first_pair - ctx->mt.mut_row0;
    }
    T.n_pairs = n_pairs;
    T.RL = M.RL;
    T.read_per = read_per;
    T.reads = reinterpret_cast<unsigned long long *>(w.d.get());
    T.tally = reinterpret_cast<unsigned long long *>(d_tally);
    HIP_TRY(ctx, hipMemsetAsync(w.d, 0, (size_t)n_pairs * 2 * sizeof(uint64_t), st));
    hipLaunchKernelGGL(iss::k_errtally_rows, dim3((unsigned)n_tiles, (unsigned)n_chunks), dim3(iss::ERRTALLY_THREADS), 0, st, T);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(iss::k_errtally_reads, dim3((unsigned)read_wgs), dim3(iss::ERRTALLY_THREADS), 0, st, T);
    HIP_TRY(ctx, hipGetLastError());
    // the slots and the flag words are this call's set: k_setup of the call after the next rewrites the flags once this event has
    // passed (iss_mutations_export); the slots are cleared on this stream, behind these kernels
    if (philox && ctx->call_seq) HIP_TRY(ctx, hipEventRecord(ctx->ev_call_done[(int)((ctx->call_seq - 1) & 1u)], st));
    return 0;
}

}  // extern "C"
