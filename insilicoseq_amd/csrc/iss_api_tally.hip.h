// iss_api_tally.hip.h -- C ABI: integer tallies of the output rows, built on the device and added to the caller's device words
// (iss_tally_words, iss_output_tally; k_tally_lines, k_tally_reads of iss_tally.hip.h).
#pragma once

extern "C" {

int64_t iss_tally_words(const iss_ctx *ctx) {
    if (!ctx || !ctx->have_model) return -1;
    return iss::tally_layout(ctx->M.RL).words;
}

int iss_output_tally(iss_ctx *ctx, int64_t first_pair, int64_t n_pairs, uint64_t *d_tally) {
    if (!ctx || !ctx->have_model) return fail(ctx, ISS_E_INVALID, "iss_output_tally: upload a model first");
    if (first_pair < 0 || n_pairs < 0 || first_pair + n_pairs > ctx->os.capacity)
        return fail(ctx, ISS_E_INVALID, "iss_output_tally: rows out of range");
    if (!n_pairs) return 0;
    if (!d_tally) return fail(ctx, ISS_E_INVALID, "iss_output_tally: d_tally is NULL");
    const iss::DevModel &M = ctx->M;
    int wgs = 0;
    if (const char *e = getenv("ISS_TALLY_WGS")) wgs = std::max(1, atoi(e));  // workgroups aimed at (tests: other launch geometries)
    iss::TallyPlan plan;
    if (!iss::tally_plan(n_pairs, M.row, wgs, &plan)) return fail(ctx, ISS_E_INVALID, "iss_output_tally: too many rows for one call");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    iss::TallyArgs T{};
    T.rows = ctx->out[0] + (size_t)first_pair * (size_t)M.row;
    T.desc = ctx->os.desc + first_pair;
    T.n_pairs = n_pairs;
    T.RL = M.RL;
    T.row = M.row;
    T.chunk = plan.chunk;
    T.read_per = plan.read_per;
    T.tally = reinterpret_cast<unsigned long long *>(d_tally);
    hipLaunchKernelGGL(iss::k_tally_lines, dim3(plan.n_lines, plan.n_chunks), dim3(iss::TALLY_THREADS), 0, ctx->stream, T);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(iss::k_tally_reads, dim3(plan.read_wgs), dim3(iss::TALLY_THREADS), iss::tally_reads_lds(M.RL), ctx->stream, T);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
