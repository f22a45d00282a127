// iss_api_variants.hip.h -- C ABI of `generate --variants`: iss_genome_upload_variants (a record and its
// variant tables -> the haplotype, spliced on the device and packed like any record), iss_genome_download (the resident ASCII copy),
// iss_variants_lift (haplotype coordinates -> record coordinates, on the device) and the host restatements of the two kernels from
// the same iss_variants_core.h (iss_variants_host_apply, iss_variants_host_lift: no GPU).
#pragma once

namespace {

const char *const VAR_RULES[] = {"", "a negative or empty variant", "a variant reaches past the record's end",
                                 "variants out of order or overlapping", "out_pos is not the running sum of the length changes",
                                 "letters outside their blob"};

// what every entry that takes tables checks first: nothing is launched, nothing is read through tables that fail it
int var_check_tables(iss_ctx *ctx, const char *who, int64_t L, int64_t n, const int64_t *pos0, const int32_t *ref_len,
                     const int32_t *alt_len, const int64_t *alt_off, int64_t n_alt, const int64_t *ref_off, int64_t n_ref,
                     const int64_t *out_pos) {
    int64_t bad_at = 0;
    const int rule = iss::var::var_tables_check(L, n, pos0, ref_len, alt_len, alt_off, n_alt, ref_off, n_ref, out_pos, &bad_at);
    if (!rule) return 0;
    char buf[200];
    snprintf(buf, sizeof buf, "%s: variant %lld: %s", who, (long long)bad_at, VAR_RULES[rule]);
    return fail(ctx, ISS_E_INVALID, buf);
}

}  // namespace

extern "C" {

int iss_genome_upload_variants(iss_ctx *ctx, const uint8_t *ascii, int64_t length, int64_t n, const int64_t *pos0,
                               const int32_t *ref_len, const int32_t *alt_len, const int64_t *alt_off, const uint8_t *alt, int64_t n_alt,
                               const int64_t *ref_off, const uint8_t *ref, int64_t n_ref, const int64_t *out_pos, int32_t *genome_id) {
    const char *who = "iss_genome_upload_variants";
    if (!ctx || !ascii || !genome_id || !out_pos || n < 0 || n_alt < 0 || n_ref < 0 ||
        (n && (!pos0 || !ref_len || !alt_len || !alt_off || !ref_off)) || (n_alt && !alt) || (n_ref && !ref))
        return fail(ctx, ISS_E_INVALID, std::string(who) + ": bad argument");
    if (length < 1 || length > iss::MAX_RECORD) return fail(ctx, ISS_E_INVALID, "genome length must be in [1, 2^34 - 4096]");
    ISS_TRY(var_check_tables(ctx, who, length, n, pos0, ref_len, alt_len, alt_off, n_alt, ref_off, n_ref, out_pos));
    const int64_t out_len = out_pos[n];
    if (out_len < 1 || out_len > iss::MAX_RECORD)
        return fail(ctx, ISS_E_INVALID, "haplotype length must be in [1, 2^34 - 4096]");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Genome G;  // (a return below frees what it owns so far)
    ISS_TRY(genome_alloc_owned(ctx, G, out_len));
    // the lift tables stay with the genome; the source letters, the two blobs and their offsets go when the call returns
    const size_t un = (size_t)n;
    const size_t keep_b = (un + 1) * 8 + un * 8 + un * 4 + un * 4;
    DEV_ALLOC(ctx, G.var_own, keep_b);
    uint8_t *kb = G.var_own;
    int64_t *d_out_pos = reinterpret_cast<int64_t *>(kb), *d_pos0 = d_out_pos + (un + 1);
    int32_t *d_ref_len = reinterpret_cast<int32_t *>(d_pos0 + un), *d_alt_len = d_ref_len + un;
    DevMem<uint8_t> d_src, d_alt, d_ref;
    DevMem<int64_t> d_alt_off, d_ref_off;
    DevMem<unsigned long long> d_status;
    DEV_ALLOC(ctx, d_src, (size_t)length);
    DEV_ALLOC(ctx, d_alt, (size_t)std::max<int64_t>(n_alt, 1));
    DEV_ALLOC(ctx, d_ref, (size_t)std::max<int64_t>(n_ref, 1));
    DEV_ALLOC(ctx, d_alt_off, std::max<size_t>(un, 1));
    DEV_ALLOC(ctx, d_ref_off, std::max<size_t>(un, 1));
    DEV_ALLOC(ctx, d_status, 2);
    hipStream_t st = ctx->stream;
    const unsigned long long init[2] = {0ull, (unsigned long long)n};
    hipError_t he = hipMemcpyAsync(d_src, ascii, (size_t)length, hipMemcpyHostToDevice, st);
    auto up = [&](void *d, const void *h, size_t bytes) {
        if (he == hipSuccess && bytes) he = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st);
    };
    up(d_out_pos, out_pos, (un + 1) * 8);
    up(d_pos0, pos0, un * 8);
    up(d_ref_len, ref_len, un * 4);
    up(d_alt_len, alt_len, un * 4);
    up(d_alt_off, alt_off, un * 8);
    up(d_ref_off, ref_off, un * 8);
    up(d_alt, alt, (size_t)n_alt);
    up(d_ref, ref, (size_t)n_ref);
    up(d_status, init, sizeof init);
    if (he != hipSuccess) { (void)hipStreamSynchronize(st); return fail(ctx, ISS_E_HIP, std::string(who) + ": " + hipGetErrorString(he)); }
    if (n)
        hipLaunchKernelGGL(iss::k_variant_check, dim3((unsigned)((n + iss::VAR_THREADS - 1) / iss::VAR_THREADS)), dim3(iss::VAR_THREADS), 0, st,
                           (const uint8_t *)d_src, n, (const int64_t *)d_pos0, (const int32_t *)d_ref_len, (const int64_t *)d_ref_off,
                           (const uint8_t *)d_ref, d_status.get());
    iss::VarTables T{};
    T.n = n;
    T.pos0 = d_pos0;
    T.ref_len = d_ref_len;
    T.alt_len = d_alt_len;
    T.out_pos = d_out_pos;
    T.alt_off = d_alt_off;
    T.alt = d_alt;
    const int64_t n_tiles = (out_len + iss::VAR_APPLY_TILE - 1) / iss::VAR_APPLY_TILE;  // (at most 2^22)
    hipLaunchKernelGGL(iss::k_variant_apply, dim3((unsigned)n_tiles), dim3(iss::VAR_THREADS), 0, st, (const uint8_t *)d_src, T, out_len,
                       G.ascii);
    he = hipGetLastError();
    unsigned long long chk[2] = {0, 0};
    if (he == hipSuccess) he = hipMemcpyAsync(chk, d_status, sizeof chk, hipMemcpyDeviceToHost, st);
    if (he != hipSuccess) { (void)hipStreamSynchronize(st); return fail(ctx, ISS_E_HIP, std::string(who) + ": " + hipGetErrorString(he)); }
    unsigned long long res[3];
    const int rc = genome_pack_owned(ctx, G, res);  // (waits for the stream: the staging buffers are free, chk has landed)
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    if (chk[0]) {  // one line: the POS, what the VCF says, what the record holds
        const int64_t i = (int64_t)chk[1];
        const int shown = (int)std::min<int64_t>(ref_len[i], 32);
        char buf[320];
        snprintf(buf, sizeof buf, "variant at POS %lld: its REF is %.*s%s but the record holds %.*s%s (%llu variants do not match the record)",
                 (long long)pos0[i] + 1, shown, reinterpret_cast<const char *>(ref + ref_off[i]), shown < ref_len[i] ? "..." : "", shown,
                 reinterpret_cast<const char *>(ascii + pos0[i]), shown < ref_len[i] ? "..." : "", chk[0]);
        return fail(ctx, ISS_E_INVALID, buf);
    }
    if (res[0]) {  // (the pack checks the haplotype's letters: the record's own and the ALT letters alike)
        uint8_t c = 0;
        (void)hipMemcpy(&c, G.ascii + res[1], 1, hipMemcpyDeviceToHost);
        char buf[200];
        snprintf(buf, sizeof buf, "haplotype letter 0x%02x at offset %llu is outside the rev_comp alphabet (%llu such letters; "
                 "the reference raises KeyError, iss/util.py:90)", c, res[1], res[0]);
        return fail(ctx, ISS_E_INVALID, buf);
    }
    G.has_exceptions = res[2] != 0;
    G.var_n = n;
    G.var_out_pos = d_out_pos;
    G.var_pos0 = d_pos0;
    G.var_ref_len = d_ref_len;
    G.var_alt_len = d_alt_len;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_inputs, ctx->stream));
    ctx->inputs_pending = true;
    ctx->genomes.push_back(std::move(G));
    *genome_id = (int32_t)ctx->genomes.size() - 1;
    return 0;
}

int iss_genome_download(iss_ctx *ctx, int32_t genome_id, uint8_t *ascii, int64_t capacity, int64_t *length) {
    if (!ctx || genome_id < 0 || (size_t)genome_id >= ctx->genomes.size() || capacity < 0 || (capacity && !ascii))
        return fail(ctx, ISS_E_INVALID, "iss_genome_download: bad argument");
    const Genome &G = ctx->genomes[(size_t)genome_id];
    if (length) *length = G.L;
    if (!ascii) return 0;  // (the length alone)
    if (capacity < G.L) return fail(ctx, ISS_E_INVALID, "iss_genome_download: the buffer is shorter than the record");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (an upload's copies and kernels run on it)
    HIP_TRY(ctx, hipMemcpy(ascii, G.ascii, (size_t)G.L, hipMemcpyDeviceToHost));
    return 0;
}

int iss_variants_lift(iss_ctx *ctx, const int32_t *d_gid, int32_t gid, const int64_t *d_in, int64_t n, int64_t *d_out) {
    if (!ctx || n < 0 || (n && (!d_in || !d_out))) return fail(ctx, ISS_E_INVALID, "iss_variants_lift: bad argument");
    if (!d_gid && (gid < 0 || (size_t)gid >= ctx->genomes.size())) return fail(ctx, ISS_E_INVALID, "iss_variants_lift: no such genome");
    if (n == 0) return 0;
    if ((n + iss::VAR_THREADS - 1) / iss::VAR_THREADS > (int64_t)0x7fffffff) return fail(ctx, ISS_E_INVALID, "iss_variants_lift: too many coordinates for one call");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->vl.n != ctx->genomes.size() || !ctx->vl.d_tabs) {  // genomes have come since the table was made (a clear empties it)
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (a lift queued earlier may read the old table)
        std::vector<iss::VarLiftTab> tabs(ctx->genomes.size());
        for (size_t g = 0; g < tabs.size(); ++g) {
            const Genome &G = ctx->genomes[g];
            tabs[g] = iss::VarLiftTab{G.var_n, G.var_pos0, G.var_ref_len, G.var_alt_len, G.var_out_pos};
        }
        DEV_ALLOC(ctx, ctx->vl.d_tabs, std::max<size_t>(tabs.size(), 1));
        if (!tabs.empty()) HIP_TRY(ctx, hipMemcpy(ctx->vl.d_tabs, tabs.data(), tabs.size() * sizeof(iss::VarLiftTab), hipMemcpyHostToDevice));
        ctx->vl.n = tabs.size();
    }
    hipLaunchKernelGGL(iss::k_variant_lift, dim3((unsigned)((n + iss::VAR_THREADS - 1) / iss::VAR_THREADS)), dim3(iss::VAR_THREADS), 0, ctx->stream,
                       (const iss::VarLiftTab *)ctx->vl.d_tabs, (int32_t)ctx->vl.n, d_gid, gid, d_in, n, d_out);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

int iss_variants_apply_tile(void) { return (int)iss::VAR_APPLY_TILE; }

int iss_variants_host_apply(const uint8_t *ascii, int64_t length, int64_t n, const int64_t *pos0, const int32_t *ref_len,
                            const int32_t *alt_len, const int64_t *alt_off, const uint8_t *alt, int64_t n_alt, const int64_t *out_pos,
                            uint8_t *out, int64_t capacity) {
    if (!ascii || !out_pos || length < 0 || n < 0 || n_alt < 0 || (n && (!pos0 || !ref_len || !alt_len || !alt_off)) || (n_alt && !alt))
        return fail(nullptr, ISS_E_INVALID, "iss_variants_host_apply: bad argument");
    ISS_TRY(var_check_tables(nullptr, "iss_variants_host_apply", length, n, pos0, ref_len, alt_len, alt_off, n_alt, nullptr, 0, out_pos));
    const int64_t out_len = out_pos[n];
    if (out_len > capacity || (out_len && !out)) return fail(nullptr, ISS_E_INVALID, "iss_variants_host_apply: the buffer is shorter than the haplotype");
    // tile by tile like the kernel: the tile's variant by search, then forward
    for (int64_t tile0 = 0; tile0 < out_len; tile0 += iss::VAR_APPLY_TILE) {
        int64_t i = iss::var::var_find(out_pos, n, tile0);
        const int64_t end = std::min(out_len, tile0 + iss::VAR_APPLY_TILE);
        for (int64_t o = tile0; o < end; ++o) {
            while (i + 1 < n && out_pos[i + 1] <= o) ++i;
            bool from_alt = false;
            const int64_t at = iss::var::var_source(o, i, pos0, ref_len, alt_len, alt_off, out_pos, &from_alt);
            out[o] = from_alt ? alt[at] : ascii[at];
        }
    }
    return 0;
}

int iss_variants_host_lift(int64_t n, const int64_t *pos0, const int32_t *ref_len, const int32_t *alt_len, const int64_t *out_pos,
                           const int64_t *in, int64_t n_coords, int64_t *out) {
    if (n < 0 || n_coords < 0 || !out_pos || (n && (!pos0 || !ref_len || !alt_len)) || (n_coords && (!in || !out)))
        return fail(nullptr, ISS_E_INVALID, "iss_variants_host_lift: bad argument");
    for (int64_t t = 0; t < n_coords; ++t) out[t] = iss::var::var_lift(in[t], n, pos0, ref_len, alt_len, out_pos);
    return 0;
}

}  // extern "C"
