// iss_host_bgzf_text.hip.h -- the BGZF stage of the two text pipes (iss_origins_compress, iss_vcf_compress; the kernels:
// iss_bgzf_text.hip.h): its buffers, the launches behind a format kernel, and what the writer thread does with a slot's members --
// fetched, their BSIZE chain walked, appended (as ubam_write does).
#pragma once

namespace {

// members of a text: its own Huffman code never needs more than 8 bits per byte plus rounding; the smoothing of the counts, the
// block headers and the members' frames are covered by the margin (a call that needs more fails, it is never cut)
size_t bgzt_comp_bytes(size_t text, size_t blocks) { return text + text / 8 + blocks * (4 * iss::BGZT_HDR_WORDS + 16 + iss::BGZF_FRAME) + 64; }
uint32_t bgzt_blocks(size_t text) { return (uint32_t)std::max<size_t>(1, (text + iss::DEFLATE_BLOCK - 1) / iss::DEFLATE_BLOCK); }

// Buffers for the members of a text of up to `text` bytes.  They grow with the pipe flushed (its file stays attached) and the
// context's stream idle: the kernels of the last call and the writer thread use them.
int bgzt_reserve(iss_ctx *ctx, AppendPipe &q, BgzfTextStage &z, size_t text) {
    if (z.d_code && text <= z.cap) return 0;
    ISS_TRY(append_flush(ctx, q, true));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    reset_part<BgzfTextBuffers>(z);
    const size_t cap = text + text / 8 + (1u << 16);
    const size_t blocks = bgzt_blocks(cap), comp_cap = bgzt_comp_bytes(cap, blocks);
    for (int sl = 0; sl < 2; ++sl) {
        DEV_ALLOC(ctx, z.d_comp[sl], comp_cap + 8);
        PIN_ALLOC(ctx, z.h_comp[sl], comp_cap);
        DEV_ALLOC(ctx, z.d_boff[sl], blocks + 1);
    }
    DEV_ALLOC(ctx, z.d_dist, cap / iss::DEFLATE_CHUNK + 1);
    DEV_ALLOC(ctx, z.d_bbytes, blocks);
    DEV_ALLOC(ctx, z.d_bcrc, blocks);
    DEV_ALLOC(ctx, z.d_hist, iss::BGZT_HIST + 5);
    DEV_ALLOC(ctx, z.d_code, 1);
    static iss::BgzfTextCode init;  // (only the CRC operators: the same for every context)
    for (int k = 0; k < 8; ++k) iss::crc_shift_operator((uint64_t)128 << k, init.crc_shift[k]);
    HIP_TRY(ctx, hipMemcpy(z.d_code, &init, sizeof init, hipMemcpyHostToDevice));
    z.cap = cap;
    z.comp_cap = comp_cap;
    z.blocks_cap = (uint32_t)blocks;
    return 0;
}

// The members of the slot's text behind its format kernel on `st`: `bound` is the host's bound of the text (<= z.cap), d_off the
// n_lines line offsets the formatter scanned, d_text_total the text's size.  That size comes back in word 2 of the slot's
// h_total; *d_total: where the members' total size stands (what append_enqueue fetches).
int bgzt_launch(iss_ctx *ctx, AppendPipe &q, BgzfTextStage &z, int slot, const uint8_t *d_text, size_t bound, const uint64_t *d_off,
                uint64_t n_lines, const uint64_t *d_text_total, hipStream_t st, const uint64_t **d_total) {
    if (bound > z.cap) return fail(ctx, ISS_E_INVALID, "BGZF stage: a text larger than the buffers reserved for it");
    const uint32_t n_blocks = bgzt_blocks(bound);
    iss::BgzfTextArgs A{};
    A.text = d_text;
    A.n_bytes = d_text_total;
    A.text_cap = bound;
    A.off = d_off;
    A.n_lines = n_lines;
    A.dist = z.d_dist;
    A.hist = z.d_hist;
    A.code = z.d_code;
    A.block_bytes = z.d_bbytes;
    A.block_crc = z.d_bcrc;
    A.block_off = z.d_boff[slot];
    A.n_blocks = n_blocks;
    A.out = z.d_comp[slot];
    A.out_cap = z.comp_cap;
    A.runs_only = getenv("ISS_DEFLATE_RUNS_ONLY") ? 1 : 0;
    iss::DeflateArgs D{};  // k_deflate_scan: the members' sizes -> their offsets
    D.n_blocks = n_blocks;
    D.block_bytes[0] = z.d_bbytes;
    D.block_off[0] = z.d_boff[slot];
    HIP_TRY(ctx, hipMemsetAsync(z.d_hist, 0, iss::BGZT_HIST * 4, st));
    HIP_TRY(ctx, hipMemsetAsync(z.d_comp[slot], 0, std::min(z.comp_cap, bgzt_comp_bytes(bound, n_blocks)) + 8, st));
    const unsigned chunk_grid = (unsigned)std::min<uint64_t>(2048, (bound / iss::DEFLATE_CHUNK + iss::DEFLATE_THREADS) / iss::DEFLATE_THREADS);
    hipLaunchKernelGGL(iss::k_bgzt_dist, dim3(chunk_grid), dim3(iss::DEFLATE_THREADS), 0, st, A);
    hipLaunchKernelGGL(iss::k_bgzt_hist, dim3(chunk_grid), dim3(iss::DEFLATE_THREADS), 0, st, A);
    hipLaunchKernelGGL(iss::k_bgzt_build, dim3(1), dim3(64), 0, st, A);
    hipLaunchKernelGGL(iss::k_bgzt_len, dim3(n_blocks), dim3(iss::DEFLATE_THREADS), 0, st, A);
    hipLaunchKernelGGL(iss::k_deflate_scan, dim3(1), dim3(1024), 0, st, D);
    hipLaunchKernelGGL(iss::k_bgzt_encode, dim3(n_blocks), dim3(iss::DEFLATE_THREADS), 0, st, A);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(q.h_total[slot] + 2, d_text_total, 8, hipMemcpyDeviceToHost, st));
    z.job_text_cap[slot] = bound;
    *d_total = z.d_boff[slot] + n_blocks;
    return 0;
}

// What the writer thread does with a slot in mode 1 (`total`: bytes of its members).  The text never reaches the host, so the
// text-mode checks of its bytes have no place here: the members' layout is checked instead.
std::string bgzt_write(AppendPipe &q, BgzfTextStage &z, int slot, uint64_t total, int64_t at, int *code, const char *noun) {
    const uint64_t text = q.h_total[slot][2];
    if (text > z.job_text_cap[slot]) return std::string(noun) + " larger than its buffer";
    if (!text && !total) return "";
    if (total > z.comp_cap) return "BGZF members larger than their buffer";
    if (hipMemcpyAsync(z.h_comp[slot], z.d_comp[slot], total, hipMemcpyDeviceToHost, q.data_stream) != hipSuccess ||
        hipStreamSynchronize(q.data_stream) != hipSuccess)
        return "device copy of the BGZF members failed";
    // invariant: the bytes are one member per 32 768 bytes of text, back to back, every BSIZE within the format's cap (a member
    // the device could not frame is left out there and breaks the chain here)
    const uint8_t *p = z.h_comp[slot];
    const uint64_t n_blocks = (text + iss::DEFLATE_BLOCK - 1) / iss::DEFLATE_BLOCK;
    uint64_t pos = 0;
    bool ok = true;
    for (uint64_t b = 0; b < n_blocks && ok; ++b) {
        ok = pos + iss::BGZF_FRAME <= total && p[pos] == 0x1f && p[pos + 1] == 0x8b && p[pos + 12] == 'B' && p[pos + 13] == 'C';
        if (ok) pos += (uint64_t)(p[pos + 16] | (p[pos + 17] << 8)) + 1u;
    }
    if (!ok || pos != total) { *code = ISS_E_INVALID; return "BGZF members do not have the layout their sizes were computed from"; }
    return pwrite_all(q.job_fd[slot], p, total, at) ? std::string("write failed: ") + strerror(errno) : "";
}

// iss_origins_compress / iss_vcf_compress: the mode of a pipe's stage, switched only while the pipe is flushed (a queued job may
// have been written already: the rule does not depend on how far the writer thread is)
int bgzt_set_mode(iss_ctx *ctx, AppendPipe &q, BgzfTextStage &z, int32_t mode, const char *who) {
    if (mode != 0 && mode != 1) return fail(ctx, ISS_E_INVALID, std::string(who) + ": mode must be 0 (text) or 1 (BGZF members)");
    if (z.mode == mode) return 0;
    if (q.unflushed) return fail(ctx, ISS_E_INVALID, std::string(who) + ": jobs were queued since the last flush (flush first)");
    z.mode = mode;
    return 0;
}

}  // namespace
