// iss_host_ubam_pipe.hip.h -- what the append pipe (iss_host_pipe.hip.h) does for iss_ubam_emit_batch: a call's BGZF members
// fetched, their BSIZE chain checked, appended; buffers.
#pragma once

namespace {

// AppendWriteFn of the BGZF members
std::string ubam_write(iss_ctx *ctx, int slot, uint64_t total, int64_t at, int *code, bool *) {
    UbamPipe &q = ctx->uq;
    if (total > q.comp_cap) return "BGZF members larger than their buffer";
    if (hipMemcpyAsync(q.h_comp[slot], q.d_comp[slot], total, hipMemcpyDeviceToHost, q.data_stream) != hipSuccess ||
        hipStreamSynchronize(q.data_stream) != hipSuccess)
        return "device copy of the BGZF members failed";
    // invariant: the bytes are job_blocks members back to back, every BSIZE within the format's cap (a member the
    // device could not frame -- larger than 65 536 bytes -- is left out there and breaks the chain here)
    const uint8_t *p = q.h_comp[slot];
    uint64_t pos = 0;
    bool ok = true;
    for (uint32_t b = 0; b < q.job_blocks[slot] && ok; ++b) {
        ok = pos + iss::BGZF_FRAME <= total && p[pos] == 0x1f && p[pos + 1] == 0x8b && p[pos + 12] == 'B' && p[pos + 13] == 'C';
        if (ok) pos += (uint64_t)(p[pos + 16] | (p[pos + 17] << 8)) + 1u;
    }
    if (!ok || pos != total) { *code = ISS_E_INVALID; return "BGZF members do not have the layout their sizes were computed from"; }
    return pwrite_all(q.job_fd[slot], p, total, at) ? std::string("write failed: ") + strerror(errno) : "";
}

void ubam_free_buffers(iss_ctx *ctx) {
    UbamPipe &q = ctx->uq;
    for (int sl = 0; sl < 2; ++sl) {
        if (q.d_text[sl]) (void)hipFree(q.d_text[sl]);
        if (q.d_comp[sl]) (void)hipFree(q.d_comp[sl]);
        if (q.h_comp[sl]) (void)hipHostFree(q.h_comp[sl]);
        if (q.d_bbytes[sl]) (void)hipFree(q.d_bbytes[sl]);
        if (q.d_bcrc[sl]) (void)hipFree(q.d_bcrc[sl]);
        if (q.d_boff[sl]) (void)hipFree(q.d_boff[sl]);
        q.d_text[sl] = q.d_comp[sl] = q.h_comp[sl] = nullptr;
        q.d_bbytes[sl] = q.d_bcrc[sl] = nullptr;
        q.d_boff[sl] = nullptr;
    }
    q.cap = q.comp_cap = 0;
    q.blocks_cap = 0;
}

void ubam_shutdown(iss_ctx *ctx) {
    UbamPipe &q = ctx->uq;
    if (!append_stop(ctx, q)) return;
    ubam_free_buffers(ctx);
    q.tab.release();
    for (int sl = 0; sl < 2; ++sl) {
        if (q.d_hist[sl]) (void)hipFree(q.d_hist[sl]);
        if (q.d_code[sl]) (void)hipFree(q.d_code[sl]);
        q.d_hist[sl] = nullptr;
        q.d_code[sl] = nullptr;
    }
}

}  // namespace
