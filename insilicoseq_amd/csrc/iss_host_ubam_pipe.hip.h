// iss_host_ubam_pipe.hip.h -- what the append pipe (iss_host_pipe.hip.h) does for iss_ubam_emit_batch: a call's BGZF members
// fetched, their BSIZE chain checked, appended.
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

}  // namespace
