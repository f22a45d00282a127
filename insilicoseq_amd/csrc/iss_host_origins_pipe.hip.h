// iss_host_origins_pipe.hip.h -- what the append pipe (iss_host_pipe.hip.h) does for iss_origins_emit_batch: a call's text fetched
// and appended.
#pragma once

namespace {

// AppendWriteFn of the origins text (a call whose text is empty copies and writes nothing)
std::string origins_write(iss_ctx *ctx, int slot, uint64_t total, int64_t at, int *code, bool *) {
    OriginsPipe &q = ctx->oq;
    if (q.z.mode) return bgzt_write(q, q.z, slot, total, at, code, "origins text");  // (iss_origins_compress: the text's BGZF members)
    if (total > q.cap) return "origins text larger than its buffer";
    if (!total) return "";
    if (hipMemcpyAsync(q.h_text[slot], q.d_text[slot], total, hipMemcpyDeviceToHost, q.data_stream) != hipSuccess ||
        hipStreamSynchronize(q.data_stream) != hipSuccess)
        return "device copy of the origins text failed";
    return pwrite_all(q.job_fd[slot], q.h_text[slot], total, at) ? std::string("write failed: ") + strerror(errno) : "";
}

}  // namespace
