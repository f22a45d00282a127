// iss_host_origins_pipe.hip.h -- what the append pipe (iss_host_pipe.hip.h) does for iss_origins_emit_batch: a call's text fetched
// and appended; buffers.
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

void origins_free_text(iss_ctx *ctx) {
    OriginsPipe &q = ctx->oq;
    for (int sl = 0; sl < 2; ++sl) {
        if (q.d_text[sl]) (void)hipFree(q.d_text[sl]);
        if (q.h_text[sl]) (void)hipHostFree(q.h_text[sl]);
        q.d_text[sl] = q.h_text[sl] = nullptr;
    }
    q.cap = 0;
}

void origins_free_work(iss_ctx *ctx) {
    OriginsPipe &q = ctx->oq;
    if (q.d_len) (void)hipFree(q.d_len);
    if (q.d_off) (void)hipFree(q.d_off);
    if (q.d_tiles) (void)hipFree(q.d_tiles);
    q.d_len = nullptr;
    q.d_off = q.d_tiles = nullptr;
    q.pairs_cap = q.tiles_cap = 0;
}

void origins_shutdown(iss_ctx *ctx) {
    OriginsPipe &q = ctx->oq;
    if (!append_stop(ctx, q)) return;
    origins_free_text(ctx);
    origins_free_work(ctx);
    bgzt_free(q.z);
    q.tab.release();
    for (auto &p : q.d_total) { if (p) (void)hipFree(p); p = nullptr; }
}

}  // namespace
