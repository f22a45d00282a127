// iss_host_origins_pipe.hip.h -- the pipeline behind iss_origins_emit_batch: writer thread (fetches a call's text once the device
// knows its size, appends it with pwrite), flush, buffers.
#pragma once

namespace {

void origins_writer_loop(iss_ctx *ctx) {
    OriginsPipe &q = ctx->oq;
    (void)hipSetDevice(ctx->device);
    for (;;) {
        OriginsJob job;
        int64_t at;
        {
            std::unique_lock<std::mutex> lk(q.mu);
            q.cv.wait(lk, [&] { return q.stop || !q.jobs.empty(); });
            if (q.jobs.empty()) return;
            job = q.jobs.front();
            at = q.off;  // (only this thread moves it while jobs are queued)
        }
        std::string err;
        uint64_t total = 0;
        if (hipEventSynchronize(q.ev_copy[job.slot]) != hipSuccess) err = "the origins text's kernels failed";
        if (err.empty()) {
            total = *q.h_total[job.slot];
            if (total > q.cap) err = "origins text larger than its buffer";
        }
        if (err.empty() && total &&
            (hipMemcpyAsync(q.h_text[job.slot], q.d_text[job.slot], total, hipMemcpyDeviceToHost, q.data_stream) != hipSuccess ||
             hipStreamSynchronize(q.data_stream) != hipSuccess))
            err = "device copy of the origins text failed";
        if (err.empty() && total && pwrite_all(job.fd, q.h_text[job.slot], total, at)) err = std::string("write failed: ") + strerror(errno);
        {
            std::lock_guard<std::mutex> lk(q.mu);
            q.jobs.pop_front();
            q.busy[job.slot] = false;
            if (!err.empty()) { if (q.error.empty()) q.error = err; }
            else q.off += (int64_t)total;
        }
        q.cv.notify_all();
    }
}

// every queued byte is in the file; the descriptor stands at the end of what was written
int origins_flush(iss_ctx *ctx, bool keep_file = false) {
    OriginsPipe &q = ctx->oq;
    if (!q.ready) return 0;
    std::string err;
    {
        std::unique_lock<std::mutex> lk(q.mu);
        q.cv.wait(lk, [&] { return q.jobs.empty(); });
        err = q.error;
        q.error.clear();
    }
    if (q.fd >= 0) (void)lseek(q.fd, (off_t)q.off, SEEK_SET);
    if (!keep_file) q.fd = -1;
    if (!err.empty()) return fail(ctx, ISS_E_IO, err);
    return 0;
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
    if (!q.ready) return;
    (void)origins_flush(ctx);
    {
        std::lock_guard<std::mutex> lk(q.mu);
        q.stop = true;
    }
    q.cv.notify_all();
    if (q.writer.joinable()) q.writer.join();
    (void)hipStreamSynchronize(ctx->stream);
    origins_free_text(ctx);
    origins_free_work(ctx);
    for (int sl = 0; sl < 2; ++sl) {
        if (q.d_total[sl]) (void)hipFree(q.d_total[sl]);
        if (q.h_total[sl]) (void)hipHostFree(q.h_total[sl]);
        if (q.h_items[sl]) (void)hipHostFree(q.h_items[sl]);
        if (q.d_items[sl]) (void)hipFree(q.d_items[sl]);
        if (q.h_ids[sl]) (void)hipHostFree(q.h_ids[sl]);
        if (q.d_ids[sl]) (void)hipFree(q.d_ids[sl]);
        q.d_total[sl] = q.h_total[sl] = nullptr;
        q.h_items[sl] = q.d_items[sl] = nullptr;
        q.h_ids[sl] = q.d_ids[sl] = nullptr;
        q.items_cap[sl] = q.ids_cap[sl] = 0;
        if (q.ev_fmt[sl]) (void)hipEventDestroy(q.ev_fmt[sl]);
        if (q.ev_copy[sl]) (void)hipEventDestroy(q.ev_copy[sl]);
        q.ev_fmt[sl] = q.ev_copy[sl] = nullptr;
    }
    if (q.copy_stream) (void)hipStreamDestroy(q.copy_stream);
    if (q.data_stream) (void)hipStreamDestroy(q.data_stream);
    q.copy_stream = q.data_stream = nullptr;
    q.ready = false;
}

}  // namespace
