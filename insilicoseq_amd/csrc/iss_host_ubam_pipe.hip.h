// iss_host_ubam_pipe.hip.h -- the pipeline behind iss_ubam_emit_batch: writer thread (fetches a call's BGZF members once the device
// knows their size, checks the BSIZE chain, appends them with pwrite), flush, buffers.
#pragma once

namespace {

void ubam_writer_loop(iss_ctx *ctx) {
    UbamPipe &q = ctx->uq;
    (void)hipSetDevice(ctx->device);
    for (;;) {
        UbamJob job;
        int64_t at;
        {
            std::unique_lock<std::mutex> lk(q.mu);
            q.cv.wait(lk, [&] { return q.stop || !q.jobs.empty(); });
            if (q.jobs.empty()) return;
            job = q.jobs.front();
            at = q.off;  // (only this thread moves it while jobs are queued)
        }
        std::string err;
        int code = ISS_E_IO;
        uint64_t total = 0;
        if (hipEventSynchronize(q.ev_copy[job.slot]) != hipSuccess) err = "the unaligned BAM's kernels failed";
        if (err.empty()) {
            total = *q.h_total[job.slot];
            if (total > q.comp_cap) err = "BGZF members larger than their buffer";
        }
        if (err.empty() && (hipMemcpyAsync(q.h_comp[job.slot], q.d_comp[job.slot], total, hipMemcpyDeviceToHost, q.data_stream) != hipSuccess ||
                            hipStreamSynchronize(q.data_stream) != hipSuccess))
            err = "device copy of the BGZF members failed";
        if (err.empty()) {
            // invariant: the bytes are n_blocks members back to back, every BSIZE within the format's cap (a member the
            // device could not frame -- larger than 65 536 bytes -- is left out there and breaks the chain here)
            const uint8_t *p = q.h_comp[job.slot];
            uint64_t pos = 0;
            bool ok = true;
            for (uint32_t b = 0; b < job.n_blocks && ok; ++b) {
                ok = pos + iss::BGZF_FRAME <= total && p[pos] == 0x1f && p[pos + 1] == 0x8b && p[pos + 12] == 'B' && p[pos + 13] == 'C';
                if (ok) pos += (uint64_t)(p[pos + 16] | (p[pos + 17] << 8)) + 1u;
            }
            if (!ok || pos != total) { err = "BGZF members do not have the layout their sizes were computed from"; code = ISS_E_INVALID; }
            else if (pwrite_all(job.fd, p, total, at)) err = std::string("write failed: ") + strerror(errno);
        }
        {
            std::lock_guard<std::mutex> lk(q.mu);
            q.jobs.pop_front();
            q.busy[job.slot] = false;
            if (!err.empty()) { if (q.error.empty()) { q.error = err; q.error_code = code; } }
            else q.off += (int64_t)total;
        }
        q.cv.notify_all();
    }
}

// every queued byte is in the file; the descriptor stands at the end of what was written
int ubam_flush(iss_ctx *ctx, bool keep_file = false) {
    UbamPipe &q = ctx->uq;
    if (!q.ready) return 0;
    std::string err;
    int code = ISS_E_IO;
    {
        std::unique_lock<std::mutex> lk(q.mu);
        q.cv.wait(lk, [&] { return q.jobs.empty(); });
        err = q.error;
        code = q.error_code;
        q.error.clear();
    }
    if (q.fd >= 0) (void)lseek(q.fd, (off_t)q.off, SEEK_SET);
    if (!keep_file) q.fd = -1;
    if (!err.empty()) return fail(ctx, code, err);
    return 0;
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
    if (!q.ready) return;
    (void)ubam_flush(ctx);
    {
        std::lock_guard<std::mutex> lk(q.mu);
        q.stop = true;
    }
    q.cv.notify_all();
    if (q.writer.joinable()) q.writer.join();
    (void)hipStreamSynchronize(ctx->stream);
    ubam_free_buffers(ctx);
    for (int sl = 0; sl < 2; ++sl) {
        if (q.d_hist[sl]) (void)hipFree(q.d_hist[sl]);
        if (q.d_code[sl]) (void)hipFree(q.d_code[sl]);
        if (q.h_total[sl]) (void)hipHostFree(q.h_total[sl]);
        if (q.h_items[sl]) (void)hipHostFree(q.h_items[sl]);
        if (q.d_items[sl]) (void)hipFree(q.d_items[sl]);
        if (q.h_ids[sl]) (void)hipHostFree(q.h_ids[sl]);
        if (q.d_ids[sl]) (void)hipFree(q.d_ids[sl]);
        q.d_hist[sl] = nullptr;
        q.d_code[sl] = nullptr;
        q.h_total[sl] = nullptr;
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
