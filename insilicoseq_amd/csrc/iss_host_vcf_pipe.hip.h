// iss_host_vcf_pipe.hip.h -- the pipeline behind iss_vcf_emit: writer thread (fetches a text once the device knows its size,
// appends it with pwrite), flush, buffers.
#pragma once

namespace {

void vcf_writer_loop(iss_ctx *ctx) {
    VcfPipe &q = ctx->vq;
    (void)hipSetDevice(ctx->device);
    for (;;) {
        int slot, fd;
        int64_t at;
        std::vector<int> wfds;
        {
            std::unique_lock<std::mutex> lk(q.mu);
            q.cv.wait(lk, [&] { return q.stop || !q.jobs.empty(); });
            if (q.jobs.empty()) return;
            slot = q.jobs.front();
            fd = q.job_fd[slot];
            wfds = q.job_wfds[slot];
            at = q.off;  // (only this thread moves it while jobs are queued)
        }
        std::string err;
        uint64_t total = 0;
        if (hipEventSynchronize(q.ev_fmt[slot]) != hipSuccess) err = "the VCF text's kernels failed";
        if (err.empty()) {
            total = *q.h_total[slot];
            if (q.job_debug[slot]) {
                const uint32_t *st = reinterpret_cast<const uint32_t *>(q.h_total[slot] + 1);
                fprintf(stderr, "[vcf] slot %d: %u slots hold a row, %u rows stay, %llu bytes of text\n", slot, st[0], st[1], (unsigned long long)total);
            }
            if (total > q.text_cap[slot]) err = "VCF text larger than its buffer";
        }
        if (err.empty() && total > q.h_cap[slot]) {  // (pinned allocations are slow: leave room)
            if (q.h_text[slot]) (void)hipHostFree(q.h_text[slot]);
            q.h_text[slot] = nullptr;
            q.h_cap[slot] = 0;
            const size_t cap = (size_t)total + (size_t)total / 4 + (1u << 20);
            void *v = nullptr;
            if (hipHostMalloc(&v, cap, hipHostMallocDefault) != hipSuccess) err = "no pinned memory for the VCF text";
            else { q.h_text[slot] = static_cast<uint8_t *>(v); q.h_cap[slot] = cap; }
        }
        if (err.empty() && total) {
            if (hipMemcpyAsync(q.h_text[slot], q.d_text[slot], total, hipMemcpyDeviceToHost, q.data_stream) != hipSuccess ||
                hipStreamSynchronize(q.data_stream) != hipSuccess)
                err = "device copy of the VCF text failed";
            // invariant: the text is whole rows (the lengths the device summed are the bytes it wrote)
            else if (q.h_text[slot][total - 1] != '\n') err = "VCF text does not end with a row";
            else if (wfds.empty()) { if (pwrite_all(fd, q.h_text[slot], total, at)) err = std::string("write failed: ") + strerror(errno); }
            else {
                // a worker set's text: range k behind what worker k's file holds (only this thread writes to it: the descriptor
                // stands at its end, and is left there)
                const uint64_t *wb = q.h_wb[slot] + wfds.size() + 1;
                for (size_t k = 0; k < wfds.size() && err.empty(); ++k) {
                    const uint64_t lo = wb[k], hi = wb[k + 1];
                    if (lo > hi || hi > total || (k + 1 == wfds.size() && hi != total)) { err = "VCF text: the workers' byte ranges do not tile it"; break; }
                    if (hi == lo) continue;
                    const off_t end = lseek(wfds[k], 0, SEEK_CUR);
                    if (end < 0 || pwrite_all(wfds[k], q.h_text[slot] + lo, hi - lo, (int64_t)end) || lseek(wfds[k], end + (off_t)(hi - lo), SEEK_SET) < 0)
                        err = std::string("write failed: ") + strerror(errno);
                }
            }
        }
        {
            std::lock_guard<std::mutex> lk(q.mu);
            q.jobs.pop_front();
            q.busy[slot] = false;
            if (!err.empty()) { if (q.error.empty()) q.error = err; }
            else if (wfds.empty()) q.off += (int64_t)total;  // (a worker set's descriptors were moved as they were written)
        }
        q.cv.notify_all();
    }
}

// every queued byte is in the file; the descriptor stands at the end of what was written
int vcf_flush(iss_ctx *ctx) {
    VcfPipe &q = ctx->vq;
    if (!q.ready) return 0;
    std::string err;
    {
        std::unique_lock<std::mutex> lk(q.mu);
        q.cv.wait(lk, [&] { return q.jobs.empty(); });
        err = q.error;
        q.error.clear();
    }
    if (q.fd >= 0) (void)lseek(q.fd, (off_t)q.off, SEEK_SET);
    q.fd = -1;
    if (!err.empty()) return fail(ctx, ISS_E_IO, err);
    return 0;
}

void vcf_free_work(iss_ctx *ctx) {
    VcfPipe &q = ctx->vq;
    for (uint32_t **p : {&q.d_key, &q.d_slot, &q.d_order, &q.d_len, &q.d_cnt}) { if (*p) (void)hipFree(*p); *p = nullptr; }
    for (uint64_t **p : {&q.d_off, &q.d_seg, &q.d_tiles}) { if (*p) (void)hipFree(*p); *p = nullptr; }
    q.slots_cap = q.pairs_cap = q.tiles_cap = 0;
}

// the same arrays of iss_mutations_export (its own set: that entry shares nothing with the text's writer thread)
void truth_free_work(iss_ctx *ctx) {
    auto &w = ctx->tw;
    for (uint32_t **p : {&w.d_key, &w.d_slot, &w.d_order, &w.d_cnt}) { if (*p) (void)hipFree(*p); *p = nullptr; }
    for (uint64_t **p : {&w.d_seg, &w.d_tiles}) { if (*p) (void)hipFree(*p); *p = nullptr; }
    w.slots_cap = w.pairs_cap = w.tiles_cap = 0;
}

void vcf_shutdown(iss_ctx *ctx) {
    VcfPipe &q = ctx->vq;
    if (!q.ready) return;
    (void)vcf_flush(ctx);
    {
        std::lock_guard<std::mutex> lk(q.mu);
        q.stop = true;
    }
    q.cv.notify_all();
    if (q.writer.joinable()) q.writer.join();
    (void)hipStreamSynchronize(ctx->stream);  // (the kernels of the last emit read the work arrays)
    vcf_free_work(ctx);
    for (int sl = 0; sl < 2; ++sl) {
        if (q.d_text[sl]) (void)hipFree(q.d_text[sl]);
        if (q.h_text[sl]) (void)hipHostFree(q.h_text[sl]);
        if (q.h_total[sl]) (void)hipHostFree(q.h_total[sl]);
        if (q.h_items[sl]) (void)hipHostFree(q.h_items[sl]);
        if (q.d_items[sl]) (void)hipFree(q.d_items[sl]);
        if (q.h_ids[sl]) (void)hipHostFree(q.h_ids[sl]);
        if (q.d_ids[sl]) (void)hipFree(q.d_ids[sl]);
        if (q.h_wb[sl]) (void)hipHostFree(q.h_wb[sl]);
        if (q.d_wb[sl]) (void)hipFree(q.d_wb[sl]);
        q.h_wb[sl] = q.d_wb[sl] = nullptr;
        q.wb_cap[sl] = 0;
        q.d_text[sl] = q.h_text[sl] = nullptr;
        q.h_total[sl] = nullptr;
        q.h_items[sl] = q.d_items[sl] = nullptr;
        q.h_ids[sl] = q.d_ids[sl] = nullptr;
        q.text_cap[sl] = q.h_cap[sl] = q.items_cap[sl] = q.ids_cap[sl] = 0;
        if (q.ev_fmt[sl]) (void)hipEventDestroy(q.ev_fmt[sl]);
        q.ev_fmt[sl] = nullptr;
    }
    if (q.h_count) (void)hipHostFree(q.h_count);
    if (q.d_stats) (void)hipFree(q.d_stats);
    q.d_stats = nullptr;
    q.h_count = nullptr;
    if (q.data_stream) (void)hipStreamDestroy(q.data_stream);
    q.data_stream = nullptr;
    q.ready = false;
}

}  // namespace
