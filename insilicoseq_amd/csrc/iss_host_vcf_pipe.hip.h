// iss_host_vcf_pipe.hip.h -- what the append pipe (iss_host_pipe.hip.h) does for iss_vcf_emit*: a text's check and its way into the
// file or the worker set's files, the pinned text grown by the writer thread, buffers.
#pragma once

namespace {

// AppendWriteFn of the VCF text
std::string vcf_write(iss_ctx *ctx, int slot, uint64_t total, int64_t at, int *code, bool *advance) {
    VcfPipe &q = ctx->vq;
    const std::vector<int> &wfds = q.job_wfds[slot];
    *advance = wfds.empty();  // (a worker set's descriptors are moved as they are written)
    if (q.job_debug[slot]) {
        const uint32_t *st = reinterpret_cast<const uint32_t *>(q.h_total[slot] + 1);
        fprintf(stderr, "[vcf] slot %d: %u slots hold a row, %u rows stay, %llu bytes of text\n", slot, st[0], st[1], (unsigned long long)total);
    }
    // iss_vcf_compress: the text's BGZF members.  The text-mode check below (the trailing line feed) reads the text on the host,
    // where it never arrives in this mode; the members' BSIZE chain is walked instead.
    if (q.z.mode) return bgzt_write(q, q.z, slot, total, at, code, "VCF text");
    if (total > q.text_cap[slot]) return "VCF text larger than its buffer";
    if (total > q.h_cap[slot]) {  // (pinned allocations are slow: leave room)
        if (q.h_text[slot]) (void)hipHostFree(q.h_text[slot]);
        q.h_text[slot] = nullptr;
        q.h_cap[slot] = 0;
        const size_t cap = (size_t)total + (size_t)total / 4 + (1u << 20);
        void *v = nullptr;
        if (hipHostMalloc(&v, cap, hipHostMallocDefault) != hipSuccess) return "no pinned memory for the VCF text";
        q.h_text[slot] = static_cast<uint8_t *>(v);
        q.h_cap[slot] = cap;
    }
    if (!total) return "";
    if (hipMemcpyAsync(q.h_text[slot], q.d_text[slot], total, hipMemcpyDeviceToHost, q.data_stream) != hipSuccess ||
        hipStreamSynchronize(q.data_stream) != hipSuccess)
        return "device copy of the VCF text failed";
    // invariant: the text is whole rows (the lengths the device summed are the bytes it wrote)
    if (q.h_text[slot][total - 1] != '\n') return "VCF text does not end with a row";
    if (wfds.empty()) return pwrite_all(q.job_fd[slot], q.h_text[slot], total, at) ? std::string("write failed: ") + strerror(errno) : "";
    // a worker set's text: range k behind what worker k's file holds (only this thread writes to it: the descriptor
    // stands at its end, and is left there)
    const uint64_t *wb = q.h_wb[slot] + wfds.size() + 1;
    for (size_t k = 0; k < wfds.size(); ++k) {
        const uint64_t lo = wb[k], hi = wb[k + 1];
        if (lo > hi || hi > total || (k + 1 == wfds.size() && hi != total)) return "VCF text: the workers' byte ranges do not tile it";
        if (hi == lo) continue;
        const off_t end = lseek(wfds[k], 0, SEEK_CUR);
        if (end < 0 || pwrite_all(wfds[k], q.h_text[slot] + lo, hi - lo, (int64_t)end) || lseek(wfds[k], end + (off_t)(hi - lo), SEEK_SET) < 0)
            return std::string("write failed: ") + strerror(errno);
    }
    return "";
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
    if (!append_stop(ctx, q)) return;
    vcf_free_work(ctx);
    bgzt_free(q.z);
    q.tab.release();
    for (int sl = 0; sl < 2; ++sl) {
        if (q.d_text[sl]) (void)hipFree(q.d_text[sl]);
        if (q.h_text[sl]) (void)hipHostFree(q.h_text[sl]);
        if (q.h_wb[sl]) (void)hipHostFree(q.h_wb[sl]);
        if (q.d_wb[sl]) (void)hipFree(q.d_wb[sl]);
        q.h_wb[sl] = q.d_wb[sl] = nullptr;
        q.d_text[sl] = q.h_text[sl] = nullptr;
        q.text_cap[sl] = q.h_cap[sl] = q.wb_cap[sl] = 0;
    }
    if (q.h_count) (void)hipHostFree(q.h_count);
    if (q.d_stats) (void)hipFree(q.d_stats);
    q.d_stats = nullptr;
    q.h_count = nullptr;
}

}  // namespace
