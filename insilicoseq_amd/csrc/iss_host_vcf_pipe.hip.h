// iss_host_vcf_pipe.hip.h -- what the append pipe (iss_host_pipe.hip.h) does for iss_vcf_emit*: a text's check and its way into the
// file or the worker set's files, the pinned text grown by the writer thread.
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
    if (total > q.text[slot].cap) return "VCF text larger than its buffer";
    VcfPipe::HostText &host = q.host[slot];
    if (total > host.cap) {  // (pinned allocations are slow: leave room)
        host = {};
        const size_t cap = (size_t)total + (size_t)total / 4 + (1u << 20);
        if (own_alloc_quiet(host.h, cap)) return "no pinned memory for the VCF text";
        host.cap = cap;
    }
    if (!total) return "";
    if (hipMemcpyAsync(host.h, q.text[slot].d, total, hipMemcpyDeviceToHost, q.data_stream) != hipSuccess ||
        hipStreamSynchronize(q.data_stream) != hipSuccess)
        return "device copy of the VCF text failed";
    // invariant: the text is whole rows (the lengths the device summed are the bytes it wrote)
    if (host.h[total - 1] != '\n') return "VCF text does not end with a row";
    if (wfds.empty()) return pwrite_all(q.job_fd[slot], host.h, total, at) ? std::string("write failed: ") + strerror(errno) : "";
    // a worker set's text: range k behind what worker k's file holds (only this thread writes to it: the descriptor
    // stands at its end, and is left there)
    const uint64_t *wb = q.wb[slot].h + wfds.size() + 1;
    for (size_t k = 0; k < wfds.size(); ++k) {
        const uint64_t lo = wb[k], hi = wb[k + 1];
        if (lo > hi || hi > total || (k + 1 == wfds.size() && hi != total)) return "VCF text: the workers' byte ranges do not tile it";
        if (hi == lo) continue;
        const off_t end = lseek(wfds[k], 0, SEEK_CUR);
        if (end < 0 || pwrite_all(wfds[k], host.h + lo, hi - lo, (int64_t)end) || lseek(wfds[k], end + (off_t)(hi - lo), SEEK_SET) < 0)
            return std::string("write failed: ") + strerror(errno);
    }
    return "";
}

}  // namespace
