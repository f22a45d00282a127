// iss_host_pipe.hip.h -- what the device-built outputs share on the host (the records: iss_host_state.hip.h): the per-slot item
// table (SlotTable), the caller's side of a writer thread (slot wait with the pending error, stop and join) and the append pipe of
// the one-file outputs -- start, attach, enqueue, flush, stop and THE writer loop.
#pragma once

namespace {

int pwrite_all(int fd, const uint8_t *p, size_t n, int64_t off) {
    while (n) {
        const ssize_t k = pwrite(fd, p, n, (off_t)off);
        if (k < 0) { if (errno == EINTR) continue; return -1; }
        p += k; n -= (size_t)k; off += k;
    }
    return 0;
}

// A call's items and ids into a FREE slot (nothing reads its tables) and on their way to the device on `st`.
template <typename Item>
int SlotTable<Item>::stage(iss_ctx *ctx, int sl, const std::vector<Item> &items, const std::string &ids, hipStream_t st) {
    Slot &s = slot[sl];
    if (items.size() > s.items_cap || ids.size() + 1 > s.ids_cap) {
        s = {};  // (an allocation that fails below leaves an empty table, not a stale capacity)
        const size_t ic = std::max<size_t>(64, 2 * items.size()), dc = std::max<size_t>(8192, 2 * (ids.size() + 1));
        PIN_ALLOC(ctx, s.h_items, ic);
        DEV_ALLOC(ctx, s.d_items, ic);
        PIN_ALLOC(ctx, s.h_ids, dc);
        DEV_ALLOC(ctx, s.d_ids, dc);
        s.items_cap = ic;
        s.ids_cap = dc;
    }
    memcpy(s.h_items, items.data(), items.size() * sizeof(Item));
    memcpy(s.h_ids, ids.data(), ids.size());
    HIP_TRY(ctx, hipMemcpyAsync(s.d_items, s.h_items, items.size() * sizeof(Item), hipMemcpyHostToDevice, st));
    if (!ids.empty()) HIP_TRY(ctx, hipMemcpyAsync(s.d_ids, s.h_ids, ids.size(), hipMemcpyHostToDevice, st));
    return 0;
}

// The caller waits for `slot` to be free.  The writer's error reaches the caller here or at the next flush, whichever comes first,
// ONCE, with its code (ISS_E_IO unless the format said otherwise), and is then cleared.
int writer_wait_slot(iss_ctx *ctx, WriterSync &q, int slot) {
    std::unique_lock<std::mutex> lk(q.mu);
    q.cv.wait(lk, [&] { return !q.busy[slot]; });
    if (q.error.empty()) return 0;
    const std::string e = q.error;
    q.error.clear();
    return fail(ctx, q.error_code, e);
}

void writer_stop(WriterSync &q) {
    {
        std::lock_guard<std::mutex> lk(q.mu);
        q.stop = true;
    }
    q.cv.notify_all();
    if (q.writer.joinable()) q.writer.join();
}

// The one writer thread of the append pipes.  `off` is moved only here, under `mu`, while jobs are queued; a job that fails does
// not move it, and the jobs behind it still run; busy[slot] falls in the critical section that pops the job.
void append_writer_loop(iss_ctx *ctx, AppendPipe *pipe) {
    AppendPipe &q = *pipe;
    (void)hipSetDevice(ctx->device);
    for (;;) {
        int slot;
        int64_t at;
        {
            std::unique_lock<std::mutex> lk(q.mu);
            q.cv.wait(lk, [&] { return q.stop || !q.jobs.empty(); });
            if (q.jobs.empty()) return;
            slot = q.jobs.front();
            at = q.off;  // (only this thread moves it while jobs are queued)
        }
        std::string err;
        int code = ISS_E_IO;
        bool advance = true;
        uint64_t total = 0;
        // the size is behind ev_copy where it came back on the copy stream, behind ev_fmt where it rode the context's stream
        if (hipEventSynchronize(q.copy_stream ? q.ev_copy[slot] : q.ev_fmt[slot]) != hipSuccess) err = std::string("the ") + q.noun + "'s kernels failed";
        else {
            total = *q.h_total[slot];
            err = q.write(ctx, slot, total, at, &code, &advance);
        }
        {
            std::lock_guard<std::mutex> lk(q.mu);
            q.jobs.pop_front();
            q.busy[slot] = false;
            if (!err.empty()) { if (q.error.empty()) { q.error = err; q.error_code = code; } }
            else if (advance) q.off += (int64_t)total;
        }
        q.cv.notify_all();
    }
}

// lazy and idempotent: streams (with_copy_stream: the size comes back beside the context's stream), events, pinned totals, writer
int append_start(iss_ctx *ctx, AppendPipe &q, bool with_copy_stream, AppendWriteFn write, const char *noun) {
    if (q.ready) return 0;
    if (with_copy_stream) ISS_TRY(stream_create(ctx, q.copy_stream, hipStreamNonBlocking));
    ISS_TRY(stream_create(ctx, q.data_stream, hipStreamNonBlocking));
    for (auto &e : q.ev_fmt) ISS_TRY(event_create(ctx, e, hipEventDisableTiming));
    if (with_copy_stream) for (auto &e : q.ev_copy) ISS_TRY(event_create(ctx, e, hipEventDisableTiming));
    for (auto &p : q.h_total) PIN_ALLOC(ctx, p, 64 / sizeof(uint64_t));
    q.write = write;
    q.noun = noun;
    q.stop = false;
    q.writer = std::thread(append_writer_loop, ctx, &q);
    q.ready = true;
    return 0;
}

// Every queued byte is in the file; the descriptor stands at `off`, the end of what was written, and is detached unless keep_file
// (buffers are about to be reallocated in the middle of a run).  A pipe that was never started: 0, nothing touched.
int append_flush(iss_ctx *ctx, AppendPipe &q, bool keep_file = false) {
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
    q.unflushed = false;
    if (q.fd >= 0) (void)lseek(q.fd, (off_t)q.off, SEEK_SET);
    if (!keep_file) q.fd = -1;
    if (!err.empty()) return fail(ctx, code, err);
    return 0;
}

// another descriptor than the attached one: what is queued for the old one lands first, the new one is appended to where it stands
int append_attach(iss_ctx *ctx, AppendPipe &q, int fd) {
    if (q.fd == fd) return 0;
    ISS_TRY(append_flush(ctx, q));
    const off_t at = lseek(fd, 0, SEEK_CUR);
    if (at < 0) return fail(ctx, ISS_E_IO, std::string("lseek failed: ") + strerror(errno));
    q.fd = fd;
    q.off = at;
    return 0;
}

// The slot's kernels are queued on the context's stream: its size (d_total) on its way to h_total, the job to the writer.
// With a copy stream: ev_fmt, then the copy behind it on that stream, then ev_copy.  Without: the copy on the context's stream,
// then ev_fmt.
int append_enqueue(iss_ctx *ctx, AppendPipe &q, int slot, int fd, const uint64_t *d_total) {
    if (q.copy_stream) {
        HIP_TRY(ctx, hipEventRecord(q.ev_fmt[slot], ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(q.copy_stream, q.ev_fmt[slot], 0));
        HIP_TRY(ctx, hipMemcpyAsync(q.h_total[slot], d_total, 8, hipMemcpyDeviceToHost, q.copy_stream));
        HIP_TRY(ctx, hipEventRecord(q.ev_copy[slot], q.copy_stream));
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(q.h_total[slot], d_total, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(q.ev_fmt[slot], ctx->stream));
    }
    {
        std::lock_guard<std::mutex> lk(q.mu);
        q.job_fd[slot] = fd;
        q.jobs.push_back(slot);
        q.busy[slot] = true;
    }
    q.cv.notify_all();
    q.next ^= 1;
    q.unflushed = true;
    return 0;
}

// Before the context goes: flush, stop and join the writer, wait for the context's stream (the kernels of the last emit use the
// format's buffers, which the pipe's members release with the context).  A pipe that was never started: nothing to wait for.
void append_stop(iss_ctx *ctx, AppendPipe &q) {
    if (!q.ready) return;
    (void)append_flush(ctx, q);
    writer_stop(q);
    (void)hipStreamSynchronize(ctx->stream);
    q.ready = false;
}

}  // namespace
