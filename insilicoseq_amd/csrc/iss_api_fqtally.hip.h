// iss_api_fqtally.hip.h -- C ABI of `report`: the tally context over FASTQ text (iss_fq_*).  The host hands over chunks of whole
// records; each goes through a pinned staging buffer to a device buffer of its slot on the copy stream, and the kernels of
// iss_fqtally.hip.h follow on the kernel stream: the copy of chunk i + 1 overlaps the kernels of chunk i.  No model, no iss_ctx: a
// session (iss_host_session.hip.h: open and close, the two timed slots, grown buffers, the first-bad word).
#pragma once

namespace {
struct FqWork {  // the arrays of the feed in flight, sized by the largest chunk (a group for reserve(); cap: bytes of a chunk)
    DevMem<uint32_t> d_tile_cnt, d_line_start, d_rec_len;
    size_t cap = 0;
    int alloc(iss_session *f, size_t n, const char *) {
        DEV_ALLOC(f, d_tile_cnt, n / iss::fq::FQ_TILE + 1);
        DEV_ALLOC(f, d_line_start, n + 1);  // (a chunk of '\n' bytes alone has as many lines as bytes)
        DEV_ALLOC(f, d_rec_len, n / 4 + 1);
        return 0;
    }
};
}  // namespace

struct iss_fq : iss_session {
    struct Slot : TimedSlot {
        Staged<uint8_t> text;  // the chunk: whole tiles and the 16 bytes k_fq_records may read past a line's end
    };
    int max_len = 0;
    Stream copy_stream, stream;
    Slot slot[SLOTS];
    int64_t feeds = 0;
    double kernel_ms = 0.0;  // of the feeds whose slot has been collected
    FqWork w;
    DevMem<iss::fq::FqHead> d_head;
    DevMem<unsigned long long> d_tally;  // fq_layout(max_len).words, then FqState
};

static_assert(iss::fq::FQ_MAX_LEN == ISS_FQ_MAX_LEN, "include/iss_mi355x.h: ISS_FQ_MAX_LEN");
static_assert(iss::fq::FQ_REC_NO_AT == ISS_FQ_REC_NO_AT && iss::fq::FQ_REC_NO_PLUS == ISS_FQ_REC_NO_PLUS &&
                  iss::fq::FQ_REC_LENGTHS == ISS_FQ_REC_LENGTHS && iss::fq::FQ_REC_TOO_LONG == ISS_FQ_REC_TOO_LONG &&
                  iss::fq::FQ_REC_QUAL_RANGE == ISS_FQ_REC_QUAL_RANGE && iss::fq::FQ_REC_TRUNCATED == ISS_FQ_REC_TRUNCATED,
              "include/iss_mi355x.h: ISS_FQ_REC_*");

// room for a chunk of n_bytes in slot s and in the arrays of the feed in flight; waits for the device only when it has to free
static int fq_reserve(iss_fq *f, iss_fq::Slot &s, size_t n_bytes) {
    const size_t text_need = (n_bytes + iss::fq::FQ_TILE - 1) / iss::fq::FQ_TILE * iss::fq::FQ_TILE + 16;
    // (the slot is idle: iss_fq_feed has waited for its last kernels)
    ISS_TRY(reserve(f, s.text, text_need, (size_t)1 << 20, "slot text"));
    if (n_bytes > f->w.cap) HIP_TRY(f, hipStreamSynchronize(f->stream));  // (the kernels of the chunk before use these arrays)
    return reserve(f, f->w, n_bytes, (size_t)1 << 20);
}

extern "C" {

int iss_fq_create(int device_ordinal, int32_t max_len, iss_fq **out) {
    if (!out) return fail(nullptr, ISS_E_INVALID, "iss_fq_create: out is NULL");
    *out = nullptr;
    if (max_len < 1 || max_len > ISS_FQ_MAX_LEN) return fail(nullptr, ISS_E_INVALID, "iss_fq_create: max_len outside 1 .. 1024");
    ISS_TRY(session_open(device_ordinal, out));
    iss_fq *f = *out;
    f->max_len = max_len;
    ISS_TRY(stream_create(f, f->copy_stream, hipStreamNonBlocking));
    ISS_TRY(stream_create(f, f->stream, hipStreamNonBlocking));
    for (iss_fq::Slot &s : f->slot) ISS_TRY(slot_create(f, s));
    static_assert(sizeof(iss::fq::FqState) % sizeof(unsigned long long) == 0, "FqState stands behind the tally's words");
    DEV_ALLOC(f, f->d_tally, (size_t)iss::fq::fq_layout(max_len).words + sizeof(iss::fq::FqState) / sizeof(unsigned long long));
    DEV_ALLOC(f, f->d_head, 1);
    return iss_fq_reset(f);
}

void iss_fq_destroy(iss_fq *f) {
    if (!f) return;
    session_close(f, {f->copy_stream, f->stream});
    delete f;
}

const char *iss_fq_last_error(const iss_fq *f) { return session_last_error(f); }

int64_t iss_fq_tally_words(const iss_fq *f) { return f ? iss::fq::fq_layout(f->max_len).words : -1; }

int iss_fq_reset(iss_fq *f) {
    if (!f) return fail(nullptr, ISS_E_INVALID, "iss_fq_reset: NULL");
    HIP_TRY(f, hipSetDevice(f->device));
    HIP_TRY(f, hipStreamSynchronize(f->copy_stream));
    const size_t words = (size_t)iss::fq::fq_layout(f->max_len).words;
    HIP_TRY(f, hipMemsetAsync(f->d_tally, 0, sizeof(unsigned long long) * words + sizeof(iss::fq::FqState), f->stream));
    HIP_TRY(f, hipMemsetAsync(reinterpret_cast<uint8_t *>(f->d_tally + words) + offsetof(iss::fq::FqState, bad), 0xFF,
                             sizeof(unsigned long long) * 2, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    for (iss_fq::Slot &s : f->slot) s.busy = false;
    f->kernel_ms = 0.0;
    return 0;
}

int iss_fq_feed(iss_fq *f, int32_t mate, const uint8_t *text, int64_t n_bytes) {
    if (!f || (mate != 0 && mate != 1) || n_bytes < 0 || n_bytes >= ((int64_t)1 << 31) || (n_bytes > 0 && !text))
        return fail(f, ISS_E_INVALID, "iss_fq_feed: bad arguments (mate 0 or 1, 0 <= n_bytes < 2^31, text)");
    if (!n_bytes) return 0;
    HIP_TRY(f, hipSetDevice(f->device));
    int wgs = 0;
    if (const char *e = getenv("ISS_FQTALLY_WGS")) wgs = std::max(1, atoi(e));  // workgroups aimed at (tests: other launch geometries)
    iss_fq::Slot &s = f->slot[f->feeds % SLOTS];
    ISS_TRY(slot_collect(f, s, s.done, f->kernel_ms));  // the one wait of a feed: the chunk that went through this slot has to be read first
    ISS_TRY(fq_reserve(f, s, (size_t)n_bytes));
    memcpy(s.text.h, text, (size_t)n_bytes);  // (the caller's memory is free again when the call returns)
    HIP_TRY(f, hipMemcpyAsync(s.text.d, s.text.h, (size_t)n_bytes, hipMemcpyHostToDevice, f->copy_stream));
    HIP_TRY(f, hipEventRecord(s.copied, f->copy_stream));
    HIP_TRY(f, hipStreamWaitEvent(f->stream, s.copied, 0));
    HIP_TRY(f, hipEventRecord(s.begin, f->stream));
    const iss::fq::FqPlan plan = iss::fq::fq_plan(n_bytes, f->max_len, wgs);
    iss::fq::FqArgs A{};
    A.text = s.text.d;
    A.n_bytes = (uint32_t)n_bytes;
    A.n_tiles = plan.n_tiles;
    A.tile_cnt = f->w.d_tile_cnt;
    A.line_start = f->w.d_line_start;
    A.rec_len = f->w.d_rec_len;
    A.head = f->d_head;
    A.tally = f->d_tally;
    A.state = reinterpret_cast<iss::fq::FqState *>(f->d_tally + iss::fq::fq_layout(f->max_len).words);
    A.mate = mate;
    A.L = f->max_len;
    const dim3 threads(iss::fq::FQ_THREADS);
    hipLaunchKernelGGL(iss::fq::k_fq_count, dim3(plan.n_tiles), threads, 0, f->stream, A);
    HIP_TRY(f, hipGetLastError());
    hipLaunchKernelGGL(iss::fq::k_fq_head, dim3(1), threads, 0, f->stream, A);
    HIP_TRY(f, hipGetLastError());
    hipLaunchKernelGGL(iss::fq::k_fq_lines, dim3(plan.n_tiles), threads, 0, f->stream, A);
    HIP_TRY(f, hipGetLastError());
    hipLaunchKernelGGL(iss::fq::k_fq_records, dim3(plan.rec_wgs), threads, iss::fq::fq_records_lds(f->max_len), f->stream, A);
    HIP_TRY(f, hipGetLastError());
    hipLaunchKernelGGL(iss::fq::k_fq_positions, dim3(plan.pos_tiles, plan.pos_chunks), threads, 0, f->stream, A);
    HIP_TRY(f, hipGetLastError());
    HIP_TRY(f, hipEventRecord(s.done, f->stream));
    s.busy = true;
    ++f->feeds;
    return 0;
}

int iss_fq_download(iss_fq *f, uint64_t *tally, int64_t *records, int64_t *bad_record, int32_t *bad_code) {
    if (!f || !tally || !records || !bad_record || !bad_code) return fail(f, ISS_E_INVALID, "iss_fq_download: bad arguments");
    HIP_TRY(f, hipSetDevice(f->device));
    const size_t words = (size_t)iss::fq::fq_layout(f->max_len).words;
    iss::fq::FqState st;
    HIP_TRY(f, hipMemcpyAsync(tally, f->d_tally, sizeof(uint64_t) * words, hipMemcpyDeviceToHost, f->stream));  // (behind every kernel fed)
    HIP_TRY(f, hipMemcpyAsync(&st, f->d_tally + words, sizeof(st), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    for (int m = 0; m < 2; ++m) {
        records[m] = (int64_t)st.records[m];
        bad_word_split(st.bad[m], &bad_record[m], &bad_code[m]);
    }
    return 0;
}

int iss_fq_kernel_ms(iss_fq *f, double *ms) {
    if (!f || !ms) return fail(f, ISS_E_INVALID, "iss_fq_kernel_ms: bad arguments");
    HIP_TRY(f, hipSetDevice(f->device));
    for (iss_fq::Slot &s : f->slot) ISS_TRY(slot_collect(f, s, s.done, f->kernel_ms));
    *ms = f->kernel_ms;
    return 0;
}

}  // extern "C"
