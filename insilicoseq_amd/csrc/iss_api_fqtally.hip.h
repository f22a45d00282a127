// iss_api_fqtally.hip.h -- C ABI of `report`: the tally context over FASTQ text (iss_fq_*).  The host hands over chunks of whole
// records; each goes through a pinned staging buffer to a device buffer of its slot on the copy stream, and the kernels of
// iss_fqtally.hip.h follow on the kernel stream: the copy of chunk i + 1 overlaps the kernels of chunk i.  No model, no iss_ctx.
#pragma once

struct iss_fq {
    static constexpr int SLOTS = 2;
    struct Slot {
        struct Text {
            PinMem<uint8_t> h_pin;
            DevMem<uint8_t> d_text;
            size_t cap = 0;            // bytes of both: whole tiles and the 16 bytes k_fq_records may read past a line's end
        } t;
        Event copied;                  // the slot's copy has landed
        Event begin;                   // in front of the kernels that read the slot,
        Event done;                    // and behind them (both timed: iss_fq_kernel_ms)
        bool busy = false;             // `done` has not been waited for
    };
    int device = 0, max_len = 0;
    Stream copy_stream, stream;
    std::string last_error;
    Slot slot[SLOTS];
    int64_t feeds = 0;
    double kernel_ms = 0.0;  // of the feeds whose slot has been collected
    struct Work {  // of the feed in flight, sized by the largest chunk
        DevMem<uint32_t> d_tile_cnt, d_line_start, d_rec_len;
        size_t bytes_cap = 0;
    } w;
    DevMem<iss::fq::FqHead> d_head;
    DevMem<unsigned long long> d_tally;  // fq_layout(max_len).words, then FqState
};

namespace {
int fail(iss_fq *f, int code, const std::string &msg) {
    if (f) f->last_error = msg;
    else g_last_error = msg;
    return code;
}
}  // namespace

static_assert(iss::fq::FQ_MAX_LEN == ISS_FQ_MAX_LEN, "include/iss_mi355x.h: ISS_FQ_MAX_LEN");
static_assert(iss::fq::FQ_REC_NO_AT == ISS_FQ_REC_NO_AT && iss::fq::FQ_REC_NO_PLUS == ISS_FQ_REC_NO_PLUS &&
                  iss::fq::FQ_REC_LENGTHS == ISS_FQ_REC_LENGTHS && iss::fq::FQ_REC_TOO_LONG == ISS_FQ_REC_TOO_LONG &&
                  iss::fq::FQ_REC_QUAL_RANGE == ISS_FQ_REC_QUAL_RANGE && iss::fq::FQ_REC_TRUNCATED == ISS_FQ_REC_TRUNCATED,
              "include/iss_mi355x.h: ISS_FQ_REC_*");

// waits for the kernels that read the slot and books their time
static int fq_collect(iss_fq *f, iss_fq::Slot &s) {
    if (!s.busy) return 0;
    HIP_TRY(f, hipEventSynchronize(s.done));
    float ms = 0.f;
    HIP_TRY(f, hipEventElapsedTime(&ms, s.begin, s.done));
    f->kernel_ms += ms;
    s.busy = false;
    return 0;
}

// room for a chunk of n_bytes in slot s and in the arrays of the feed in flight; waits for the device only when it has to free
static int fq_reserve(iss_fq *f, iss_fq::Slot &s, size_t n_bytes) {
    const size_t text_need = (n_bytes + iss::fq::FQ_TILE - 1) / iss::fq::FQ_TILE * iss::fq::FQ_TILE + 16;
    if (text_need > s.t.cap) {  // (the slot is idle: iss_fq_feed has waited for its last kernels)
        s.t = {};
        const size_t cap = std::max(text_need, (size_t)1 << 20);
        PIN_ALLOC(f, s.t.h_pin, cap);
        DEV_ALLOC(f, s.t.d_text, cap);
        s.t.cap = cap;
    }
    if (n_bytes > f->w.bytes_cap) {
        HIP_TRY(f, hipStreamSynchronize(f->stream));  // (the kernels of the chunk before use these arrays)
        f->w = {};
        const size_t cap = std::max(n_bytes, (size_t)1 << 20);
        DEV_ALLOC(f, f->w.d_tile_cnt, cap / iss::fq::FQ_TILE + 1);
        DEV_ALLOC(f, f->w.d_line_start, cap + 1);  // (a chunk of '\n' bytes alone has as many lines as bytes)
        DEV_ALLOC(f, f->w.d_rec_len, cap / 4 + 1);
        f->w.bytes_cap = cap;
    }
    return 0;
}

extern "C" {

int iss_fq_create(int device_ordinal, int32_t max_len, iss_fq **out) {
    if (!out) return fail(nullptr, ISS_E_INVALID, "iss_fq_create: out is NULL");
    *out = nullptr;
    if (max_len < 1 || max_len > ISS_FQ_MAX_LEN) return fail(nullptr, ISS_E_INVALID, "iss_fq_create: max_len outside 1 .. 1024");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(nullptr, ISS_E_HIP, std::string("no HIP device available: ") + hipGetErrorString(e));
    if (device_ordinal < 0 || device_ordinal >= n) return fail(nullptr, ISS_E_INVALID, "device ordinal out of range");
    iss_fq *f = new iss_fq();
    *out = f;
    f->device = device_ordinal;
    f->max_len = max_len;
    HIP_TRY(f, hipSetDevice(device_ordinal));
    ISS_TRY(stream_create(f, f->copy_stream, hipStreamNonBlocking));
    ISS_TRY(stream_create(f, f->stream, hipStreamNonBlocking));
    for (iss_fq::Slot &s : f->slot) {
        ISS_TRY(event_create(f, s.copied, hipEventDisableTiming));
        ISS_TRY(event_create(f, s.begin, hipEventDefault));
        ISS_TRY(event_create(f, s.done, hipEventDefault));
    }
    static_assert(sizeof(iss::fq::FqState) % sizeof(unsigned long long) == 0, "FqState stands behind the tally's words");
    DEV_ALLOC(f, f->d_tally, (size_t)iss::fq::fq_layout(max_len).words + sizeof(iss::fq::FqState) / sizeof(unsigned long long));
    DEV_ALLOC(f, f->d_head, 1);
    return iss_fq_reset(f);
}

void iss_fq_destroy(iss_fq *f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->copy_stream) (void)hipStreamSynchronize(f->copy_stream);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    delete f;  // (its members release the buffers, events and streams)
}

const char *iss_fq_last_error(const iss_fq *f) { return f ? f->last_error.c_str() : g_last_error.c_str(); }

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
    iss_fq::Slot &s = f->slot[f->feeds % iss_fq::SLOTS];
    if (int rc = fq_collect(f, s)) return rc;  // the one wait of a feed: the chunk that went through this slot has to be read first
    if (int rc = fq_reserve(f, s, (size_t)n_bytes)) return rc;
    memcpy(s.t.h_pin, text, (size_t)n_bytes);  // (the caller's memory is free again when the call returns)
    HIP_TRY(f, hipMemcpyAsync(s.t.d_text, s.t.h_pin, (size_t)n_bytes, hipMemcpyHostToDevice, f->copy_stream));
    HIP_TRY(f, hipEventRecord(s.copied, f->copy_stream));
    HIP_TRY(f, hipStreamWaitEvent(f->stream, s.copied, 0));
    HIP_TRY(f, hipEventRecord(s.begin, f->stream));
    const iss::fq::FqPlan plan = iss::fq::fq_plan(n_bytes, f->max_len, wgs);
    iss::fq::FqArgs A{};
    A.text = s.t.d_text;
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
        bad_record[m] = st.bad[m] == ~0ull ? -1 : (int64_t)(st.bad[m] >> 8);
        bad_code[m] = st.bad[m] == ~0ull ? 0 : (int32_t)(st.bad[m] & 0xFF);
    }
    return 0;
}

int iss_fq_kernel_ms(iss_fq *f, double *ms) {
    if (!f || !ms) return fail(f, ISS_E_INVALID, "iss_fq_kernel_ms: bad arguments");
    HIP_TRY(f, hipSetDevice(f->device));
    for (iss_fq::Slot &s : f->slot)
        if (int rc = fq_collect(f, s)) return rc;
    *ms = f->kernel_ms;
    return 0;
}

}  // extern "C"
