// iss_api_bamreads.hip.h -- C ABI of `report --bam`: the tally context over BAM records (iss_br_*).  The host hands over chunks of
// whole records and iss_bam_scan's offsets; each goes through pinned staging buffers to device buffers of its slot on the copy
// stream, and the kernels of iss_bamreads.hip.h follow on the kernel stream: the copy of chunk i + 1 overlaps the kernels of chunk i
// (iss_api_fqtally.hip.h).  No model, no iss_ctx.
#pragma once

struct iss_br {
    static constexpr int SLOTS = 2;
    struct Slot {
        struct Bytes {
            PinMem<uint8_t> h_pin;
            DevMem<uint8_t> d_data;
            size_t cap = 0;            // bytes of both: the chunk and the BR_PAD bytes k_br_records may read past a record's end
        } b;
        struct Offsets {
            PinMem<uint32_t> h_pin;
            DevMem<uint32_t> d_offs;
            size_t cap = 0;            // records
        } o;
        Event copied;                  // the slot's copies have landed
        Event begin;                   // in front of the kernels that read the slot,
        Event done;                    // and behind them (both timed: iss_br_kernel_ms)
        bool busy = false;             // `done` has not been waited for
    };
    int device = 0, max_len = 0;
    Stream copy_stream, stream;
    std::string last_error;
    Slot slot[SLOTS];
    int64_t feeds = 0;
    int64_t fed = 0;         // records of all feeds since the last reset: the index of the next feed's record 0
    double kernel_ms = 0.0;  // of the feeds whose slot has been collected
    struct Work {  // of the feed in flight, sized by the largest chunk
        DevMem<uint4> d_desc;
        size_t cap = 0;
    } w;
    DevMem<iss::br::BrHead> d_head;
    DevMem<unsigned long long> d_tally;  // fq_layout(max_len).words, then BrState
};

namespace {
int fail(iss_br *f, int code, const std::string &msg) {
    if (f) f->last_error = msg;
    else g_last_error = msg;
    return code;
}
}  // namespace

static_assert(iss::br::BR_MAX_LEN == ISS_BR_MAX_LEN && ISS_BR_MAX_LEN == ISS_FQ_MAX_LEN, "include/iss_mi355x.h: ISS_BR_MAX_LEN");
static_assert(iss::br::BR_REC_SHORT == ISS_BR_REC_SHORT && iss::br::BR_REC_TOO_LONG == ISS_BR_REC_TOO_LONG &&
                  iss::br::BR_REC_NO_QUAL == ISS_BR_REC_NO_QUAL && iss::br::BR_REC_QUAL_RANGE == ISS_BR_REC_QUAL_RANGE,
              "include/iss_mi355x.h: ISS_BR_REC_*");
static_assert(iss::br::BR_MAX_LEN <= (int)iss::br::BR_D_LEN, "a descriptor holds the read length in 11 bits");

// waits for the kernels that read the slot and books their time
static int br_collect(iss_br *f, iss_br::Slot &s) {
    if (!s.busy) return 0;
    HIP_TRY(f, hipEventSynchronize(s.done));
    float ms = 0.f;
    HIP_TRY(f, hipEventElapsedTime(&ms, s.begin, s.done));
    f->kernel_ms += ms;
    s.busy = false;
    return 0;
}

// room for a chunk of n_bytes and n_records in slot s and in the array of the feed in flight; waits for the device only when it has to free
static int br_reserve(iss_br *f, iss_br::Slot &s, size_t n_bytes, size_t n_records) {
    if (n_bytes + iss::br::BR_PAD > s.b.cap) {  // (the slot is idle: iss_br_feed has waited for its last kernels)
        s.b = {};
        const size_t cap = std::max(n_bytes + iss::br::BR_PAD, (size_t)1 << 20);
        PIN_ALLOC(f, s.b.h_pin, cap);
        DEV_ALLOC(f, s.b.d_data, cap);
        s.b.cap = cap;
    }
    if (n_records > s.o.cap) {
        s.o = {};
        const size_t cap = std::max(n_records, (size_t)1 << 16);
        PIN_ALLOC(f, s.o.h_pin, cap);
        DEV_ALLOC(f, s.o.d_offs, cap);
        s.o.cap = cap;
    }
    if (n_records > f->w.cap) {
        HIP_TRY(f, hipStreamSynchronize(f->stream));  // (the kernels of the chunk before use this array)
        f->w = {};
        const size_t cap = std::max(n_records, (size_t)1 << 16);
        DEV_ALLOC(f, f->w.d_desc, cap);
        f->w.cap = cap;
    }
    return 0;
}

extern "C" {

int iss_br_create(int device_ordinal, int32_t max_len, iss_br **out) {
    if (!out) return fail(nullptr, ISS_E_INVALID, "iss_br_create: out is NULL");
    *out = nullptr;
    if (max_len < 1 || max_len > ISS_BR_MAX_LEN) return fail(nullptr, ISS_E_INVALID, "iss_br_create: max_len outside 1 .. 1024");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(nullptr, ISS_E_HIP, std::string("no HIP device available: ") + hipGetErrorString(e));
    if (device_ordinal < 0 || device_ordinal >= n) return fail(nullptr, ISS_E_INVALID, "device ordinal out of range");
    iss_br *f = new iss_br();
    *out = f;
    f->device = device_ordinal;
    f->max_len = max_len;
    HIP_TRY(f, hipSetDevice(device_ordinal));
    ISS_TRY(stream_create(f, f->copy_stream, hipStreamNonBlocking));
    ISS_TRY(stream_create(f, f->stream, hipStreamNonBlocking));
    for (iss_br::Slot &s : f->slot) {
        ISS_TRY(event_create(f, s.copied, hipEventDisableTiming));
        ISS_TRY(event_create(f, s.begin, hipEventDefault));
        ISS_TRY(event_create(f, s.done, hipEventDefault));
    }
    static_assert(sizeof(iss::br::BrState) % sizeof(unsigned long long) == 0, "BrState stands behind the tally's words");
    DEV_ALLOC(f, f->d_tally, (size_t)iss::fq::fq_layout(max_len).words + sizeof(iss::br::BrState) / sizeof(unsigned long long));
    DEV_ALLOC(f, f->d_head, 1);
    return iss_br_reset(f);
}

void iss_br_destroy(iss_br *f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->copy_stream) (void)hipStreamSynchronize(f->copy_stream);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    delete f;  // (its members release the buffers, events and streams)
}

const char *iss_br_last_error(const iss_br *f) { return f ? f->last_error.c_str() : g_last_error.c_str(); }

int64_t iss_br_tally_words(const iss_br *f) { return f ? iss::fq::fq_layout(f->max_len).words : -1; }

int iss_br_reset(iss_br *f) {
    if (!f) return fail(nullptr, ISS_E_INVALID, "iss_br_reset: NULL");
    HIP_TRY(f, hipSetDevice(f->device));
    HIP_TRY(f, hipStreamSynchronize(f->copy_stream));
    const size_t words = (size_t)iss::fq::fq_layout(f->max_len).words;
    HIP_TRY(f, hipMemsetAsync(f->d_tally, 0, sizeof(unsigned long long) * words + sizeof(iss::br::BrState), f->stream));
    HIP_TRY(f, hipMemsetAsync(reinterpret_cast<uint8_t *>(f->d_tally + words) + offsetof(iss::br::BrState, bad), 0xFF,
                             sizeof(unsigned long long), f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    for (iss_br::Slot &s : f->slot) s.busy = false;
    f->fed = 0;
    f->kernel_ms = 0.0;
    return 0;
}

int iss_br_feed(iss_br *f, const uint8_t *data, int64_t n_bytes, const int64_t *offsets, int64_t n_records) {
    if (!f || n_bytes < 0 || n_records < 0 || (n_records && (!data || !offsets)))
        return fail(f, ISS_E_INVALID, "iss_br_feed: bad arguments");
    if (n_bytes >= ((int64_t)1 << 31)) return fail(f, ISS_E_INVALID, "iss_br_feed: chunks are limited to 2^31 - 1 bytes");
    if (!n_records) return 0;
    // every record must lie inside the chunk: the kernels trust these offsets (iss_bam_scan makes them, ascending)
    int64_t before = -1;
    for (int64_t r = 0; r < n_records; ++r) {
        const int64_t o = offsets[r];
        if (o < 0 || o + 4 + 32 > n_bytes) return fail(f, ISS_E_INVALID, "iss_br_feed: record offset outside the chunk");
        if (o <= before) return fail(f, ISS_E_INVALID, "iss_br_feed: record offsets do not ascend");
        int32_t bs;
        memcpy(&bs, data + o, 4);
        if (bs < 32 || o + 4 + (int64_t)bs > n_bytes) return fail(f, ISS_E_INVALID, "iss_br_feed: record outside the chunk");
        before = o;
    }
    HIP_TRY(f, hipSetDevice(f->device));
    int wgs = 0;
    if (const char *e = getenv("ISS_BR_WGS")) wgs = std::max(1, atoi(e));  // workgroups aimed at (tests: other launch geometries)
    iss_br::Slot &s = f->slot[f->feeds % iss_br::SLOTS];
    if (int rc = br_collect(f, s)) return rc;  // the one wait of a feed: the chunk that went through this slot has to be read first
    if (int rc = br_reserve(f, s, (size_t)n_bytes, (size_t)n_records)) return rc;
    memcpy(s.b.h_pin, data, (size_t)n_bytes);  // (the caller's memory is free again when the call returns)
    memset(s.b.h_pin + n_bytes, 0, iss::br::BR_PAD);
    for (int64_t r = 0; r < n_records; ++r) s.o.h_pin[r] = (uint32_t)offsets[r];
    HIP_TRY(f, hipMemcpyAsync(s.b.d_data, s.b.h_pin, (size_t)n_bytes + iss::br::BR_PAD, hipMemcpyHostToDevice, f->copy_stream));
    HIP_TRY(f, hipMemcpyAsync(s.o.d_offs, s.o.h_pin, sizeof(uint32_t) * (size_t)n_records, hipMemcpyHostToDevice, f->copy_stream));
    HIP_TRY(f, hipEventRecord(s.copied, f->copy_stream));
    HIP_TRY(f, hipStreamWaitEvent(f->stream, s.copied, 0));
    HIP_TRY(f, hipEventRecord(s.begin, f->stream));
    const iss::br::BrPlan plan = iss::br::br_plan(n_records, f->max_len, wgs);
    iss::br::BrArgs A{};
    A.data = s.b.d_data;
    A.offs = s.o.d_offs;
    A.desc = f->w.d_desc;
    A.head = f->d_head;
    A.tally = f->d_tally;
    A.state = reinterpret_cast<iss::br::BrState *>(f->d_tally + iss::fq::fq_layout(f->max_len).words);
    A.first_rec = (uint64_t)f->fed;
    A.n_bytes = (uint32_t)n_bytes;
    A.n_rec = (uint32_t)n_records;
    A.L = f->max_len;
    const dim3 threads(iss::br::BR_THREADS);
    HIP_TRY(f, hipMemsetAsync(f->d_head, 0, sizeof(iss::br::BrHead), f->stream));
    hipLaunchKernelGGL(iss::br::k_br_records, dim3(plan.rec_wgs), threads, iss::br::br_records_lds(f->max_len), f->stream, A);
    HIP_TRY(f, hipGetLastError());
    hipLaunchKernelGGL(iss::br::k_br_positions, dim3(plan.pos_tiles, plan.pos_chunks), threads, 0, f->stream, A);
    HIP_TRY(f, hipGetLastError());
    HIP_TRY(f, hipEventRecord(s.done, f->stream));
    s.busy = true;
    ++f->feeds;
    f->fed += n_records;
    return 0;
}

int iss_br_download(iss_br *f, uint64_t *tally, int64_t *records, int64_t *skipped, int64_t *bad_record, int32_t *bad_code) {
    if (!f || !tally || !records || !skipped || !bad_record || !bad_code) return fail(f, ISS_E_INVALID, "iss_br_download: bad arguments");
    HIP_TRY(f, hipSetDevice(f->device));
    const size_t words = (size_t)iss::fq::fq_layout(f->max_len).words;
    iss::br::BrState st;
    HIP_TRY(f, hipMemcpyAsync(tally, f->d_tally, sizeof(uint64_t) * words, hipMemcpyDeviceToHost, f->stream));  // (behind every kernel fed)
    HIP_TRY(f, hipMemcpyAsync(&st, f->d_tally + words, sizeof(st), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    for (int m = 0; m < 2; ++m) {
        records[m] = (int64_t)st.records[m];
        skipped[m] = (int64_t)st.skipped[m];
    }
    *bad_record = st.bad == ~0ull ? -1 : (int64_t)(st.bad >> 8);
    *bad_code = st.bad == ~0ull ? 0 : (int32_t)(st.bad & 0xFF);
    return 0;
}

int iss_br_kernel_ms(iss_br *f, double *ms) {
    if (!f || !ms) return fail(f, ISS_E_INVALID, "iss_br_kernel_ms: bad arguments");
    HIP_TRY(f, hipSetDevice(f->device));
    for (iss_br::Slot &s : f->slot)
        if (int rc = br_collect(f, s)) return rc;
    *ms = f->kernel_ms;
    return 0;
}

}  // extern "C"
