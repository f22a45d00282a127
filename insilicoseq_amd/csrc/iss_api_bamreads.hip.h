// iss_api_bamreads.hip.h -- C ABI of `report --bam`: the tally context over BAM records (iss_br_*).  The host hands over chunks of
// whole records and iss_bam_scan's offsets; each goes through pinned staging buffers to device buffers of its slot on the copy
// stream, and the kernels of iss_bamreads.hip.h follow on the kernel stream: the copy of chunk i + 1 overlaps the kernels of chunk i.
// No model, no iss_ctx: a session (iss_host_session.hip.h: open and close, the two timed slots, grown buffers, the first-bad word).
// With iss_br_errors_enable a third stage follows in every feed: the alignments' errors (iss_bamerrors.hip.h), words of their own.
// With iss_br_depth_enable a fourth: the alignments' reference intervals marked into the caller's difference array (iss_bamdepth.hip.h).
#pragma once

struct iss_br : iss_session {
    struct Slot : TimedSlot {
        Staged<uint8_t> bytes;   // the chunk and the BR_PAD bytes k_br_records may read past a record's end
        Staged<uint32_t> offs;   // per record
    };
    int max_len = 0;
    Stream copy_stream, stream;
    Slot slot[SLOTS];
    int64_t feeds = 0;
    int64_t fed = 0;         // records of all feeds since the last reset: the index of the next feed's record 0
    double kernel_ms = 0.0;  // of the feeds whose slot has been collected
    Grown<DevMem<uint4>> desc;  // per record of the feed in flight, sized by the largest chunk
    DevMem<iss::br::BrHead> d_head;
    DevMem<unsigned long long> d_tally;  // fq_layout(max_len).words, then BrState
    bool errors = false;                 // iss_br_errors_enable: every feed also runs k_be_records and k_be_bases
    DevMem<unsigned long long> d_err;    // be_words(max_len), then BeState
    Grown<DevMem<unsigned long long>> marks;  // [records][ceil(max_len / 64)] of the feed in flight: k_be_records' aligned columns
    bool depth = false;                  // iss_br_depth_enable: every feed also runs k_bd_records
    DevMem<iss::bd::BdState> d_depth;    // its counts and first-bad word
    const int64_t *depth_table = nullptr;  // the caller's device memory, both: nothing but the pointers is kept
    int32_t *depth_diff = nullptr;
    int32_t depth_n_table = 0;
    uint32_t depth_flags = 0, depth_min_mapq = 0;
};

static_assert(iss::br::BR_MAX_LEN == ISS_BR_MAX_LEN && ISS_BR_MAX_LEN == ISS_FQ_MAX_LEN, "include/iss_mi355x.h: ISS_BR_MAX_LEN");
static_assert(iss::br::BR_REC_SHORT == ISS_BR_REC_SHORT && iss::br::BR_REC_TOO_LONG == ISS_BR_REC_TOO_LONG &&
                  iss::br::BR_REC_NO_QUAL == ISS_BR_REC_NO_QUAL && iss::br::BR_REC_QUAL_RANGE == ISS_BR_REC_QUAL_RANGE,
              "include/iss_mi355x.h: ISS_BR_REC_*");
static_assert(iss::br::BR_MAX_LEN <= (int)iss::br::BR_D_LEN, "a descriptor holds the read length in 11 bits");
static_assert(iss::be::BE_ALN_CIGAR == ISS_BR_ALN_CIGAR && iss::be::BE_ALN_TAGS == ISS_BR_ALN_TAGS && iss::be::BE_ALN_MD == ISS_BR_ALN_MD,
              "include/iss_mi355x.h: ISS_BR_ALN_*");
static_assert(sizeof(iss::be::BeState) % sizeof(unsigned long long) == 0, "BeState stands behind the error words");
static_assert(iss::bd::BD_CIGAR == ISS_BR_DEPTH_CIGAR && iss::bd::BD_REF == ISS_BR_DEPTH_REF && iss::bd::BD_SPAN == ISS_BR_DEPTH_SPAN &&
                  iss::bd::BD_COUNT_DEL == ISS_BR_DEPTH_COUNT_DEL,
              "include/iss_mi355x.h: ISS_BR_DEPTH_*");

// room for a chunk of n_bytes and n_records in slot s and in the array of the feed in flight; waits for the device only when it has to free
static int br_reserve(iss_br *f, iss_br::Slot &s, size_t n_bytes, size_t n_records) {
    // (the slot is idle: iss_br_feed has waited for its last kernels)
    ISS_TRY(reserve(f, s.bytes, n_bytes + iss::br::BR_PAD, (size_t)1 << 20, "slot bytes"));
    ISS_TRY(reserve(f, s.offs, n_records, (size_t)1 << 16, "slot offsets"));
    if (n_records > f->desc.cap) HIP_TRY(f, hipStreamSynchronize(f->stream));  // (the kernels of the chunk before use this array)
    ISS_TRY(reserve(f, f->desc, n_records, (size_t)1 << 16, "descriptors"));
    if (!f->errors) return 0;
    const size_t marks = n_records * (size_t)((f->max_len + 63) / 64);
    if (marks > f->marks.cap) HIP_TRY(f, hipStreamSynchronize(f->stream));  // (likewise)
    return reserve(f, f->marks, marks, (size_t)1 << 16, "aligned-column marks");
}

// the error words and their state zeroed, the first-bad word all ones (on the kernel stream; the caller waits)
static int br_errors_clear(iss_br *f) {
    const size_t words = sizeof(unsigned long long) * (size_t)iss::be::be_words(f->max_len);
    return bad_state_clear(f, f->stream, f->d_err, words + sizeof(iss::be::BeState), words + offsetof(iss::be::BeState, bad));
}

// the depth stage's counts zeroed, its first-bad word all ones (on the kernel stream; the caller waits)
static int br_depth_clear(iss_br *f) {
    return bad_state_clear(f, f->stream, f->d_depth, sizeof(iss::bd::BdState), offsetof(iss::bd::BdState, bad));
}

extern "C" {

int iss_br_create(int device_ordinal, int32_t max_len, iss_br **out) {
    if (!out) return fail(nullptr, ISS_E_INVALID, "iss_br_create: out is NULL");
    *out = nullptr;
    if (max_len < 1 || max_len > ISS_BR_MAX_LEN) return fail(nullptr, ISS_E_INVALID, "iss_br_create: max_len outside 1 .. 1024");
    ISS_TRY(session_open(device_ordinal, out));
    iss_br *f = *out;
    f->max_len = max_len;
    ISS_TRY(stream_create(f, f->copy_stream, hipStreamNonBlocking));
    ISS_TRY(stream_create(f, f->stream, hipStreamNonBlocking));
    for (iss_br::Slot &s : f->slot) ISS_TRY(slot_create(f, s));
    static_assert(sizeof(iss::br::BrState) % sizeof(unsigned long long) == 0, "BrState stands behind the tally's words");
    DEV_ALLOC(f, f->d_tally, (size_t)iss::fq::fq_layout(max_len).words + sizeof(iss::br::BrState) / sizeof(unsigned long long));
    DEV_ALLOC(f, f->d_head, 1);
    return iss_br_reset(f);
}

void iss_br_destroy(iss_br *f) {
    if (!f) return;
    session_close(f, {f->copy_stream, f->stream});
    delete f;
}

const char *iss_br_last_error(const iss_br *f) { return session_last_error(f); }

int64_t iss_br_tally_words(const iss_br *f) { return f ? iss::fq::fq_layout(f->max_len).words : -1; }

int iss_br_reset(iss_br *f) {
    if (!f) return fail(nullptr, ISS_E_INVALID, "iss_br_reset: NULL");
    HIP_TRY(f, hipSetDevice(f->device));
    HIP_TRY(f, hipStreamSynchronize(f->copy_stream));
    const size_t words = sizeof(unsigned long long) * (size_t)iss::fq::fq_layout(f->max_len).words;
    ISS_TRY(bad_state_clear(f, f->stream, f->d_tally, words + sizeof(iss::br::BrState), words + offsetof(iss::br::BrState, bad)));
    if (f->errors) ISS_TRY(br_errors_clear(f));
    if (f->depth) ISS_TRY(br_depth_clear(f));  // (the caller's array stays as it is, and the stage on)
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
    if (f->depth && n_records > (int64_t)0x7fffffff - f->fed)  // (a record adds at most 1 to a base: the depths stay below 2^31)
        return fail(f, ISS_E_INVALID, "iss_br_feed: more than 2^31 - 1 records fed while the depth stage is on");
    ISS_TRY(records_inside(f, "iss_br_feed", data, n_bytes, offsets, n_records, true));
    HIP_TRY(f, hipSetDevice(f->device));
    int wgs = 0;
    if (const char *e = getenv("ISS_BR_WGS")) wgs = std::max(1, atoi(e));  // workgroups aimed at (tests: other launch geometries)
    iss_br::Slot &s = f->slot[f->feeds % SLOTS];
    ISS_TRY(slot_collect(f, s, s.done, f->kernel_ms));  // the one wait of a feed: the chunk that went through this slot has to be read first
    ISS_TRY(br_reserve(f, s, (size_t)n_bytes, (size_t)n_records));
    memcpy(s.bytes.h, data, (size_t)n_bytes);  // (the caller's memory is free again when the call returns)
    memset(s.bytes.h + n_bytes, 0, iss::br::BR_PAD);
    for (int64_t r = 0; r < n_records; ++r) s.offs.h[r] = (uint32_t)offsets[r];
    HIP_TRY(f, hipMemcpyAsync(s.bytes.d, s.bytes.h, (size_t)n_bytes + iss::br::BR_PAD, hipMemcpyHostToDevice, f->copy_stream));
    HIP_TRY(f, hipMemcpyAsync(s.offs.d, s.offs.h, sizeof(uint32_t) * (size_t)n_records, hipMemcpyHostToDevice, f->copy_stream));
    HIP_TRY(f, hipEventRecord(s.copied, f->copy_stream));
    HIP_TRY(f, hipStreamWaitEvent(f->stream, s.copied, 0));
    HIP_TRY(f, hipEventRecord(s.begin, f->stream));
    const iss::br::BrPlan plan = iss::br::br_plan(n_records, f->max_len, wgs);
    iss::br::BrArgs A{};
    A.data = s.bytes.d;
    A.offs = s.offs.d;
    A.desc = f->desc.p;
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
    if (f->errors) {
        iss::be::BeArgs E{};
        E.R = A;
        E.err = f->d_err;
        E.state = reinterpret_cast<iss::be::BeState *>(f->d_err + iss::be::be_words(f->max_len));
        E.mask = f->marks.p;
        E.tiles = plan.pos_tiles;
        const uint32_t record_wgs = iss::br::wave_record_wgs(n_records, wgs);
        E.rounds = iss::be::be_record_rounds(n_records, record_wgs);
        hipLaunchKernelGGL(iss::be::k_be_records, dim3(record_wgs), threads, 0, f->stream, E);
        HIP_TRY(f, hipGetLastError());
        hipLaunchKernelGGL(iss::be::k_be_bases, dim3(plan.pos_tiles, plan.pos_chunks), threads, 0, f->stream, E);
        HIP_TRY(f, hipGetLastError());
    }
    if (f->depth) {
        iss::bd::BdArgs D{};
        D.R = A;
        D.table = f->depth_table;
        D.diff = f->depth_diff;
        D.state = f->d_depth;
        D.n_table = f->depth_n_table;
        D.flags = f->depth_flags;
        D.min_mapq = f->depth_min_mapq;
        hipLaunchKernelGGL(iss::bd::k_bd_records, dim3(iss::br::wave_record_wgs(n_records, wgs)), threads, 0, f->stream, D);
        HIP_TRY(f, hipGetLastError());
    }
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
    bad_word_split(st.bad, bad_record, bad_code);
    return 0;
}

int iss_br_errors_enable(iss_br *f) {
    if (!f) return fail(nullptr, ISS_E_INVALID, "iss_br_errors_enable: NULL");
    if (f->fed) return fail(f, ISS_E_INVALID, "iss_br_errors_enable: records have been fed since the last reset");
    if (f->errors) return 0;
    HIP_TRY(f, hipSetDevice(f->device));
    DEV_ALLOC(f, f->d_err, (size_t)iss::be::be_words(f->max_len) + sizeof(iss::be::BeState) / sizeof(unsigned long long));
    ISS_TRY(br_errors_clear(f));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    f->errors = true;
    return 0;
}

int64_t iss_br_error_words(const iss_br *f) { return f && f->errors ? iss::be::be_words(f->max_len) : -1; }

int iss_br_errors_download(iss_br *f, uint64_t *words, int64_t *counts, int64_t *bad_record, int32_t *bad_code) {
    if (!f || !words || !counts || !bad_record || !bad_code) return fail(f, ISS_E_INVALID, "iss_br_errors_download: bad arguments");
    if (!f->errors) return fail(f, ISS_E_INVALID, "iss_br_errors_download: errors are not enabled");
    HIP_TRY(f, hipSetDevice(f->device));
    const size_t n = (size_t)iss::be::be_words(f->max_len);
    iss::be::BeState st;
    HIP_TRY(f, hipMemcpyAsync(words, f->d_err, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, f->stream));  // (behind every kernel fed)
    HIP_TRY(f, hipMemcpyAsync(&st, f->d_err + n, sizeof(st), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    for (int k = 0; k < 4; ++k) counts[k] = (int64_t)st.counts[k];
    bad_word_split(st.bad, bad_record, bad_code);
    return 0;
}

int iss_br_depth_enable(iss_br *f, const int64_t *d_table, int32_t n_table, int32_t *d_diff, uint32_t flags, int32_t min_mapq) {
    if (!f) return fail(nullptr, ISS_E_INVALID, "iss_br_depth_enable: NULL");
    if (f->fed) return fail(f, ISS_E_INVALID, "iss_br_depth_enable: records have been fed since the last reset");
    if (!d_table || !d_diff || n_table < 1) return fail(f, ISS_E_INVALID, "iss_br_depth_enable: no table or no difference array");
    if (flags & ~(uint32_t)ISS_BR_DEPTH_COUNT_DEL) return fail(f, ISS_E_INVALID, "iss_br_depth_enable: unknown flag bits");
    if (min_mapq < 0 || min_mapq > 255) return fail(f, ISS_E_INVALID, "iss_br_depth_enable: min_mapq outside 0 .. 255");
    if (reinterpret_cast<uintptr_t>(d_diff) % sizeof(int32_t) || reinterpret_cast<uintptr_t>(d_table) % sizeof(int64_t))
        return fail(f, ISS_E_INVALID, "iss_br_depth_enable: misaligned table or difference array");
    HIP_TRY(f, hipSetDevice(f->device));
    if (!f->d_depth) DEV_ALLOC(f, f->d_depth, 1);
    ISS_TRY(br_depth_clear(f));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    f->depth_table = d_table;
    f->depth_diff = d_diff;
    f->depth_n_table = n_table;
    f->depth_flags = flags;
    f->depth_min_mapq = (uint32_t)min_mapq;
    f->depth = true;
    return 0;
}

int iss_br_depth_download(iss_br *f, int64_t *counts, int64_t *bad_record, int32_t *bad_code) {
    if (!f || !counts || !bad_record || !bad_code) return fail(f, ISS_E_INVALID, "iss_br_depth_download: bad arguments");
    if (!f->depth) return fail(f, ISS_E_INVALID, "iss_br_depth_download: the depth stage is not enabled");
    HIP_TRY(f, hipSetDevice(f->device));
    iss::bd::BdState st;
    HIP_TRY(f, hipMemcpyAsync(&st, f->d_depth, sizeof(st), hipMemcpyDeviceToHost, f->stream));  // (behind every kernel fed)
    HIP_TRY(f, hipStreamSynchronize(f->stream));  // (the caller's array is complete: iss_depth_finish on any stream may follow)
    for (int k = 0; k < 6; ++k) counts[k] = (int64_t)st.counts[k];
    bad_word_split(st.bad, bad_record, bad_code);
    return 0;
}

int iss_br_kernel_ms(iss_br *f, double *ms) {
    if (!f || !ms) return fail(f, ISS_E_INVALID, "iss_br_kernel_ms: bad arguments");
    HIP_TRY(f, hipSetDevice(f->device));
    for (iss_br::Slot &s : f->slot) ISS_TRY(slot_collect(f, s, s.done, f->kernel_ms));
    *ms = f->kernel_ms;
    return 0;
}

}  // extern "C"
