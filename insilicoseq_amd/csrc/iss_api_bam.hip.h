// iss_api_bam.hip.h -- C ABI of `model` (iss model, iss/bam.py:103-227): record boundaries of inflated BAM bytes (host), the tally
// context (device tallies over fed chunks, their download) and the kernel density estimates from the tallies.  Device code: iss_bam.hip.h.
// The context is a session (iss_host_session.hip.h: open and close, grown buffers, the first-bad word); its feed is synchronous, no slots.
#pragma once

namespace {
struct BamRecords {  // per record of a chunk (a group for reserve()); each array is at least 1 MiB, as the chunk's bytes are
    DevMem<uint32_t> d_offs;
    DevMem<uint8_t> d_sel;
    DevMem<uint2> d_meta;
    size_t cap = 0;
    int alloc(iss_session *b, size_t n, const char *) {
        DEV_ALLOC(b, d_offs, std::max(n, ((size_t)1 << 20) / sizeof(uint32_t)));
        DEV_ALLOC(b, d_sel, std::max(n, (size_t)1 << 20));
        DEV_ALLOC(b, d_meta, std::max(n, ((size_t)1 << 20) / sizeof(uint2)));
        return 0;
    }
};
}  // namespace

struct iss_bam : iss_session {
    Stream stream;
    Grown<DevMem<uint8_t>> data;  // a chunk's bytes
    BamRecords rec;
    DevMem<unsigned long long> d_tally;  // TALLY_WORDS, then the error word
    DevMem<double> d_qcdf, d_isize;
    int64_t fed = 0;
    int n_cu = 256;
    std::vector<uint32_t> h_offs;
};

static_assert(iss::bam::TALLY_WORDS == ISS_BAM_TALLY_WORDS, "include/iss_mi355x.h: ISS_BAM_TALLY_WORDS");
static_assert(iss::bam::OFF_QHIST == ISS_BAM_OFF_QHIST && iss::bam::OFF_TLEN == ISS_BAM_OFF_TLEN && iss::bam::OFF_NREAD == ISS_BAM_OFF_NREAD,
              "include/iss_mi355x.h: tally layout");

extern "C" {

int iss_bam_scan(const uint8_t *data, int64_t n_bytes, int64_t *offsets, int64_t capacity, int64_t *n_records, int64_t *consumed) {
    if (!data || n_bytes < 0 || !n_records || !consumed || (capacity > 0 && !offsets))
        return fail(nullptr, ISS_E_INVALID, "iss_bam_scan: bad arguments");
    int64_t off = 0, n = 0;
    while (off + 4 <= n_bytes && n < capacity) {
        int32_t bs;
        memcpy(&bs, data + off, 4);
        if (bs < 32) {
            *n_records = n;
            *consumed = off;
            return fail(nullptr, ISS_E_INVALID, "corrupt BAM record: block_size " + std::to_string(bs) + " after " +
                                                        std::to_string(n) + " records of the chunk");
        }
        if (off + 4 + (int64_t)bs > n_bytes) break;
        offsets[n++] = off;
        off += 4 + (int64_t)bs;
    }
    *n_records = n;
    *consumed = off;
    return 0;
}

int iss_bam_create(int device_ordinal, iss_bam **out) {
    if (!out) return fail(nullptr, ISS_E_INVALID, "iss_bam_create: out is NULL");
    *out = nullptr;
    ISS_TRY(session_open(device_ordinal, out));
    iss_bam *b = *out;
    hipDeviceProp_t prop;
    HIP_TRY(b, hipGetDeviceProperties(&prop, device_ordinal));
    b->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIP_TRY(b, hipFuncSetAttribute(reinterpret_cast<const void *>(iss::bam::k_bam_tally), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)iss::bam::TALLY_LDS));
    HIP_TRY(b, hipFuncSetAttribute(reinterpret_cast<const void *>(iss::bam::k_bam_qhist), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)iss::bam::QHIST_LDS));
    ISS_TRY(stream_create(b, b->stream, hipStreamNonBlocking));
    DEV_ALLOC(b, b->d_tally, ISS_BAM_TALLY_WORDS + 1);
    DEV_ALLOC(b, b->d_qcdf, ISS_BAM_QCDF_WORDS);
    DEV_ALLOC(b, b->d_isize, ISS_BAM_NTLEN);
    return iss_bam_reset(b);
}

void iss_bam_destroy(iss_bam *b) {
    if (!b) return;
    session_close(b, {b->stream});
    delete b;
}

const char *iss_bam_last_error(const iss_bam *b) { return session_last_error(b); }

int iss_bam_reset(iss_bam *b) {
    if (!b) return fail(nullptr, ISS_E_INVALID, "iss_bam_reset: NULL");
    HIP_TRY(b, hipSetDevice(b->device));
    std::vector<unsigned long long> init(ISS_BAM_TALLY_WORDS + 1, 0ull);
    for (int s = 0; s < 8; ++s) init[ISS_BAM_OFF_MINLEN + s] = ~0ull;
    init[ISS_BAM_TALLY_WORDS] = ~0ull;  // error word: ((record << 8) | code), the smallest wins
    HIP_TRY(b, hipMemcpyAsync(b->d_tally, init.data(), init.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    b->fed = 0;
    return 0;
}


int iss_bam_feed(iss_bam *b, const uint8_t *data, int64_t n_bytes, const int64_t *offsets, const uint8_t *select, int64_t n_records) {
    if (!b || n_bytes < 0 || n_records < 0 || (n_records && (!data || !offsets || !select)))
        return fail(b, ISS_E_INVALID, "iss_bam_feed: bad arguments");
    if (n_bytes > (int64_t)UINT32_MAX) return fail(b, ISS_E_INVALID, "iss_bam_feed: chunks are limited to 4 GiB");
    if (!n_records) return 0;
    HIP_TRY(b, hipSetDevice(b->device));
    ISS_TRY(records_inside(b, "iss_bam_feed", data, n_bytes, offsets, n_records, false));
    b->h_offs.assign(offsets, offsets + n_records);  // (below 2^32: inside the chunk)
    // (the stream is idle between feeds, the wait in front of a replacement costs nothing)
    if ((size_t)n_records > b->rec.cap || (size_t)n_bytes > b->data.cap) HIP_TRY(b, hipStreamSynchronize(b->stream));
    ISS_TRY(reserve(b, b->rec, (size_t)n_records, (size_t)1 << 16));
    ISS_TRY(reserve(b, b->data, (size_t)n_bytes, (size_t)1 << 20, "chunk bytes"));
    HIP_TRY(b, hipMemcpyAsync(b->data.p, data, (size_t)n_bytes, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(b, hipMemcpyAsync(b->rec.d_offs, b->h_offs.data(), (size_t)n_records * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(b, hipMemcpyAsync(b->rec.d_sel, select, (size_t)n_records, hipMemcpyHostToDevice, b->stream));
    const int64_t per_wg = iss::bam::TALLY_WAVES;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_records + per_wg - 1) / per_wg, 2LL * b->n_cu));
    const int64_t per_iter = (int64_t)grid * per_wg;
    hipLaunchKernelGGL(iss::bam::k_bam_tally, dim3(grid), dim3(iss::bam::TALLY_THREADS), iss::bam::TALLY_LDS, b->stream, b->data.p, b->rec.d_offs,
                       b->rec.d_sel, n_records, (n_records + per_iter - 1) / per_iter, b->fed, b->rec.d_meta, b->d_tally, b->d_tally + ISS_BAM_TALLY_WORDS);
    HIP_TRY(b, hipGetLastError());
    const unsigned qgrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_records + per_wg - 1) / per_wg, (int64_t)b->n_cu / 4));
    hipLaunchKernelGGL(iss::bam::k_bam_qhist, dim3(qgrid, iss::bam::N_SLICE), dim3(iss::bam::TALLY_THREADS), iss::bam::QHIST_LDS, b->stream,
                       b->data.p, b->rec.d_meta, n_records, b->d_tally);
    HIP_TRY(b, hipGetLastError());
    // the host buffers may be reused as soon as the call returns
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    b->fed += n_records;
    return 0;
}

int iss_bam_tally_download(iss_bam *b, uint64_t *tally, int64_t *bad_record, int32_t *bad_code) {
    if (!b || !tally || !bad_record || !bad_code) return fail(b, ISS_E_INVALID, "iss_bam_tally_download: bad arguments");
    HIP_TRY(b, hipSetDevice(b->device));
    std::vector<unsigned long long> h(ISS_BAM_TALLY_WORDS + 1);
    HIP_TRY(b, hipMemcpyAsync(h.data(), b->d_tally, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    memcpy(tally, h.data(), ISS_BAM_TALLY_WORDS * sizeof(uint64_t));
    bad_word_split(h[ISS_BAM_TALLY_WORDS], bad_record, bad_code);
    return 0;
}

int iss_bam_kde(iss_bam *b, int32_t read_length, int32_t with_isize, double *qcdf, double *isize_cdf) {
    if (!b || !qcdf || (with_isize && !isize_cdf) || read_length < 0 || read_length > ISS_BAM_MAX_LEN)
        return fail(b, ISS_E_INVALID, "iss_bam_kde: bad arguments");
    HIP_TRY(b, hipSetDevice(b->device));
    const int nqb = (iss::bam::N_SLICE * iss::bam::MAX_LEN + iss::bam::KDE_THREADS - 1) / iss::bam::KDE_THREADS;
    hipLaunchKernelGGL(iss::bam::k_kde_cdf, dim3(nqb + (with_isize ? 1 : 0)), dim3(iss::bam::KDE_THREADS), 0, b->stream, b->d_tally, b->d_qcdf,
                       b->d_isize, (int)read_length, nqb);
    HIP_TRY(b, hipGetLastError());
    HIP_TRY(b, hipMemcpyAsync(qcdf, b->d_qcdf, sizeof(double) * ISS_BAM_QCDF_WORDS, hipMemcpyDeviceToHost, b->stream));
    if (with_isize)
        HIP_TRY(b, hipMemcpyAsync(isize_cdf, b->d_isize, sizeof(double) * ISS_BAM_NTLEN, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    return 0;
}

}  // extern "C"
