// iss_api_bam.hip.h -- C ABI of `model` (iss model, iss/bam.py:103-227): record boundaries of inflated BAM bytes (host), the tally
// context (device tallies over fed chunks, their download) and the kernel density estimates from the tallies.  Device code: iss_bam.hip.h.
#pragma once

struct iss_bam {
    int device = 0;
    Stream stream;
    std::string last_error;
    struct Data {  // a chunk's bytes
        DevMem<uint8_t> d;
        size_t cap = 0;
    } data;
    struct Records {  // per record of a chunk
        DevMem<uint32_t> d_offs;
        DevMem<uint8_t> d_sel;
        DevMem<uint2> d_meta;
        size_t cap = 0;
    } rec;
    DevMem<unsigned long long> d_tally;  // TALLY_WORDS, then the error word
    DevMem<double> d_qcdf, d_isize;
    int64_t fed = 0;
    int n_cu = 256;
    std::vector<uint32_t> h_offs;
};

namespace {
int fail(iss_bam *b, int code, const std::string &msg) {
    if (b) b->last_error = msg;
    else g_last_error = msg;
    return code;
}
}  // namespace

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
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(nullptr, ISS_E_HIP, std::string("no HIP device available: ") + hipGetErrorString(e));
    if (device_ordinal < 0 || device_ordinal >= n) return fail(nullptr, ISS_E_INVALID, "device ordinal out of range");
    iss_bam *b = new iss_bam();
    *out = b;
    b->device = device_ordinal;
    HIP_TRY(b, hipSetDevice(device_ordinal));
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
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    delete b;  // (its members release the buffers and the stream)
}

const char *iss_bam_last_error(const iss_bam *b) { return b ? b->last_error.c_str() : g_last_error.c_str(); }

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
    // every record must lie inside the chunk: the kernels trust these offsets (iss_bam_scan makes them)
    b->h_offs.resize((size_t)n_records);
    for (int64_t r = 0; r < n_records; ++r) {
        const int64_t o = offsets[r];
        if (o < 0 || o + 4 + 32 > n_bytes) return fail(b, ISS_E_INVALID, "iss_bam_feed: record offset outside the chunk");
        int32_t bs;
        memcpy(&bs, data + o, 4);
        if (bs < 32 || o + 4 + (int64_t)bs > n_bytes) return fail(b, ISS_E_INVALID, "iss_bam_feed: record outside the chunk");
        b->h_offs[(size_t)r] = (uint32_t)o;
    }
    // (each array is at least 1 MiB, as the chunk's bytes are; the stream is idle between feeds, the wait costs nothing)
    if ((size_t)n_records > b->rec.cap) {
        const size_t n = std::max((size_t)n_records, (size_t)1 << 16);
        HIP_TRY(b, hipStreamSynchronize(b->stream));
        b->rec = {};
        DEV_ALLOC(b, b->rec.d_offs, std::max(n, ((size_t)1 << 20) / sizeof(uint32_t)));
        DEV_ALLOC(b, b->rec.d_sel, std::max(n, (size_t)1 << 20));
        DEV_ALLOC(b, b->rec.d_meta, std::max(n, ((size_t)1 << 20) / sizeof(uint2)));
        b->rec.cap = n;
    }
    if ((size_t)n_bytes > b->data.cap) {
        const size_t n = std::max((size_t)n_bytes, (size_t)1 << 20);
        HIP_TRY(b, hipStreamSynchronize(b->stream));
        b->data = {};
        DEV_ALLOC(b, b->data.d, n);
        b->data.cap = n;
    }
    HIP_TRY(b, hipMemcpyAsync(b->data.d, data, (size_t)n_bytes, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(b, hipMemcpyAsync(b->rec.d_offs, b->h_offs.data(), (size_t)n_records * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(b, hipMemcpyAsync(b->rec.d_sel, select, (size_t)n_records, hipMemcpyHostToDevice, b->stream));
    const int64_t per_wg = iss::bam::TALLY_WAVES;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_records + per_wg - 1) / per_wg, 2LL * b->n_cu));
    const int64_t per_iter = (int64_t)grid * per_wg;
    hipLaunchKernelGGL(iss::bam::k_bam_tally, dim3(grid), dim3(iss::bam::TALLY_THREADS), iss::bam::TALLY_LDS, b->stream, b->data.d, b->rec.d_offs,
                       b->rec.d_sel, n_records, (n_records + per_iter - 1) / per_iter, b->fed, b->rec.d_meta, b->d_tally, b->d_tally + ISS_BAM_TALLY_WORDS);
    HIP_TRY(b, hipGetLastError());
    const unsigned qgrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_records + per_wg - 1) / per_wg, (int64_t)b->n_cu / 4));
    hipLaunchKernelGGL(iss::bam::k_bam_qhist, dim3(qgrid, iss::bam::N_SLICE), dim3(iss::bam::TALLY_THREADS), iss::bam::QHIST_LDS, b->stream,
                       b->data.d, b->rec.d_meta, n_records, b->d_tally);
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
    const unsigned long long e = h[ISS_BAM_TALLY_WORDS];
    *bad_record = e == ~0ull ? -1 : (int64_t)(e >> 8);
    *bad_code = e == ~0ull ? 0 : (int32_t)(e & 0xFF);
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
