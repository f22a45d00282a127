// iss_api_inflate.hip.h -- C ABI of the device inflate (iss_bgzf_scan, iss_inflate_*): the BSIZE chain of a buffer on the host, and a
// context that takes groups of whole BGZF members and hands their inflated bytes back.  A group goes through one of two pinned staging
// buffers to the device on the copy-in stream, k_bgzf_inflate (iss_inflate.hip.h) follows on the kernel stream, and the bytes and the
// members' statuses leave for a pinned result buffer on the copy-out stream, each step ordered behind the one before by an event: group
// i + 1 copies in while group i inflates and group i - 1 copies out.  No model, no iss_ctx: a session (iss_host_session.hip.h: open
// and close, the two timed slots -- here with a fourth event, `fetched`, that a feed waits for --, grown buffers, the first-bad word);
// the pool of result buffers (results / flight / idle / held) is this file's own.
#pragma once

struct iss_inflate : iss_session {
    struct Slot : TimedSlot {  // what a group holds on its way through the device
        Staged<uint8_t> in;
        Staged<uint32_t> meta;  // [5][cap / 5]: payload offset, payload length, output offset, ISIZE, CRC-32
        Grown<DevMem<uint8_t>> status, out;
        Event fetched;  // the results have left the slot's device buffers
    };
    struct Result {  // a group's inflated bytes and statuses on the host
        Grown<PinMem<uint8_t>> out, status;
        Event ready;
        int64_t n_bytes = 0, n_members = 0;
    };
    int n_cu = 256;
    Stream copy_in, stream, copy_out;
    Slot slot[SLOTS];
    std::vector<std::unique_ptr<Result>> results;  // all of them; the three lists below are views
    std::deque<Result *> flight;                   // fed, not collected: the oldest first
    std::vector<Result *> idle;
    Result *held = nullptr;                        // what the last collect handed out
    DevMem<uint32_t> d_ops;
    DevMem<unsigned long long> d_bad;
    int64_t feeds = 0, fed_members = 0;
    double kernel_ms = 0.0;  // of the groups whose slot has been waited for
};

static_assert(iss_inf::ST_OK == ISS_BGZF_OK && iss_inf::ST_BAD_BTYPE == ISS_BGZF_BAD_BTYPE && iss_inf::ST_STORED_LEN == ISS_BGZF_STORED_LEN &&
                  iss_inf::ST_BAD_CODE == ISS_BGZF_BAD_CODE && iss_inf::ST_BAD_SYMBOL == ISS_BGZF_BAD_SYMBOL &&
                  iss_inf::ST_BAD_DISTANCE == ISS_BGZF_BAD_DISTANCE && iss_inf::ST_IN_OVERRUN == ISS_BGZF_IN_OVERRUN &&
                  iss_inf::ST_OUT_OVERRUN == ISS_BGZF_OUT_OVERRUN && iss_inf::ST_SHORT == ISS_BGZF_SHORT &&
                  iss_inf::ST_TRAILING == ISS_BGZF_TRAILING && iss_inf::ST_CRC == ISS_BGZF_CRC,
              "include/iss_mi355x.h: ISS_BGZF_*");

extern "C" {

int iss_bgzf_scan(const uint8_t *data, int64_t n_bytes, int64_t *member_off, int64_t *pay_off, uint32_t *pay_len, uint32_t *crc,
                  uint32_t *isize, int64_t capacity, int64_t *n_members, int64_t *consumed) {
    if (!data || n_bytes < 0 || capacity < 0 || !n_members || !consumed || (capacity > 0 && (!member_off || !pay_off || !pay_len || !crc || !isize)))
        return fail(nullptr, ISS_E_INVALID, "iss_bgzf_scan: bad arguments");
    int64_t pos = 0, n = 0;
    int rc = 0;
    while (n < capacity && pos + 4 <= n_bytes) {
        const uint8_t *p = data + pos;
        if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 0x08 || p[3] != 0x04) {
            rc = fail(nullptr, ISS_E_INVALID, "no BGZF member at byte " + std::to_string(pos) + " (gzip magic with the extra-field flag expected)");
            break;
        }
        if (pos + 12 > n_bytes) break;
        const int64_t xlen = (int64_t)p[10] | (int64_t)p[11] << 8;
        if (pos + 12 + xlen > n_bytes) break;
        int64_t total = -1;
        for (int64_t x = 12; x + 4 <= 12 + xlen;) {
            const int64_t slen = (int64_t)p[x + 2] | (int64_t)p[x + 3] << 8;
            if (p[x] == 'B' && p[x + 1] == 'C' && slen == 2 && x + 6 <= 12 + xlen) total = ((int64_t)p[x + 4] | (int64_t)p[x + 5] << 8) + 1;
            x += 4 + slen;
        }
        if (total < 0) {
            rc = fail(nullptr, ISS_E_INVALID, "gzip member at byte " + std::to_string(pos) + " without the BGZF BC field");
            break;
        }
        if (total < 12 + xlen + 8) {
            rc = fail(nullptr, ISS_E_INVALID, "BGZF member at byte " + std::to_string(pos) + ": BSIZE + 1 = " + std::to_string(total) +
                                                  " is less than its header and footer");
            break;
        }
        if (pos + total > n_bytes) break;
        member_off[n] = pos;
        pay_off[n] = pos + 12 + xlen;
        pay_len[n] = (uint32_t)(total - 12 - xlen - 8);
        memcpy(&crc[n], p + total - 8, 4);
        memcpy(&isize[n], p + total - 4, 4);
        ++n;
        pos += total;
    }
    *n_members = n;
    *consumed = pos;
    return rc;
}

int iss_inflate_create(int device_ordinal, iss_inflate **out) {
    if (!out) return fail(nullptr, ISS_E_INVALID, "iss_inflate_create: out is NULL");
    *out = nullptr;
    ISS_TRY(session_open(device_ordinal, out));
    iss_inflate *z = *out;
    hipDeviceProp_t prop;
    HIP_TRY(z, hipGetDeviceProperties(&prop, device_ordinal));
    z->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIP_TRY(z, hipFuncSetAttribute(reinterpret_cast<const void *>(iss::inf::k_bgzf_inflate), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)iss::inf::INF_LDS));
    ISS_TRY(stream_create(z, z->copy_in, hipStreamNonBlocking));
    ISS_TRY(stream_create(z, z->stream, hipStreamNonBlocking));
    ISS_TRY(stream_create(z, z->copy_out, hipStreamNonBlocking));
    for (iss_inflate::Slot &s : z->slot) {
        ISS_TRY(slot_create(z, s));
        ISS_TRY(event_create(z, s.fetched, hipEventDisableTiming));
    }
    std::vector<uint32_t> tab(256), ops((size_t)iss_inf::N_OPS * 32);
    iss_inf::crc_tables(tab.data(), ops.data());
    DEV_ALLOC(z, z->d_ops, ops.size());
    DEV_ALLOC(z, z->d_bad, 1);
    HIP_TRY(z, hipMemcpy(z->d_ops, ops.data(), ops.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return iss_inflate_reset(z);
}

void iss_inflate_destroy(iss_inflate *z) {
    if (!z) return;
    session_close(z, {z->copy_in, z->stream, z->copy_out});
    delete z;
}

const char *iss_inflate_last_error(const iss_inflate *z) { return session_last_error(z); }

int iss_inflate_reset(iss_inflate *z) {
    if (!z) return fail(z, ISS_E_INVALID, "iss_inflate_reset: NULL");
    HIP_TRY(z, hipSetDevice(z->device));
    HIP_TRY(z, hipStreamSynchronize(z->copy_in));
    HIP_TRY(z, hipStreamSynchronize(z->stream));
    HIP_TRY(z, hipStreamSynchronize(z->copy_out));
    HIP_TRY(z, hipMemsetAsync(z->d_bad, 0xFF, sizeof(unsigned long long), z->stream));  // ((member << 8) | status, the smallest wins)
    HIP_TRY(z, hipStreamSynchronize(z->stream));
    for (iss_inflate::Slot &s : z->slot) s.busy = false;
    for (iss_inflate::Result *r : z->flight) z->idle.push_back(r);
    z->flight.clear();
    if (z->held) z->idle.push_back(z->held);
    z->held = nullptr;
    z->feeds = z->fed_members = 0;
    z->kernel_ms = 0.0;
    return 0;
}

int iss_inflate_feed(iss_inflate *z, const uint8_t *data, int64_t n_bytes, const int64_t *pay_off, const uint32_t *pay_len,
                     const uint32_t *crc, const uint32_t *isize, int64_t n_members) {
    if (!z || n_bytes < 0 || n_members < 0 || (n_members && (!data || !pay_off || !pay_len || !crc || !isize)))
        return fail(z, ISS_E_INVALID, "iss_inflate_feed: bad arguments");
    if (n_bytes >= ((int64_t)1 << 31) || n_members >= ((int64_t)1 << 31))
        return fail(z, ISS_E_INVALID, "iss_inflate_feed: a group holds less than 2^31 compressed bytes");
    if (!n_members) return 0;
    // the kernel trusts these arrays (iss_bgzf_scan makes them): payloads ascending inside the buffer, a member's size within BGZF's
    int64_t at = 0, total_out = 0;
    for (int64_t m = 0; m < n_members; ++m) {
        if (pay_off[m] < at || pay_off[m] > n_bytes || (int64_t)pay_len[m] > n_bytes - pay_off[m])
            return fail(z, ISS_E_INVALID, "iss_inflate_feed: the payload of member " + std::to_string(m) + " is not ascending inside the buffer");
        if (pay_len[m] > 65536u || isize[m] > 65536u)
            return fail(z, ISS_E_INVALID, "iss_inflate_feed: member " + std::to_string(m) + " is larger than a BGZF member (64 KiB)");
        at = pay_off[m] + (int64_t)pay_len[m];
        total_out += isize[m];
        if (total_out >= ((int64_t)1 << 31)) return fail(z, ISS_E_INVALID, "iss_inflate_feed: a group inflates to less than 2^31 bytes");
    }
    HIP_TRY(z, hipSetDevice(z->device));
    iss_inflate::Slot &s = z->slot[z->feeds % SLOTS];
    // the one wait of a feed: for the group that went through the slot to have left it, never for a collect
    ISS_TRY(slot_collect(z, s, s.fetched, z->kernel_ms));
    const size_t nm = (size_t)n_members;
    ISS_TRY(reserve(z, s.in, (size_t)n_bytes, (size_t)1 << 20, "slot input"));
    ISS_TRY(reserve(z, s.meta, 5 * nm, (size_t)5 << 12, "slot member arrays"));
    ISS_TRY(reserve(z, s.status, nm, (size_t)1 << 12, "slot statuses"));
    ISS_TRY(reserve(z, s.out, (size_t)total_out + 1, (size_t)1 << 20, "slot output"));
    iss_inflate::Result *r = nullptr;
    if (!z->idle.empty()) {
        r = z->idle.back();
        z->idle.pop_back();
    } else {
        z->results.emplace_back(new iss_inflate::Result());
        r = z->results.back().get();
        if (int rc = event_create(z, r->ready, hipEventDisableTiming)) {
            z->results.pop_back();
            return rc;
        }
    }
    z->idle.push_back(r);  // (until it is queued: a failure below leaves it idle)
    ISS_TRY(reserve(z, r->out, (size_t)total_out + 1, (size_t)1 << 20, "result bytes"));
    ISS_TRY(reserve(z, r->status, nm, (size_t)1 << 12, "result statuses"));
    memcpy(s.in.h, data, (size_t)n_bytes);  // (the caller's memory is free again when the call returns)
    uint32_t *meta = s.meta.h;
    uint32_t off = 0;
    for (size_t m = 0; m < nm; ++m) {
        meta[m] = (uint32_t)pay_off[m];
        meta[nm + m] = pay_len[m];
        meta[2 * nm + m] = off;
        meta[3 * nm + m] = isize[m];
        meta[4 * nm + m] = crc[m];
        off += isize[m];
    }
    HIP_TRY(z, hipMemcpyAsync(s.in.d, s.in.h, (size_t)n_bytes, hipMemcpyHostToDevice, z->copy_in));
    HIP_TRY(z, hipMemcpyAsync(s.meta.d, s.meta.h, 5 * nm * sizeof(uint32_t), hipMemcpyHostToDevice, z->copy_in));
    HIP_TRY(z, hipEventRecord(s.copied, z->copy_in));
    HIP_TRY(z, hipStreamWaitEvent(z->stream, s.copied, 0));
    HIP_TRY(z, hipEventRecord(s.begin, z->stream));
    iss::inf::InflateArgs A{};
    A.in = s.in.d;
    A.out = s.out.p;
    A.pay_off = s.meta.d;
    A.pay_len = s.meta.d + nm;
    A.out_off = s.meta.d + 2 * nm;
    A.isize = s.meta.d + 3 * nm;
    A.crc = s.meta.d + 4 * nm;
    A.status = s.status.p;
    A.ops = z->d_ops;
    A.bad = z->d_bad;
    A.n_members = (uint32_t)n_members;
    A.member_base = (unsigned long long)z->fed_members;
    int wgs = z->n_cu;  // (a workgroup fills a CU's LDS: more of them would only queue)
    if (const char *e = getenv("ISS_INFLATE_WGS")) wgs = std::max(1, atoi(e));  // workgroups aimed at (tests: other member-to-wave mappings)
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_members + iss::inf::INF_WAVES - 1) / iss::inf::INF_WAVES, wgs));
    hipLaunchKernelGGL(iss::inf::k_bgzf_inflate, dim3(grid), dim3(iss::inf::INF_THREADS), iss::inf::INF_LDS, z->stream, A);
    HIP_TRY(z, hipGetLastError());
    HIP_TRY(z, hipEventRecord(s.done, z->stream));
    HIP_TRY(z, hipStreamWaitEvent(z->copy_out, s.done, 0));
    if (total_out) HIP_TRY(z, hipMemcpyAsync(r->out.p, s.out.p, (size_t)total_out, hipMemcpyDeviceToHost, z->copy_out));
    HIP_TRY(z, hipMemcpyAsync(r->status.p, s.status.p, nm, hipMemcpyDeviceToHost, z->copy_out));
    HIP_TRY(z, hipEventRecord(r->ready, z->copy_out));
    HIP_TRY(z, hipEventRecord(s.fetched, z->copy_out));
    s.busy = true;
    r->n_bytes = total_out;
    r->n_members = n_members;
    z->idle.pop_back();
    z->flight.push_back(r);
    ++z->feeds;
    z->fed_members += n_members;
    return 0;
}

int iss_inflate_collect(iss_inflate *z, const uint8_t **data, int64_t *n_bytes, const uint8_t **status, int64_t *n_members) {
    if (!z || !data || !n_bytes || !status || !n_members) return fail(z, ISS_E_INVALID, "iss_inflate_collect: bad arguments");
    if (z->flight.empty()) return fail(z, ISS_E_INVALID, "iss_inflate_collect: no group in flight");
    HIP_TRY(z, hipSetDevice(z->device));
    iss_inflate::Result *r = z->flight.front();
    HIP_TRY(z, hipEventSynchronize(r->ready));
    z->flight.pop_front();
    if (z->held) z->idle.push_back(z->held);
    z->held = r;
    *data = r->out.p;
    *n_bytes = r->n_bytes;
    *status = r->status.p;
    *n_members = r->n_members;
    return 0;
}

int iss_inflate_first_bad(iss_inflate *z, int64_t *member, int32_t *code) {
    if (!z || !member || !code) return fail(z, ISS_E_INVALID, "iss_inflate_first_bad: bad arguments");
    HIP_TRY(z, hipSetDevice(z->device));
    unsigned long long e = 0;
    HIP_TRY(z, hipMemcpyAsync(&e, z->d_bad, sizeof e, hipMemcpyDeviceToHost, z->stream));  // (behind every kernel fed)
    HIP_TRY(z, hipStreamSynchronize(z->stream));
    bad_word_split(e, member, code);
    return 0;
}

int iss_inflate_kernel_ms(iss_inflate *z, double *ms) {
    if (!z || !ms) return fail(z, ISS_E_INVALID, "iss_inflate_kernel_ms: bad arguments");
    HIP_TRY(z, hipSetDevice(z->device));
    for (iss_inflate::Slot &s : z->slot) ISS_TRY(slot_collect(z, s, s.fetched, z->kernel_ms));
    *ms = z->kernel_ms;
    return 0;
}

}  // extern "C"
