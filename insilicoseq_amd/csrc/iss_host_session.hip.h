// iss_host_session.hip.h -- what the stand-alone device contexts share on the host (iss_api_bam.hip.h, iss_api_fqtally.hip.h,
// iss_api_inflate.hip.h, iss_api_bamreads.hip.h, iss_api_fasta.hip.h; struct iss_session and its fail(): iss_host_util.hip.h): the front of a create and
// of a destroy, the slot of a two-slot pipeline with its timed kernels, grow-only buffers with their capacity, the first-bad word, the
// check of a BAM chunk's record offsets.
#pragma once

namespace {

// The front of a create, behind its own argument checks: the ordinal is one of this machine's devices (nothing exists yet: these
// errors are the thread's), then the new session stands in *out before its first HIP call -- a create that fails later leaves a
// handle whose last error can be read and which destroy takes -- and its device is the current one.
template <typename S>
int session_open(int device_ordinal, S **out) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(nullptr, ISS_E_HIP, std::string("no HIP device available: ") + hipGetErrorString(e));
    if (device_ordinal < 0 || device_ordinal >= n) return fail(nullptr, ISS_E_INVALID, "device ordinal out of range");
    S *s = new S();
    *out = s;
    s->device = device_ordinal;
    HIP_TRY(s, hipSetDevice(device_ordinal));
    return 0;
}

// The front of a destroy: nothing the session queued is in flight any more; `delete` follows, and the members release the buffers,
// events and streams (a stream a failed create never made is NULL).
void session_close(iss_session *s, std::initializer_list<hipStream_t> streams) {
    (void)hipSetDevice(s->device);
    for (hipStream_t st : streams)
        if (st) (void)hipStreamSynchronize(st);
}

const char *session_last_error(const iss_session *s) { return s ? s->last_error.c_str() : g_last_error.c_str(); }

// One of the two slots a pipelined context alternates between (feed i uses slot i % SLOTS): the copy of chunk i + 1 overlaps the
// kernels of chunk i, and a feed waits once, for the chunk that went through its slot before.
constexpr int SLOTS = 2;
struct TimedSlot {
    Event copied;       // the slot's copies have landed
    Event begin;        // in front of the kernels that read the slot,
    Event done;         // and behind them (both timed: the context's kernel_ms)
    bool busy = false;  // the slot's last feed has not been waited for
};

int slot_create(iss_session *s, TimedSlot &t) {
    ISS_TRY(event_create(s, t.copied, hipEventDisableTiming));
    ISS_TRY(event_create(s, t.begin, hipEventDefault));
    return event_create(s, t.done, hipEventDefault);
}

// waits until the device has finished with the slot -- `last`: the event behind everything that reads it -- and books its kernels' time
int slot_collect(iss_session *s, TimedSlot &t, hipEvent_t last, double &kernel_ms) {
    if (!t.busy) return 0;
    HIP_TRY(s, hipEventSynchronize(last));
    float ms = 0.f;
    HIP_TRY(s, hipEventElapsedTime(&ms, t.begin, t.done));
    kernel_ms += ms;
    t.busy = false;
    return 0;
}

// Grow-only buffers stand with their capacity in one small struct: `cap` elements and alloc(owner, n, what),
// which fills the group's handles for n of them.  reserve(): room for `need`, `floor` at least.  The group is emptied first, so a
// failed allocation leaves capacity 0.  A handle frees, it never waits: where the device may still use what is let go, the
// caller synchronises in front.
template <typename G>
int reserve(iss_session *owner, G &g, size_t need, size_t floor, const char *what = "") {
    if (need <= g.cap) return 0;
    g = {};
    const size_t n = std::max(need, floor);
    ISS_TRY(g.alloc(owner, n, what));
    g.cap = n;
    return 0;
}
template <typename T>
struct Staged {  // a pinned staging buffer and the device buffer it is copied to
    PinMem<T> h;
    DevMem<T> d;
    size_t cap = 0;
    int alloc(iss_session *owner, size_t n, const char *what) {
        ISS_TRY(pin_alloc(owner, h, n, what));
        return dev_alloc(owner, d, n, what);
    }
};
template <typename Handle>
struct Grown {  // one buffer: Grown<DevMem<T>>, Grown<PinMem<T>>
    Handle p;
    size_t cap = 0;
    int alloc(iss_session *owner, size_t n, const char *what) { return own_alloc(owner, p, n, what); }
};

// Every record of a BAM chunk must lie inside the chunk, its fixed fields and its block_size both: the kernels trust these offsets
// (iss_bam_scan makes them, ascending).  who: the entry point, for the message.
int records_inside(iss_session *s, const char *who, const uint8_t *data, int64_t n_bytes, const int64_t *offsets, int64_t n_records, bool ascending) {
    int64_t before = -1;
    for (int64_t r = 0; r < n_records; ++r) {
        const int64_t o = offsets[r];
        if (o < 0 || o + 4 + 32 > n_bytes) return fail(s, ISS_E_INVALID, std::string(who) + ": record offset outside the chunk");
        if (ascending && o <= before) return fail(s, ISS_E_INVALID, std::string(who) + ": record offsets do not ascend");
        int32_t bs;
        memcpy(&bs, data + o, 4);
        if (bs < 32 || o + 4 + (int64_t)bs > n_bytes) return fail(s, ISS_E_INVALID, std::string(who) + ": record outside the chunk");
        before = o;
    }
    return 0;
}

// A first-bad word as the kernels keep it, (index << 8) | code with the smallest winning; all ones: none, index -1 and code 0.
// bad_state_clear: n_bytes at p zeroed (counters, a state struct) and the first-bad word bad_at bytes in set to none; the caller waits.
int bad_state_clear(iss_session *s, hipStream_t stream, void *p, size_t n_bytes, size_t bad_at) {
    HIP_TRY(s, hipMemsetAsync(p, 0, n_bytes, stream));
    HIP_TRY(s, hipMemsetAsync(static_cast<uint8_t *>(p) + bad_at, 0xFF, sizeof(unsigned long long), stream));
    return 0;
}
void bad_word_split(unsigned long long word, int64_t *index, int32_t *code) {
    *index = word == ~0ull ? -1 : (int64_t)(word >> 8);
    *code = word == ~0ull ? 0 : (int32_t)(word & 0xFF);
}

}  // namespace
