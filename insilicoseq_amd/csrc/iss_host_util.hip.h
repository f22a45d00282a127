// iss_host_util.hip.h -- helpers every entry point uses: error reporting (into a context, or into the session base of the stand-alone
// device contexts), checked allocations into owning handles, checked uploads, the environment switches, what a model upload or a new
// reservation empties, the choice of the hot kernel's instantiation (k_main / k_main_g), its LDS size, timing, synchronisation.
#pragma once

// What the stand-alone device contexts (iss_bam, iss_fq, iss_inflate, iss_br) have in common: each derives from it and stays a C type
// of its own (include/iss_mi355x.h declares them opaque).  What works on it: iss_host_session.hip.h.
struct iss_session {
    int device = 0;
    std::string last_error;
};

namespace {

// What takes an error: a context (NULL: only the thread's last error), or a session -- its own last error, or the thread's when there
// is no session.
int fail(iss_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->last_error = msg;
    g_last_error = msg;
    return code;
}
int fail(std::nullptr_t, int code, const std::string &msg) { return fail(static_cast<iss_ctx *>(nullptr), code, msg); }
int fail(iss_session *s, int code, const std::string &msg) {
    (s ? s->last_error : g_last_error) = msg;
    return code;
}

// `owner`: whatever fail() takes
#define HIP_TRY(owner, expr)                                                                     \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return fail(owner, ISS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));    \
    } while (0)

// a call that returns the library's codes: pass a failure on
#define ISS_TRY(expr)                                                                            \
    do {                                                                                         \
        const int rc_ = (expr);                                                                  \
        if (rc_) return rc_;                                                                     \
    } while (0)

// The handle releases what it held, then holds `count` elements of device (pinned: host) memory; on failure it stays empty and
// the error names `what`.  (own_alloc_quiet, for the callers that format their own message: iss_host_state.hip.h.)
template <typename Owner, typename T, void (*Free)(void *)>
int own_alloc(Owner owner, iss_own::Owned<T, Free> &h, size_t count, const char *what) {
    hipError_t e = hipSuccess;
    const size_t bytes = count * sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
    if (own_alloc_quiet(h, bytes, &e))
        return fail(owner, ISS_E_HIP, std::string(Free == own_free_pin ? "hipHostMalloc(" : "hipMalloc(") + what + ", " + std::to_string(bytes) + "): " + hipGetErrorString(e));
    return 0;
}
template <typename Owner, typename T>
int dev_alloc(Owner owner, DevMem<T> &h, size_t count, const char *what) { return own_alloc(owner, h, count, what); }
template <typename Owner, typename T>
int pin_alloc(Owner owner, PinMem<T> &h, size_t count, const char *what) { return own_alloc(owner, h, count, what); }
#define DEV_ALLOC(owner, handle, count) ISS_TRY(dev_alloc(owner, handle, count, #handle))
#define PIN_ALLOC(owner, handle, count) ISS_TRY(pin_alloc(owner, handle, count, #handle))

template <typename Owner>
int event_create(Owner owner, Event &ev, unsigned flags) {
    ev.reset();
    hipEvent_t e = nullptr;
    HIP_TRY(owner, hipEventCreateWithFlags(&e, flags));
    ev.reset(e);
    return 0;
}
template <typename Owner>
int stream_create(Owner owner, Stream &st, unsigned flags) {
    st.reset();
    hipStream_t s = nullptr;
    HIP_TRY(owner, hipStreamCreateWithFlags(&s, flags));
    st.reset(s);
    return 0;
}
template <typename Owner>
int stream_create(Owner owner, Stream &st, unsigned flags, int priority) {
    st.reset();
    hipStream_t s = nullptr;
    HIP_TRY(owner, hipStreamCreateWithPriority(&s, flags, priority));
    st.reset(s);
    return 0;
}

template <typename T>
int upload(iss_ctx *ctx, const T *host, size_t n, T **dev, std::vector<DevMem<void>> *track) {
    DevMem<void> d;
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    ISS_TRY(dev_alloc(ctx, d, bytes, "model table"));
    if (n) HIP_TRY(ctx, hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice));
    *dev = static_cast<T *>(d.get());  // a view: `track` keeps the allocation
    track->push_back(std::move(d));
    return 0;
}

// A record that owns its three buffers (iss_genome_upload's large records, iss_genome_upload_variants): allocated here, views set.
int genome_alloc_owned(iss_ctx *ctx, Genome &G, int64_t length) {
    const size_t n_mk = (size_t)(length + 31) / 32, n_pk = 2 * n_mk;
    G.L = length;
    DEV_ALLOC(ctx, G.packed_own, n_pk + PK_PAD);
    DEV_ALLOC(ctx, G.mask_own, n_mk + 4);
    DEV_ALLOC(ctx, G.ascii_own, (size_t)length);
    G.packed = G.packed_own + 1;
    G.mask = G.mask_own + 1;
    G.ascii = G.ascii_own;
    return 0;
}

// ... and packed from its ASCII copy, which what is queued on the context's stream so far has put into G.ascii: k_pack_genome,
// then its status read back (waits for the stream) -- res[0] letters outside the alphabet, res[1] the offset of the first,
// res[2] exception letters.
int genome_pack_owned(iss_ctx *ctx, Genome &G, unsigned long long res[3]) {
    const size_t n_mk = (size_t)(G.L + 31) / 32, n_pk = 2 * n_mk;
    unsigned long long *status = reinterpret_cast<unsigned long long *>(ctx->fix_count.get()) + 24;  // 3 words at +192 B
    const unsigned long long init[3] = {0ull, (unsigned long long)G.L, 0ull};
    hipError_t he = hipMemsetAsync(G.packed_own, 0, (n_pk + PK_PAD) * sizeof(uint32_t), ctx->stream);
    if (he == hipSuccess) he = hipMemsetAsync(G.mask_own, 0, (n_mk + 4) * sizeof(uint32_t), ctx->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(status, init, sizeof init, hipMemcpyHostToDevice, ctx->stream);
    if (he != hipSuccess) return fail(ctx, ISS_E_HIP, std::string("genome upload: ") + hipGetErrorString(he));
    hipLaunchKernelGGL(iss::k_pack_genome, dim3((unsigned)((n_mk + 255) / 256)), dim3(256), 0, ctx->stream, G.ascii, G.L,
                       G.packed, G.mask, status);
    res[0] = res[1] = res[2] = 0;
    he = hipMemcpyAsync(res, status, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(ctx->stream);
    if (he != hipSuccess) return fail(ctx, ISS_E_HIP, std::string("genome pack: ") + hipGetErrorString(he));
    return 0;
}

// The switches of the library -- each selects a code path the tests force: which indel path a model
// takes, the tile / guide-bit sweeps, the rounding guard of MT mode.  Read at iss_ctx_create, at every model upload and once
// per generate call (never per launch).
void read_switches(iss_ctx *ctx) {
    const char *e;
    ctx->light_below = (e = getenv("ISS_LIGHT_INDELS")) ? atof(e) : 2e-3;
    ctx->env_tiles = (e = getenv("ISS_TILES")) ? atoi(e) : 0;
    ctx->env_guide_bits = (e = getenv("ISS_GUIDE_BITS")) ? std::min(8, std::max(6, atoi(e))) : 0;
    ctx->mt_guard = (e = getenv("ISS_MT_GUARD")) ? atof(e) : 1e-6;
    ctx->debug_model = getenv("ISS_DEBUG_MODEL") != nullptr;
    ctx->env_chunk_pairs = (e = getenv("ISS_CHUNK_PAIRS")) ? std::max<int64_t>(1, atoll(e)) : 0;
    ctx->env_main_wgs = (e = getenv("ISS_MAIN_WGS")) ? std::max(1, atoi(e)) : 0;
    ctx->env_group = (e = getenv("ISS_MAIN_GROUP")) ? atoi(e) : -1;
    ctx->env_group_min = (e = getenv("ISS_MAIN_GROUP_MIN")) ? atoi(e) : 0;
    ctx->env_perfect = (e = getenv("ISS_PERFECT_KERNEL")) ? atoi(e) : 1;
}

void free_model(iss_ctx *ctx) {
    ctx->model_allocs.clear();
    ctx->have_model = false;
}

// the output set and the views into it (free_outputs follows a sync_all: nothing of the old buffers is in flight)
void free_outputs(iss_ctx *ctx) {
    ctx->os = {};
    for (auto &p : ctx->out) p = nullptr;
    ctx->flags = ctx->fix_list = nullptr;
    for (int k = 0; k < 2; ++k) { ctx->ev_count[k] = ctx->ev_list[k] = nullptr; ctx->read_list[k] = nullptr; ctx->read_list1[k] = nullptr; }
    for (auto &v : ctx->ev_call_valid) v = false;
    for (auto &v : ctx->ev_slot_valid) v = false;
}

// k_main_g: the instantiations (iterations per pass NI, passes per group NP) the library holds -- a group is at most five
// iterations (8 registers of rows each) -- and the choice of NP for a model.  X(NI, NP) with a trailing separator per entry.
#define ISS_MAIN_G_LIST(X) X(5, 1) X(4, 1) X(3, 1) X(2, 2) X(2, 1) X(1, 2)
#define ISS_MAIN_G_PTR(NI_, NP_) reinterpret_cast<const void *>(iss::k_main_g<true, NI_, NP_>),
constexpr uint32_t MAIN_GROUP_MIN_ROUND = 1;
constexpr int64_t MAIN_CHUNK_PAIRS = 12582912;  // pairs per launch of a call at most (generate_core; ISS_CHUNK_PAIRS overrides)
// Passes per group (0: k_main).  `want` (ISS_MAIN_GROUP) if the library holds it.  Else by the lane-items a wavefront defers per
// iteration, E = 64 (1 - (1 - p_defer)^16): a group should end with about one round's worth of entries (64 / E iterations), and a
// model that defers little gains less from patches in time than a closing round per group costs.  Measured, interleaved on one
// box (profiles/r06_ab_runs.txt; k_main ms per 5 M pairs, k_main -> k_main_g): HiSeq (E 18) 1.235 -> 1.12 with groups of 2 x 2
// iterations, 1.17 with 1 x 2; MiSeq (E 29) 4.03 -> 3.44 with 1 x 2, 3.64 with 2 x 2; NextSeq (E 23, four iterations per
// pass) 2.85 -> 2.60; NovaSeq (E 9, five iterations per pass) 1.155 -> 1.20: k_main stays.
static int main_group_passes(const iss::DevModel &M, int ni, int want) {
    const double e = 64.0 * (1.0 - std::pow(1.0 - std::min(std::max((double)M.p_defer, 0.0), 1.0), 16.0));
    if (want < 0 && e < 15.0) return 0;
    const int target = want > 0 ? want : std::max(1, (int)std::lround(64.0 / std::max(e, 1.0) / (double)ni));
    int best = 0;
#define ISS_MAIN_G_PICK(NI_, NP_) if (ni == NI_ && (want > 0 ? NP_ == want : (NP_ <= target && NP_ > best))) best = NP_;
    ISS_MAIN_G_LIST(ISS_MAIN_G_PICK)
#undef ISS_MAIN_G_PICK
    if (!best && want <= 0) {  // (no instantiation that small: the smallest one for ni)
#define ISS_MAIN_G_PICK(NI_, NP_) if (ni == NI_ && (!best || NP_ < best)) best = NP_;
        ISS_MAIN_G_LIST(ISS_MAIN_G_PICK)
#undef ISS_MAIN_G_PICK
    }
    return best;
}

// dynamic LDS of k_main: quality rows + deferred-work queues
size_t main_lds_bytes(const iss::DevModel &M) {
    return ((size_t)iss::MAIN_LUT_WORDS + M.tile_words + iss::MAIN_MUT_WORDS + (size_t)2 * M.TP * 4 + (size_t)(iss::MAIN_THREADS / 64) * iss::SLOW_RING * 3) * 4;
}

int settle_timing(iss_ctx *ctx) {
    static const int first[4] = {0, 1, 3, 5};
    for (auto &t : ctx->timed) {
        HIP_TRY(ctx, hipEventSynchronize(t.ev[2]));
        if (t.has_scan && t.ev[6]) HIP_TRY(ctx, hipEventSynchronize(t.ev[6]));
        for (int k = 0; k < 4; ++k) {
            if (k >= 2 && !t.has_scan) continue;
            hipEvent_t e_end = t.ev[first[k] + 1];
            if (k == 0 && t.scan_first && t.ev[3]) e_end = t.ev[3];
            if (k == 0 && t.ev[7]) e_end = t.ev[7];
            if (!t.ev[first[k]] || !e_end) continue;  // k_main-only timing
            float ms = 0.f;
            HIP_TRY(ctx, hipEventElapsedTime(&ms, t.ev[first[k]], e_end));
            ctx->ms_acc[k] += ms;
        }
    }
    ctx->timed.clear();  // (with their events)
    return 0;
}

// everything queued on both streams has finished
int sync_all(iss_ctx *ctx) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->setup_stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->indel_stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->fill_stream));
    if (ctx->emit_stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->emit_stream));
    return 0;
}

}  // namespace
