// iss_host_util.hip.h -- helpers every entry point uses: error reporting (into a context, or into the session base of the stand-alone
// device contexts), checked allocations into owning handles, checked uploads, the environment switches, what a model upload or a new
// reservation empties, the choice of the hot kernel's instantiation (k_main / k_main_g), its LDS size, timing, synchronisation.
#pragma once

// What the stand-alone device contexts (iss_bam, iss_fq, iss_inflate, iss_br, iss_fa) have in common: each derives from it and stays a C type
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

// iss_genome_upload_group and iss_genome_upload_fasta: where the records of a group stand (iss_generate_batch's arena layout) and how
// the group's one block is cut -- ascii | starts | status | packed | mask.
struct GroupPlan {
    std::vector<int64_t> starts;  // arena coordinates of the records that get a place, ascending
    std::vector<int32_t> which;   // starts[i] is record which[i] of the call
    size_t C = 0;                 // arena bases (a multiple of 32, 64 of padding behind the last record)
    size_t asc_b = 0, st_b = 0, stat_b = 0, pk_b = 0, mk_b = 0, total = 0;
};

// `ascii` (NULL: every record is there): a record without letters, of too many, or that is not there gets no place -- its id stays
// -1 and its single upload reports it
int group_plan(iss_ctx *ctx, const char *who, int32_t n, const int64_t *lengths, const uint8_t *const *ascii, GroupPlan &P) {
    P.starts.reserve((size_t)n + 1);
    P.which.reserve((size_t)n);
    int64_t coord = 64;
    for (int32_t k = 0; k < n; ++k) {
        if (lengths[k] < 1 || lengths[k] > iss::MAX_RECORD || (ascii && !ascii[k])) continue;
        P.starts.push_back(coord);
        P.which.push_back(k);
        coord += ((lengths[k] + 31) / 32) * 32 + 64;
        if (coord >= iss::MAX_RECORD) return fail(ctx, ISS_E_INVALID, std::string(who) + ": the records of one group must stay below 2^34 - 4096 bases");
    }
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t m = P.which.size();
    P.C = (size_t)coord;
    P.asc_b = up(P.C + 64), P.st_b = up(m * 8), P.stat_b = up(m * 16);
    P.pk_b = up((P.C / 16 + 2 + 16) * 4), P.mk_b = up((P.C / 32 + 2 + 8) * 4);
    P.total = P.asc_b + P.st_b + P.stat_b + P.pk_b + P.mk_b;
    return 0;
}

int group_stage_reserve(iss_ctx *ctx, size_t bytes) {
    if (bytes > ctx->group_stage.cap) {
        ctx->group_stage = {};
        PIN_ALLOC(ctx, ctx->group_stage.h, bytes);
        ctx->group_stage.cap = bytes;
    }
    return 0;
}

// the group's block, from the arena or its own, and the views into it
int group_block(iss_ctx *ctx, const GroupPlan &P, GenomeGroup &grp) {
    hipError_t he = hipSuccess;
    if (P.total <= ARENA_SLAB / 4) {
        grp.block = ctx->arena.take(P.total, &he);
    } else {
        (void)own_alloc_quiet(grp.own, P.total, &he);
        grp.block = grp.own;
    }
    if (!grp.block) return fail(ctx, ISS_E_HIP, std::string("genome group upload: ") + hipGetErrorString(he));
    grp.ascii = grp.block;
    grp.packed = reinterpret_cast<uint32_t *>(grp.block + P.asc_b + P.st_b + P.stat_b) + 2;
    grp.mask = reinterpret_cast<uint32_t *>(grp.block + P.asc_b + P.st_b + P.stat_b + P.pk_b) + 2;
    return 0;
}

// Behind what brings the arena's letters and the start coordinates into the block on the context's stream: status, packed and mask
// cleared, k_pack_group, the records' status rows read back into `res` (pinned, two words per placed record); waits for the stream.
int group_pack(iss_ctx *ctx, const GroupPlan &P, GenomeGroup &grp, unsigned long long *res) {
    const int32_t m = (int32_t)P.which.size();
    const int64_t *d_starts = reinterpret_cast<const int64_t *>(grp.block + P.asc_b);
    unsigned long long *d_status = reinterpret_cast<unsigned long long *>(grp.block + P.asc_b + P.st_b);
    hipError_t he = hipMemsetAsync(grp.block + P.asc_b + P.st_b, 0, P.stat_b + P.pk_b + P.mk_b, ctx->stream);
    if (he != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); return fail(ctx, ISS_E_HIP, std::string("genome group upload: ") + hipGetErrorString(he)); }
    const int64_t n_words = (int64_t)(P.C / 32);
    hipLaunchKernelGGL(iss::k_pack_group, dim3((unsigned)((n_words + iss::PACK_GROUP_THREADS - 1) / iss::PACK_GROUP_THREADS)),
                       dim3(iss::PACK_GROUP_THREADS), 0, ctx->stream, grp.ascii, n_words, d_starts, m, grp.packed, grp.mask, d_status);
    he = hipGetLastError();
    if (he == hipSuccess) he = hipMemcpyAsync(res, d_status, (size_t)m * 16, hipMemcpyDeviceToHost, ctx->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(ctx->stream);  // (also: the staging buffer is free again)
    if (he != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); return fail(ctx, ISS_E_HIP, std::string("genome group pack: ") + hipGetErrorString(he)); }
    return 0;
}

// the group joins the context, and its records that hold no letter outside the alphabet become genomes (the others: id -1)
int group_adopt(iss_ctx *ctx, const GroupPlan &P, GenomeGroup grp, const int64_t *lengths, const unsigned long long *res, int32_t *genome_ids) {
    const int32_t m = (int32_t)P.which.size();
    const int32_t gi = (int32_t)ctx->groups.size();
    uint32_t *const grp_packed = grp.packed, *const grp_mask = grp.mask;
    uint8_t *const grp_ascii = grp.ascii;
    ctx->groups.push_back(std::move(grp));
    for (int32_t i = 0; i < m; ++i) {
        if (res[2 * (size_t)i]) continue;  // letters outside the alphabet: id -1
        const int64_t s = P.starts[(size_t)i];
        Genome G;
        G.L = lengths[P.which[(size_t)i]];
        G.packed = grp_packed + s / 16;  // (views into the group's block: freed with the group)
        G.mask = grp_mask + s / 32;
        G.ascii = grp_ascii + s;
        G.has_exceptions = res[2 * (size_t)i + 1] != 0;
        G.group = gi;
        G.coord = s;
        ctx->genomes.push_back(std::move(G));
        genome_ids[P.which[(size_t)i]] = (int32_t)ctx->genomes.size() - 1;
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_inputs, ctx->stream));
    ctx->inputs_pending = true;
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
