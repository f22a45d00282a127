// iss_api_mt.hip.h -- C ABI: the reference-identical mode (rng="mt") -- one worker per context (iss_generate_mt) and W workers side by side
// (iss_generate_mt_workers), custom fragment lengths, --store_mutations rows.  Both run a worker's chain (MtChain) through
// the same rules: mt_chain_generate is the single-worker path, the set's turn loop takes its other workers side by side.
#pragma once

namespace {

iss::DevGenome dev_genome(const Genome &G) { return iss::DevGenome{G.packed, G.mask, G.ascii, G.L, G.has_exceptions ? 1 : 0}; }

// ISS_MT_GUARD: how close to a rounding boundary the device still decides (tests widen it); read once per call
double mt_guard_env() {
    const char *e = getenv("ISS_MT_GUARD");
    return e ? atof(e) : 1e-6;
}

// The resolver (k_mt_resolve / k_mt_resolve_w + k_mt_emit) for plain runs; the sequential walker for indel-heavy models, the
// BasicErrorModel and perfect mode (walker only -- the resolver knows the KDE draws), and for the single pairs the resolver
// hands back.  The candidates (py ring, numpy ring in KB, digit rows in LDS) in order of preference: digit rows in LDS first,
// then the smallest rings that show a whole pair; each path maps the pick to its instantiation through this one list.  The 4 K python
// ring only ever wins where it makes room for the rows -- (4, 4, .) would need more than 246 positions for the numpy ring and at
// most 160 for the python ring, and (8, 2, no rows) fits wherever (4, 2, no rows) does -- so these five are all a model can reach.
#define ISS_MT_RESOLVERS(X) X(8, 2, true) X(4, 2, true) X(8, 4, true) X(8, 2, false) X(8, 4, false)
#define ISS_MT_RESOLVE_ONE(P_, N_, R_) iss::k_mt_resolve<P_, N_, R_>,
#define ISS_MT_RESOLVE_SET(P_, N_, R_) iss::k_mt_resolve_w<P_, N_, R_>,
constexpr size_t MT_LDS_BUDGET = 160 * 1024 - 256;
struct MtResolverPick { int idx = -1; size_t lds = 0; };  // idx: position in ISS_MT_RESOLVERS (-1: the walker only)
MtResolverPick mt_pick_resolver(const iss_ctx *ctx) {
    const iss::DevModel &M = ctx->M;
    const char *force = getenv("ISS_MT_PATH");  // "walk": sequential walker only (testing aid)
    MtResolverPick pick;
    if ((force && !strcmp(force, "walk")) || !(ctx->mt_bounce_rate < 0.05) || M.n_isize > 4096 || M.quality_mode != 0) return pick;
    struct Cand { int pyv, npv; bool rows; };
#define ISS_MT_CAND(P_, N_, R_) Cand{P_, N_, R_},
    const Cand cands[] = {ISS_MT_RESOLVERS(ISS_MT_CAND)};
#undef ISS_MT_CAND
    const uint32_t need_py = iss::mt_res_need_py(M.RL), need_np = iss::mt_res_need_np(M.RL);
    for (int i = 0; i < (int)(sizeof cands / sizeof cands[0]); ++i) {
        const Cand &c = cands[i];
        if (need_py > (uint32_t)c.pyv * 1024u || need_np > (uint32_t)c.npv * 1024u) continue;
        const size_t b = iss::mt_res_lds_bytes(M, c.pyv, c.npv, c.rows);
        if (b > MT_LDS_BUDGET) continue;
        pick.idx = i;
        pick.lds = b;
        break;
    }
    return pick;
}

// the walker's LDS: a fixed part, and the 16-bit digit rows (KDE models, where they fit) for turns of more than 64 pairs
struct MtWalkLds { size_t fixed, rows; bool use_rows; };
MtWalkLds mt_walk_lds(const iss::DevModel &M) {
    MtWalkLds l;
    l.fixed = iss::mt_walk_fixed_lds_bytes(M.RL);
    l.rows = (((size_t)2 * M.NB * M.RL * M.mt_row_w + 1) & ~(size_t)1) * 4;
    l.use_rows = M.quality_mode == 0 && l.rows + l.fixed <= 150 * 1024;
    return l;
}

// what both paths give the resolver of one worker's turn: its words, the turn, its results
iss::MtResolveArgs mt_resolve_args(const MtChain &c, int64_t n, int32_t sequence_type, int32_t gc_bias, iss::MtPairRec *rec, double guard) {
    iss::MtResolveArgs R{};
    R.py_base = c.buf[0][c.cur[0]];
    R.np_base = c.buf[1][c.cur[1]];
    R.py_off = (uint32_t)c.used[0];
    R.np_off = (uint32_t)c.used[1];
    R.py_fill = (uint32_t)c.fill[0];
    R.np_fill = (uint32_t)c.fill[1];
    R.py_cap = (uint32_t)c.cap[0];
    R.np_cap = (uint32_t)c.cap[1];
    R.n_pairs = n;
    R.sequence_type = sequence_type;
    R.gc_bias = gc_bias ? 1 : 0;
    R.gc_thr = MT_GC_THR;
    R.res = c.d_res;
    R.rec = rec;
    R.guard = guard;
    R.gauss = c.d_gauss;
    return R;
}

// ... and the walker: the words in front of the chain, the turn, its rows from row0
iss::MtWalkArgs mt_walk_args(const iss_ctx *ctx, const MtChain &c, int64_t n, int64_t row0, int64_t pair_base, int32_t sequence_type,
                             int32_t gc_bias, bool use_rows, double guard) {
    iss::MtWalkArgs A{};
    A.py = c.buf[0][c.cur[0]] + c.used[0];
    A.np = c.buf[1][c.cur[1]] + c.used[1];
    A.py_avail = (uint32_t)(c.fill[0] - c.used[0]);
    A.np_avail = (uint32_t)(c.fill[1] - c.used[1]);
    A.n_pairs = n;
    A.sequence_type = sequence_type;
    A.gc_bias = gc_bias ? 1 : 0;
    A.gc_thr = MT_GC_THR;
    for (int k = 0; k < 4; ++k) A.out[k] = ctx->out[k] + (size_t)row0 * ctx->M.row;
    A.res = c.d_res;
    A.use_rows = use_rows && n > 64 ? 1 : 0;  // staging the rows (one wavefront, tens of KB) only pays for a real batch
    A.pair_base = pair_base;
    A.guard = guard;
    A.gauss = c.d_gauss;
    return A;
}

// Words wanted for a turn: those of n + 1 pairs, plus `boost` more when a turn made no progress on them -- with gc_bias every
// rejected candidate pair (generator.py:82-92) consumes a whole pair's draws, and a turn of one pair that meets three
// rejections in a row needs more than two pairs' worth.  A turn that stopped starved with `want` words in front of it grows it.
int mt_grow_boost(iss_ctx *ctx, const iss::MtWalkResult &res, size_t py_avail, size_t np_avail, const size_t want[2], int64_t &boost) {
    if (res.n_done != 0 || !res.starved || py_avail < want[0] || np_avail < want[1]) return 0;
    if (boost >= 256) return fail(ctx, ISS_E_INVALID, "MT stream buffers too small for one read pair");
    boost = 2 * boost + 4;
    return 0;
}

// the context's own chain: buffers of at least cap_py / cap_np words, the unconsumed words carried over
int mt_reserve(iss_ctx *ctx, size_t cap_py, size_t cap_np) {
    MtChain &c = ctx->mt.chain;
    MtChainMem &own = ctx->mt.own;
    const size_t want[2] = {cap_py, cap_np};
    for (int s = 0; s < 2; ++s) {
        if (c.cap[s] >= want[s]) continue;
        std::vector<uint32_t> keep(c.fill[s] - c.used[s]);  // the unconsumed words
        if (!keep.empty()) HIP_TRY(ctx, hipMemcpy(keep.data(), c.buf[s][c.cur[s]] + c.used[s], keep.size() * 4, hipMemcpyDeviceToHost));
        c.cap[s] = 0;
        for (int b = 0; b < 2; ++b) { own.buf[s][b].reset(); c.buf[s][b] = nullptr; }
        for (int b = 0; b < 2; ++b) { DEV_ALLOC(ctx, own.buf[s][b], want[s]); c.buf[s][b] = own.buf[s][b]; }
        if (!keep.empty()) HIP_TRY(ctx, hipMemcpy(c.buf[s][0], keep.data(), keep.size() * 4, hipMemcpyHostToDevice));
        c.fill[s] = keep.size();
        c.cur[s] = 0;
        c.used[s] = 0;
        c.cap[s] = want[s];
    }
    return 0;
}

int mt_chain_peek(iss_ctx *ctx, MtChain &c, uint32_t *py_words, uint32_t *np_words, int32_t n) {
    const size_t want[2] = {(size_t)n, (size_t)n};
    ISS_TRY(mt_ensure(ctx, c, want));
    if (py_words) HIP_TRY(ctx, hipMemcpyAsync(py_words, c.buf[0][c.cur[0]] + c.used[0], (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (np_words) HIP_TRY(ctx, hipMemcpyAsync(np_words, c.buf[1][c.cur[1]] + c.used[1], (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// where a chain's --store_mutations rows go (mut NULL: nowhere): the context's own buffer (iss_generate_mt), or the region of a
// worker of the set; n: rows of the call so far, row0: the output row of the call's pair 0
struct MtRowSink { iss::MutRecord *mut; int64_t cap, n, row0; };

// The single-worker path: n_pairs pairs of genome_id into rows [out_first_pair, + n_pairs) from chain c's streams, in turns of
// c.ch pairs, the pairs counted in n_resolved / n_walked.  The context's own chain (iss_generate_mt), or a worker of the set for
// what its side-by-side loop does not do itself.  The chain's buffers are its owner's, reserved before the call.
int mt_chain_generate(iss_ctx *ctx, MtChain &c, int32_t genome_id, int64_t n_pairs, int32_t sequence_type, int32_t gc_bias,
                      int64_t out_first_pair, double guard, int64_t *n_done, int64_t &n_resolved, int64_t &n_walked, MtRowSink &rows) {
    const Genome &G = ctx->genomes[genome_id];
    const iss::DevModel &M = ctx->M;
    auto &m = ctx->mt;
    const int64_t CH = c.ch;
    const bool basic = M.quality_mode == 1;
    const bool kde = M.quality_mode == 0;  // (basic and perfect: walker only -- the resolver knows the KDE draws)
    const size_t py_need = iss::mt_py_need(M.RL), np_need = iss::mt_np_need(M.RL, M.quality_mode);
    if (!(M.RL < G.L)) {
        // the reference draws the insert size BEFORE its assertion fails (generator.py:121-126, 130)
        if (m.has_frag) {
            // np.random.normal(mu, sd) (generator.py:122): numpy's legacy polar Box-Muller -- a cached second value is used up,
            // else candidates of two doubles each are drawn until 0 < r2 < 1 and f * x1 is cached -- replayed on the host (libm)
            iss::MtGauss gs;
            HIP_TRY(ctx, hipMemcpy(&gs, c.d_gauss, sizeof gs, hipMemcpyDeviceToHost));
            if (gs.has_gauss) {
                gs.has_gauss = 0;
            } else {
                for (size_t used = 0;;) {
                    const size_t want[2] = {0, used + 256};
                    ISS_TRY(mt_ensure(ctx, c, want));
                    uint32_t w[256];
                    // (on the context's stream, which mt_ensure has made wait for the refill: the streams are non-blocking, a copy
                    //  on the null stream would not be ordered behind the fill kernel and the leftover copy)
                    HIP_TRY(ctx, hipMemcpyAsync(w, c.buf[1][c.cur[1]] + c.used[1] + used, sizeof w, hipMemcpyDeviceToHost, ctx->stream));
                    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                    bool done = false;
                    for (int k = 0; k < 64 && !done; ++k) {
                        auto res53 = [](uint32_t a, uint32_t b) { return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0); };
                        volatile double x1 = 2.0 * res53(w[4 * k], w[4 * k + 1]) - 1.0, x2 = 2.0 * res53(w[4 * k + 2], w[4 * k + 3]) - 1.0;
                        volatile double a2 = x1 * x1, b2 = x2 * x2;
                        volatile double r2 = a2 + b2;
                        used += 4;
                        if (r2 >= 1.0 || r2 == 0.0) continue;
                        volatile double f = -2.0 * log(r2);
                        f = f / r2;
                        f = sqrt(f);
                        gs.gauss = f * x1;
                        gs.has_gauss = 1;
                        gs.x1 = x1;
                        gs.x2 = x2;
                        done = true;
                    }
                    if (done) { c.used[1] += used; break; }
                }
            }
            HIP_TRY(ctx, hipMemcpyAsync(c.d_gauss, &gs, sizeof gs, hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            return fail(ctx, ISS_E_SHORT_RECORD, "record shorter than read length for this ErrorModel");
        }
        if (kde) {  // (Basic / PerfectErrorModel.random_insert_size is a constant: nothing is drawn)
            const size_t want[2] = {0, 2};
            ISS_TRY(mt_ensure(ctx, c, want));
            c.used[1] += 2;
        }
        return fail(ctx, ISS_E_SHORT_RECORD, "record shorter than read length for this ErrorModel");
    }
    if (n_pairs == 0) return 0;
    const iss::DevGenome dg = dev_genome(G);
    const MtWalkLds lds = mt_walk_lds(M);
    typedef void (*resolve_fn)(iss::DevModel, iss::DevGenome, iss::MtResolveArgs, iss::PairDesc *);
    static const resolve_fn resolvers[] = {ISS_MT_RESOLVERS(ISS_MT_RESOLVE_ONE)};
    const MtResolverPick pick = mt_pick_resolver(ctx);
    const resolve_fn resolve = pick.idx >= 0 ? resolvers[pick.idx] : nullptr;
    if (resolve) {
        HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(resolve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MT_LDS_BUDGET));
        if (!c.d_rec) {  // (the context's own chain; a worker of the set has its records from mt_set_reserve)
            DEV_ALLOC(ctx, m.own.d_rec, (size_t)CH);
            c.d_rec = m.own.d_rec;
        }
        if (!m.d_mut_off) {  // (sized for the longest turn: a set worker's chain takes shorter ones; the marker: the second of the two)
            DEV_ALLOC(ctx, m.d_mut_cnt, (size_t)2 * 8192);
            DEV_ALLOC(ctx, m.d_mut_off, (size_t)2 * 8192);
        }
    }
    if (basic && !m.d_amb) DEV_ALLOC(ctx, m.d_amb, 2 * iss::MT_AMB_CAP);  // phreds the host has to round, and its answers
    std::vector<iss::MtPhredAmb> ovq;  // answers for the pair that restarts
    int64_t done = 0;
    rows.n = 0;
    rows.row0 = out_first_pair;
    bool ov_valid = false, walk_one = false;
    int64_t ov_frag = 0;
    int64_t boost = gc_bias ? 4 : 0;  // (mt_grow_boost)
    while (done < n_pairs) {
        const int64_t n = walk_one ? 1 : std::min(CH, n_pairs - done);
        const size_t want[2] = {std::min(c.cap[0] / 624 * 624 - 624, (size_t)(n + 1 + boost) * py_need),
                                std::min(c.cap[1] / 624 * 624 - 624, (size_t)(n + 1 + boost) * np_need)};
        ISS_TRY(mt_ensure(ctx, c, want));
        MtPrefetch pf;
        if (!walk_one && done + n < n_pairs) {  // produce the next chunk's words while this chunk runs
            const int64_t n_next = std::min(CH, n_pairs - done - n);
            const size_t want_next[2] = {(size_t)(n_next + 1) * py_need, (size_t)(n_next + 1) * np_need};
            ISS_TRY(mt_prefetch_begin(ctx, c, want, want_next, &pf));
        }
        const int64_t row0 = out_first_pair + done;
        iss::MtWalkResult res{};
        if (resolve && !walk_one) {
            iss::MtResolveArgs R = mt_resolve_args(c, n, sequence_type, gc_bias, c.d_rec, guard);
            R.has_frag = m.has_frag ? 1 : 0;
            R.frag_mu = m.frag_mu;
            R.frag_sd = m.frag_sd;
            hipLaunchKernelGGL(resolve, dim3(1), dim3(iss::RES_THREADS), pick.lds, ctx->stream, M, dg, R, ctx->os.desc + row0);
            HIP_TRY(ctx, hipMemcpyAsync(&res, c.d_res, sizeof res, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipGetLastError());
            if (res.n_done > 0) {
                auto emit = [&](const iss::MtEmitMut &E) {
                    hipLaunchKernelGGL(iss::k_mt_emit, dim3((unsigned)((2 * res.n_done + 3) / 4)), dim3(256), 0, ctx->stream, M, dg,
                                       R.py_base, R.np_base, res.n_done, ctx->os.desc + row0, c.d_rec,
                                       ctx->out[0] + (size_t)row0 * M.row, ctx->out[1] + (size_t)row0 * M.row,
                                       ctx->out[2] + (size_t)row0 * M.row, ctx->out[3] + (size_t)row0 * M.row, E);
                };
                iss::MtEmitMut E{};
                if (!rows.mut) {
                    emit(E);
                } else {
                    // --store_mutations: count the rows of every mate, place them with a prefix sum, write them in order
                    const size_t items = (size_t)(2 * res.n_done);
                    E.mut_cnt = m.d_mut_cnt;
                    emit(E);
                    std::vector<int32_t> cnt(items);
                    HIP_TRY(ctx, hipMemcpyAsync(cnt.data(), m.d_mut_cnt, items * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
                    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                    std::vector<int64_t> off(items);
                    int64_t at = rows.n;
                    for (size_t k = 0; k < items; ++k) { off[k] = at; at += cnt[k]; }
                    HIP_TRY(ctx, hipMemcpyAsync(m.d_mut_off, off.data(), items * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
                    E.mut_cnt = nullptr;
                    E.mut_off = m.d_mut_off;
                    E.mut = rows.mut;
                    E.mut_cap = rows.cap;
                    E.pair_base = done;
                    emit(E);
                    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // `off` is pageable host memory
                    rows.n = at;
                }
            }
            c.used[0] += res.py_used;
            c.used[1] += res.np_used;
            ISS_TRY(mt_prefetch_commit(ctx, c, pf));
            done += res.n_done;
            n_resolved += res.n_done;
            if (res.pad) { walk_one = true; continue; }  // the next pair is not plain: one turn of the walker
            ISS_TRY(mt_grow_boost(ctx, res, R.py_fill - R.py_off, R.np_fill - R.np_off, want, boost));
            continue;
        }
        iss::MtWalkArgs A = mt_walk_args(ctx, c, n, row0, done, sequence_type, gc_bias, lds.use_rows, guard);
        A.mut = rows.mut;
        A.mut_cap = rows.cap;
        A.mut_base = rows.n;
        A.has_frag = m.has_frag ? 1 : 0;
        A.frag_mu = m.frag_mu;
        A.frag_sd = m.frag_sd;
        A.ov_valid = ov_valid ? 1 : 0;
        A.ov_frag = ov_frag;
        if (basic && A.guard > 0.45) A.guard = 0.45;  // (a test aid: > 0.5 would make every phred "ambiguous" twice over)
        A.amb = m.d_amb;
        A.ovq = m.d_amb ? m.d_amb + iss::MT_AMB_CAP : nullptr;
        A.n_ovq = (int32_t)ovq.size();
        if (!ovq.empty())
            HIP_TRY(ctx, hipMemcpyAsync(m.d_amb + iss::MT_AMB_CAP, ovq.data(), ovq.size() * sizeof(iss::MtPhredAmb),
                                        hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(iss::k_mt_walk, dim3(1), dim3(64), A.use_rows ? lds.fixed + lds.rows : lds.fixed, ctx->stream, M, dg, A,
                           ctx->os.desc + row0);
        HIP_TRY(ctx, hipMemcpyAsync(&res, c.d_res, sizeof res, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipGetLastError());
        c.used[0] += res.py_used;
        c.used[1] += res.np_used;
        ISS_TRY(mt_prefetch_commit(ctx, c, pf));
        done += res.n_done;
        n_walked += res.n_done;
        rows.n += res.n_mut;
        // host answers (phreds, fragment length) belong to the attempt that started the launch: they stay only if the
        // walk stopped again at that very attempt (gc_bias rejections move on to a new attempt of the same pair)
        const bool same_attempt = res.n_done == 0 && res.py_used == 0 && res.np_used == 0;
        if (!same_attempt) ovq.clear();
        if (res.need_host == 2) {
            // BasicErrorModel: phreds within the guard of a rounding boundary -- evaluated here exactly as numpy / the
            // reference do (libm): legacy_gauss f = sqrt(-2*log(r2)/r2); loc + scale*g; min(q, 0.9999);
            // int(round(-10 * log10(1 - p)))  (basic.py:52-53, util.py:44); the same pair restarts with the answers
            const int n_amb = std::min<int>(res.n_amb, iss::MT_AMB_CAP);
            std::vector<iss::MtPhredAmb> amb((size_t)n_amb);
            HIP_TRY(ctx, hipMemcpy(amb.data(), m.d_amb, amb.size() * sizeof(iss::MtPhredAmb), hipMemcpyDeviceToHost));
            for (auto &e : amb) {
                e.q = host_basic_phred(e.x1, e.x2, e.cached != 0, M.basic_mean, M.basic_sd, M.basic_cap);
                ovq.push_back(e);
            }
            if (ovq.size() > (size_t)iss::MT_AMB_CAP) return fail(ctx, ISS_E_INVALID, "too many undecidable phred scores in one pair");
            if (!same_attempt) ov_valid = false;  // (a restart of the SAME attempt keeps its host-evaluated fragment length)
            continue;
        }
        ov_valid = false;
        if (res.need_host) {
            // int(np.random.normal(mu, sd)) of the next pair with the host's libm, exactly as numpy's legacy_gauss:
            // f = sqrt(-2*log(r2)/r2); fresh value f*x2, cached value f*x1; loc + scale*g; int() truncates
            ov_frag = host_int_normal(res.host_x1, res.host_x2, res.host_cached != 0, m.frag_mu, m.frag_sd);
            ov_valid = true;
            continue;
        }
        ISS_TRY(mt_grow_boost(ctx, res, A.py_avail, A.np_avail, want, boost));
        if (res.n_done > 0) walk_one = false;
    }
    if (n_done) *n_done = done;
    return 0;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ reference-compatible MT mode
int iss_mt_seed(iss_ctx *ctx, uint64_t seed) {
    if (!ctx) return fail(nullptr, ISS_E_INVALID, "ctx is NULL");
    if (seed > 0xffffffffull) return fail(ctx, ISS_E_INVALID, "seed must be < 2^32 (numpy's legacy seeding raises)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ISS_TRY(sync_all(ctx));
    auto &c = ctx->mt.chain;
    if (!c.d_gauss) {  // (the marker: the last of the three)
        auto &own = ctx->mt.own;
        DEV_ALLOC(ctx, own.d_state, 2);
        DEV_ALLOC(ctx, own.d_res, 1);
        DEV_ALLOC(ctx, own.d_gauss, 1);
        c.d_state = own.d_state;
        c.d_res = own.d_res;
        c.d_gauss = own.d_gauss;
    }
    HIP_TRY(ctx, hipMemset(c.d_gauss, 0, sizeof(iss::MtGauss)));  // np.random.seed() drops the cached gaussian
    iss::MtState st[2];
    mt_seed_streams(st, (uint32_t)seed);
    HIP_TRY(ctx, hipMemcpy(c.d_state, st, sizeof st, hipMemcpyHostToDevice));
    c.fill[0] = c.fill[1] = c.used[0] = c.used[1] = 0;
    ctx->mt.seeded = true;
    return 0;
}

int iss_generate_mt(iss_ctx *ctx, int32_t genome_id, int64_t n_pairs, int32_t sequence_type, int32_t gc_bias,
                    int64_t out_first_pair, int64_t *n_done) {
    if (n_done) *n_done = 0;
    if (!ctx || !ctx->have_model) return fail(ctx, ISS_E_INVALID, "iss_generate_mt: upload a model first");
    if (!ctx->mt.seeded) return fail(ctx, ISS_E_INVALID, "iss_generate_mt: call iss_mt_seed first");
    if (genome_id < 0 || genome_id >= (int32_t)ctx->genomes.size()) return fail(ctx, ISS_E_INVALID, "unknown genome id");
    if (sequence_type != ISS_SEQ_METAGENOMICS && sequence_type != ISS_SEQ_AMPLICON)
        return fail(ctx, ISS_E_INVALID, "sequence type is not supported");
    if (n_pairs < 0 || out_first_pair < 0 || out_first_pair + n_pairs > ctx->os.capacity)
        return fail(ctx, ISS_E_INVALID, "output rows out of the reserved range");
    const iss::DevModel &M = ctx->M;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ISS_TRY(sync_all(ctx));
    ctx->last_first.clear();  // (this call's descriptors carry record coordinates: no batch's arena offsets apply to the rows any more)
    ctx->last_off.clear();
    auto &c = ctx->mt.chain;
    const size_t py_need = iss::mt_py_need(M.RL), np_need = iss::mt_np_need(M.RL, M.quality_mode);
    ISS_TRY(mt_reserve(ctx, 3 * ((size_t)(c.ch + 1) * py_need + 1248), 3 * ((size_t)(c.ch + 1) * np_need + 1248)));
    auto &m = ctx->mt;
    MtRowSink rows{m.d_mut, m.mut_cap, m.mut_n, m.mut_row0};
    const int rc = mt_chain_generate(ctx, c, genome_id, n_pairs, sequence_type, gc_bias, out_first_pair, mt_guard_env(), n_done,
                                     m.n_resolved, m.n_walked, rows);
    m.mut_n = rows.n;
    m.mut_row0 = rows.row0;
    m.mut_call = rc == 0 && m.d_mut != nullptr;
    return rc;
}

// ------------------------------------------------------------------ MT mode: W workers per launch (round 5)
// The reference's own parallelism is N workers, each a sequential chain over ITS two MT19937 streams seeded seed + cpu_number
// (iss/generator.py:234-236, iss/app.py:81-106).  One chain keeps one workgroup busy (k_mt_resolve: 2.3 us per NovaSeq pair);
// a set of W workers is W chains side by side: per turn ONE launch of each kernel of the path with one workgroup (k_mt_fill_w,
// k_mt_resolve_w, k_mt_walk_w) or one grid row (k_mt_emit_w) per worker, the jobs in tables in HBM.  Every worker's rows and
// stream positions are exactly those of iss_mt_seed(seed_w) + iss_generate_mt(...) in a context of its own.
namespace {

// the rows of a seeded set's workers, where iss_mt_workers_mutations_reserve asked for them: the pool, the counts (zero), the
// events of the ordering rule (mt_workers_generate).  The per-turn counts and places follow with the first call (they need the
// turn length).
int mt_set_rows_alloc(iss_ctx *ctx) {
    auto &t = ctx->mts;
    if (!t.W || !t.mut_rows || t.d_mut) return 0;
    const size_t W = (size_t)t.W;
    MtSetRows r;  // (all or nothing: a failure below leaves the set without rows, and d_mut -- the marker -- empty)
    if (own_alloc_quiet(r.d_mut, W * (size_t)t.mut_rows * sizeof(iss::MutRecord)))
        return fail(ctx, ISS_E_NOMEM, "iss_mt_workers_mutations_reserve: no device memory for " + std::to_string(t.W) + " x " + std::to_string(t.mut_rows) + " rows");
    DEV_ALLOC(ctx, r.d_mut_n, W);
    HIP_TRY(ctx, hipMemset(r.d_mut_n, 0, W * sizeof(int64_t)));
    PIN_ALLOC(ctx, r.h_mut_n, W);
    ISS_TRY(event_create(ctx, r.ev_place, hipEventDisableTiming));
    ISS_TRY(event_create(ctx, r.ev_walk, hipEventDisableTiming));
    r.mut_n.assign(W, 0);
    r.mut_row0.assign(W, 0);
    r.mut_pairs.assign(W, 0);
    static_cast<MtSetRows &>(t) = std::move(r);
    return 0;
}

}  // namespace

int iss_mt_workers_seed(iss_ctx *ctx, int32_t n_workers, const uint64_t *seeds) {
    if (!ctx || n_workers < 1 || n_workers > 1024 || !seeds) return fail(ctx, ISS_E_INVALID, "iss_mt_workers_seed: 1 .. 1024 workers");
    for (int32_t w = 0; w < n_workers; ++w)
        if (seeds[w] > 0xffffffffull) return fail(ctx, ISS_E_INVALID, "seed must be < 2^32 (numpy's legacy seeding raises)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ISS_TRY(sync_all(ctx));
    auto &t = ctx->mts;
    reset_part<MtSetRows>(t);  // the old set: its rows (the request, mut_rows, stays), its pools, its workers
    reset_part<MtSetPools>(t);
    reset_part<MtSetWorkers>(t);
    const size_t W = (size_t)n_workers;
    DEV_ALLOC(ctx, t.d_state, 2 * W);
    DEV_ALLOC(ctx, t.d_res, W);
    DEV_ALLOC(ctx, t.d_gauss, W);
    HIP_TRY(ctx, hipMemset(t.d_gauss, 0, W * sizeof(iss::MtGauss)));  // np.random.seed() drops the cached gaussian
    PIN_ALLOC(ctx, t.h_res, W);
    std::vector<iss::MtState> st(2 * W);
    for (size_t w = 0; w < W; ++w) mt_seed_streams(&st[2 * w], (uint32_t)seeds[w]);
    HIP_TRY(ctx, hipMemcpy(t.d_state, st.data(), st.size() * sizeof(iss::MtState), hipMemcpyHostToDevice));
    t.W = n_workers;
    t.started = t.poisoned = false;
    t.chains.assign(W, MtChain{});
    for (size_t w = 0; w < W; ++w) {
        MtChain &c = t.chains[w];
        c.d_state = t.d_state + 2 * w;
        c.d_res = t.d_res + w;
        c.d_gauss = t.d_gauss + w;
    }
    t.last_read.assign(4 * W, -1);
    t.n_resolved = t.n_walked = 0;
    return mt_set_rows_alloc(ctx);  // (a standing iss_mt_workers_mutations_reserve: the new workers' regions, their counts zero)
}

namespace {

// stream buffers, pair records and job tables of the set, sized for the model (called by every generate call; a model with longer
// reads than the buffers were cut for is refused: seed the set again)
int mt_set_reserve(iss_ctx *ctx) {
    auto &t = ctx->mts;
    const iss::DevModel &M = ctx->M;
    const size_t W = (size_t)t.W;
    const size_t need[2] = {iss::mt_py_need(M.RL), iss::mt_np_need(M.RL, M.quality_mode)};
    if (!t.ch) {
        const char *e = getenv("ISS_MT_SET_TURN");  // pairs per worker and turn (tests: many turns)
        // (98 304 / W within 512 .. 4096: a worker whose resolver meets a pair for the walker loses the rest of its turn, a turn costs
        //  ~0.4 ms beside its resolver -- measured flat between 1024 and 1536 at W = 64, 512 and 768 at W = 256; 4096 against 8192
        //  at W = 8: + 7 %)
        t.ch = e ? std::max<int64_t>(1, std::min<int64_t>(8192, atoll(e))) : std::max<int64_t>(512, std::min<int64_t>(4096, 98304 / (int64_t)W));
    }
    // A buffer holds K turns' words (worst case): the words produced ahead are APPENDED behind a stream's valid words while there
    // is room, and only at a buffer's end the stream moves to the other buffer, its unconsumed words copied in front (round 5: with
    // K = 3 and a move every turn, the moves of the workers whose turn had ended early -- nearly a whole turn's words each, ~ 400 MB
    // per turn at W = 64 -- were 1 ms of a 6.5 ms turn, on the critical path).  K = 8 where 32 GB (and half of the free memory) hold it, 3 at least.
    const size_t turn_words[2] = {(size_t)(t.ch + 1) * need[0] + 1248, (size_t)(t.ch + 1) * need[1] + 1248};
    if (!t.buf_turns) {
        const char *e = getenv("ISS_MT_SET_BUF_TURNS");  // (tests: 3 = a move every second turn)
        const size_t per_k = W * 2 * (turn_words[0] + turn_words[1]) * sizeof(uint32_t);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)64 << 30; }
        const size_t budget = std::min((size_t)32 << 30, free_b / 2);  // (half of what is free at most: other engines share the device)
        t.buf_turns = e ? std::max(3, std::min(8, atoi(e))) : (int)std::max<size_t>(3, std::min<size_t>(8, budget / per_k));
    }
    const size_t want[2] = {(size_t)t.buf_turns * turn_words[0], (size_t)t.buf_turns * turn_words[1]};
    if (t.cap[0] && (t.cap[0] < want[0] || t.cap[1] < want[1]))
        return fail(ctx, ISS_E_INVALID, "iss_generate_mt_workers: the set's stream buffers were sized for a model with shorter reads (seed the set again)");
    if (!t.cap[0]) {
        // (all or nothing: a reservation that failed half way leaves nothing behind and can be repeated -- the pools are made
        //  aside and moved into the set whole; cap[] marks the reservation as made)
        MtSetPools pools;
        const size_t jobs_bytes = (((4 * 2 * W) * std::max(sizeof(iss::MtFillJob), sizeof(iss::MtMoveJob)) +
                                    W * (sizeof(iss::MtResolveJob) + sizeof(iss::MtWalkJob) + sizeof(iss::MtEmitJob))) + 255) & ~(size_t)255;
        bool ok = true;
        for (int s = 0; s < 2 && ok; ++s)
            for (int b = 0; b < 2 && ok; ++b) ok = own_alloc_quiet(pools.buf[s][b], W * want[s] * sizeof(uint32_t)) == 0;
        ok = ok && own_alloc_quiet(pools.d_rec, 2 * W * (size_t)t.ch * sizeof(iss::MtPairRec)) == 0;
        ok = ok && own_alloc_quiet(pools.h_jobs, 2 * jobs_bytes) == 0;
        ok = ok && own_alloc_quiet(pools.d_jobs, 2 * jobs_bytes) == 0;
        if (!ok) {
            return fail(ctx, ISS_E_NOMEM, "iss_generate_mt_workers: no memory for the workers' stream buffers (W x " + std::to_string((want[0] + want[1]) * 2 * 4) + " bytes)");
        }
        for (auto &ev : pools.ev_emit) ISS_TRY(event_create(ctx, ev, hipEventDisableTiming));
        ISS_TRY(event_create(ctx, pools.ev_side, hipEventDisableTiming));
        ISS_TRY(event_create(ctx, pools.ev_turn, hipEventDisableTiming));
        pools.jobs_bytes = jobs_bytes;
        pools.cap[0] = want[0];
        pools.cap[1] = want[1];
        static_cast<MtSetPools &>(t) = std::move(pools);
        for (size_t w = 0; w < W; ++w) {  // the workers' slices
            MtChain &c = t.chains[w];
            for (int s = 0; s < 2; ++s) {
                c.cap[s] = want[s];
                for (int b = 0; b < 2; ++b) c.buf[s][b] = t.buf[s][b] + w * want[s];
            }
            c.d_rec = t.d_rec + w * (size_t)t.ch;  // (the first of its two sets of pair records: the single-worker path's)
            c.ch = t.ch;
        }
    }
    return 0;
}

}  // namespace

static int mt_workers_generate(iss_ctx *ctx, int32_t n_workers, const int32_t *genome_ids, const int64_t *n_pairs, const int64_t *out_first_pair,
                               int32_t sequence_type, int32_t gc_bias, int64_t *n_done, int32_t *status);

// A call that fails once it has begun (a HIP error, a draw the side-by-side path cannot take, stream buffers too small) returns in
// the middle of a turn: some workers' streams have advanced, rows are partly written, n_done / status say nothing for the others.
// The set is then POISONED -- every later call fails until iss_mt_workers_seed starts the workers anew -- instead of carrying on
// from undefined stream positions.  (A short record is not a failure: status[w] = ISS_E_SHORT_RECORD, the set goes on.)
int iss_generate_mt_workers(iss_ctx *ctx, int32_t n_workers, const int32_t *genome_ids, const int64_t *n_pairs, const int64_t *out_first_pair,
                            int32_t sequence_type, int32_t gc_bias, int64_t *n_done, int32_t *status) {
    if (ctx && ctx->mts.poisoned)
        return fail(ctx, ISS_E_INVALID, "iss_generate_mt_workers: an earlier call failed half way (the workers' streams and rows are undefined): call iss_mt_workers_seed again");
    if (ctx) ctx->mts.started = false;
    if (ctx) { ctx->last_first.clear(); ctx->last_off.clear(); }  // (record coordinates, as in iss_generate_mt)
    const int rc = mt_workers_generate(ctx, n_workers, genome_ids, n_pairs, out_first_pair, sequence_type, gc_bias, n_done, status);
    if (rc < 0 && ctx && ctx->mts.started) ctx->mts.poisoned = true;
    return rc;
}

static int mt_workers_generate(iss_ctx *ctx, int32_t n_workers, const int32_t *genome_ids, const int64_t *n_pairs, const int64_t *out_first_pair,
                               int32_t sequence_type, int32_t gc_bias, int64_t *n_done, int32_t *status) {
    if (!ctx || !ctx->have_model) return fail(ctx, ISS_E_INVALID, "iss_generate_mt_workers: upload a model first");
    auto &t = ctx->mts;
    if (n_workers < 1 || n_workers != t.W || !genome_ids || !n_pairs || !out_first_pair)
        return fail(ctx, ISS_E_INVALID, "iss_generate_mt_workers: call iss_mt_workers_seed for this many workers first");
    if (sequence_type != ISS_SEQ_METAGENOMICS && sequence_type != ISS_SEQ_AMPLICON)
        return fail(ctx, ISS_E_INVALID, "sequence type is not supported");
    if (ctx->mt.d_mut) return fail(ctx, ISS_E_INVALID, "iss_generate_mt_workers: this context holds single-worker --store_mutations rows (iss_mt_mutations_reserve): free them, the set's rows are iss_mt_workers_mutations_reserve");
    const int W = n_workers;
    const iss::DevModel &M = ctx->M;
    for (int w = 0; w < W; ++w) {
        if (n_done) n_done[w] = 0;
        if (status) status[w] = 0;
        if (n_pairs[w] == 0) continue;
        if (genome_ids[w] < 0 || genome_ids[w] >= (int32_t)ctx->genomes.size()) return fail(ctx, ISS_E_INVALID, "unknown genome id");
        if (n_pairs[w] < 0 || out_first_pair[w] < 0 || out_first_pair[w] + n_pairs[w] > ctx->os.capacity)
            return fail(ctx, ISS_E_INVALID, "output rows out of the reserved range");
        for (int v = 0; v < w; ++v)  // (the workers' rows must not overlap)
            if (n_pairs[v] > 0 && out_first_pair[w] < out_first_pair[v] + n_pairs[v] && out_first_pair[v] < out_first_pair[w] + n_pairs[w])
                return fail(ctx, ISS_E_INVALID, "iss_generate_mt_workers: two workers' output rows overlap");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ISS_TRY(sync_all(ctx));
    ISS_TRY(mt_set_reserve(ctx));
    // --store_mutations (iss_mt_workers_mutations_reserve): the rows of this call, per worker from 0
    const bool rows_on = t.d_mut != nullptr;
    if (rows_on && !t.d_mut_off) {  // (a worker's counts and places of one turn; the stride keeps them 16-byte aligned)
        const size_t stride = ((size_t)2 * (size_t)t.ch + 7) & ~(size_t)7;
        DEV_ALLOC(ctx, t.d_mut_cnt, (size_t)W * stride);
        DEV_ALLOC(ctx, t.d_mut_off, (size_t)W * stride);
        t.mut_stride = stride;
    }
    if (rows_on)
        for (int w = 0; w < W; ++w) {
            t.h_mut_n[w] = 0;
            t.mut_n[w] = 0;
            t.mut_row0[w] = out_first_pair[w];
            t.mut_pairs[w] = n_pairs[w];
        }
    auto region = [&](int w) { return rows_on ? t.d_mut + (size_t)w * (size_t)t.mut_rows : nullptr; };
    t.started = true;  // (from here on a failure leaves the set undefined)
    auto &m = ctx->mt;
    const bool basic = M.quality_mode == 1;
    const double guard = mt_guard_env();
    // the resolver (k_mt_resolve_w + k_mt_emit_w) for plain runs, the walker for indel-heavy models and for the single pairs the
    // resolver hands back -- the choice of the single-worker path
    typedef void (*resolve_fn)(iss::DevModel, const iss::MtResolveJob *);
    static const resolve_fn resolvers[] = {ISS_MT_RESOLVERS(ISS_MT_RESOLVE_SET)};
    const MtResolverPick pick = mt_pick_resolver(ctx);
    const resolve_fn resolve = pick.idx >= 0 ? resolvers[pick.idx] : nullptr;
    if (resolve) HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(resolve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MT_LDS_BUDGET));
    HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(iss::k_mt_walk_w), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MT_LDS_BUDGET));
    // ---- what the side-by-side loop does not do itself goes through the single-worker path, one worker after the other: records
    //      shorter than a read (the reference draws before its assertion fails), custom fragment lengths and the BasicErrorModel
    //      (draws the host's libm has to settle)
    struct WS { int64_t n = 0, done = 0, row0 = 0; int32_t gid = 0; bool walk_one = false; int64_t boost = 0; };
    std::vector<WS> ws((size_t)W);
    const bool one_by_one = m.has_frag || basic;
    for (int w = 0; w < W; ++w) {
        if (n_pairs[w] == 0) continue;
        const Genome &G = ctx->genomes[genome_ids[w]];
        if (one_by_one || !(M.RL < G.L)) {
            int64_t dn = 0;
            MtRowSink rows{region(w), t.mut_rows, 0, 0};  // (its own region of the pool, through the single-worker path's host placement)
            const int rc = mt_chain_generate(ctx, t.chains[w], genome_ids[w], n_pairs[w], sequence_type, gc_bias, out_first_pair[w], guard, &dn,
                                             t.n_resolved, t.n_walked, rows);
            if (rows_on) t.h_mut_n[w] = rows.n;
            if (n_done) n_done[w] = dn;
            if (rc == ISS_E_SHORT_RECORD) { if (status) status[w] = rc; continue; }
            if (rc) return rc;
            continue;
        }
        ws[w].n = n_pairs[w];
        ws[w].row0 = out_first_pair[w];
        ws[w].gid = genome_ids[w];
        ws[w].boost = gc_bias ? 4 : 0;
    }
    const size_t need[2] = {iss::mt_py_need(M.RL), iss::mt_np_need(M.RL, M.quality_mode)};
    // Words a turn is given: `need` is the most ONE attempt at a pair can consume (the kernels stop in front of a pair they
    // might not finish: "starved"), but a turn of n pairs consumes n times the USUAL amount -- a plain pair takes 2 x (10 (RL - 1)
    // + 2 RL) + ~2 words of `random` and 2 + 2 x (2 + 2 RL + 2 per substitution) (+ 2) of numpy, a gc_bias rejection a whole
    // pair's more (10 %) -- and what is left over is moved in front of the next turn's words: sized for the usual amount (+ 3 %,
    // + a few whole attempts), a turn leaves a few per cent of its words instead of half of numpy's.  A turn that runs out early
    // ends early, with its pairs done; the next one carries on.
    const double gcf = gc_bias ? 1.15 : 1.0;
    const double est[2] = {gcf * 1.03 * (2.0 * (10.0 * (M.RL - 1) + 2.0 * M.RL) + 4.0),
                           gcf * 1.03 * (2.0 + 2.0 * (2.0 + 2.0 * M.RL) + 8.0 * (0.02 * 2.0 * M.RL) + 4.0)};  // (2 words per substitution pick and mate... 2 % of the bases substituted: generous for every shipped model)
    auto words_for = [&](int s, int64_t n, int64_t boost) {
        return std::min((size_t)(n + 1 + boost) * need[s], (size_t)((double)n * est[s]) + (size_t)(4 + boost) * need[s]);
    };
    const MtWalkLds lds = mt_walk_lds(M);
    if (!m.ev_main) {
        ISS_TRY(event_create(ctx, m.ev_fill, hipEventDisableTiming));
        ISS_TRY(event_create(ctx, m.ev_main, hipEventDisableTiming));  // (the marker of the pair: last)
    }
    const size_t fm_sz = std::max(sizeof(iss::MtFillJob), sizeof(iss::MtMoveJob));
    std::vector<int64_t> n_w((size_t)W);
    std::vector<size_t> want(2 * (size_t)W);
    struct PF { bool on = false, append = false; size_t at = 0; uint32_t blocks = 0; };
    std::vector<PF> pf(2 * (size_t)W);
    std::vector<int> res_buf(2 * (size_t)W);
    const bool dbg = getenv("ISS_MT_SET_DEBUG") != nullptr;  // per call: turns, words produced / moved, pairs handed to the walker
    uint64_t dbg_turns = 0, dbg_moved[2] = {0, 0}, dbg_filled[2] = {0, 0}, dbg_bounce = 0, dbg_moves = 0, dbg_big = 0, dbg_pairs = 0, dbg_appends = 0, dbg_starved = 0, dbg_own = 0, dbg_skip = 0, dbg_ensure = 0;
    std::fill(t.last_read.begin(), t.last_read.end(), (int64_t)-1);  // (everything before this call has been waited for: sync_all above)
    // The running row counts live in device memory (zero; the rows of the workers that went one by one).  ORDER OF A WORKER'S ROWS
    // (the reference's: pairs in order, mate 0 before mate 1, positions ascending) -- whoever appends to a worker's region takes
    // its place from the worker's count and moves the count on, so the appenders of one worker must follow one another:
    //     place + write of turn t (emit stream)  ->  the walker behind turn t (main stream), or the worker's walker turn t + 1
    //     (side stream)  ->  place of turn t + 1 (emit stream).
    // Two events say so, and nothing else does: ev_place, recorded on the emit stream behind k_mt_mut_place_w (in front of the
    // writing pass: that one only reads the places), is waited for by the stream of every walker launch; ev_walk, recorded on the
    // main stream behind its walker (and behind its wait for the side stream's), is waited for by the emit stream in front of the
    // next k_mt_mut_place_w.  An event is re-recorded every turn and a wait takes its latest record: the one before in stream order.
    // A wait for an event that has no record yet (the first turn, or a walker before any emitter ran) is a no-op by HIP's rule:
    // nothing has been appended then, and the counts' upload below is on the main stream, in front of every launch of this call.
    if (rows_on) HIP_TRY(ctx, hipMemcpyAsync(t.d_mut_n, t.h_mut_n, (size_t)W * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    for (;;) {
        bool any = false;
        for (int w = 0; w < W; ++w) {
            n_w[w] = ws[w].done < ws[w].n ? (ws[w].walk_one ? 1 : std::min(t.ch, ws[w].n - ws[w].done)) : 0;
            any |= n_w[w] > 0;
        }
        if (!any) break;
        const int64_t turn = ++t.turns;  // (>= 1)
        const int par = (int)(turn & 1);
        // a buffer about to be WRITTEN (produced into, moved into) may still be read by an emitter: the one of two turns ago has
        // been waited for at the top of the turn, the one of the turn before only if a target says so
        auto read_by_last_turn = [&](int k, int b) { return t.last_read[(size_t)k * 2 + b] == turn - 1; };
        uint8_t *hj = t.h_jobs + (size_t)par * t.jobs_bytes, *dj = t.d_jobs + (size_t)par * t.jobs_bytes;
        auto tab = [&](size_t k, uint8_t *base) { return base + k * 2 * (size_t)W * fm_sz; };  // tables 0..3 (fill / move), then the rest
        iss::MtFillJob *h_fill_e = reinterpret_cast<iss::MtFillJob *>(tab(0, hj)), *h_fill_a = reinterpret_cast<iss::MtFillJob *>(tab(1, hj));
        iss::MtMoveJob *h_move_e = reinterpret_cast<iss::MtMoveJob *>(tab(2, hj)), *h_move_c = reinterpret_cast<iss::MtMoveJob *>(tab(3, hj));
        uint8_t *h_rest = tab(4, hj), *d_rest = tab(4, dj);
        iss::MtResolveJob *h_rj = reinterpret_cast<iss::MtResolveJob *>(h_rest);
        iss::MtWalkJob *h_wj = reinterpret_cast<iss::MtWalkJob *>(h_rest + (size_t)W * sizeof(iss::MtResolveJob));
        iss::MtEmitJob *h_ej = reinterpret_cast<iss::MtEmitJob *>(h_rest + (size_t)W * (sizeof(iss::MtResolveJob) + sizeof(iss::MtWalkJob)));
        auto dev_of = [&](const void *h) { return dj + (reinterpret_cast<const uint8_t *>(h) - hj); };
        hipStream_t s_side = ctx->setup_stream;  // the walker beside the resolver, the emitter beside the NEXT turn's resolver
        hipStream_t s_emit = ctx->emit_stream;
        // ---- (a) every worker of the turn has the words of n + 1 pairs (+ boost) in front of it: mt_ensure, for all at once
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, m.ev_fill, 0));  // (words produced ahead during the turn before)
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, t.ev_emit[par], 0));  // (this parity's pair records: their last reader, two turns ago)
        bool fill_e = false, move_e = false, wait_prev_e = false;
        for (int w = 0; w < W; ++w)
            for (int s = 0; s < 2; ++s) {
                const int k = 2 * w + s;
                MtChain &c = t.chains[w];
                h_fill_e[k] = iss::MtFillJob{nullptr, nullptr, 0u, 0u};
                h_move_e[k] = iss::MtMoveJob{nullptr, nullptr, 0u, 0u};
                want[k] = n_w[w] ? std::min(t.cap[s] / 624 * 624 - 624, words_for(s, n_w[w], ws[w].boost)) : 0;
                const size_t left = c.fill[s] - c.used[s];
                if (left >= want[k]) continue;
                const size_t missing = (want[k] - left + 623) / 624;
                ++dbg_ensure;
                if (c.fill[s] + missing * 624 <= t.cap[s]) {  // appended in place: nothing moves, nobody reads behind `fill`
                    h_fill_e[k] = iss::MtFillJob{c.d_state + s, c.buf[s][c.cur[s]] + c.fill[s], (uint32_t)missing, 0u};
                    c.fill[s] += missing * 624;
                    fill_e = true;
                    continue;
                }
                move_e = true;
                const int nxt = c.cur[s] ^ 1;
                h_move_e[k] = iss::MtMoveJob{c.buf[s][c.cur[s]] + c.used[s], c.buf[s][nxt], (uint32_t)left, 0u};
                const size_t room = (t.cap[s] - left) / 624;
                const uint32_t blocks = (uint32_t)std::min(room, (want[k] - left + 623) / 624);
                h_fill_e[k] = iss::MtFillJob{c.d_state + s, c.buf[s][nxt] + left, blocks, 0u};
                wait_prev_e |= read_by_last_turn(k, nxt);
                c.cur[s] = nxt;
                c.used[s] = 0;
                c.fill[s] = left + (size_t)blocks * 624;
                fill_e = true;
            }
        if (fill_e) {
            if (wait_prev_e) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, t.ev_emit[par ^ 1], 0));  // (the emitter of the turn before reads a buffer written now)
            if (move_e) {
                HIP_TRY(ctx, hipMemcpyAsync(dev_of(h_move_e), h_move_e, 2 * (size_t)W * sizeof(iss::MtMoveJob), hipMemcpyHostToDevice, ctx->stream));
                hipLaunchKernelGGL(iss::k_mt_move_w, dim3(2 * W, iss::MOVE_BLOCKS), dim3(256), 0, ctx->stream, reinterpret_cast<const iss::MtMoveJob *>(dev_of(h_move_e)));
            }
            HIP_TRY(ctx, hipEventRecord(m.ev_main, ctx->stream));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->fill_stream, m.ev_main, 0));  // (incl. the main stream's wait for that emitter)
            HIP_TRY(ctx, hipMemcpyAsync(dev_of(h_fill_e), h_fill_e, 2 * (size_t)W * sizeof(iss::MtFillJob), hipMemcpyHostToDevice, ctx->fill_stream));
            hipLaunchKernelGGL(iss::k_mt_fill_w, dim3(2 * W), dim3(iss::FILL_THREADS), 0, ctx->fill_stream, reinterpret_cast<const iss::MtFillJob *>(dev_of(h_fill_e)));
            HIP_TRY(ctx, hipEventRecord(m.ev_fill, ctx->fill_stream));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, m.ev_fill, 0));
        }
        // ---- (b) the words of the turn AFTER this one are produced beside it (mt_prefetch_begin)
        bool fill_a = false;
        for (int w = 0; w < W; ++w)
            for (int s = 0; s < 2; ++s) {
                const int k = 2 * w + s;
                MtChain &c = t.chains[w];
                pf[k] = PF{};
                h_fill_a[k] = iss::MtFillJob{nullptr, nullptr, 0u, 0u};
                if (!n_w[w] || ws[w].walk_one || ws[w].done + n_w[w] >= ws[w].n) continue;
                const int64_t n_next = std::min(t.ch, ws[w].n - ws[w].done - n_w[w]);
                const size_t want_next = words_for(s, n_next, 0);
                const size_t avail = c.fill[s] - c.used[s];
                if (avail >= want[k] + want_next) continue;
                // (only what is missing: everything in front of the turn is moved behind it -- a backlog would be copied every turn)
                const size_t blocks = (want[k] + want_next - avail + 623) / 624;
                if (c.fill[s] + blocks * 624 <= t.cap[s]) {  // appended in place (committed in (f) by moving `fill` on: no copy)
                    pf[k].on = true; pf[k].append = true; pf[k].blocks = (uint32_t)blocks;
                    h_fill_a[k] = iss::MtFillJob{c.d_state + s, c.buf[s][c.cur[s]] + c.fill[s], (uint32_t)blocks, 0u};
                    fill_a = true;
                    continue;
                }
                if (avail + blocks * 624 > t.cap[s]) continue;
                pf[k].on = true; pf[k].at = avail; pf[k].blocks = (uint32_t)blocks;
                h_fill_a[k] = iss::MtFillJob{c.d_state + s, c.buf[s][c.cur[s] ^ 1] + avail, (uint32_t)blocks, 0u};
                fill_a = true;
            }
        if (fill_a) {  // (behind everything queued on the main stream so far -- incl. its wait for the emitter of two turns ago -- and
                       //  ALWAYS behind the emitter of the turn before, whether that one still reads a target (the other buffer of a
                       //  stream at its buffer's end) or not (words appended): fill, emitter and resolver all three together is what
                       //  the resolver -- the chain the turn waits for -- loses by: 1.53 against 1.79e7 pairs/s at W = 64, 3.3
                       //  against 4.7e7 at W = 256 with the wait left out for appended words)
            HIP_TRY(ctx, hipEventRecord(m.ev_main, ctx->stream));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->fill_stream, m.ev_main, 0));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->fill_stream, t.ev_emit[par ^ 1], 0));
            HIP_TRY(ctx, hipMemcpyAsync(dev_of(h_fill_a), h_fill_a, 2 * (size_t)W * sizeof(iss::MtFillJob), hipMemcpyHostToDevice, ctx->fill_stream));
            hipLaunchKernelGGL(iss::k_mt_fill_w, dim3(2 * W), dim3(iss::FILL_THREADS), 0, ctx->fill_stream, reinterpret_cast<const iss::MtFillJob *>(dev_of(h_fill_a)));
            HIP_TRY(ctx, hipEventRecord(m.ev_fill, ctx->fill_stream));
        }
        // ---- (c) the turn: the resolver for the workers on the fast path, the walker for the others
        bool any_res = false, any_walk = false, walk_rows = false;
        for (int w = 0; w < W; ++w) {
            const MtChain &c = t.chains[w];
            const int64_t row0 = ws[w].row0 + ws[w].done;
            const bool walker = n_w[w] > 0 && (!resolve || ws[w].walk_one);
            iss::MtResolveJob &rj = h_rj[w];
            rj = iss::MtResolveJob{};
            iss::MtWalkJob &wj = h_wj[w];
            wj = iss::MtWalkJob{};
            if (n_w[w] > 0 && !walker) {
                rj.A = mt_resolve_args(c, n_w[w], sequence_type, gc_bias, t.d_rec + ((size_t)par * (size_t)W + (size_t)w) * (size_t)t.ch, guard);
                res_buf[2 * w] = c.cur[0];
                res_buf[2 * w + 1] = c.cur[1];
                rj.g = dev_genome(ctx->genomes[ws[w].gid]);
                rj.desc = ctx->os.desc + row0;
                any_res = true;
            } else if (walker) {
                wj.A = mt_walk_args(ctx, c, n_w[w], row0, ws[w].done, sequence_type, gc_bias, lds.use_rows, guard);
                wj.A.mut = region(w);
                wj.A.mut_cap = t.mut_rows;
                wj.A.mut_count = rows_on ? t.d_mut_n + w : nullptr;
                wj.g = dev_genome(ctx->genomes[ws[w].gid]);
                wj.desc = ctx->os.desc + row0;
                any_walk = true;
                walk_rows |= wj.A.use_rows != 0;
            }
        }
        HIP_TRY(ctx, hipMemcpyAsync(d_rest, h_rest, (size_t)W * (sizeof(iss::MtResolveJob) + sizeof(iss::MtWalkJob)), hipMemcpyHostToDevice, ctx->stream));
        if (any_walk) {  // (beside the resolver: other workers; behind the words and tables the main stream has waited for / copied)
            HIP_TRY(ctx, hipEventRecord(t.ev_turn, ctx->stream));
            HIP_TRY(ctx, hipStreamWaitEvent(s_side, t.ev_turn, 0));
            if (rows_on) HIP_TRY(ctx, hipStreamWaitEvent(s_side, t.ev_place, 0));  // (the rows of the turn before have their places)
            hipLaunchKernelGGL(iss::k_mt_walk_w, dim3(W), dim3(64), walk_rows ? lds.fixed + lds.rows : lds.fixed, s_side, M, reinterpret_cast<const iss::MtWalkJob *>(dev_of(h_wj)));
            HIP_TRY(ctx, hipEventRecord(t.ev_side, s_side));
        }
        if (any_res) hipLaunchKernelGGL(resolve, dim3(W), dim3(iss::RES_THREADS), pick.lds, ctx->stream, M, reinterpret_cast<const iss::MtResolveJob *>(dev_of(h_rj)));
        if (any_walk) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, t.ev_side, 0));
        if (any_walk && rows_on) HIP_TRY(ctx, hipEventRecord(t.ev_walk, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(t.h_res, t.d_res, (size_t)W * sizeof(iss::MtWalkResult), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipGetLastError());
        // ---- (d) the reads of the resolved pairs, all workers in one launch
        int64_t emit_max = 0;
        for (int w = 0; w < W; ++w) {
            iss::MtEmitJob &ej = h_ej[w];
            ej = iss::MtEmitJob{};
            if (!(n_w[w] > 0 && h_rj[w].A.n_pairs > 0) || t.h_res[w].n_done <= 0) continue;
            const int64_t row0 = ws[w].row0 + ws[w].done;
            ej.py = h_rj[w].A.py_base;
            ej.np = h_rj[w].A.np_base;
            ej.n_pairs = t.h_res[w].n_done;
            ej.desc = ctx->os.desc + row0;
            ej.rec = h_rj[w].A.rec;
            for (int k = 0; k < 4; ++k) ej.out[k] = ctx->out[k] + (size_t)row0 * M.row;
            ej.g = h_rj[w].g;
            if (rows_on) {
                ej.mut_cnt = t.d_mut_cnt + (size_t)w * t.mut_stride;
                ej.mut_off = t.d_mut_off + (size_t)w * t.mut_stride;
                ej.mut = region(w);
                ej.mut_cap = t.mut_rows;
                ej.pair_base = ws[w].done;
            }
            emit_max = std::max(emit_max, ej.n_pairs);
            for (int s = 0; s < 2; ++s) t.last_read[(size_t)(2 * w + s) * 2 + res_buf[2 * w + s]] = turn;
        }
        if (emit_max > 0) {  // (on its own stream: the next turn's resolver does not wait for it.  Launched here, in front of the walk
                             //  behind the turn, not after it: the walk would run on a quiet chip -- 0.19 ms beside the emitter --
                             //  but the emitter would reach 0.1 ms further into the next resolver: 1.89 against 1.92e7 pairs/s at
                             //  W = 64, 4.96 against 5.12e7 at W = 256)
            HIP_TRY(ctx, hipMemcpyAsync(dev_of(h_ej), h_ej, (size_t)W * sizeof(iss::MtEmitJob), hipMemcpyHostToDevice, s_emit));
            hipLaunchKernelGGL(iss::k_mt_emit_w, dim3((unsigned)((2 * emit_max + 3) / 4), (unsigned)W), dim3(256), 0, s_emit, M,
                               reinterpret_cast<const iss::MtEmitJob *>(dev_of(h_ej)));
            if (rows_on) {  // the counts of the pass above -> places (one workgroup per worker) -> the rows, and only the rows
                HIP_TRY(ctx, hipStreamWaitEvent(s_emit, t.ev_walk, 0));
                hipLaunchKernelGGL(iss::k_mt_mut_place_w, dim3((unsigned)W), dim3(iss::PLACE_THREADS), 0, s_emit,
                                   reinterpret_cast<const iss::MtEmitJob *>(dev_of(h_ej)), t.d_mut_n);
                HIP_TRY(ctx, hipEventRecord(t.ev_place, s_emit));
                hipLaunchKernelGGL(iss::k_mt_emit_rows_w, dim3((unsigned)((2 * emit_max + 3) / 4), (unsigned)W), dim3(256), 0, s_emit, M,
                                   reinterpret_cast<const iss::MtEmitJob *>(dev_of(h_ej)));
            }
        }
        HIP_TRY(ctx, hipEventRecord(t.ev_emit[par], s_emit));
        // ---- (e) what the turn consumed and produced; a resolver that stopped in front of a pair for the walker (an indel candidate,
        //      a letter outside ACGT, a genome end in a template) gets that ONE pair walked right here, behind the turn, so that
        //      its worker is back on the fast path with the next turn (a turn of its own for one pair cost a worker 1.5 turns
        //      per such pair: 21 turns instead of 16 for a call of 16 full ones at W = 64)
        bool any_odd = false;
        for (int w = 0; w < W; ++w) {
            if (!n_w[w]) continue;
            MtChain &c = t.chains[w];
            const iss::MtWalkResult &res = t.h_res[w];
            if (res.need_host) return fail(ctx, ISS_E_INVALID, "iss_generate_mt_workers: a draw for the host's libm on the side-by-side path");
            c.used[0] += res.py_used;
            c.used[1] += res.np_used;
            ws[w].done += res.n_done;
            if (dbg) { dbg_starved += res.starved != 0; dbg_own += ws[w].walk_one; }
            if (h_wj[w].A.n_pairs > 0) {  // (the walker's)
                const iss::MtWalkArgs &A = h_wj[w].A;
                t.n_walked += res.n_done;
                ISS_TRY(mt_grow_boost(ctx, res, A.py_avail, A.np_avail, &want[2 * w], ws[w].boost));
                if (res.n_done > 0) ws[w].walk_one = false;
            } else {
                const iss::MtResolveArgs &R = h_rj[w].A;
                t.n_resolved += res.n_done;
                if (res.pad) {
                    ++dbg_bounce;
                    ws[w].walk_one = true;  // (unless the walk behind this turn takes it)
                    any_odd = true;
                } else {
                    ISS_TRY(mt_grow_boost(ctx, res, R.py_fill - R.py_off, R.np_fill - R.np_off, &want[2 * w], ws[w].boost));
                }
            }
        }
        if (any_odd) {
            int n_odd = 0;
            for (int w = 0; w < W; ++w) {
                const bool odd = n_w[w] > 0 && h_rj[w].A.n_pairs > 0 && t.h_res[w].pad && ws[w].done < ws[w].n;
                const MtChain &c = t.chains[w];
                iss::MtWalkJob &wj = h_wj[w];
                wj = iss::MtWalkJob{};
                // (the words of one attempt at a pair must stand in front of the walker: else the pair waits for its own turn)
                const bool short_of_words = c.fill[0] - c.used[0] < 2 * need[0] || c.fill[1] - c.used[1] < 2 * need[1];
                if (dbg && odd && short_of_words) ++dbg_skip;
                if (!odd || short_of_words) continue;
                const int64_t row0 = ws[w].row0 + ws[w].done;
                wj.A = mt_walk_args(ctx, c, 1, row0, ws[w].done, sequence_type, gc_bias, false, guard);
                wj.A.mut = region(w);
                wj.A.mut_cap = t.mut_rows;
                wj.A.mut_count = rows_on ? t.d_mut_n + w : nullptr;
                wj.g = dev_genome(ctx->genomes[ws[w].gid]);
                wj.desc = ctx->os.desc + row0;
                ++n_odd;
            }
            if (n_odd) {
                HIP_TRY(ctx, hipMemcpyAsync(dev_of(h_wj), h_wj, (size_t)W * sizeof(iss::MtWalkJob), hipMemcpyHostToDevice, ctx->stream));
                if (rows_on) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, t.ev_place, 0));  // (this turn's rows have their places: the walked pair's come behind them)
                hipLaunchKernelGGL(iss::k_mt_walk_w, dim3(W), dim3(64), lds.fixed, ctx->stream, M, reinterpret_cast<const iss::MtWalkJob *>(dev_of(h_wj)));
                if (rows_on) HIP_TRY(ctx, hipEventRecord(t.ev_walk, ctx->stream));
                HIP_TRY(ctx, hipMemcpyAsync(t.h_res, t.d_res, (size_t)W * sizeof(iss::MtWalkResult), hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                HIP_TRY(ctx, hipGetLastError());
                for (int w = 0; w < W; ++w) {
                    if (h_wj[w].A.n_pairs <= 0) continue;
                    const iss::MtWalkResult &res = t.h_res[w];
                    if (res.need_host) return fail(ctx, ISS_E_INVALID, "iss_generate_mt_workers: a draw for the host's libm on the side-by-side path");
                    t.chains[w].used[0] += res.py_used;
                    t.chains[w].used[1] += res.np_used;
                    ws[w].done += res.n_done;
                    t.n_walked += res.n_done;
                    if (res.n_done > 0) ws[w].walk_one = false;  // (a gc_bias rejection, or starved: the pair takes a turn of its own)
                }
            }
        }
        // ---- (f) the streams move on (mt_prefetch_commit: the unconsumed words in front of those produced ahead)
        bool move_c = false, wait_prev_c = false;
        for (int w = 0; w < W; ++w)
            for (int s = 0; s < 2; ++s) {
                const int k = 2 * w + s;
                MtChain &c = t.chains[w];
                h_move_c[k] = iss::MtMoveJob{nullptr, nullptr, 0u, 0u};
                if (!n_w[w] || !pf[k].on) continue;
                if (pf[k].append) {
                    c.fill[s] += (size_t)pf[k].blocks * 624;
                    if (dbg) { dbg_filled[s] += (uint64_t)pf[k].blocks * 624; ++dbg_appends; }
                    continue;
                }
                const size_t left = c.fill[s] - c.used[s];  // <= pf.at
                const int nxt = c.cur[s] ^ 1;
                h_move_c[k] = iss::MtMoveJob{c.buf[s][c.cur[s]] + c.used[s], c.buf[s][nxt] + (pf[k].at - left), (uint32_t)left, 0u};
                wait_prev_c |= read_by_last_turn(k, nxt);
                if (dbg) { dbg_moved[s] += left; dbg_filled[s] += (uint64_t)pf[k].blocks * 624; ++dbg_moves; dbg_big += left > want[k] / 4; }
                c.cur[s] = nxt;
                c.used[s] = pf[k].at - left;
                c.fill[s] = pf[k].at + (size_t)pf[k].blocks * 624;
                move_c = true;
            }
        if (move_c) {
            if (wait_prev_c) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, t.ev_emit[par ^ 1], 0));  // (a target the emitter of the turn before reads)
            HIP_TRY(ctx, hipMemcpyAsync(dev_of(h_move_c), h_move_c, 2 * (size_t)W * sizeof(iss::MtMoveJob), hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(iss::k_mt_move_w, dim3(2 * W, iss::MOVE_BLOCKS), dim3(256), 0, ctx->stream, reinterpret_cast<const iss::MtMoveJob *>(dev_of(h_move_c)));
        }
        HIP_TRY(ctx, hipGetLastError());
        ++dbg_turns;
    }
    if (dbg) {
        for (int w = 0; w < W; ++w) dbg_pairs += (uint64_t)ws[w].done;
        fprintf(stderr, "[mt set] turns ended starved %llu, one-pair walker turns %llu, walks behind a turn skipped for words %llu, fills in front of a turn %llu\n",
                (unsigned long long)dbg_starved, (unsigned long long)dbg_own, (unsigned long long)dbg_skip, (unsigned long long)dbg_ensure);
        fprintf(stderr, "[mt set] W %d turn %lld: %llu turns, %llu pairs, %llu to the walker; %llu appended, commits with a move %llu (%llu moved > want / 4); words moved py %llu np %llu, "
                        "produced ahead py %llu np %llu\n", W, (long long)t.ch, (unsigned long long)dbg_turns, (unsigned long long)dbg_pairs,
                (unsigned long long)dbg_bounce, (unsigned long long)dbg_appends, (unsigned long long)dbg_moves, (unsigned long long)dbg_big, (unsigned long long)dbg_moved[0],
                (unsigned long long)dbg_moved[1], (unsigned long long)dbg_filled[0], (unsigned long long)dbg_filled[1]);
    }
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, m.ev_fill, 0));
    for (auto &e : t.ev_emit) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, e, 0));  // (the rows are complete once the main stream is)
    for (int w = 0; w < W; ++w)
        if (n_done && ws[w].n) n_done[w] = ws[w].done;
    if (rows_on) {  // the workers' row counts: what iss_vcf_emit_workers / iss_mt_workers_mutations_download take, and the overflow check
        HIP_TRY(ctx, hipMemcpyAsync(t.h_mut_n, t.d_mut_n, (size_t)W * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int w = 0; w < W; ++w) t.mut_n[w] = t.h_mut_n[w];
        for (int w = 0; w < W; ++w)
            if (t.mut_n[w] > t.mut_rows)  // (the rows past the region were dropped, never written elsewhere: the call fails, the set is poisoned)
                return fail(ctx, ISS_E_NOMEM, "iss_generate_mt_workers: worker " + std::to_string(w) + " made " + std::to_string(t.mut_n[w]) +
                                                  " mutation rows, iss_mt_workers_mutations_reserve holds " + std::to_string(t.mut_rows) + " per worker");
    }
    return 0;
}

int iss_mt_workers_mutations_reserve(iss_ctx *ctx, int64_t rows_per_worker) {
    if (!ctx || rows_per_worker < 0 || rows_per_worker > 0x7fffffff) return fail(ctx, ISS_E_INVALID, "iss_mt_workers_mutations_reserve: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ISS_TRY(sync_all(ctx));
    ISS_TRY(append_flush(ctx, ctx->vq));  // (a queued text's kernels read the pool)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    reset_part<MtSetRows>(ctx->mts);
    ctx->mts.mut_rows = rows_per_worker;
    return mt_set_rows_alloc(ctx);  // (a set seeded later gets its rows then)
}

int iss_mt_workers_mutations_download(iss_ctx *ctx, int32_t worker, iss_mutation *out, int64_t capacity, int64_t *n_total) {
    if (n_total) *n_total = 0;
    if (!ctx || worker < 0 || worker >= ctx->mts.W || capacity < 0) return fail(ctx, ISS_E_INVALID, "iss_mt_workers_mutations_download: bad argument");
    const auto &t = ctx->mts;
    if (!t.d_mut) return 0;
    if (n_total) *n_total = t.mut_n[(size_t)worker];
    const int64_t n = std::min(std::min(t.mut_n[(size_t)worker], t.mut_rows), capacity);
    if (n > 0 && out) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipMemcpy(out, t.d_mut + (size_t)worker * (size_t)t.mut_rows, (size_t)n * sizeof(iss::MutRecord), hipMemcpyDeviceToHost));
    }
    return 0;
}

/* iss_mt_peek for worker w of the set (tests: the stream positions after a run) */
int iss_mt_workers_peek(iss_ctx *ctx, int32_t worker, uint32_t *py_words, uint32_t *np_words, int32_t n) {
    if (!ctx || worker < 0 || worker >= ctx->mts.W || n < 0 || n > 624) return fail(ctx, ISS_E_INVALID, "iss_mt_workers_peek: bad argument");
    if (!ctx->have_model) return fail(ctx, ISS_E_INVALID, "iss_mt_workers_peek: upload a model first");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ISS_TRY(sync_all(ctx));
    ISS_TRY(mt_set_reserve(ctx));
    return mt_chain_peek(ctx, ctx->mts.chains[worker], py_words, np_words, n);
}

int iss_set_fragment(iss_ctx *ctx, int32_t enabled, double fragment_length, double fragment_sd) {
    if (!ctx) return fail(nullptr, ISS_E_INVALID, "ctx is NULL");
    ctx->has_frag = enabled != 0;
    ctx->frag_mu = fragment_length;
    ctx->frag_sd = fragment_sd;
    return 0;
}

int iss_mutations_reserve(iss_ctx *ctx, int64_t capacity) {
    if (!ctx || capacity < 0 || capacity > 0x7fffffff) return fail(ctx, ISS_E_INVALID, "iss_mutations_reserve: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ISS_TRY(sync_all(ctx));
    ctx->pmut = {};
    ctx->pmut_call = false;
    if (capacity) {
        DEV_ALLOC(ctx, ctx->pmut.d, (size_t)capacity);
        ctx->pmut.cap = capacity;
    }
    return 0;
}

int iss_mutations_download(iss_ctx *ctx, iss_mutation *out, int64_t capacity, int64_t *n_rows) {
    if (n_rows) *n_rows = 0;
    if (!ctx || capacity < 0) return fail(ctx, ISS_E_INVALID, "iss_mutations_download: bad argument");
    if (!ctx->pmut.d) return 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ISS_TRY(sync_all(ctx));
    uint32_t reserved = 0;
    HIP_TRY(ctx, hipMemcpy(&reserved, ctx->d_pmut_count, sizeof reserved, hipMemcpyDeviceToHost));
    if ((int64_t)reserved > ctx->pmut.cap) {
        if (n_rows) *n_rows = (int64_t)reserved;  // (the slots the call asked for: what a retry has to reserve)
        return fail(ctx, ISS_E_NOMEM, "mutation buffer too small for this call (reserve more with iss_mutations_reserve)");
    }
    std::vector<iss::MutRecord> rows(reserved);
    std::vector<uint32_t> flags((size_t)ctx->last_n);
    if (reserved) HIP_TRY(ctx, hipMemcpy(rows.data(), ctx->pmut.d, (size_t)reserved * sizeof(iss::MutRecord), hipMemcpyDeviceToHost));
    if (ctx->last_n)
        HIP_TRY(ctx, hipMemcpy(flags.data(), ctx->flags + ctx->last_row0, (size_t)ctx->last_n * sizeof(uint32_t),
                               hipMemcpyDeviceToHost));
    // keep: used slots; k_main's rows only for mates the fix-up did not rebuild.  Order: pair, mate, indel rows in
    // loop order (step, insertion slot / deletion) before the substitution rows in position order.
    std::vector<std::pair<uint64_t, uint32_t>> keyed;
    keyed.reserve(rows.size());
    for (uint32_t i = 0; i < rows.size(); ++i) {
        const iss::MutRecord &r = rows[i];
        if (r.pair < 0) continue;
        const int t = (uint8_t)r.type;
        const bool from_fixup = (t & 32) != 0;
        if (!from_fixup && (((flags[(size_t)r.pair] >> r.mate) | (flags[(size_t)r.pair] >> (2 + r.mate))) & 1u)) continue;
        const uint64_t phase = (t & 3) == 0 ? 1 : 0;
        const uint64_t key = ((uint64_t)(uint32_t)r.pair << 32) | ((uint64_t)(r.mate & 1) << 31) | (phase << 30) |
                             ((uint64_t)(uint16_t)r.position << 8) | (uint64_t)((t >> 2) & 7);
        keyed.emplace_back(key, i);
    }
    std::sort(keyed.begin(), keyed.end());
    if (n_rows) *n_rows = (int64_t)keyed.size();
    const int64_t n = std::min<int64_t>((int64_t)keyed.size(), capacity);
    for (int64_t i = 0; i < n && out; ++i) {
        const iss::MutRecord &r = rows[keyed[(size_t)i].second];
        out[i].pair = r.pair; out[i].mate = r.mate; out[i].type = (int8_t)(r.type & 3); out[i].position = r.position;
        out[i].ref = r.ref; out[i].alt = r.alt; out[i].quality = r.quality;
    }
    return 0;
}

int iss_mt_set_fragment(iss_ctx *ctx, int32_t enabled, double fragment_length, double fragment_sd) {
    if (!ctx) return fail(nullptr, ISS_E_INVALID, "ctx is NULL");
    ctx->mt.has_frag = enabled != 0;
    ctx->mt.frag_mu = fragment_length;
    ctx->mt.frag_sd = fragment_sd;
    return 0;
}

int iss_mt_mutations_reserve(iss_ctx *ctx, int64_t capacity) {
    if (!ctx || capacity < 0) return fail(ctx, ISS_E_INVALID, "iss_mt_mutations_reserve: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ISS_TRY(sync_all(ctx));
    auto &m = ctx->mt;
    m.d_mut.reset();
    m.mut_cap = m.mut_n = 0;
    m.mut_call = false;
    if (capacity) {
        DEV_ALLOC(ctx, m.d_mut, (size_t)capacity);
        m.mut_cap = capacity;
    }
    return 0;
}

int iss_mt_mutations_download(iss_ctx *ctx, iss_mutation *out, int64_t capacity, int64_t *n_total) {
    if (!ctx || capacity < 0) return fail(ctx, ISS_E_INVALID, "iss_mt_mutations_download: bad argument");
    static_assert(sizeof(iss_mutation) == sizeof(iss::MutRecord), "ABI and device mutation records differ");
    auto &m = ctx->mt;
    if (n_total) *n_total = m.mut_n;
    const int64_t n = std::min(std::min(m.mut_n, m.mut_cap), capacity);
    if (n > 0 && out) HIP_TRY(ctx, hipMemcpy(out, m.d_mut, (size_t)n * sizeof(iss::MutRecord), hipMemcpyDeviceToHost));
    return 0;
}

int iss_mt_path_counts(iss_ctx *ctx, int64_t *n_resolved, int64_t *n_walked) {
    if (!ctx) return fail(nullptr, ISS_E_INVALID, "ctx is NULL");
    if (n_resolved) *n_resolved = ctx->mt.n_resolved + ctx->mts.n_resolved;  // (single-worker calls + the worker set)
    if (n_walked) *n_walked = ctx->mt.n_walked + ctx->mts.n_walked;
    return 0;
}

int iss_mt_resolver_pick(iss_ctx *ctx, int32_t out[3]) {
    if (!ctx || !out) return fail(ctx, ISS_E_INVALID, "iss_mt_resolver_pick: bad argument");
    if (!ctx->have_model) return fail(ctx, ISS_E_INVALID, "iss_mt_resolver_pick: upload a model first");
    struct Cand { int32_t pyv, npv, rows; };
#define ISS_MT_CAND(P_, N_, R_) Cand{P_, N_, R_ ? 1 : 0},
    static const Cand cands[] = {ISS_MT_RESOLVERS(ISS_MT_CAND)};
#undef ISS_MT_CAND
    const MtResolverPick pick = mt_pick_resolver(ctx);
    out[0] = out[1] = out[2] = 0;
    if (pick.idx >= 0) { out[0] = cands[pick.idx].pyv; out[1] = cands[pick.idx].npv; out[2] = cands[pick.idx].rows; }
    return 0;
}

int iss_mt_peek(iss_ctx *ctx, uint32_t *py_words, uint32_t *np_words, int32_t n) {
    if (!ctx || !ctx->mt.seeded || n < 0 || n > 624) return fail(ctx, ISS_E_INVALID, "iss_mt_peek: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ISS_TRY(mt_reserve(ctx, 4 * 624, 4 * 624));
    return mt_chain_peek(ctx, ctx->mt.chain, py_words, np_words, n);
}

}  // extern "C"
