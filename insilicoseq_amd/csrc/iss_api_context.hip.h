// iss_api_context.hip.h -- C ABI: version, build id, errors, context creation / destruction, the caller's stream.
#pragma once

extern "C" {

int iss_abi_version(void) { return ISS_ABI_VERSION; }

#ifndef ISS_BUILD_ID
#define ISS_BUILD_ID "unknown"
#endif
const char *iss_build_id(void) { return ISS_BUILD_ID; }

const char *iss_last_error(const iss_ctx *ctx) { return ctx ? ctx->last_error.c_str() : g_last_error.c_str(); }

int iss_ctx_create(int device_ordinal, iss_ctx **out) {
    if (!out) return fail(nullptr, ISS_E_INVALID, "iss_ctx_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, ISS_E_HIP, std::string("no HIP device available: ") + hipGetErrorString(e));
    if (device_ordinal < 0 || device_ordinal >= n) return fail(nullptr, ISS_E_INVALID, "device ordinal out of range");
    // (held until everything below has succeeded: a failure destroys the context, *out stays NULL and the message is the
    //  thread's last error, iss_last_error(NULL))
    std::unique_ptr<iss_ctx, void (*)(iss_ctx *)> guard(new iss_ctx(), iss_ctx_destroy);
    iss_ctx *ctx = guard.get();
    ctx->device = device_ordinal;
    HIP_TRY(ctx, hipSetDevice(device_ordinal));
    {
        hipDeviceProp_t prop;
        HIP_TRY(ctx, hipGetDeviceProperties(&prop, device_ordinal));
        ctx->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        const void *mains[8] = {reinterpret_cast<const void *>(iss::k_main<false, false, false>), reinterpret_cast<const void *>(iss::k_main<false, true, false>),
                                reinterpret_cast<const void *>(iss::k_main<true, false, false>), reinterpret_cast<const void *>(iss::k_main<true, true, false>),
                                reinterpret_cast<const void *>(iss::k_main<false, false, true>), reinterpret_cast<const void *>(iss::k_main<false, true, true>),
                                reinterpret_cast<const void *>(iss::k_main<true, false, true>), reinterpret_cast<const void *>(iss::k_main<true, true, true>)};
        for (const void *f : mains) HIP_TRY(ctx, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
        const void *grouped[] = {ISS_MAIN_G_LIST(ISS_MAIN_G_PTR)};
        for (const void *f : grouped) HIP_TRY(ctx, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
        HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(iss::k_mt_walk),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
        HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(iss::k_indel_fixup),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
        HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(iss::k_setup),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
        HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(iss::k_indel_scan),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
        const void *scripts[] = {reinterpret_cast<const void *>(iss::k_indel_script<false, 12, false>), reinterpret_cast<const void *>(iss::k_indel_script<true, 12, false>),
                                 reinterpret_cast<const void *>(iss::k_indel_script<false, 26, false>), reinterpret_cast<const void *>(iss::k_indel_script<true, 26, false>),
                                 reinterpret_cast<const void *>(iss::k_indel_script<false, 12, true>), reinterpret_cast<const void *>(iss::k_indel_script<true, 12, true>),
                                 reinterpret_cast<const void *>(iss::k_indel_script<false, 26, true>), reinterpret_cast<const void *>(iss::k_indel_script<true, 26, true>)};
        for (const void *f : scripts) HIP_TRY(ctx, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
    }
    ISS_TRY(stream_create(ctx, ctx->own_stream, hipStreamNonBlocking));
    ctx->stream = ctx->own_stream;
    ISS_TRY(stream_create(ctx, ctx->indel_stream, hipStreamNonBlocking));
    {   // The setup stream gets the highest priority: its hardware queue then comes from another pool than the main stream's
        // (streams of one priority share a few queues), and its small kernels are dispatched as soon as a CU has room.  Measured
        // with engines created one after the other in one process (tools/placement_probe.py, default bench's step): 1.25-1.26 ms
        // per step for every engine, against 1.24-1.29 (one box) and 1.28 / 1.41 alternating (another) at the default priority.
        int prio_least = 0, prio_greatest = 0;
        HIP_TRY(ctx, hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
        ISS_TRY(stream_create(ctx, ctx->setup_stream, hipStreamNonBlocking, prio_greatest));
        ISS_TRY(stream_create(ctx, ctx->fill_stream, hipStreamNonBlocking, prio_least));  // (MT mode: see iss_ctx::fill_stream)
        ISS_TRY(stream_create(ctx, ctx->emit_stream, hipStreamNonBlocking, prio_least));  // (MT mode's worker set: see iss_ctx::emit_stream)
    }
    for (auto &e : ctx->ev_call_done) ISS_TRY(event_create(ctx, e, hipEventDisableTiming));
    for (auto &e : ctx->ev_setup_done) ISS_TRY(event_create(ctx, e, hipEventDisableTiming));
    for (auto &e : ctx->ev_slot_done) ISS_TRY(event_create(ctx, e, hipEventDisableTiming));
    for (auto &e : ctx->ev_fork) ISS_TRY(event_create(ctx, e, hipEventDisableTiming));
    for (auto &e : ctx->ev_join) ISS_TRY(event_create(ctx, e, hipEventDisableTiming));
    ISS_TRY(event_create(ctx, ctx->ev_inputs, hipEventDisableTiming));
    if (const char *e = getenv("ISS_SETUP_AHEAD")) ctx->setup_ahead = atoi(e) != 0;  // 0: everything in order on one stream
    read_switches(ctx);
    DEV_ALLOC(ctx, ctx->fix_count, 256 / sizeof(uint32_t));  // FIX_SLOTS counters; +128 B stats; +192 B genome-pack status
    ctx->stats = reinterpret_cast<uint64_t *>(ctx->fix_count + 32);
    HIP_TRY(ctx, hipMemset(ctx->fix_count, 0, 256));
    DEV_ALLOC(ctx, ctx->read_count, (size_t)FIX_SLOTS * 2 * iss::SCAN_MAX_WGS);
    HIP_TRY(ctx, hipMemset(ctx->read_count, 0, sizeof(uint32_t) * FIX_SLOTS * 2 * iss::SCAN_MAX_WGS));
    ctx->max_main_grid = 2u * (unsigned)ctx->n_cu;
    *out = guard.release();
    return 0;
}

// What has an order: the writer threads stop (each flushes its pipe and waits for the kernels that use its buffers), the streams
// run dry, and the context goes -- its members release every buffer, event and stream.
void iss_ctx_destroy(iss_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    fastq_shutdown(ctx);
    append_stop(ctx, ctx->vq);
    append_stop(ctx, ctx->uq);
    append_stop(ctx, ctx->oq);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->indel_stream) (void)hipStreamSynchronize(ctx->indel_stream);
    if (ctx->fill_stream) (void)hipStreamSynchronize(ctx->fill_stream);
    if (ctx->setup_stream) (void)hipStreamSynchronize(ctx->setup_stream);
    if (ctx->emit_stream) (void)hipStreamSynchronize(ctx->emit_stream);
    ctx->timed.clear();  // (timings nobody read: their events)
    delete ctx;
}

int iss_ctx_set_stream(iss_ctx *ctx, void *hip_stream) {
    if (!ctx) return fail(nullptr, ISS_E_INVALID, "ctx is NULL");
    ISS_TRY(sync_all(ctx));
    ctx->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    return 0;
}

}  // extern "C"
