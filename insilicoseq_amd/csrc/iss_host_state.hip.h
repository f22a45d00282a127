// iss_host_state.hip.h -- host-side state of the engine: the records of the device-built outputs (the slot table, the writer's state and the
// append pipe they share; the FASTQ, VCF, unaligned-BAM and origins pipes), timed launches, and struct iss_ctx
// (one per GPU: streams, uploaded model and genomes, output rows, MT-mode chains and worker sets).  Included by iss_mi355x.hip.
#pragma once

namespace {

thread_local std::string g_last_error;

// Who owns what: a field a struct allocates and frees is one of these handles (iss_own.h: move-only, empty
// by default, released once, reads like a T*); a raw pointer beside them is a view, with a comment naming the block it points
// into.  A handle frees; it never waits for the device -- the synchronisation in front of a release stays where it was.
// (dev_alloc / pin_alloc, event_create / stream_create: iss_host_util.hip.h.)
inline void own_free_dev(void *p) { (void)hipFree(p); }
inline void own_free_pin(void *p) { (void)hipHostFree(p); }
inline void own_free_event(void *p) { (void)hipEventDestroy(static_cast<hipEvent_t>(p)); }
inline void own_free_stream(void *p) { (void)hipStreamDestroy(static_cast<hipStream_t>(p)); }
template <typename T> using DevMem = iss_own::Owned<T, own_free_dev>;
template <typename T> using PinMem = iss_own::Owned<T, own_free_pin>;
using Event = iss_own::Owned<std::remove_pointer_t<hipEvent_t>, own_free_event>;
using Stream = iss_own::Owned<std::remove_pointer_t<hipStream_t>, own_free_stream>;

// The handle releases what it held, then holds `bytes` of device (pinned: host) memory, or stays empty: ISS_E_NOMEM for out of
// memory, ISS_E_HIP for anything else, *err the HIP error.  No message: for the callers that format their own.
template <typename T, void (*Free)(void *)>
int own_alloc_quiet(iss_own::Owned<T, Free> &h, size_t bytes, hipError_t *err = nullptr) {
    h.reset();
    void *p = nullptr;
    const hipError_t e = Free == own_free_pin ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
    if (err) *err = e;
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? ISS_E_NOMEM : ISS_E_HIP;
    }
    h.reset(static_cast<T *>(p));
    return 0;
}

struct Genome {
    // a large record owns its three buffers (one leading pad word in packed and mask); a small one and a record of a group hold
    // none: packed, mask and ascii below then point into a GenomeArena slab or into their GenomeGroup's block
    DevMem<uint32_t> packed_own, mask_own;
    DevMem<uint8_t> ascii_own;
    uint32_t *packed = nullptr;  // views: packed_own + 1, or into the slab / the group's block
    uint32_t *mask = nullptr;    //        mask_own + 1, likewise
    uint8_t *ascii = nullptr;    //        ascii_own, likewise
    int64_t L = 0;
    bool has_exceptions = false;
    int32_t group = -1;     // iss_genome_upload_group: index into iss_ctx::groups; the buffers point into the group's arena
    int64_t coord = 0;      //   at this coordinate
    // iss_genome_upload_variants: the haplotype's lift tables, kept for iss_variants_lift (var_n == 0: none, the identity)
    DevMem<uint8_t> var_own;  // one block: out_pos [var_n + 1] | pos0 [var_n] | ref_len [var_n] | alt_len [var_n]
    int64_t var_n = 0;
    const int64_t *var_out_pos = nullptr, *var_pos0 = nullptr;    // views into var_own
    const int32_t *var_ref_len = nullptr, *var_alt_len = nullptr;  // likewise
};

// iss_genome_upload_group: records packed side by side in iss_generate_batch's arena layout (coordinate 64 first, 32-base
// aligned, 64 bases of padding between records); the arena iss_generate_batch uses as it is when a call's records are all
// of one group.  `block` is a GenomeArena slice, or for large groups an allocation of the group's own (`own`).
struct GenomeGroup {
    DevMem<uint8_t> own;
    uint8_t *block = nullptr;                     // view: `own`, or into a GenomeArena slab
    uint32_t *packed = nullptr, *mask = nullptr;  // views into block: word 0 = coordinate 0 (two readable words in front)
    uint8_t *ascii = nullptr;                     // view: block
};

// Records of a long work list (draft genomes: thousands of contigs) are small: their buffers are cut from slabs
// instead of three hipMallocs each, and their letters are checked on the host instead of waiting for the pack kernel.
constexpr size_t PK_PAD = 12;  // padding words of a packed genome: one in front (windows start a word early), the rest behind (the
                               // 16-byte window loads of k_indel_script may reach a few words past a read's window)
constexpr int64_t SMALL_RECORD = 1 << 20;
constexpr size_t ARENA_SLAB = 64u << 20;
struct GenomeArena {
    std::vector<DevMem<uint8_t>> slabs;
    size_t used = ARENA_SLAB;  // of the last slab
    uint8_t *take(size_t bytes, hipError_t *err) {  // a view into a slab
        bytes = (bytes + 255) & ~(size_t)255;
        if (used + bytes > ARENA_SLAB) {
            DevMem<uint8_t> slab;
            if (own_alloc_quiet(slab, ARENA_SLAB, err)) return nullptr;
            slabs.push_back(std::move(slab));
            used = 0;
        }
        uint8_t *r = slabs.back() + used;
        used += bytes;
        return r;
    }
};

// 0: outside util.rev_comp's alphabet (iss/util.py:57-88), 1: plain A/C/G/T, 2: IUPAC or lower case (an "exception")
inline int letter_class(uint8_t c) {
    if (c == 'A' || c == 'T' || c == 'C' || c == 'G') return 1;
    const bool letter = (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z');
    const uint8_t u = c & ~0x20u;
    const bool ok = letter && (u == 'A' || u == 'C' || u == 'G' || u == 'T' || u == 'Y' || u == 'R' || u == 'W' || u == 'S' ||
                               u == 'K' || u == 'M' || u == 'N' || u == 'B' || u == 'V' || u == 'D' || u == 'H');
    return ok ? 2 : 0;
}

constexpr int FIX_SLOTS_C = 16;  // (= FIX_SLOTS below)
struct TimedLaunch {
    // ev0 setup [ev3 scan + script ev4] ev1 main ev2 ev5 fixup ev6;  ev7: the end of the setup-stream kernels (k_setup, and for
    // models with frequent indels k_indel_scan + k_indel_script) when they run beside the previous call's kernels
    Event ev[8];
    bool has_scan;
    bool scan_first;  // the scan stands between k_setup and k_main on one stream (ev0 setup ev3 scan ev4 = ev1 main ev2)
};

constexpr int FIX_SLOTS = FIX_SLOTS_C;  // ring of fix-list / read-list counters (one per chunk in flight)

// What every device-built output shares on the host (the functions: iss_host_pipe.hip.h).
// The item table and the record ids of an emit call, per slot: a pinned host copy and the device copy the format kernels read.
template <typename Item>
struct SlotTable {
    struct Slot {
        PinMem<Item> h_items;
        DevMem<Item> d_items;
        PinMem<char> h_ids;
        DevMem<char> d_ids;
        size_t items_cap = 0, ids_cap = 0;
    } slot[2];
    int stage(iss_ctx *ctx, int slot, const std::vector<Item> &items, const std::string &ids, hipStream_t st);
};
// A pipeline's writer thread and what the caller shares with it: two slots, a pending error.
struct WriterSync {
    std::thread writer;
    std::mutex mu;
    std::condition_variable cv;
    bool busy[2] = {false, false};
    bool stop = false;
    std::string error;          // the first error of the writer since the caller last took it
    int error_code = ISS_E_IO;  // of `error`
};
// What a format does with a slot's bytes once their count is known: fetch them, check them, write them at `at`.  Returns the error
// ("": none) with *code (preset: ISS_E_IO); *advance (preset: true) says whether the pipe's `off` moves by `total`.
typedef std::string (*AppendWriteFn)(iss_ctx *ctx, int slot, uint64_t total, int64_t at, int *code, bool *advance);
// A device-built output appended to ONE file (VCF text, unaligned BAM, origins text): the format kernels run on the context's
// stream behind the generation, the size of a slot's bytes comes back in h_total, the writer thread fetches exactly those bytes
// on data_stream and appends them.  A format's per-job payload lies in slot-indexed arrays beside job_fd (a slot is busy from
// the moment its job is queued until the writer has popped it).
struct AppendPipe : WriterSync {
    bool ready = false;
    Stream data_stream;   // the writer thread's copies
    Stream copy_stream;   // the size's way back; empty: it rides the context's stream (VCF)
    Event ev_fmt[2], ev_copy[2];  // the writer waits for ev_copy, without a copy stream for ev_fmt
    PinMem<uint64_t> h_total[2];  // 64 bytes: bytes of the slot's output first
    int next = 0;
    int fd = -1;
    int64_t off = 0;  // of the file's next byte: moved by the writer thread (under `mu`) by what it wrote
    std::deque<int> jobs;  // slots, in call order
    int job_fd[2] = {-1, -1};
    bool unflushed = false;  // a job was queued since the last flush (the caller's side only: a text pipe's mode is switched while false)
    AppendWriteFn write = nullptr;
    const char *noun = nullptr;  // "the {noun}'s kernels failed"
};

// Device-formatted FASTQ on its way to the files: two slots of (device text, pinned host text) per mate; the
// format kernel runs on the context's stream, the copy back on a copy stream, the file writes on a writer thread.
struct FastqJob {
    int slot;
    size_t bytes;     // text bytes per file
    int fd[2];
    int64_t off[2];   // plain text: final offsets of this job's bytes (compressed: the writer keeps the running offsets)
    int threads;
    bool gzip;
    uint32_t n_blocks;
    std::vector<uint64_t> item_off;  // text offsets of the job's work items (the writer checks the record structure there)
    std::vector<int64_t> item_file_off;  // iss_fastq_emit_scatter: where each item's text goes in BOTH files (empty: the job is one piece at `off`)
};
// What a FASTQ text size reserves, [slot][mate], with the capacities it was made for: replaced as one (`= {}`) when a text outgrows it
// or the mode changes.  compressed mode: the compressed bytes land in h_text.
struct FastqBuffers {
    DevMem<uint8_t> d_text[2][2];
    PinMem<uint8_t> h_text[2][2];
    DevMem<uint8_t> d_comp[2][2];
    DevMem<uint32_t> d_bbytes[2][2], d_bcrc[2][2];
    DevMem<uint64_t> d_boff[2][2];
    PinMem<uint32_t> h_bcrc[2][2];
    size_t cap = 0;
    size_t comp_cap = 0;                 // bytes of d_comp / h_text per (slot, mate)
    uint32_t blocks_cap = 0;
};
struct FastqPipe : WriterSync, FastqBuffers {
    bool ready = false;
    Stream copy_stream;
    Event ev_fmt[2], ev_copy[2];
    SlotTable<iss::FastqItem> tab;
    int next = 0;
    int fd[2] = {-1, -1};
    // Offsets of the next byte of each file.  ONLY touched with `mu` held once the writer thread runs: in text mode the
    // caller advances them when it queues a job, in compressed mode the writer does when it knows a member's size
    // (round 2 advanced them outside the lock in text mode while the writer added its -- zero -- byte count under it:
    // a lost update there made the next job overwrite the previous one's bytes).
    int64_t off[2] = {0, 0};
    int64_t attached_off[2] = {0, 0};  // offsets when the files were attached ...
    int64_t accounted[2] = {0, 0};     // ... and the bytes queued (text) / written (gzip) since: off == attached_off + accounted
    std::deque<FastqJob> jobs;
    // compressed mode (iss_fastq_compress): per slot and mate the device-side state of iss_deflate.hip.h, the
    // compressed bytes land in h_text; the writer thread fetches exactly the bytes a member has
    int gzip = 0;
    Stream data_stream;
    DevMem<uint32_t> d_hist[2][2];
    DevMem<iss::DeflateCode> d_code[2][2];
    PinMem<uint64_t> h_total[2][2];  // one value
    uint32_t op_block[32];               // CRC operator "append DEFLATE_BLOCK zero bytes"
};
constexpr size_t FASTQ_ID_MAX = 4096;

// The BGZF stage of a text pipe (iss_origins_compress / iss_vcf_compress, iss_bgzf_text.hip.h; the functions:
// iss_host_bgzf_text.hip.h): per slot the members and their offsets (the writer thread and the copy stream read them), one set of
// work arrays (only kernels of the context's stream touch them, in order).  `cap` is the text size the buffers were made for.
struct BgzfTextBuffers {                       // replaced as one (`= {}`) when a text outgrows them
    size_t cap = 0, comp_cap = 0;
    uint32_t blocks_cap = 0;
    DevMem<uint8_t> d_comp[2];                 // the members, back to back
    PinMem<uint8_t> h_comp[2];
    DevMem<uint64_t> d_boff[2];                // [blocks_cap + 1]
    DevMem<uint32_t> d_dist;                   // [cap / 32 + 1]
    DevMem<uint32_t> d_bbytes, d_bcrc;         // [blocks_cap]
    DevMem<uint32_t> d_hist;
    DevMem<iss::BgzfTextCode> d_code;
};
struct BgzfTextStage : BgzfTextBuffers {
    int mode = 0;                              // 0: the pipe appends its text, 1: the text's BGZF members
    size_t job_text_cap[2] = {0, 0};           // the bound of the slot's text (the text's size comes back behind h_total: word 2)
};

// Device-formatted VCF text (--store_mutations): the kernels of iss_vcf.hip.h.  Its size copy rides the context's stream (no copy
// stream).  Two slots of text; the work arrays are one set (only kernels of the context's stream touch them, in order).
// work arrays: [slots_cap] key, slot, order, len; [slots_cap + 1] off; [pairs_cap] cnt; [pairs_cap + 1] seg; tile sums of the scans
struct VcfWork {                              // replaced as one (`= {}`) when a call outgrows them
    DevMem<uint32_t> d_key, d_slot, d_order, d_len, d_cnt;
    DevMem<uint64_t> d_off, d_seg, d_tiles;
    size_t slots_cap = 0, pairs_cap = 0, tiles_cap = 0;
};
struct VcfPipe : AppendPipe, VcfWork {
    struct Text {
        DevMem<uint8_t> d;
        size_t cap = 0;
    } text[2];
    struct HostText {                    // grown by the writer thread to the size a text has
        PinMem<uint8_t> h;
        size_t cap = 0;
    } host[2];
    SlotTable<iss::VcfItem> tab;
    PinMem<uint32_t> h_count;            // the slots a Philox call reserved
    DevMem<uint32_t> d_stats;            // ISS_VCF_DEBUG: k_vcf_count's two counters (they come back behind h_total)
    bool job_debug[2] = {false, false};
    // iss_vcf_emit_workers: the text of a slot is W byte ranges, range k appended to job_wfds[k] (empty: one file, job_fd)
    std::vector<int> job_wfds[2];
    struct WorkerBytes {                 // [wb_cap]: the workers' first rows (wbase), then their byte offsets
        PinMem<uint64_t> h;
        DevMem<uint64_t> d;
        size_t cap = 0;
    } wb[2];
    BgzfTextStage z;                     // iss_vcf_compress
};

// Unaligned BAM (--ubam): the records (k_ubam_format) and their BGZF members (iss_ubam.hip.h); the members' total size comes back
// on the copy stream.
struct UbamBuffers {                           // replaced as one (`= {}`) when a call outgrows them
    DevMem<uint8_t> d_text[2];                 // the record bytes (never leave the device)
    DevMem<uint8_t> d_comp[2];                 // the BGZF members, back to back
    PinMem<uint8_t> h_comp[2];
    size_t cap = 0, comp_cap = 0;
    uint32_t blocks_cap = 0;
    DevMem<uint32_t> d_bbytes[2], d_bcrc[2];
    DevMem<uint64_t> d_boff[2];
};
struct UbamPipe : AppendPipe, UbamBuffers {
    DevMem<uint32_t> d_hist[2];
    DevMem<iss::DeflateCode> d_code[2];
    SlotTable<iss::FastqItem> tab;
    uint32_t job_blocks[2] = {0, 0};           // members of the slot's job
};

// The origins text (--origins, iss_origins.hip.h): lengths, scan and format; the text's size comes back on the copy stream.  Two
// slots of (device text, pinned host text, item table, total); the work arrays (len, off, tile sums) are one set: only kernels of
// the context's stream touch them, in order.
struct OriginsText {                            // replaced as one (`= {}`) when a text outgrows it
    DevMem<uint8_t> d_text[2];
    PinMem<uint8_t> h_text[2];
    size_t cap = 0;                             // bytes of each of the four
};
struct OriginsWork {                            // likewise
    DevMem<uint32_t> d_len;                     // [pairs_cap]
    DevMem<uint64_t> d_off, d_tiles;            // [pairs_cap], [tiles_cap]
    size_t pairs_cap = 0, tiles_cap = 0;
};
struct OriginsPipe : AppendPipe, OriginsText, OriginsWork {
    DevMem<uint64_t> d_total[2];                // bytes of the slot's text (the scan's grand total)
    SlotTable<iss::OriginsItem> tab;
    BgzfTextStage z;                            // iss_origins_compress
};

// MT mode: one worker's chain -- its two MT19937 streams (CPython random, numpy), their word buffers and cursors.  A struct of
// VIEWS (it is copied): the chain of a context's own worker (iss_mt_seed / iss_generate_mt) points at the buffers of MtChainMem
// below, a worker of a set (iss_mt_workers_seed) at slices of the set's pools.  Only the owner allocates or frees them: the
// single-worker path (mt_chain_generate) works on whichever chain it is given.
struct MtChain {
    iss::MtState *d_state = nullptr;      // [2]: CPython random, numpy
    uint32_t *buf[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // stream x ping-pong (the next buffer: cur ^ 1)
    int cur[2] = {0, 0};
    size_t cap[2] = {0, 0}, fill[2] = {0, 0}, used[2] = {0, 0};
    iss::MtWalkResult *d_res = nullptr;
    iss::MtGauss *d_gauss = nullptr;
    iss::MtPairRec *d_rec = nullptr;  // k_mt_resolve -> k_mt_emit: stream offsets of one launch's pairs (`ch` of them)
    int64_t ch = 8192;                // pairs per turn of the single-worker path
};
// what the chain of a context's own worker points at (its cursors and capacities live in the chain: both are reset together)
struct MtChainMem {
    DevMem<iss::MtState> d_state;
    DevMem<uint32_t> buf[2][2];
    DevMem<iss::MtWalkResult> d_res;
    DevMem<iss::MtGauss> d_gauss;
    DevMem<iss::MtPairRec> d_rec;
};

// MT mode, W workers per launch (iss_mt_workers_seed / iss_generate_mt_workers): the reference's N workers (seed + cpu_number,
// iss/generator.py:234-236) as N chains side by side -- one workgroup per worker and kernel, job tables in HBM.  Three parts by
// who makes them, each with its sizes and each replaced as one (reset_part): the workers (iss_mt_workers_seed), the pools
// (mt_set_reserve, all or nothing) and the --store_mutations rows (mt_set_rows_alloc and the first call).
struct MtSetWorkers {
    int W = 0;
    int64_t ch = 0;                      // pairs per worker and turn
    int buf_turns = 0;                   // a stream buffer holds this many turns' words (worst case)
    DevMem<iss::MtState> d_state;        // [W][2]: CPython random, numpy
    std::vector<int64_t> last_read;      // [W * 2][2]: the turn whose emitter reads that buffer (-1: none in flight)
    DevMem<iss::MtWalkResult> d_res;     // [W]
    DevMem<iss::MtGauss> d_gauss;        // [W]
    PinMem<iss::MtWalkResult> h_res;     // [W]
    // [W]: the workers' chains, slices of the allocations here and in the pools (iss_mt_workers_seed; buffers and records from
    // mt_set_reserve)
    std::vector<MtChain> chains;
};
struct MtSetPools {
    size_t cap[2] = {0, 0};              // words per (worker, stream, ping-pong buffer); 0: the reservation has not been made
    // [stream][buffer]: W x cap[stream] words, two buffers.  A stream's words are appended to its current buffer turn after
    // turn; at the buffer's end the stream moves to the other one (mt_set_reserve).  Two: the words of turn t + 1 then go into
    // the buffer the emitter of turn t - 1 may still read, so that fill starts behind it.  (Three -- the fill never waits for
    // an emitter -- were built and measured in round 5: 3.1e7 against 4.2e7 pairs/s at W = 256: fill, emitter and resolver
    // then all start together and the resolver, the chain everything waits for, is the one that loses.)
    DevMem<uint32_t> buf[2][2];
    DevMem<iss::MtPairRec> d_rec;        // [2][W][ch]: the resolver of turn t + 1 runs beside the emitter of turn t
    Event ev_emit[2];                    // the emitter of the last turn of either parity
    Event ev_side, ev_turn;              // side stream (the walker beside the resolver) <-> main stream
    // job tables: pinned host staging + device copies, two sets (turn parity) of
    // [fill: ensure 2W | fill: ahead 2W | move: ensure 2W | move: commit 2W] and [resolve W | walk W | emit W]
    PinMem<uint8_t> h_jobs;
    DevMem<uint8_t> d_jobs;
    size_t jobs_bytes = 0;               // of ONE set
};
// --store_mutations in the set (iss_mt_workers_mutations_reserve): worker w owns rows
// [w * mut_rows, + mut_rows) of ONE pool and a running row count in device memory.
struct MtSetRows {
    DevMem<iss::MutRecord> d_mut;        // [W][mut_rows]
    DevMem<int64_t> d_mut_n;             // [W]: rows of the running call so far
    PinMem<int64_t> h_mut_n;             // [W]: set at a call's start, read back at its end
    DevMem<int32_t> d_mut_cnt;           // [W][mut_stride]: k_mt_emit_w's rows per (pair, mate) of a turn
    DevMem<int64_t> d_mut_off;           // [W][mut_stride]: their places (k_mt_mut_place_w)
    size_t mut_stride = 0;
    Event ev_place;                      // emit stream: the last k_mt_mut_place_w -> the walkers of the main and side streams
    Event ev_walk;                       // main stream: the last walker -> the next k_mt_mut_place_w
    std::vector<int64_t> mut_n, mut_row0, mut_pairs;  // [W]: rows, first output row and pairs of the last call's workers
};
struct MtSet : MtSetWorkers, MtSetPools, MtSetRows {
    bool started = false, poisoned = false;  // a call that fails after it began leaves streams and rows undefined: re-seed (iss_generate_mt_workers)
    int64_t turns = 0;
    int64_t n_resolved = 0, n_walked = 0;
    int64_t mut_rows = 0;                // rows per worker (0: off).  The request outlives a re-seeding, the storage is the set's.
};

// One group of a record -- its buffers with the sizes they were made for -- back to empty in one statement.
template <typename Part, typename Whole>
void reset_part(Whole &w) { static_cast<Part &>(w) = Part{}; }

}  // namespace

struct iss_ctx {
    int device = 0;
    int n_cu = 256;
    Stream own_stream;
    hipStream_t stream = nullptr;      // setup + main kernels.  A view: own_stream, or the caller's (iss_ctx_set_stream*)
    Stream indel_stream;  // the second k_indel_script launch of a heavy model's step, beside the first
    // MT mode: the stream words are produced here, one turn ahead of their consumption.  LOWEST priority: its hardware queue then
    // comes from another pool than the main stream's (as the setup stream's does, at the highest).  Streams of one priority share
    // four hardware queues, handed out as the streams are first used: with another engine and torch's streams alive in the process
    // (bench.py) the fill stream and the main stream of an MT-mode engine sat on ONE queue, fill and resolver ran one after the
    // other and a worker made 2.3e5 pairs/s instead of 3.8e5 (round 4's "2.2e5 in the bench line, 3.7e5 by itself";
    // tools/mt_context_probe2.py: 2.31e5 -> 3.84e5 with GPU_MAX_HW_QUEUES=8, and with this priority without the variable).
    Stream fill_stream;
    // k_setup of a call runs on its own stream, beside the kernels of the call (or chunk) before: it reads nothing they
    // write, and what it writes -- descriptors, flags, the fix-up list -- is double-buffered by call parity (`desc`, `flags`,
    // `fix_list` below point at the current call's set).  ISS_SETUP_AHEAD=0: everything in order on one stream.
    Stream setup_stream;
    // The worker set's emitter (k_mt_emit_w: 0.5 TB/s of reads over the whole chip, beside the NEXT turn's resolver): a stream of
    // its own at the lowest priority.  On the setup stream (highest priority) it took the resolvers' issue slots -- the chain the
    // turn waits for: 1.79 -> 1.90e7 pairs/s at W = 64, 4.70 -> 5.04e7 at W = 256.  A stream bound to a subset of the CUs
    // (hipExtStreamCreateWithCUMask, 32 .. 128 CUs) was worse than either: the emitter needs the chip (1.2 -> 2.1e7 at W = 64).
    Stream emit_stream;
    bool setup_ahead = true;
    Event ev_call_done[2];  // the last kernel of the last call that used the set
    bool ev_call_valid[2] = {false, false};
    Event ev_setup_done[FIX_SLOTS_C];         // k_setup of a chunk -> its k_main (ring, like the counters)
    Event ev_fork[FIX_SLOTS_C], ev_join[FIX_SLOTS_C];  // the two k_indel_script launches of a chunk side by side
    Event ev_slot_done[FIX_SLOTS_C];          // the last kernel of the chunk that used a counter slot: the setup stream waits
    bool ev_slot_valid[FIX_SLOTS_C] = {};     //   for it before the slot's next user clears the counters
    Event ev_inputs;                          // tables / arena copies queued on the main stream for this call's k_setup
    Event ev_handover[5];                     // iss_ctx_set_stream_ordered: the tails of the five streams, for the new main stream to wait for
    uint64_t call_seq = 0;
    bool inputs_pending = false;  // copies for this call's k_setup were queued on the main stream (ev_inputs)
    bool timing_all = false;      // HIP events around every kernel: one stream
    GenomeArena arena;
    // iss_generate_batch: the records of the last batch copied side by side into one arena (ids + items cached)
    struct Community {  // the arena's three buffers with what they hold (ids + items cached); replaced as one (`= {}`)
        std::vector<int32_t> ids;
        std::vector<iss::BatchItem> items;
        DevMem<uint32_t> packed, mask;
        DevMem<uint8_t> ascii;
        bool exceptions = false;
        int64_t cap = 0;  // bases the arena buffers hold
    } comm;
    struct ItemTables {  // device / pinned host, two sets: a call's launches may still read its set while the next is filled
        DevMem<iss::BatchItem> d_items[2];
        PinMem<iss::BatchItem> h_items[2];
        DevMem<int64_t> d_item_first[2];
        PinMem<int64_t> h_item_first[2];
        Event ev_items[2];
        size_t cap = 0;
    } it;
    uint64_t batch_seq = 0;
    uint64_t chunk_seq = 0;
    std::string last_error;
    // model
    bool have_model = false;
    iss::DevModel M{};
    std::vector<DevMem<void>> model_allocs;  // what the pointers of M point into
    // genomes
    std::vector<Genome> genomes;
    std::vector<GenomeGroup> groups;
    struct GroupStage {  // pinned staging of iss_genome_upload_group (letters, start coordinates, status read-back)
        PinMem<uint8_t> h;
        size_t cap = 0;
    } group_stage;
    struct VarLift {  // iss_variants_lift: the genomes' lift tables by genome id, rebuilt when genomes have come or gone
        DevMem<iss::VarLiftTab> d_tabs;
        size_t n = 0;  // genomes it covers
    } vl;
    // outputs: what iss_output_reserve allocates for `capacity` pairs, replaced as one (`= {}`, free_outputs)
    struct OutputSet {
        int64_t capacity = 0;
        DevMem<uint8_t> rows;  // ONE allocation of interleaved rows (iss::xp)
        struct Stage {         // iss_output_download: the four plain arrays of the rows being copied
            DevMem<uint8_t> d;
            size_t cap = 0;
        } stage;
        DevMem<iss::PairDesc> desc_buf[2], desc;  // desc: what the host reads (iss_output_download_coords) and the MT kernels write
        DevMem<uint32_t> flags_buf[2], fixl_buf[2];
        // indel events (k_indel_scan -> k_indel_script -> k_main), per row; two sets for the models whose scan runs on the setup
        // stream, beside the kernels of the call before (light models: one set, see the views below)
        DevMem<uint32_t> ev_count[2], ev_list[2];
        DevMem<uint4> read_list[2];
        DevMem<uint2> read_list1[2];  // (the reads with one event step: RunArgs::read_list1)
        // models with frequent indels: the edit scripts of the reads with an event (k_indel_script -> k_main), DevModel::sc_stride
        // bytes per read, two sets like the event lists
        DevMem<uint8_t> script[2];
    } os;
    // views of the output set, set by iss_output_reserve and free_outputs
    uint8_t *out[4] = {nullptr, nullptr, nullptr, nullptr};  // into os.rows: out[k] = os.rows + iss::row_array_off(k)
    uint32_t *flags = nullptr;     // os.flags_buf[0] (generate_core passes the current call's set itself)
    uint32_t *fix_list = nullptr;  // os.fixl_buf[0], likewise
    // the event and read lists by call parity: os.*[k] for a heavy model, os.*[0] for both parities of a light one
    uint32_t *ev_count[2] = {nullptr, nullptr}, *ev_list[2] = {nullptr, nullptr};
    uint4 *read_list[2] = {nullptr, nullptr};
    uint2 *read_list1[2] = {nullptr, nullptr};
    DevMem<uint32_t> fix_count;   // 256 bytes: one counter per launch chunk is reset in-stream; +128 B stats; +192 B genome-pack status
    DevMem<uint32_t> read_count;  // FIX_SLOTS x 2 x SCAN_MAX_WGS segment lengths of the two read lists, like fix_count
    double light_below = 2e-3;  // ISS_LIGHT_INDELS (read once, at iss_ctx_create): models whose reads have an event less often are "light"
    int env_tiles = 0, env_guide_bits = 0;  // ISS_TILES / ISS_GUIDE_BITS: tuning aids of the tile sweeps (0: the cost model decides)
    bool debug_model = false;               // ISS_DEBUG_MODEL
    int64_t env_chunk_pairs = 0;            // ISS_CHUNK_PAIRS: pairs per launch chunk at most (tests: a call of many chunks)
    int env_main_wgs = 0;                   // ISS_MAIN_WGS: workgroups of k_main / k_main_g at most (tests: many passes per workgroup from few pairs)
    int env_perfect = 1;  // ISS_PERFECT_KERNEL: quality mode 2 through k_perfect (1) or through k_main on the perfect tables (0)
    int env_group = -1, env_group_min = 0;  // ISS_MAIN_GROUP: passes per group of k_main_g (0: k_main; unset: chosen per model); ISS_MAIN_GROUP_MIN: min_round
    double mt_guard = 1e-6;                 // ISS_MT_GUARD: how close to a rounding boundary the device still decides (tests widen it)
    bool light = false;  // reads with an indel are rare (< ISS_LIGHT_INDELS of the reads, default 2e-3): all of them take k_indel_fixup
    double mt_bounce_rate = 0;  // MT mode: expected indel candidates per pair (decides resolver vs. sequential walker)
    // custom fragment length on the Philox path
    bool has_frag = false;
    double frag_mu = 0, frag_sd = 0;
    struct FragWork {  // replaced as one (`= {}`) when a call has more pairs
        DevMem<iss::FragAmb> d_amb;
        DevMem<uint32_t> d_ov_pairs;
        DevMem<int64_t> d_ov_frags;
        int64_t cap = 0;
    } fw;
    uint32_t *d_amb_count = nullptr;  // view into fix_count's block (+224 B)
    // --store_mutations on the Philox path
    struct PhiloxRows {
        DevMem<iss::MutRecord> d;
        int64_t cap = 0;
    } pmut;
    uint32_t *d_pmut_count = nullptr;  // view into fix_count's block (+240 B)
    bool pmut_call = false;              // a generate call has recorded rows under the reservation in force (iss_mutations_export)
    // iss_mutations_export's work arrays for the event rows (stages a and b of iss_vcf.hip.h): [slots] key, slot, order;
    // [pairs] cnt; [pairs + 1] seg; tile sums of the scan.  Only kernels of the context's stream touch them, in order.
    struct TruthWork {
        DevMem<uint32_t> d_key, d_slot, d_order, d_cnt;
        DevMem<uint64_t> d_seg, d_tiles;
        size_t slots_cap = 0, pairs_cap = 0, tiles_cap = 0;
    } tw;
    // iss_depth_finish's work array (tile sums of the scan, the table's rows in use and first windows: iss::DepthPlan), grown on
    // demand.  Only kernels of the context's stream touch it, in order.
    struct DepthWork {
        DevMem<uint8_t> d;
        size_t cap = 0;
    } dw;
    // iss_mutations_tally's work array: [pairs][2] u64, a read's rows by type (iss_errtally.hip.h), sized for the output rows on
    // first use and replaced when they grow.  Only kernels of the context's stream touch it, in order.
    struct ErrTallyWork {
        DevMem<uint64_t> d;
        size_t pairs_cap = 0;
    } ew;
    int64_t last_row0 = 0, last_n = 0;  // rows of the last iss_generate call (their flags tell which rows are stale)
    std::vector<int64_t> last_first;     // the last call was a batch: its item_first (rows last_row0 + ...), else empty
    std::vector<int64_t> last_off;       // ... and the arena offsets its descriptors carry
    unsigned max_main_grid = 0;
    std::string main_kernel;             // the hot kernel of the last Philox-mode call (iss_main_kernel)
    uint64_t *stats = nullptr;  // view into fix_count's block (+128 B)
    // reference-compatible MT19937 mode (iss_mt_compat.hip.h)
    struct {
        bool seeded = false;
        MtChain chain;  // the context's own worker: views of `own`
        MtChainMem own;
        bool has_frag = false;
        double frag_mu = 0, frag_sd = 0;
        DevMem<iss::MutRecord> d_mut;     // --store_mutations rows of the last iss_generate_mt call
        int64_t mut_cap = 0, mut_n = 0;
        int64_t mut_row0 = 0;             // ... whose pair 0 is this output row
        bool mut_call = false;            // an iss_generate_mt call has recorded rows under the reservation in force (iss_mutations_tally)
        Event ev_main, ev_fill;           // ordering between ctx->stream and the fill stream
        DevMem<iss::MtPhredAmb> d_amb;    // BasicErrorModel: [0, CAP) phreds for the host, [CAP, 2 CAP) its answers
        DevMem<int32_t> d_mut_cnt;        // k_mt_emit, --store_mutations: rows per (pair, mate), then their offsets
        DevMem<int64_t> d_mut_off;
        int64_t n_resolved = 0, n_walked = 0;  // pairs by path (statistics, iss_mt_path_counts)
    } mt;
    MtSet mts;
    FastqPipe fq;
    VcfPipe vq;
    UbamPipe uq;
    OriginsPipe oq;
    // timing
    bool timing = false, timing_main_only = false;
    std::vector<TimedLaunch> timed;
    double ms_acc[4] = {0, 0, 0, 0};
    int64_t n_launches = 0;
};
