/*
 * iss_mi355x.h -- C ABI of the MI355X (gfx950) read-generation engine.
 *
 * Drop-in boundary for ONE hot path of InSilicoSeq v2.0.1: the per-read loop of
 * `iss generate`.  Every entry point names the reference
 * interface it replaces (file:line into the reference tree).  Plain pointers and
 * sizes only; no torch / numpy types.  All functions return 0 on success and a
 * negative ISS_E_* code on failure (never exit()); iss_last_error() returns the
 * message of the last failure on that context (or the global one when ctx == NULL).
 *
 * Threading: one context per GPU; calls on one context are serialised by the
 * caller; contexts are independent across threads / processes (the reference's
 * workers share nothing either, iss/app.py:99-106).
 *
 * Arithmetic contract: every f64 comparison of the reference is carried out as an
 * exact integer comparison on 53-bit uniforms m = (w0>>5)*2^26 + (w1>>6) against
 * thresholds prepared on the host (floor/ceil of table*2^53, exact), see DESIGN.md.
 * Uniform words come from Philox4x32 (Salmon et al., SC'11; ten rounds, seven -- the fewest that pass
 * BigCrush -- for the hot digit blocks since ABI 6) addressed by
 * (seed, pair ordinal, attempt, kind, index, sub) -- the address map is part of the
 * contract and is documented in DESIGN.md ("RNG address map").
 */
#ifndef ISS_MI355X_H
#define ISS_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 8: (additive) iss_fa_create / iss_fa_destroy / iss_fa_last_error / iss_fa_index / iss_fasta_host_index / iss_fasta_tile /
 *    iss_fasta_scan_span / iss_genome_upload_fasta: a genome FASTA indexed and stripped on the device.
 *    (additive) iss_genome_upload_variants / iss_genome_download / iss_variants_lift / iss_variants_apply_tile / iss_variants_host_apply /
 *    iss_variants_host_lift: a VCF's alleles spliced into a record on the device, coordinates lifted back.
 *    (additive) iss_origins_compress / iss_vcf_compress / iss_bgzf_text_code_build: the origins and VCF text as BGZF members built on the device, copies
 *    from the line above.
 *    (additive) iss_origins_emit_batch / iss_origins_flush / iss_origins_host_text: every pair's source intervals as BEDPE text built
 *    on the device.
 *    (additive) iss_ubam_emit_batch / iss_ubam_flush / iss_ubam_host_records: the rows as unaligned BAM, records and BGZF
 *    blocks built on the device.
 *    (additive) iss_mt_workers_mutations_reserve / iss_mt_workers_mutations_download / iss_vcf_emit_workers: --store_mutations for
 *    the W workers of a set (rows per worker, placed on the device; one text job per call).
 *    (additive, like the three entries before them) iss_vcf_emit / iss_vcf_flush: the --store_mutations text built on the device.
 *    iss_main_kernel (which instantiation of the hot kernel the last Philox-mode call launched: k_main or k_main_g -- the
 *    rows of a group of passes wait in registers for their byte patches).
 * 7: W workers of the reference-identical mode side by side in one context (iss_mt_workers_seed, iss_generate_mt_workers,
 *    iss_mt_workers_peek); 36-bit coordinates in MT mode and the batch arena.
 * 6: indels inside k_main (edit scripts): iss_stats_read reports the scripted reads too; iss_build_id.
 * 5: the ErrorModel methods as batched entries (iss_gen_phred_scores, ...), iss_ev_step.
 * 4: device rows interleaved per pair (whole 128-byte lines per store, see iss_output_reserve), iss_output_row;
 *    Philox address map of the hot draws: three blocks per 16 bases.
 * 3: iss_fastq_compress / iss_deflate_code_build (gzip members built on the device), iss_generate_batch,
 *    iss_fastq_emit_batch (a whole work list per call).  2: iss_fastq_emit / iss_fastq_flush, MT-mode path counters. */
#define ISS_ABI_VERSION 8

#define ISS_E_INVALID (-1)     /* bad argument / model / genome content            */
#define ISS_E_HIP (-2)         /* HIP runtime failure (message has the hip error)  */
#define ISS_E_NOMEM (-3)
#define ISS_E_SHORT_RECORD (-4) /* read_length >= len(record): the reference's AssertionError,
                                   iss/generator.py:130 -> record skipped at :77-80 */
#define ISS_E_IO (-5)

#define ISS_SEQ_METAGENOMICS 0 /* iss/generator.py:134-135, 164-166 */
#define ISS_SEQ_AMPLICON 1     /* iss/generator.py:136-137, 167-169 */

typedef struct iss_ctx iss_ctx;

int iss_abi_version(void);
/* A hash of the kernel sources this library was compiled from (hex string; "unknown" for a build that did not pass
 * -DISS_BUILD_ID).  bench.py ties committed PMC traffic figures (profiles/ *_traffic.json) to the binary that runs. */
const char *iss_build_id(void);

/* One context = one GPU = one reference worker (`cpu_number`), iss/generator.py:223. */
int iss_ctx_create(int device_ordinal, iss_ctx **out);
void iss_ctx_destroy(iss_ctx *ctx);
const char *iss_last_error(const iss_ctx *ctx);

/* Optional: launch on a caller-owned hipStream_t (e.g. torch's current stream) instead of
 * the context's own stream.  NULL restores the context stream. */
int iss_ctx_set_stream(iss_ctx *ctx, void *hip_stream);

/*
 * Model tables, replaces KDErrorModel.__init__ / load_npz (iss/error_models/kde.py:24-50,
 * iss/error_models/__init__.py:27-50): the 13-key .npz flattened on the host
 * (insilicoseq_amd/model.py) and uploaded once to HBM.  All thresholds are integers in
 * [0, 2^53] (see header comment); orientation 0 = forward, 1 = reverse; base order A,T,C,G.
 */
typedef struct {
    int32_t read_length;
    int32_t n_isize;
    int32_t n_q;                 /* entries per per-position quality CDF (41)              */
    const uint64_t *isize_thr;   /* [n_isize]        floor(cdf*2^53): insert = #(thr <  m)  kde.py:97   */
    const uint64_t *bin_thr;     /* [2][4]           ceil (cdf*2^53): bin    = #(thr <= m)  kde.py:74   */
    const uint8_t *bin_nonempty; /* [2][4]                                                  kde.py:80   */
    const uint64_t *q_thr;       /* [2][4][RL][n_q]  floor: phred = #(thr < m)              kde.py:84   */
    const uint64_t *subst_thr;   /* [2][RL][4][3]    ceil : alt index = #(thr <= m)  __init__.py:95-97 */
    const uint8_t *subst_alt;    /* [2][RL][4][3]    ASCII alternatives                                */
    const uint64_t *ins_thr;     /* [2][RL][4]       ceil : insert iff m < thr       __init__.py:194   */
    const uint8_t *ins_letter;   /* [2][RL][4]       ASCII, in the dict's iteration order              */
    const uint64_t *del_thr;     /* [2][RL][4]       ceil : delete iff m < thr       __init__.py:209   */
    const uint64_t *mut_thr;     /* [n_q+1]          floor(phred_to_prob(q)*2^53): error iff m > thr   */
    /* BasicErrorModel (iss/error_models/basic.py:18-63), quality_mode 1: constant insert size (no draw), phred
     * scores int(round(-10 * log10(1 - min(np.random.normal(basic_mean, basic_sd), basic_cap)))) per position
     * (n_q + 1 must cover the phreds: 41 -> 0..41).  The reference-compatible mode (iss_generate_mt) draws the
     * normal deviates in the reference's order; iss_generate / iss_generate_batch invert q_thr like a KDE row, so
     * the caller puts the distribution of that score there (the same row at every position, in every bin;
     * insilicoseq_amd/model.py basic_phred_cdf).  The insert-size and bin tables are unused.
     * PerfectErrorModel (iss/error_models/perfect.py:14-52), quality_mode 2: constant insert size basic_insert_size (no
     * draw), every phred 40 (no quality draw; n_q + 1 must cover 0..40), mut_sequence's per-base draws as usual -- the caller
     * gives the substitution tables that make an error the base itself, upper-cased, and all-zero indel tables
     * (insilicoseq_amd/model.py DenseModel.perfect).  iss_generate / iss_generate_batch run k_perfect (the environment
     * switch ISS_PERFECT_KERNEL=0: k_main on the same tables, q_thr then all mass on 40); k_perfect writes no
     * --store_mutations rows (the reference's perfect model records none).  basic_mean / sd / cap are unused. */
    int32_t quality_mode;        /* 0: KDE tables (kde.py), 1: basic, 2: perfect                          */
    int32_t basic_insert_size;   /* basic.py:21 / perfect.py:19 (200)                                    */
    double basic_mean;           /* util.phred_to_prob(30), basic.py:24, :52                             */
    double basic_sd;             /* 0.01, basic.py:52                                                     */
    double basic_cap;            /* 0.9999, basic.py:52                                                   */
} iss_model_tables;

int iss_model_upload(iss_ctx *ctx, const iss_model_tables *tables);

/*
 * Genome upload, replaces handing `record.seq` to the worker (iss/generator.py:116,
 * pickled through iss/app.py:99-106).  ASCII in, validated against the reference's
 * rev_comp alphabet (iss/util.py:57-88; any other letter is the reference's KeyError and is
 * rejected here with ISS_E_INVALID); stored in HBM as 2-bit codes (A,T,C,G = 0..3) + a
 * 1-bit "exception" mask (IUPAC / lower case) + the ASCII copy the exceptions are read from.
 * 1 <= length <= 2^34 - 4096 (ABI 6: the reference takes records of 2^31 - 1 bases and more through its memmap
 * spill, iss/generator.py:313-331; ABI 7: iss_generate_mt takes them too -- 36-bit coordinates, two stream words per
 * `randrange` candidate once the bound passes 2^32, as CPython's getrandbits).
 */
int iss_genome_upload(iss_ctx *ctx, const uint8_t *ascii, int64_t length, int32_t *genome_id);
/* The same for a record of plain A/C/G/T handed over as 2-bit codes (16 bases per little-endian 32-bit word, base i in
 * bits 2*(i%16).., A,T,C,G = 0..3), from host memory or -- codes_on_device != 0 -- from device memory of this GPU: what a
 * rank of a multi-GPU run receives in the one RCCL broadcast of the packed genomes (no ASCII, no host bounce). */
int iss_genome_upload_packed(iss_ctx *ctx, const uint32_t *codes, int64_t length, int32_t codes_on_device, int32_t *genome_id);
/* n records in one go (draft contigs: thousands of short records): the host stages their letters in iss_generate_batch's
 * arena layout (the first record at coordinate 64, every record at a multiple of 32 bases, 64 bases of 'A' between records),
 * one copy takes them to the device, one kernel (k_pack_group) packs the whole group, and one read-back of a per-record
 * status table validates them.  genome_ids[k] is an ordinary genome id (every call takes it), or -1 for a record of no
 * letters, of letters outside the rev_comp alphabet or longer than iss_genome_upload takes: its iss_genome_upload reports
 * the error.  An iss_generate_batch call whose records are all of one group uses the group's buffers as its arena, with no
 * copy.  Groups are freed by iss_genome_clear.  (Additive in ABI 8.) */
int iss_genome_upload_group(iss_ctx *ctx, int32_t n, const uint8_t *const *ascii, const int64_t *lengths, int32_t *genome_ids);
int iss_genome_clear(iss_ctx *ctx);

/* Device output rows (R1 bases, R1 phred, R2 bases, R2 phred).  Reserve before generating.
 * On the HOST (iss_output_download, iss_fastq_write) they are four arrays [pairs][pitch],
 * pitch = 8*ceil(read_length/8) (ask iss_output_pitch).  On the DEVICE a pair owns one row of
 * row = 128*ceil(pitch/32) bytes; the 32 positions 32l..32l+31 are line l (128 bytes) of the row: bytes 0-63
 * mate 1, 64-127 mate 2, each four 16-byte pieces [8 bases][8 phreds], i.e. position p of array k
 * (0 R1 bases, 1 R1 phred, 2 R2 bases, 3 R2 phred) of pair i is byte
 * i*row + 128*(p/32) + 64*(k/2) + 16*((p/8)%4) + 8*(k%2) + p%8 (the kernel writes whole lines this way). */
int iss_output_reserve(iss_ctx *ctx, int64_t capacity_pairs);
int iss_output_pitch(const iss_ctx *ctx);
/* raw device pointers (for a caller that consumes the reads on the GPU / benchmarks): byte 0 of
 * each array's part of row 0 (layout above); iss_output_row = row */
int iss_output_device_ptrs(const iss_ctx *ctx, void **r1_base, void **r1_qual, void **r2_base, void **r2_qual);
int iss_output_row(const iss_ctx *ctx);

/*
 * The hot path: n_pairs read pairs from one record, replaces
 *   reads_generator + simulate_read            iss/generator.py:69-95, 98-192
 *   ErrorModel.introduce_indels / adjust_seq_length / introduce_error_scores / mut_sequence
 *                                              iss/error_models/__init__.py:158-228, 114-156, 52-67, 69-112
 *   KDErrorModel.gen_phred_scores / random_insert_size   iss/error_models/kde.py:52-98
 * Asynchronous on the context stream.  Pair k of the call is written to row
 * (out_first_pair + k) and draws its uniforms at Philox address (seed, first_ordinal + k).
 * `seed` is the worker seed (reference: seed + cpu_number, iss/generator.py:234-236).
 * Returns ISS_E_SHORT_RECORD (nothing launched) when read_length >= genome length.
 */
int iss_generate(iss_ctx *ctx, int32_t genome_id, int64_t n_pairs, uint64_t first_ordinal, uint64_t seed,
                 int32_t sequence_type, int32_t gc_bias, int64_t out_first_pair);

/*
 * The same for a whole work list in ONE set of launches (reads_generator over several work items,
 * iss/generator.py:69-95 + the loop of worker_iterator, :245-249): item k = (genome_ids[k], n_pairs[k]); its pairs take
 * the ordinals and output rows that n_items consecutive iss_generate calls would give them (first_ordinal /
 * out_first_pair onwards), so the rows are identical to those calls' -- without a kernel launch sequence per record.
 * The records are laid side by side in one device arena (kept until a call names another list of records) and pair
 * descriptors carry arena coordinates (36-bit like a single record's: the records of one call may hold 2^34 - 4096 bases
 * together, ISS_E_INVALID beyond -- ABI 7; 2^31 until then); iss_output_download_coords returns record coordinates as before.  Custom
 * fragment lengths (iss_set_fragment) apply as in iss_generate.  A record not longer than the read
 * length: ISS_E_SHORT_RECORD, nothing generated (leave such records out, as reads_generator skips them).
 */
int iss_generate_batch(iss_ctx *ctx, int32_t n_items, const int32_t *genome_ids, const int64_t *n_pairs,
                       uint64_t first_ordinal, uint64_t seed, int32_t sequence_type, int32_t gc_bias,
                       int64_t out_first_pair);

/* Custom fragment length on the Philox path (--fragment-length / --fragment-length-sd, iss/generator.py:121-123):
 * fragment = int(mu + sd * gaussian), each pair running its own polar Box-Muller loop on its K_FRAG uniforms
 * (nothing is cached across pairs).  Negative inserts, templates cut by the genome end and Python's slice rules
 * are honoured.  Values within 1e-6 of an integer are re-evaluated by the host with libm. */
int iss_set_fragment(iss_ctx *ctx, int32_t enabled, double fragment_length, double fragment_sd);

int iss_synchronize(iss_ctx *ctx);

/*
 * The inner plugin surface: the per-read methods of the reference's ErrorModel duck type, batched (n reads per call, read i
 * drawing at Philox ordinal first_ordinal + i of the worker stream `seed`, attempt 0; same address map as iss_generate, so a
 * read generated by iss_generate at that ordinal saw exactly these draws).  Host arrays in and out, rows of read_length bytes.
 *   iss_gen_phred_scores   KDErrorModel.gen_phred_scores(cdfs, orientation)      iss/error_models/kde.py:52-86
 *                          (through ErrorModel.introduce_error_scores, iss/error_models/__init__.py:52-67)
 *   iss_mut_sequence       ErrorModel.mut_sequence(record, orientation)           iss/error_models/__init__.py:69-112
 *                          seq in place (ASCII), quality = its phred scores; status[i] = 2: a letter the substitution table
 *                          does not hold (the reference's KeyError)
 *   iss_random_insert_size KDErrorModel.random_insert_size()                      iss/error_models/kde.py:88-98
 *   iss_introduce_indels   ErrorModel.introduce_indels(record, orientation, full_seq, bounds) incl. adjust_seq_length
 *                          iss/error_models/__init__.py:158-228, 114-156.  seq: n rows of read_length bytes holding seq_len[i]
 *                          letters in read direction; bounds: n x (read_start, read_end) in full_seq; status[i]: 0, 2 KeyError,
 *                          3 IndexError
 * orientation: 0 "forward", 1 "reverse".  Kept out of the hot path: one lane per read, exact 53-bit comparisons.
 */
int iss_gen_phred_scores(iss_ctx *ctx, int32_t orientation, int64_t n, uint64_t first_ordinal, uint64_t seed, uint8_t *quality);
int iss_mut_sequence(iss_ctx *ctx, int32_t orientation, int64_t n, uint64_t first_ordinal, uint64_t seed, uint8_t *seq,
                     const uint8_t *quality, int32_t *status);
int iss_random_insert_size(iss_ctx *ctx, int64_t n, uint64_t first_ordinal, uint64_t seed, int64_t *insert_size);
int iss_introduce_indels(iss_ctx *ctx, int32_t orientation, int64_t n, uint64_t first_ordinal, uint64_t seed, const uint8_t *seq,
                         const int32_t *seq_len, const uint8_t *full_seq, int64_t full_len, const int64_t *bounds, uint8_t *out,
                         int32_t *status);
/* One draw of the Philox path's indel event process, the sampler behind the tests `random() < p` of introduce_indels
 * (iss/error_models/__init__.py:193-196, :209), for n independent inputs: state cur[i] (the last test
 * slot decided, -1 .. 5 (read_length - 1) - 2), numerator m53[i] of the draw's uniform and v53[i] of the deletion sub-draw
 * (< 2^53) -> next[i] (new state), slot[i] (the test that fires, or -1: none in the rest of the state's segment), mask[i]
 * (bits 0-3: insertion of letter slot x, bits 4-7: the deletion fires if the base is A, T, C, G).  A test hook: the kernels
 * loop over the same device function; the CPU tests pin its CPU twin to the reference's probabilities. */
int iss_ev_step(iss_ctx *ctx, int32_t orientation, int64_t n, const int32_t *cur, const uint64_t *m53, const uint64_t *v53,
                int32_t *next, int32_t *slot, uint8_t *mask);

/* --store_mutations: one VCF row of the reference (iss/error_models/__init__.py:98-108, 197-221, written by
 * write_mutations, iss/generator.py:598-620). */
typedef struct {
    int32_t pair;     /* pair index i within the call (read id {record.id}_{i}_{cpu}/{mate+1}) */
    int8_t mate;      /* 0 forward, 1 reverse */
    int8_t type;      /* 0 substitution, 1 insertion (VCF alt = ref + alt), 2 deletion (alt '.') */
    int16_t position; /* 0-based (VCF POS = position + 1) */
    uint8_t ref, alt; /* ASCII */
    int16_t quality;  /* phred for substitutions, -1 ('.') otherwise */
} iss_mutation;
/* Philox path: after iss_mutations_reserve(capacity > 0) iss_generate records the rows of each call (capacity
 * counts 256-row reservation chunks per wavefront, so reserve generously: ~2 rows per expected mutation + 64 k);
 * iss_mutations_download waits for the call, drops the rows of reads the indel fix-up rebuilt, sorts into the
 * reference's order (pair, mate, indel rows in loop order, substitution rows by position) and returns them.
 * ISS_E_NOMEM when the buffer was too small for the call; *n_rows is then the number of row slots the call asked for. */
int iss_mutations_reserve(iss_ctx *ctx, int64_t capacity);
int iss_mutations_download(iss_ctx *ctx, iss_mutation *out, int64_t capacity, int64_t *n_rows);

/* Copy rows [first_pair, first_pair + n_pairs) to host arrays of pitch iss_output_pitch(). */
int iss_output_download(iss_ctx *ctx, int64_t first_pair, int64_t n_pairs, uint8_t *r1_base, uint8_t *r1_qual,
                        uint8_t *r2_base, uint8_t *r2_qual);

/* Per-pair coordinates (forward_start, reverse_start, reverse_end, insert_size) of rows
 * [first_pair, first_pair+n_pairs) as int64[n][4] -- iss/generator.py:135, 165-176. */
int iss_output_download_coords(iss_ctx *ctx, int64_t first_pair, int64_t n_pairs, int64_t *coords);

/*
 * Rows [first_pair, first_pair + n_pairs) as dense arrays in DEVICE memory the caller owns (a consumer that stays on the GPU: a
 * training or evaluation loop; additive in ABI 8).  Any of the four pointers may be NULL:
 *   d_bases  uint8 [n_pairs][2][read_length]  mate 1, then mate 2, bases as sequenced, no pitch padding -- a pair's 2 * read_length
 *            bytes start wherever they fall, no alignment is asked of the pointer.  ISS_EXPORT_ASCII: the bytes
 *            iss_output_download returns; ISS_EXPORT_CODES: A, C, G, T -> 0, 1, 2, 3 (alphabetical -- not the engine's A, T, C, G),
 *            upper or lower case, every other letter 4
 *   d_qual   uint8 [n_pairs][2][read_length]  the phred scores iss_output_download returns
 *   d_coords int64 [n_pairs][4]               what iss_output_download_coords returns (record coordinates, not arena coordinates)
 *   d_item   int32 [n_pairs]                  the pair's item in the last iss_generate_batch call; 0 for every other row (those of
 *                                             iss_generate, iss_generate_mt, older calls)
 * Asynchronous on the context's current stream -- the caller's after iss_ctx_set_stream / iss_ctx_set_stream_ordered -- behind the
 * generation it reads: no wait on the host, no device allocation.  The arrays are ready when that stream reaches the end of the
 * call's kernel; the rows may be generated anew as soon as the call returns (the next call is ordered behind it on the stream).
 * Rows outside the reserved range or an unknown encoding: ISS_E_INVALID, nothing launched.  n_pairs == 0: 0, nothing launched.
 */
#define ISS_EXPORT_ASCII 0
#define ISS_EXPORT_CODES 1
int iss_output_export(iss_ctx *ctx, int64_t first_pair, int64_t n_pairs, int32_t encoding, void *d_bases, void *d_qual,
                      int64_t *d_coords, int32_t *d_item);
/*
 * The mutation rows of the last iss_generate / iss_generate_batch call (Philox path, after iss_mutations_reserve: "source 0" of
 * iss_vcf_emit) as dense arrays in DEVICE memory the caller owns: per-base truth for a quality or error-correction model that
 * stays on the GPU (additive in ABI 8).  The labels are the reference's VCF rows (iss/error_models/__init__.py:98-108, 197-221)
 * and nothing more.  Window: output rows [first_pair, first_pair + n_pairs).
 *   truth    uint8 [n_pairs][2][read_length]  shape and `encoding` of iss_output_export's d_bases: at every position that carries
 *            a substitution row (type 0) the row's `ref` letter -- what stood there before mut_sequence changed it; under
 *            ISS_EXPORT_CODES recoded like the bases, in either letter case (ASCII keeps the case: a lower-case record gives a
 *            lower-case ref) -- and the exported base everywhere else.  NULL: not wanted
 *   events   int32 [capacity][6]  (pair - first_pair, mate, type, position, ref, alt) of every row of the window's pairs, in the
 *            order of iss_mutations_download (pair, mate, indel rows in loop order, then substitution rows by position); ref and
 *            alt are ASCII whatever the encoding, alt of a deletion is '.'.  Rows from `capacity` on are not written
 *   n_events int64 [1]  the rows of the window -- it may exceed `capacity`.  events and n_events go together (both, or both NULL)
 * Two quirks come with the reference's rows:
 *   1. a substitution whose new letter equals annotations["original"][position] is applied but not recorded (:98): truth then
 *      shows the base as read, not the one it replaced (after an indel shifted the read "original" is another base's letter);
 *   2. an indel row's position is a position in the sequence as it stood when the event fired (:201, :215), not in the read as
 *      it came out: indels are delivered as rows and never painted into the dense image.
 * A call that asked for more row slots than iss_mutations_reserve gave it has no row that can be trusted: the device itself
 * writes n_events = -1 then and leaves the plain bases in truth (iss_mutations_download and iss_vcf_emit say ISS_E_NOMEM behind a
 * wait on the host; this entry has no such wait).
 * Stream and ownership as for iss_output_export: asynchronous on the context's current stream behind the generation, no wait on
 * the host; the arrays are the caller's, ready when that stream reaches the end of the call's last kernel; the rows may be
 * generated anew as soon as the call returns.  (The first call that asks for events under a reservation allocates work arrays
 * of the reservation's size; a call after the reservation or the output rows grew waits for the stream to replace them.)
 * ISS_E_INVALID, nothing launched: no reservation in force, no Philox generate call since it was made, a window outside the
 * reserved output rows, an unknown encoding, events without n_events or the other way round.  MT mode's rows are not served.
 */
int iss_mutations_export(iss_ctx *ctx, int64_t first_pair, int64_t n_pairs, int32_t encoding, uint8_t *truth, int32_t *events,
                         int64_t capacity, int64_t *n_events);
/*
 * Integer tallies of rows [first_pair, first_pair + n_pairs), built ON THE DEVICE and ADDED to d_tally: device memory of
 * iss_tally_words(ctx) uint64 words that the caller owns and zeroes, so that a run accumulates over its batches -- what a run
 * produced (per-position quality profile, base composition, GC distribution, insert sizes) without writing a byte of FASTQ
 * (additive in ABI 8).  For read length L, Q = ISS_TALLY_PHREDS, I = ISS_TALLY_INSERT_BINS, the fields in
 * this order, no padding:
 *   pairs  [1]          pairs tallied
 *   qual   [2][L][Q]    (mate, position, phred byte of the row); a byte above Q - 1 counts in bin Q - 1
 *   base   [2][L][5]    (mate, position, ISS_EXPORT_CODES code of the base: A, C, G, T -> 0..3 in either case, every other letter 4)
 *   gc     [2][L + 1]   reads of the mate by their number of G, C, g, c letters
 *   meanq  [2][Q]       reads of the mate by floor(sum of the read's phred bytes / L) (Q - 1 at most)
 *   insert [I]          pairs by insert_size (the fourth coordinate of iss_output_download_coords), clamped to [0, I - 1]
 * Every count is an exact integer sum: the words depend neither on the launch geometry nor on the order of arrival.
 * Stream and ownership as for iss_output_export: asynchronous on the context's current stream behind the generation it reads, no
 * wait on the host, no device allocation; the rows may be generated anew as soon as the call returns.  Rows of iss_generate,
 * iss_generate_batch and iss_generate_mt alike.  ISS_E_INVALID, nothing launched: no model, rows outside the reserved range,
 * d_tally NULL with n_pairs > 0.  n_pairs == 0: 0, nothing launched.  iss_tally_words: -1 without a model.
 */
#define ISS_TALLY_PHREDS 94
#define ISS_TALLY_INSERT_BINS 2048
int64_t iss_tally_words(const iss_ctx *ctx); /* 1 + 2*L*94 + 2*L*5 + 2*(L+1) + 2*94 + 2048 */
int iss_output_tally(iss_ctx *ctx, int64_t first_pair, int64_t n_pairs, uint64_t *d_tally);
/*
 * Per-base coverage depth of the generated reads, built ON THE DEVICE (additive in ABI 8): where on the
 * records the reads fell, without a byte of FASTQ, an aligner or a depth tool.
 *
 * Definition.  For a pair let (fs, rs, re, isz) be what iss_output_download_coords returns, RL the read length and len the length
 * of the pair's record.  The pair covers the half-open intervals [fs, fs + RL) (forward) and [rs, re) (reverse) of record
 * coordinates, each CLAMPED to the record: [min(max(s, 0), len), min(max(e, 0), len)), empty when that leaves s >= e.  It is a
 * clamp, not Python's negative-index wrap, and it only bites with custom fragment lengths (negative inserts, templates cut by
 * the record's end).  The depth of a base is the number of such intervals over it.  It is the NOMINAL depth: the template
 * intervals the reads were cut from (iss/generator.py:146-147, 165-177).  A third quirk beside the two of iss_mutations_export:
 *   3. indels make a read consume a few bases more or fewer than its interval (adjust_seq_length); the depth ignores that.
 *
 * Accumulator.  The caller owns it and its layout.  A record table is int64 [n][2] of (offset, length) in device memory; record
 * k owns the length + 1 int32 words [offset, offset + length] of a difference array, the last one being the record's sink.  An
 * interval adds +1 at offset + s and -1 at offset + e (e <= length: in the sink at the latest).  So every record's words sum
 * to zero, a plain inclusive prefix sum over the whole array is the depth of every base of every record at once, and the array
 * is additive over calls, batches, record groups, workers and GPUs.  The caller zeroes it.
 *
 * iss_depth_mark adds the intervals of rows [first_pair, first_pair + n_pairs) to d_diff.  d_table[item] is the record of the
 * pair's item: its item in the last iss_generate_batch call (as iss_output_export's d_item says), 0 for every other row (those of
 * iss_generate, iss_generate_mt).  A row of the table with offset < 0: the pair is skipped.  One lane per pair, up to four int32
 * global atomic adds without return; an empty interval adds nothing.  The table's rows must lie inside the caller's array: the
 * entry has no way to check that.  Stream and ownership as for iss_output_tally: asynchronous on the context's current stream
 * behind the generation, no wait on the host, no device allocation; the rows may be generated anew as soon as the call returns.
 * It needs no mutation reservation and serves Philox and iss_generate_mt rows alike (not the rows of iss_generate_mt_workers).
 * ISS_E_INVALID, nothing launched: no model, rows outside the reserved range, d_table or d_diff NULL with n_pairs > 0, n_table
 * smaller than the item count of the last batch call when the window touches its rows (or < 1).  n_pairs == 0: 0, nothing launched.
 * BOUND: the depth of a base must stay below 2^31.  The device does not check it.  A pair adds at most 2 to a base, so a caller
 * that marks no more than 2^30 pairs into one accumulator is safe (the Python callers keep that count on the host and refuse
 * more); a C caller keeps the rule itself.
 *
 * iss_depth_finish turns a difference array of n_words words into
 *   d_depth uint32 [n_words]    its inclusive prefix sum: the depth of every base (a sink holds the depth behind the record's
 *                               last base: 0).  It may be d_diff itself (in place; no other overlap), or NULL
 *   d_stats uint64 [n_table][4] per record over its `length` bases, the sink left out: sum of depth, sum of depth squared (mod
 *                               2^64), bases with depth > 0, maximum depth.  Overwritten, not added to.  NULL: not wanted
 *   d_bins  uint64 [sum over the table's rows of ceil(length / bin)]  with bin > 0: the sum of depth over every bin-base window
 *                               of every record, the records in table order, a record's last window short.  Overwritten.  NULL
 *                               (or bin == 0): not wanted
 * The rows of d_table used here must not overlap, must lie within n_words and must ascend by offset in table order; a row with
 * offset < 0 is skipped wherever it stands (its statistics and windows are zero; it still owns its windows in d_bins).  Words
 * that belong to no record (gaps) are scanned like the rest and counted nowhere.  The scan is a reduce-then-scan over tiles of
 * ISS_DEPTH_TILE_WORDS words with 16-byte loads and stores when d_diff and d_depth are 16-byte aligned (4-byte accesses
 * otherwise).  All results are exact integers and depend neither on the launch geometry nor on the order of arrival.
 * It works on a context with no model and no genome.  Same stream rule as above, with one exception: the first call allocates a
 * work array (tile sums, the table's rows in use) on the device, and a call that needs a larger one waits for the stream, frees
 * it and allocates anew.  ISS_E_INVALID, nothing launched: negative n_words, n_table or bin, d_diff NULL with n_words > 0, d_table
 * NULL with statistics or windows wanted.  Nothing wanted: 0, nothing launched.
 * ISS_DEPTH_WGS (environment, read per call like ISS_TALLY_WGS): the workgroups k_depth_mark and the scan's passes aim at.
 */
#define ISS_DEPTH_TILE_WORDS 4096
int iss_depth_mark(iss_ctx *ctx, int64_t first_pair, int64_t n_pairs, const int64_t *d_table, int32_t n_table, int32_t *d_diff);
int iss_depth_finish(iss_ctx *ctx, const int32_t *d_diff, int64_t n_words, uint32_t *d_depth, const int64_t *d_table, int32_t n_table,
                     int32_t bin, uint64_t *d_stats, uint64_t *d_bins);
/*
 * Integer tallies of the MUTATION ROWS of the last generate call, built ON THE DEVICE and ADDED to d_tally: device memory of
 * iss_error_tally_words(ctx) uint64 words that the caller owns and zeroes, so that a run accumulates over its batches -- what
 * the run did to the reads (substitutions by position, phred and letters, insertions, deletions, events per read) without a
 * row on the host or a byte of VCF (additive in ABI 8).  For read length L, Q = ISS_ERRTALLY_PHREDS,
 * K = ISS_ERRTALLY_READ_BINS, the fields in this order, no padding:
 *   dropped  [1]            calls whose rows could not be trusted (see Overflow); such a call adds here and nowhere else
 *   pairs    [1]            pairs of the windows tallied
 *   sub_q    [2][L][Q]      substitution rows by (mate, position, quality); a quality above Q - 1 counts in bin Q - 1
 *   sub_mat  [2][L][5][5]   substitution rows by (mate, position, code of ref, code of alt): the ISS_EXPORT_CODES code -- A, C, G,
 *                           T -> 0..3 in either case, every other byte 4
 *   ins      [2][L][5]      insertion rows by (mate, position, code of alt): the inserted letter
 *   del      [2][L][5]      deletion rows by (mate, position, code of ref): the letter that stands at `position` after the pop
 *   per_read [2][3][K]      reads of the mate by their number of rows of the type (0 substitution, 1 insertion, 2 deletion),
 *                           clamped to K - 1; bin 0 counts the reads with none
 * 2 + 258 L + 6 K words.  A position outside [0, L - 1] counts in the nearest end bin (a guard: the loops that make the rows keep
 * every position inside).  The rows that count are exactly those of iss_mutations_download (source 0: the last iss_generate /
 * iss_generate_batch call, stale rows of rebuilt reads filtered out) or iss_mt_mutations_download (source 1: the last
 * iss_generate_mt call) whose pair lies in rows [first_pair, first_pair + n_pairs) -- the window of iss_mutations_export, which
 * may reach over either end of the call.  Both quirks of iss_mutations_export hold: a substitution back to the original letter
 * is not a row, and indel positions are positions at the time of the event.  The rows of iss_generate_mt_workers are not served.
 * Every count is an exact integer sum: the words depend neither on the launch geometry nor on the order of arrival.
 * Stream and ownership as for iss_output_tally: asynchronous on the context's current stream behind the generation, no wait on
 * the host; the rows may be generated anew as soon as the call returns.  (The first call allocates one work array of the output
 * rows' size -- 16 bytes a pair; a call after the output rows grew waits for the stream to replace it.)
 * Overflow: the device decides.  The kernels read the call's slot counter themselves; when it exceeds iss_mutations_reserve's
 * capacity they add 1 to `dropped` and nothing else.  Source 1 with more rows than iss_mt_mutations_reserve holds: ISS_E_INVALID.
 * ISS_E_INVALID, nothing launched: no model, no reservation in force or no generate call of that source since it was made, a
 * window outside the reserved output rows, an unknown source, d_tally NULL with n_pairs > 0.  n_pairs == 0: 0, nothing launched.
 * iss_error_tally_words: -1 without a model.
 * ISS_ERRTALLY_WGS (environment, read per call like ISS_TALLY_WGS): the slot chunks k_errtally_rows runs per position tile.
 */
#define ISS_ERRTALLY_PHREDS 94 /* = ISS_TALLY_PHREDS */
#define ISS_ERRTALLY_READ_BINS 64
int64_t iss_error_tally_words(const iss_ctx *ctx); /* 2 + 258*L + 6*64 */
int iss_mutations_tally(iss_ctx *ctx, int32_t source, int64_t first_pair, int64_t n_pairs, uint64_t *d_tally);
/* iss_ctx_set_stream without the wait on the host (additive in ABI 8): everything queued on the context's streams so far is
 * ordered in front of what the context queues on `hip_stream` from now on, by events.  NULL: back to the context's own stream. */
int iss_ctx_set_stream_ordered(iss_ctx *ctx, void *hip_stream);

/* HIP-event timing of the kernels launched by iss_generate (on the launch stream).
 * enable: 0 off, 1 every kernel, 2 k_main only (an event is a bubble in the stream: the five-kernel timing costs
 * about 6 % of a step).  iss_timing_read synchronises, returns accumulated milliseconds per kernel
 * (setup, main, indel-scan, indel-fixup) and the number of iss_generate launches, then
 * resets the accumulators. */
int iss_timing_enable(iss_ctx *ctx, int enable);
int iss_timing_read(iss_ctx *ctx, double ms[4], int64_t *n_launches);

/* Counters since the last read: reads rebuilt by the indel fix-up kernel (one wavefront per read), reads k_main built from an
 * edit script (models whose reads often have indels).  Either pointer may be NULL. */
int iss_stats_read(iss_ctx *ctx, int64_t *n_fixup_reads, int64_t *n_scripted_reads);

/* Name of the kernel the last iss_generate / iss_generate_batch call launched for the hot path (simulate_read's per-base work,
 * iss/generator.py:146-180 + iss/error_models/kde.py:52-86): "k_main<mutations, plain, indel>", "k_main_g<NI, NP>" or, for
 * quality mode 2, "k_perfect" -- what a
 * profile of the call lists, so that a measurement can name what it measured.  Returns the name's length (it is cut to
 * capacity - 1 characters and always closed by a NUL), 0 before the first call. */
int iss_main_kernel(iss_ctx *ctx, char *name, int capacity);

/*
 * Reference-compatible RNG mode (sequential; for bit-identity with the reference, not throughput).
 * iss_mt_seed == `random.seed(seed); np.random.seed(seed)` of worker_iterator (iss/generator.py:234-236,
 * seed = args.seed + cpu_number, must be < 2^32 like numpy's legacy seeding).  iss_generate_mt consumes the
 * two MT19937 streams exactly as reads_generator/simulate_read do (iss/generator.py:69-192), so rows
 * [out_first_pair, +*n_done) equal the reference's reads for that worker byte for byte; the stream state
 * carries over to the next call (the next work item of the worker).  On ISS_E_SHORT_RECORD the one numpy
 * double the reference draws before its assertion is consumed too.  iss_mt_peek copies the next n <= 624 words of both streams (not consumed).
 */
int iss_mt_seed(iss_ctx *ctx, uint64_t seed);
int iss_generate_mt(iss_ctx *ctx, int32_t genome_id, int64_t n_pairs, int32_t sequence_type, int32_t gc_bias,
                    int64_t out_first_pair, int64_t *n_done);
int iss_mt_peek(iss_ctx *ctx, uint32_t *py_words, uint32_t *np_words, int32_t n);
/* Pairs produced so far by each device path of iss_generate_mt: the offset resolver + parallel emitter
 * (plain pairs) and the sequential walker (pairs with an indel candidate, letters outside ACGT or a template cut by
 * a genome end; indel-heavy models, the BasicErrorModel; everything when ISS_MT_PATH=walk is set in the environment). */
int iss_mt_path_counts(iss_ctx *ctx, int64_t *n_resolved, int64_t *n_walked);
/* The resolver instantiation iss_generate_mt / iss_generate_mt_workers take for the loaded model and the current ISS_MT_PATH:
 * out = (python ring half in K words, numpy ring half in K words, 1 if the digit rows are staged in LDS), or (0, 0, 0) when
 * every pair goes to the walker.  Launches nothing and changes no state. */
int iss_mt_resolver_pick(iss_ctx *ctx, int32_t out[3]);
/*
 * W reference workers side by side in ONE context (ABI 7).  The reference's own parallelism is N workers, each a sequential
 * chain over its two MT19937 streams seeded `seed + cpu_number` (pool.starmap over worker_iterator: iss/app.py:99-106,
 * iss/generator.py:234-236).  iss_mt_workers_seed(ctx, W, seeds) == W times iss_mt_seed(seeds[w]);
 * iss_generate_mt_workers == for every worker w: iss_generate_mt(genome_ids[w], n_pairs[w], ..., out_first_pair[w]) on ITS streams
 * -- same rows, same stream positions afterwards -- but every kernel of the path is launched once for all workers, one workgroup
 * per worker (n_pairs[w] == 0: the worker sits this call out).  status[w] (may be NULL): 0, or ISS_E_SHORT_RECORD for a worker whose
 * record is not longer than a read (its draw is consumed like iss_generate_mt does); any other failure fails the call.  The
 * workers' row ranges must not overlap.  Custom fragment lengths and the BasicErrorModel run the workers one after the other
 * through iss_generate_mt (draws the host's libm settles); --store_mutations rows of the set: iss_mt_workers_mutations_reserve below
 * (a context that holds single-worker rows, iss_mt_mutations_reserve, is refused here: ISS_E_INVALID).
 * iss_mt_workers_peek: iss_mt_peek for worker w.  iss_mt_path_counts counts the set's pairs too.
 */
int iss_mt_workers_seed(iss_ctx *ctx, int32_t n_workers, const uint64_t *seeds);
int iss_generate_mt_workers(iss_ctx *ctx, int32_t n_workers, const int32_t *genome_ids, const int64_t *n_pairs,
                            const int64_t *out_first_pair, int32_t sequence_type, int32_t gc_bias, int64_t *n_done, int32_t *status);
int iss_mt_workers_peek(iss_ctx *ctx, int32_t worker, uint32_t *py_words, uint32_t *np_words, int32_t n);
/* Custom fragment length in MT mode (--fragment-length / --fragment-length-sd, iss/generator.py:121-123):
 * fragment = int(np.random.normal(mu, sd)) with numpy's legacy polar Box-Muller incl. its cached second value
 * (reset by iss_mt_seed like np.random.seed does).  The device evaluates it; draws that land within 1e-6 of an
 * integer are re-evaluated on the host with libm so the truncation provably equals numpy's. */
int iss_mt_set_fragment(iss_ctx *ctx, int32_t enabled, double fragment_length, double fragment_sd);

/* --store_mutations in MT mode: after iss_mt_mutations_reserve(capacity > 0) every iss_generate_mt call records
 * its rows (iss_mutation, in the reference's order) from index 0; iss_mt_mutations_download copies
 * min(rows, capacity) of them and reports the total row count. */
int iss_mt_mutations_reserve(iss_ctx *ctx, int64_t capacity);
int iss_mt_mutations_download(iss_ctx *ctx, iss_mutation *out, int64_t capacity, int64_t *n_total);
/* --store_mutations for the workers of a set: after iss_mt_workers_mutations_reserve with rows_per_worker > 0 every
 * iss_generate_mt_workers call records each worker's rows from index 0 of the worker's own region, in the reference's order -- the
 * rows iss_generate_mt records for that worker in a context of its own; 0 frees the storage and switches the capture off.  The
 * request outlives iss_mt_workers_seed (the new workers get their regions).  A worker that makes more rows than its region holds:
 * the surplus is dropped, the call returns ISS_E_NOMEM and the set is poisoned like after any failure half way (seed it again).
 * iss_mt_workers_mutations_download copies min(rows, capacity) rows of one worker of the last call and reports its row count. */
int iss_mt_workers_mutations_reserve(iss_ctx *ctx, int64_t rows_per_worker);
int iss_mt_workers_mutations_download(iss_ctx *ctx, int32_t worker, iss_mutation *out, int64_t capacity, int64_t *n_total);

/*
 * FASTQ text built ON THE DEVICE (the host formatter below tops out near 3 GB/s of text, four hundred times
 * under the kernel's rate): rows [first_pair, +n_pairs) of the output buffers become the records of
 * simulate_reads' SeqIO.write calls (iss/generator.py:64-65, ids per :150, 181, i from first_i) -- one wavefront
 * per record, byte offsets in closed form -- and are appended to fd_r1 / fd_r2 at their current positions.
 * Asynchronous: the format kernel runs on the context's stream behind the generation it reads, the copy to
 * pinned host memory on a copy stream, the file writes (pwrite, n_threads pieces per file) on a writer thread,
 * so the next batch can be generated meanwhile (two text slots).  iss_fastq_flush waits until every queued
 * byte is in the files and leaves the descriptors positioned at the end; call it before using the files.
 */
int iss_fastq_emit(iss_ctx *ctx, int fd_r1, int fd_r2, const char *record_id, int64_t first_i, int32_t cpu_number,
                   int64_t first_pair, int64_t n_pairs, int32_t n_threads);
/* The same for the rows of several work items in ONE text job (one format launch, one pair of copies, one write per
 * file): item k = rows [first_pair[k], +n_pairs[k]) under record_ids[k] with pair ids from first_i[k].  The bytes
 * appended are those of n_items iss_fastq_emit calls in item order (compressed mode: one gzip member for the call). */
int iss_fastq_emit_batch(iss_ctx *ctx, int fd_r1, int fd_r2, int32_t n_items, const char *const *record_ids,
                         const int64_t *first_i, const int64_t *first_pair, const int64_t *n_pairs, int32_t cpu_number);
/* The same for items that belong to DIFFERENT workers and go to DIFFERENT places of the two files (text mode only): item k is
 * worker cpu_numbers[k]'s ("{id}_{i}_{cpu_numbers[k]}/1") and its text is written at byte file_off[k] of fd_r1 and of fd_r2 -- the
 * two files of a pair hold records of equal lengths.  The reference's parent concatenates its workers' temp files in worker order
 * (iss/app.py:123-127, iss/util.py:213-234); a worker's text size is arithmetic (constant read length, decimal pair numbers), so
 * the W workers of a set (iss_generate_mt_workers) write straight into the final files and the concatenation -- a second copy of
 * every byte under the destination's inode lock -- disappears.  The files' running offsets (iss_fastq_emit) are not moved; the
 * caller sizes the files (ftruncate) and owns the layout. */
int iss_fastq_emit_scatter(iss_ctx *ctx, int fd_r1, int fd_r2, int32_t n_items, const char *const *record_ids, const int64_t *first_i,
                           const int64_t *first_pair, const int64_t *n_pairs, const int32_t *cpu_numbers, const int64_t *file_off,
                           int32_t n_threads);
int iss_fastq_flush(iss_ctx *ctx);

/*
 * The --store_mutations VCF rows as text built ON THE DEVICE: what write_mutations (iss/generator.py:598-620) writes per
 * mutation -- "{record.id}_{i}_{cpu}/{mate + 1}\t{position + 1}\t.\t{ref}\t{alt}\t{qual}\t\t\n", alt = ref + alt for an
 * insertion (iss/error_models/__init__.py:203), qual = the phred of a substitution, '.' otherwise -- for the rows of the last
 * generate call, appended to fd at its current position, in call order.  source 0: the rows of the last iss_generate /
 * iss_generate_batch call (the filter and the order of iss_mutations_download, applied on the device); source 1: the rows of the
 * last iss_generate_mt call.  Item k is output rows [first_pair[k], +n_pairs[k]) of that call under record_ids[k] with pair ids
 * from first_i[k] (the item table of iss_fastq_emit_batch); the items stand in ascending row order and do not overlap, rows of
 * pairs outside every item are left out.  Asynchronous like iss_fastq_emit: the kernels run on the context's stream behind the
 * generation; a writer thread fetches the text and appends it (pwrite) behind the next batch.  Only text crosses to the host,
 * apart from one counter: a Philox call that reserved more row slots than iss_mutations_reserve gave it returns ISS_E_NOMEM,
 * *slots_needed = the slots it asked for, and appends nothing (reading that counter waits for the generation).  On success
 * *slots_needed is 0.  source 1 with more rows than iss_mt_mutations_reserve holds: ISS_E_INVALID.
 * iss_vcf_flush waits until every queued byte is in the file and leaves the descriptor at its end (iss_fastq_flush does not).
 */
int iss_vcf_emit(iss_ctx *ctx, int fd, int32_t source, int32_t n_items, const char *const *record_ids, const int64_t *first_i,
                 const int64_t *first_pair, const int64_t *n_pairs, int32_t cpu_number, int64_t *slots_needed);
/* The same for the rows of the last iss_generate_mt_workers call, ALL workers in one text job (one sequence of the kernels, one
 * copy): entry k is worker k's piece -- output rows [first_pair[k], +n_pairs[k]), which must start at the worker's first row of that
 * call, under record_ids[k] with pair ids from first_i[k] and worker number cpu_numbers[k]; n_pairs[k] == 0: the worker sat the call
 * out.  Worker k's byte range of the text is appended to fds[k] at its current position by the writer thread, the descriptors are
 * left at their ends. */
int iss_vcf_emit_workers(iss_ctx *ctx, int32_t n_workers, const int *fds, const char *const *record_ids, const int64_t *first_i,
                         const int64_t *first_pair, const int64_t *n_pairs, const int32_t *cpu_numbers);
int iss_vcf_flush(iss_ctx *ctx);

/*
 * `--compress` (iss/app.py:134-143 -> util.compress, iss/util.py:255-268: gzip of the finished FASTQ files) moved in
 * front of the files: with mode 1 every iss_fastq_emit appends ONE GZIP MEMBER per file (RFC 1952) holding the
 * batch's text instead of the text -- DEFLATE blocks with a dynamic Huffman code, run and previous-record matches, built on the device
 * from the batch's own token histogram, so only the compressed bytes (about 1/3.5) cross PCIe and reach the file
 * system.  Concatenated members are one valid .gz file whose content is the text mode 0 writes.  mode 0 (default):
 * plain text.  Changing the mode flushes.
 */
int iss_fastq_compress(iss_ctx *ctx, int32_t mode);

/*
 * The code builder of the compressed mode as a host function (tests, tools): hist[273] token counts (literals
 * 0..255, [256] the number of blocks, [257..272] the length codes of matches of 3..32 bytes) and the batch's record
 * length (the distance of the "previous record" matches; 0: only runs, distance 1) -> entry[s] = bit-reversed code |
 * length << 16 for the 273 symbols, the dynamic-block header (BFINAL = 0 ... both code-length tables) as hdr_bits
 * bits, least significant first, in hdr_words[64], and dist_code[3] = {distance symbol, extra bits, their value} of
 * the record length: a run's length code (+ its extra bits) is followed by the bit 0, a previous-record match's by the
 * bit 1 and the distance's extra bits.  No GPU needed.
 */
int iss_deflate_code_build(const uint32_t *hist, uint32_t record_distance, uint32_t *entry, uint32_t *hdr_bits,
                           uint32_t *hdr_words, uint32_t *dist_code);

/*
 * FASTQ emission, replaces SeqIO.write(record, handle, "fastq-sanger") in
 * simulate_reads (iss/generator.py:64-65): records "@{record_id}_{i}_{cpu_number}/{1|2}\n
 * SEQ\n+\nQUAL\n" with QUAL = chr(33+q), ids per iss/generator.py:150, 181; i runs from
 * first_i.  Host-side formatter (multi-threaded) appending to two file descriptors.
 */
int iss_fastq_write(int fd_r1, int fd_r2, const char *record_id, int64_t first_i, int32_t cpu_number,
                    int64_t n_pairs, int32_t read_length, int32_t pitch, const uint8_t *r1_base,
                    const uint8_t *r1_qual, const uint8_t *r2_base, const uint8_t *r2_qual, int32_t n_threads);

/*
 * Unaligned BAM built ON THE DEVICE (additive in ABI 8): the FASTQ's content in the other container that
 * pipelines take directly (the uBAM convention of GATK / Picard).  The item table is iss_fastq_emit_batch's.  Rows
 * [first_pair[k], +n_pairs[k]) become alignment records (SAM/BAM specification 4.2) in ONE stream, R1 then R2 of every pair:
 * refID / pos / next_refID / next_pos -1, mapq 0, bin 4680, no CIGAR, flag 77 (R1) / 141 (R2), tlen 0, read name
 * "{id}_{i}_{cpu_number}" (no /1, /2: the flags carry the mate), the bases as 4-bit codes of "=ACMGRSVTWYHKDBN" (lower-case
 * letters count as their capitals -- BAM has no case -- and any other byte is N), the raw phreds, no tags.  The call's record
 * bytes are cut into blocks of 32 768 bytes, each written as one complete BGZF member (specification 4.1: a gzip member with the
 * `BC` field, its own CRC-32 and ISIZE) that inflates on its own, and the members are appended to fd at its current position.  A
 * call writes record blocks only: the BAM header in front and the 28-byte EOF block behind are the caller's.  Asynchronous like
 * iss_fastq_emit_batch -- kernels on the context's stream behind the generation, the size on a copy stream, the bytes fetched and
 * appended (pwrite) by a writer thread, two slots; iss_ubam_flush waits until every queued byte is in the file and leaves the
 * descriptor at its end.  A member never exceeds BGZF's 65 536 bytes (32 768 literals at the 15-bit code limit stay under it); the
 * writer walks the BSIZE chain of what it fetched before it writes, and a chain that does not hold is ISS_E_INVALID at the next
 * emit or flush, never a wrapped BSIZE in the file.  A read name of more than 254 characters does not fit l_read_name: ISS_E_INVALID naming the record id,
 * before anything is launched or written.
 *
 * iss_ubam_host_records (host only, no GPU; single-threaded): the same record bytes, uncompressed, from host rows
 * ([pairs][pitch] arrays as iss_output_download returns them), appended to fd -- the counterpart of iss_fastq_write.
 */
int iss_ubam_emit_batch(iss_ctx *ctx, int fd, int32_t n_items, const char *const *record_ids, const int64_t *first_i,
                        const int64_t *first_pair, const int64_t *n_pairs, int32_t cpu_number);
int iss_ubam_flush(iss_ctx *ctx);
int iss_ubam_host_records(int fd, const char *record_id, int64_t first_i, int32_t cpu_number, int64_t n_pairs, int32_t read_length,
                          int32_t pitch, const uint8_t *r1_base, const uint8_t *r1_qual, const uint8_t *r2_base, const uint8_t *r2_qual);

/*
 * Origins built ON THE DEVICE (additive in ABI 8): where every pair came from, as BEDPE text, one line per
 * pair, tab separated, no header:
 *     {id} s1 e1 {id} s2 e2 {id}_{i}_{cpu_number} . + - isz \n
 * With (fs, rs, re, isz) what iss_output_download_coords returns for the row, RL the read length and len = record_len[k]:
 * [s1, e1) = [fs, fs + RL) is the template interval read 1 was cut from (iss/generator.py:135-147), [s2, e2) = [rs, re) that of
 * read 2 (generator.py:165-177), each clamped like the depth's intervals: s' = min(max(s, 0), len), e' = max(min(max(e, 0), len), s')
 * -- an interval that is empty after the clamp reads "s' s'"; the clamp bites only with custom fragment lengths.  Read 1 is always
 * '+' and read 2 always '-' (generator.py:149, 180), the score is '.', the name is the FASTQ read name without /1, /2 and isz the
 * insert size as drawn, signed.  Plain decimals, no padding.  Nothing is read from the mutation rows.
 *
 * The item table is iss_fastq_emit_batch's plus the record lengths; items stand in ascending row order and do not overlap.
 * Asynchronous like iss_ubam_emit_batch -- line lengths, a scan and the format kernel on the context's stream behind the
 * generation (rows may be generated anew right behind the call), the text's size on a copy stream, the bytes fetched and appended
 * (pwrite) at fd's current position by a writer thread, two slots; iss_origins_flush waits until every queued byte is in the file
 * and leaves the descriptor at its end.  ISS_E_INVALID with nothing launched or written: rows outside the reserved range, a
 * record_len below 1, items out of order or overlapping.  No pairs at all: nothing is appended.  ISS_ORIGINS_TILE (read per call):
 * pairs per workgroup of the format kernel; the text does not depend on it.
 *
 * iss_origins_host_text (host only, no GPU; single-threaded): the same lines for one item from coords[n_pairs][4] as
 * iss_output_download_coords returns them, appended to fd.
 */
int iss_origins_emit_batch(iss_ctx *ctx, int fd, int32_t n_items, const char *const *record_ids, const int64_t *first_i,
                           const int64_t *first_pair, const int64_t *n_pairs, const int64_t *record_len, int32_t cpu_number);
int iss_origins_flush(iss_ctx *ctx);
int iss_origins_host_text(int fd, const char *record_id, int64_t first_i, int32_t cpu_number, int64_t n_pairs, int32_t read_length,
                          int64_t record_len, const int64_t *coords);

/*
 * `--bgzip` (additive in ABI 8): the two one-file texts as BGZF, compressed ON THE DEVICE, with the
 * semantics of iss_fastq_compress.  mode 0 (default): iss_origins_emit_batch / iss_vcf_emit append their text.  mode 1: they
 * append the BGZF members of that call's text instead -- every 32 768 bytes of it one complete member (`BC` field, its own CRC-32
 * and ISIZE) that inflates on its own, all members of a call under one dynamic Huffman code built from the call's own tokens.
 * Inside 32-byte chunks a match is a run (distance 1) or a copy from the LINE ABOVE: the distance of a chunk is the byte length of
 * the line in front of the line that holds the chunk's first byte, taken from the offsets the formatter computed; there is no
 * such candidate in the text's first line, past 32 768 bytes, or where the source would start before the chunk's own block.  The
 * concatenated members inflate to exactly the bytes mode 0 writes.  A call without text appends nothing; the file's frame -- a
 * header member in front, the 28-byte EOF block behind -- is the caller's.  The text never reaches the host: the writer thread
 * walks the BSIZE chain of the members it fetched before it writes them, and a chain that does not hold is ISS_E_INVALID at the
 * next emit or flush.  The mode is switched only while nothing is queued (after a flush): otherwise ISS_E_INVALID.
 * iss_vcf_emit_workers in mode 1: ISS_E_INVALID, nothing written (a worker set's text is split over W descriptors).
 */
int iss_origins_compress(iss_ctx *ctx, int32_t mode);
int iss_vcf_compress(iss_ctx *ctx, int32_t mode);
/* The code builder of that stage as a host function (tests, tools; no GPU needed): hist[273 + 30] -- the token counts of
 * iss_deflate_code_build, then the matches per DEFLATE distance code (a run counts under code 0) -> entry[273] and dentry[30]
 * (bit-reversed code | length << 16; a distance code nobody uses has length 0) and the dynamic-block header, hdr_bits bits, least
 * significant first, in hdr_words[80]. */
int iss_bgzf_text_code_build(const uint32_t *hist, uint32_t *entry, uint32_t *dentry, uint32_t *hdr_bits, uint32_t *hdr_words);

/*
 * `model`: the reference's `iss model` (iss/app.py:147-169 -> iss/bam.py:103-227, iss/modeller.py) from a BAM file.  Additive to
 * ABI 8.  The host inflates the BGZF blocks; these entries find the records, tally them on the device and evaluate the quality and
 * insert-size kernel density estimates from the tallies.
 *
 * iss_bam_scan (host only, no GPU): the block_size chain of inflated record bytes -- the byte offsets of up to `capacity` whole
 * records, how many were found and the bytes they cover (the rest starts the next chunk).  ISS_E_INVALID on a block_size under 32.
 *
 * The tally context: iss_bam_feed adds the records of one chunk (offsets from iss_bam_scan, select[r] != 0: the record is taken --
 * mapped and in the subsample) to the device tallies; iss_bam_tally_download copies the ISS_BAM_TALLY_WORDS u64 words below and the
 * first bad record (index over all fed records, -1: none) with its ISS_BAM_REC_* code; iss_bam_kde evaluates the 41-point quality
 * CDFs of every (mate, bin, position) into qcdf[8][301][41] (NaN rows: fewer than two reads in the bin, or a position at or past the
 * bin's shortest read) and, when with_isize, the 2000-point insert-size CDF for read_length (the caller checks there are two template
 * lengths or more, not all equal).  iss_bam_reset zeroes the tallies.
 *
 * Tally words (u64): subst [2][301][16] at 0 (dispatch_subst's columns), indel [2][301][9] at ISS_BAM_OFF_INDEL (column 0 unused),
 * quality histograms [2 mates][4 bins][301][94] at ISS_BAM_OFF_QHIST, template lengths [2000] at ISS_BAM_OFF_TLEN, reads per
 * (mate, bin) [8] at ISS_BAM_OFF_NREAD, their shortest length [8] at ISS_BAM_OFF_MINLEN (~0: none), records tallied at ISS_BAM_OFF_TAKEN.
 */
#define ISS_BAM_MAX_LEN 301
#define ISS_BAM_NQ 94
#define ISS_BAM_NTLEN 2000
#define ISS_BAM_OFF_INDEL 9632
#define ISS_BAM_OFF_QHIST 15050
#define ISS_BAM_OFF_TLEN 241402
#define ISS_BAM_OFF_NREAD 243402
#define ISS_BAM_OFF_MINLEN 243410
#define ISS_BAM_OFF_TAKEN 243418
#define ISS_BAM_TALLY_WORDS 243426
#define ISS_BAM_QCDF_WORDS (8 * 301 * 41)

#define ISS_BAM_REC_MALFORMED 1   /* record fields run past its block_size, or a broken optional field */
#define ISS_BAM_REC_TOO_LONG 2    /* l_seq > 301 */
#define ISS_BAM_REC_NO_QUAL 3     /* read1 / read2 without qualities (0xFF) or without bases */
#define ISS_BAM_REC_CIGAR_OP 4    /* a CIGAR operation other than M, I, D, S, H */
#define ISS_BAM_REC_NO_MD 5       /* no MD:Z tag */
#define ISS_BAM_REC_BAD_MD 6      /* the MD tag does not cover the aligned columns */
#define ISS_BAM_REC_INDEL_INDEX 7 /* dispatch_indels would index past the read (IndexError in the reference) */
#define ISS_BAM_REC_QUAL_RANGE 8  /* a quality above 93 */
#define ISS_BAM_REC_CIGAR_LEN 9   /* M + I + S lengths differ from l_seq */

typedef struct iss_bam iss_bam;
int iss_bam_scan(const uint8_t *data, int64_t n_bytes, int64_t *offsets, int64_t capacity, int64_t *n_records, int64_t *consumed);
int iss_bam_create(int device_ordinal, iss_bam **out);
void iss_bam_destroy(iss_bam *bam);
const char *iss_bam_last_error(const iss_bam *bam);
int iss_bam_reset(iss_bam *bam);
int iss_bam_feed(iss_bam *bam, const uint8_t *data, int64_t n_bytes, const int64_t *offsets, const uint8_t *select, int64_t n_records);
int iss_bam_tally_download(iss_bam *bam, uint64_t *tally, int64_t *bad_record, int32_t *bad_code);
int iss_bam_kde(iss_bam *bam, int32_t read_length, int32_t with_isize, double *qcdf, double *isize_cdf);

/*
 * `report`: the tallies of iss_output_tally over FASTQ TEXT, built ON THE DEVICE (additive in ABI 8): what a
 * read set from a sequencer, or a file written earlier, looks like -- to put beside the tally of a run.  A context of its own, no
 * iss_ctx and no model.  max_len (1 .. ISS_FQ_MAX_LEN) is the longest read the context takes; its words are iss_output_tally's
 * layout at L = max_len and one field behind it, iss_fq_tally_words words in all (-1 for NULL):
 *   pairs [1] | qual [2][L][Q] | base [2][L][5] | gc [2][L + 1] | meanq [2][Q] | insert [I] | length [2][L + 1]
 * A feed is one mate: R1's file feeds mate 0, R2's mate 1.  The phred is the quality byte - 33; base codes and the G / C test are
 * iss_output_tally's.  qual and base count positions 0 .. len - 1 of a read of length len; meanq is floor(sum of phreds / len) of
 * the read's own length; a read of length 0 counts in length[mate][0] and gc[mate][0] and nowhere else; pairs counts the good
 * records of mate 0; insert stays zero (a FASTQ file does not say it).  Every count is an exact integer sum: the words depend
 * neither on the launch geometry nor on how the text was cut into chunks.
 *
 * iss_fq_feed: `text` is HOST memory, n_bytes of FASTQ text that holds whole four-line records (@name, bases, +, qualities; a line
 * ends at '\n', one '\r' directly before it belongs to the terminator; wrapped FASTQ is not taken and shows as ISS_FQ_REC_LENGTHS
 * or ISS_FQ_REC_NO_AT).  Records are found by line number modulo 4, never by looking for '@'.  The caller may reuse `text` as soon
 * as the call returns: the bytes go through one of the context's pinned staging buffers, so that the copy of one chunk overlaps the
 * kernels of the chunk before.  The first feed that needs more room allocates it; a feed waits for the device only to get its
 * staging buffer back.  A bad record is not tallied, the records after it are; the FIRST bad record per mate (index over all records
 * fed for the mate) is kept with its ISS_FQ_REC_* code -- the smallest code that applies to it -- and the caller decides what to
 * do with it.  ISS_E_INVALID, nothing launched: mate outside {0, 1}, n_bytes < 0 or >= 2^31, text NULL with n_bytes > 0.
 * n_bytes == 0: 0, nothing launched.
 * iss_fq_download waits for everything fed, then copies the words, the whole records seen per mate (records[2]) and the first bad
 * record per mate (bad_record[2]: -1 for none; bad_code[2]).  iss_fq_reset zeroes the words and the counts.
 * iss_fq_kernel_ms waits for everything fed, then gives the time the kernels of all feeds since the last reset took on the device,
 * from HIP events around each feed's launches (tools/report_bench.py: the kernels apart from the reading and the copies).
 * ISS_FQTALLY_WGS (environment, read per call like ISS_TALLY_WGS): the workgroups the record kernels aim at (the per-position
 * kernel: per column of 64 positions).
 */
#define ISS_FQ_MAX_LEN 1024
#define ISS_FQ_REC_NO_AT 1      /* line 0 of the record does not start with '@' */
#define ISS_FQ_REC_NO_PLUS 2    /* line 2 does not start with '+' */
#define ISS_FQ_REC_LENGTHS 3    /* the bases and the quality line differ in length */
#define ISS_FQ_REC_TOO_LONG 4   /* a read longer than the context's max_len */
#define ISS_FQ_REC_QUAL_RANGE 5 /* a quality byte below 33 or above 126 */
#define ISS_FQ_REC_TRUNCATED 6  /* the chunk's line count is no multiple of 4, or its last byte is not '\n': the record behind
                                 * the chunk's last whole one */

typedef struct iss_fq iss_fq;
int iss_fq_create(int device_ordinal, int32_t max_len, iss_fq **out);
void iss_fq_destroy(iss_fq *fq);
const char *iss_fq_last_error(const iss_fq *fq);
int iss_fq_reset(iss_fq *fq);
int64_t iss_fq_tally_words(const iss_fq *fq); /* iss_tally_words at L = max_len, + 2 * (max_len + 1) */
int iss_fq_feed(iss_fq *fq, int32_t mate, const uint8_t *text, int64_t n_bytes);
int iss_fq_download(iss_fq *fq, uint64_t *tally, int64_t *records, int64_t *bad_record, int32_t *bad_code);
int iss_fq_kernel_ms(iss_fq *fq, double *ms);

/*
 * BGZF inflate ON THE DEVICE (additive in ABI 8): the BAM input of `model` and BGZF-compressed FASTQ in `report`.
 * A BGZF file (SAM/BAM specification 4.1) is a series of gzip members that each inflate alone, yield at most 64 KiB and carry
 * their own size (the BC subfield, BSIZE = size - 1), CRC-32 and inflated size (ISIZE).
 *
 * iss_bgzf_scan (host only, no GPU): the BSIZE chain of `data` -- up to `capacity` whole members: where each starts, where its
 * DEFLATE payload starts and how long it is, its CRC-32 and ISIZE; *consumed is the bytes they cover, an incomplete member at the end
 * is left for the next call.  Any XLEN is taken, with the BC subfield anywhere among the subfields.  ISS_E_INVALID with one line in
 * iss_inflate_last_error(NULL): no gzip magic with the extra-field flag (1f 8b 08 04), a member without BC, a BSIZE + 1 smaller than
 * the member's header and footer; the members in front of the bad one are returned all the same.
 *
 * The context: iss_inflate_feed takes HOST bytes and the scan's arrays of one group of whole members (the offsets relative to
 * `data`) and returns as soon as the bytes are in one of the context's two pinned staging buffers; the copy to the device, the kernel
 * and the copy of the result to pinned host memory follow on three streams, so that group i + 1 copies in while group i inflates and
 * group i - 1 copies out.  A feed waits for the device only to get its staging buffer back, never for a collect: any number of
 * groups may be in flight (each holds a result buffer).  iss_inflate_collect waits for the OLDEST group in flight and hands out its
 * inflated bytes -- member m at the exclusive sum of ISIZE -- and one ISS_BGZF_* status per member; the pointers are the context's
 * memory, good until the next collect, reset or destroy.  A bad member does not stop the others; its bytes are unspecified.  The
 * smallest (member index over all feeds << 8) | status is kept on the device: iss_inflate_first_bad waits for every kernel fed and
 * returns it (member -1: none).  iss_inflate_reset drops what is in flight, the first-bad word, the member count and the kernel time.
 * iss_inflate_kernel_ms waits for everything fed and gives the kernels' time from HIP events.
 * ISS_E_INVALID, nothing launched: NULL arguments, negative sizes, a group of 2^31 bytes or more on either side, payloads that are
 * not ascending inside the buffer, a member with more than 64 KiB on either side; collect with no group in flight.  n_members == 0: 0,
 * nothing launched, no group queued.
 * ISS_INFLATE_WGS (environment, read per feed): the workgroups a launch aims at.
 *
 * Status of a member, the first that applies while decoding; behind the final block SHORT, then CRC, then TRAILING:
 */
#define ISS_BGZF_OK 0
#define ISS_BGZF_BAD_BTYPE 1     /* block type 3 */
#define ISS_BGZF_STORED_LEN 2    /* a stored block's LEN and ~LEN disagree */
#define ISS_BGZF_BAD_CODE 3      /* a code-length set zlib refuses (over-subscribed, incomplete, no end-of-block code, a repeat with
                                  * nothing to repeat or past HLIT + HDIST, more than 286 / 30 codes), or bits that are no code */
#define ISS_BGZF_BAD_SYMBOL 4    /* literal/length symbol 286 or 287, distance symbol 30 or 31 */
#define ISS_BGZF_BAD_DISTANCE 5  /* a distance greater than the bytes produced so far */
#define ISS_BGZF_IN_OVERRUN 6    /* the stream wants bits behind the payload's end */
#define ISS_BGZF_OUT_OVERRUN 7   /* more than ISIZE bytes */
#define ISS_BGZF_SHORT 8         /* fewer than ISIZE bytes */
#define ISS_BGZF_TRAILING 9      /* whole payload bytes left behind the final block; the bytes are produced and checked all the same */
#define ISS_BGZF_CRC 10          /* the CRC-32 of the bytes produced is not the footer's */

typedef struct iss_inflate iss_inflate;
int iss_bgzf_scan(const uint8_t *data, int64_t n_bytes, int64_t *member_off, int64_t *pay_off, uint32_t *pay_len, uint32_t *crc,
                  uint32_t *isize, int64_t capacity, int64_t *n_members, int64_t *consumed);
int iss_inflate_create(int device_ordinal, iss_inflate **out);
void iss_inflate_destroy(iss_inflate *inf);
const char *iss_inflate_last_error(const iss_inflate *inf);
int iss_inflate_reset(iss_inflate *inf);
int iss_inflate_feed(iss_inflate *inf, const uint8_t *data, int64_t n_bytes, const int64_t *pay_off, const uint32_t *pay_len,
                     const uint32_t *crc, const uint32_t *isize, int64_t n_members);
int iss_inflate_collect(iss_inflate *inf, const uint8_t **data, int64_t *n_bytes, const uint8_t **status, int64_t *n_members);
int iss_inflate_first_bad(iss_inflate *inf, int64_t *member, int32_t *code);
int iss_inflate_kernel_ms(iss_inflate *inf, double *ms);

/*
 * `report --bam`: the tallies of iss_fq_* over BAM RECORDS, built ON THE DEVICE (additive in ABI 8): the reads of an
 * aligned BAM, or of `generate --ubam`, as the sequencer gave them -- and the insert sizes, which only a BAM holds.  A context of its
 * own, no iss_ctx and no model.  The words are exactly iss_fq_*'s at L = max_len (1 .. ISS_BR_MAX_LEN, fixed at creation),
 * iss_br_tally_words words in all (-1 for NULL):
 *   pairs [1] | qual [2][L][Q] | base [2][L][5] | gc [2][L + 1] | meanq [2][Q] | insert [I] | length [2][L + 1]
 * A record as read: its bases are "=ACMGRSVTWYHKDBN"[code] of the 4-bit codes of SEQ, its phreds the quality bytes as stored.  With
 * flag 0x10 the read as sequenced is the reverse complement of SEQ and the reversed QUAL; the complement of a code is the code with
 * its four bits in reverse order (A 1 <-> T 8, C 2 <-> G 4, N 15 and '=' 0 fixed).  The letters count as FASTQ letters do (A, C, G, T
 * base codes 0 .. 3, every other letter 4; G and C in gc).  qual, base, gc, meanq (floor of the phred sum over the read's own
 * length), length, the read of length 0 and pairs (the good records of mate 0) are iss_fq_*'s, word for word.
 * Which records count: with 0x100 or 0x800 set a record is skipped (skipped[0]); of the rest a record with 0x1 clear is mate 0; with
 * 0x1 set, 0x40 alone is mate 0 and 0x80 alone mate 1, both or neither is skipped (skipped[1]).  Unmapped records (0x4) count like
 * any other.
 * insert: a taken, good record of mate 0 with 0x1 set, 0x4 and 0x8 clear, refID == next_refID >= 0 and tlen != 0 adds one to
 * insert[clip(|tlen| - 2 * l_seq, 0, 2047)], |tlen| in 64 bits: the gap between the mates as `generate --report` counts it, exact
 * where the two mates have the same length.
 * A bad record gets the first ISS_BR_REC_* code that applies, before the skip rules (a malformed secondary record is reported); it
 * is not tallied, the records after it are, and the smallest (record index over all records fed, skipped ones included) << 8 | code
 * is kept.
 * Every count is an exact integer sum: the words depend neither on the launch geometry nor on how the records were cut into chunks.
 *
 * iss_br_feed: `data` is HOST memory, n_bytes of inflated BAM bytes that hold whole records, `offsets` the byte offset of every
 * record's block_size field as iss_bam_scan gives them.  The caller may reuse both as soon as the call returns: they go through the
 * context's pinned staging buffers, so that the copy of one chunk overlaps the kernels of the chunk before.  ISS_E_INVALID, nothing
 * launched, the tally as it was: NULL arguments, negative counts, n_bytes >= 2^31, an offset below 0 or with less than 36 bytes
 * behind it, a block_size below 32 or past the chunk's end, offsets that do not ascend.  n_records == 0: 0, nothing launched.
 * iss_br_download waits for everything fed, then copies the words, the good records taken per mate (records[2]), the skipped
 * records (skipped[2]: secondary or supplementary; mate flags) and the first bad record (*bad_record: -1 for none; *bad_code).
 * iss_br_reset zeroes the words and the counts.  iss_br_kernel_ms: as iss_fq_kernel_ms.
 * ISS_BR_WGS (environment, read per call like ISS_FQTALLY_WGS): the workgroups the record kernel aims at (the per-position kernel:
 * per column of 64 positions).
 */
#define ISS_BR_MAX_LEN 1024
#define ISS_BR_REC_SHORT 1      /* l_read_name == 0, l_seq < 0, or 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq > block_size */
#define ISS_BR_REC_TOO_LONG 2   /* l_seq > max_len */
#define ISS_BR_REC_NO_QUAL 3    /* l_seq > 0 and the first quality byte is 0xFF */
#define ISS_BR_REC_QUAL_RANGE 4 /* a quality byte above 93 */

typedef struct iss_br iss_br;
int iss_br_create(int device_ordinal, int32_t max_len, iss_br **out);
void iss_br_destroy(iss_br *br);
const char *iss_br_last_error(const iss_br *br);
int iss_br_reset(iss_br *br);
int64_t iss_br_tally_words(const iss_br *br); /* = iss_fq_tally_words at the same max_len */
int iss_br_feed(iss_br *br, const uint8_t *data, int64_t n_bytes, const int64_t *offsets, int64_t n_records);
int iss_br_download(iss_br *br, uint64_t *tally, int64_t *records, int64_t *skipped, int64_t *bad_record, int32_t *bad_code);
int iss_br_kernel_ms(iss_br *br, double *ms);

/*
 * `report --bam --errors`: the errors of an aligned BAM's reads, as CIGAR and MD tell them, tallied ON THE DEVICE by a third stage of
 * the context above (additive in ABI 8).  The words are iss_mutations_tally's at L = max_len, followed by the
 * aligned bases, 2 + 446 L + 384 in all:
 *   dropped [1] | pairs [1] | sub_q [2][L][Q] | sub_mat [2][L][5][5] | ins [2][L][5] | del [2][L][5] | per_read [2][3][K]
 *   | bases [2][L][Q]
 * A record the read tally took (good, mate 0 or 1) is ALIGNED when 0x4 is clear, n_cigar_op > 0 and l_seq > 0; one that is not adds
 * 1 to counts[2].  An aligned record is validated, the first ISS_BR_ALN_* code that applies deciding; a walk of the optional fields
 * that ends cleanly without an MD:Z adds 1 to counts[3], and the record is neither bad nor tallied.  A bad record adds 1 to
 * `dropped` and nothing else -- it is validated completely before any of its counts is added -- and the smallest (record index over
 * all records fed) << 8 | code is kept.  It stays in the read tally, whose words do not depend on this stage.
 * A valid record of mate m and length len counts at the positions and with the letters of the read as sequenced: SEQ index q at q,
 * with 0x10 at len - 1 - q and every letter complemented (letters by code: A, C, G, T in either case 0 .. 3, every other byte 4;
 * the complement 0 <-> 3, 1 <-> 2, 4 fixed).  bases[m][pos][phred] takes every column of an M, = or X operation; every MD letter at
 * SEQ index q one substitution row, sub_q[m][pos][QUAL[q]] and sub_mat[m][pos][ref][alt] (ref the MD letter, alt the SEQ letter,
 * counted also where the codes are equal); every base of an I one insertion row, ins[m][pos][alt]; every letter of a '^' group one
 * deletion row del[m][pos][ref], with q query bases in front of the D at min(q, len - 1), with 0x10 at min(len - q, len - 1): the
 * base behind the gap in sequencing order.  per_read[m][type][min(rows, K - 1)] takes the read once per type, pairs the records of
 * mate 0, counts[0 .. 1] the records per mate.  N and P consume nothing, S and H add nothing.
 * Enabling is allowed only while nothing has been fed since the context was created or reset (ISS_E_INVALID afterwards, nothing
 * changed); from then on every feed runs the stage, and the feeds' kernel time includes it.  A reset zeroes these words too and
 * leaves the stage enabled.  The word count is -1 for NULL or while the stage is off; the download returns ISS_E_INVALID for NULL
 * arguments or while the stage is off, else counts[4] (tallied per mate [2], not aligned, without MD) and the first bad alignment
 * (*bad_record: -1 for none).
 */
#define ISS_BR_ALN_CIGAR 1 /* an op code above 8, or the lengths of M, I, S, =, X do not add up to l_seq (in 64 bits) */
#define ISS_BR_ALN_TAGS 2  /* unknown type byte, value past block_size, Z / H without NUL, B with unknown subtype or negative count */
#define ISS_BR_ALN_MD 3    /* the MD string does not fit the CIGAR */
int iss_br_errors_enable(iss_br *br);
int64_t iss_br_error_words(const iss_br *br);
int iss_br_errors_download(iss_br *br, uint64_t *words, int64_t *counts /* [4] */, int64_t *bad_record, int32_t *bad_code);

/*
 * `report --bam --depth`: where an aligned BAM's reads fall on the references, as their CIGARs tell it, marked ON THE DEVICE by a
 * fourth stage of the context above (additive in ABI 8) into the CALLER's accumulator in iss_depth_*'s layout:
 * d_table is device memory, int64 [n_table][2] of (offset, length), row = refID; d_diff the int32 difference array the rows point
 * into, zeroed by the caller, 4-byte aligned.  iss_depth_finish makes depths, statistics and window sums of it.  The context keeps
 * nothing but the two pointers: both arrays have to live until the last download, and the entry CANNOT check that every row's
 * length + 1 words lie inside the array -- that is the caller's to see to.
 * A record the read tally took (good, mate 0 or 1, neither secondary nor supplementary) counts once, the first that applies:
 *   counts[1]  not aligned: 0x4 set, n_cigar_op == 0 or refID < 0
 *   counts[2]  filtered: 0x200 or 0x400 set
 *   counts[3]  mapq < min_mapq
 * -- `samtools depth`'s default filter without the supplementary records, which the context skips anyway -- and is otherwise
 * validated completely before any word is touched, the first ISS_BR_DEPTH_* code that applies deciding; a record whose row has
 * offset < 0 (checked behind _CIGAR and _REF; its length is not looked at) adds 1 to counts[4] and marks nothing.  A bad record adds
 * nothing, to no count either, and the smallest (record index over all records fed) << 8 | code is kept.  A valid record adds 1 to
 * counts[0] (marked) and is walked with a reference cursor that starts at pos: M, = and X cover [cursor, cursor + len) and advance;
 * D advances, and covers only with ISS_BR_DEPTH_COUNT_DEL; N advances and never covers; I, S, H and P do nothing.  Every covered run
 * adds +1 at offset + start and -1 at offset + end, and its length to counts[5] (covered bases).  A record's runs are disjoint, so it
 * adds at most 1 to a base: while the stage is on iss_br_feed refuses (ISS_E_INVALID, nothing launched) the records that would take
 * the records fed past 2^31 - 1.  All results are exact integers, independent of the launch geometry (ISS_BR_WGS) and of how the
 * records were cut into feeds.
 * iss_br_depth_enable is allowed only while nothing has been fed since the context was created or reset (ISS_E_INVALID afterwards,
 * nothing changed); also ISS_E_INVALID: NULL or misaligned pointers, n_table < 1, flag bits other than ISS_BR_DEPTH_COUNT_DEL,
 * min_mapq outside 0 .. 255.  Enabling again (before a feed) replaces the pointers and zeroes the counts.  From then on every feed
 * runs the stage, and the feeds' kernel time includes it.  iss_br_reset zeroes the counts and the first-bad word; it leaves the
 * caller's array alone and the stage on.  iss_br_depth_download (ISS_E_INVALID for NULL arguments or while the stage is off) waits
 * for everything fed: when it returns the array is complete, and work on any other stream -- iss_depth_finish -- may read it.
 */
#define ISS_BR_DEPTH_COUNT_DEL 1u /* flags: the bases of a D count as covered */
#define ISS_BR_DEPTH_CIGAR 1 /* an op code above 8 */
#define ISS_BR_DEPTH_REF 2   /* refID >= n_table */
#define ISS_BR_DEPTH_SPAN 3  /* pos < 0, or pos + the lengths of M, D, N, =, X (summed in 64 bits) > the row's length */
int iss_br_depth_enable(iss_br *br, const int64_t *d_table, int32_t n_table, int32_t *d_diff, uint32_t flags, int32_t min_mapq);
int iss_br_depth_download(iss_br *br, int64_t *counts /* [6] */, int64_t *bad_record, int32_t *bad_code);

/*
 * `generate --variants`: a record with a VCF's alleles spliced in ON THE DEVICE, in front of the pack kernel (additive in ABI 8;
 * DESIGN.md section 30).  The tables of a record of `length` letters with n variants, sorted and disjoint (pos0[i + 1] >= pos0[i] +
 * ref_len[i]; no two pure insertions at one pos0; none empty; none past the record's end):
 *   pos0 [n] int64: the first replaced letter, 0-based; ref_len / alt_len [n] int32: letters replaced / put in; alt_off / ref_off [n]
 *   int64: where the variant's ALT / REF letters start in the blobs alt [n_alt] / ref [n_ref]; out_pos [n + 1] int64: pos0[i] plus the
 *   sum of alt_len[j] - ref_len[j] over j < i, out_pos[n] the haplotype's length L'.
 * Output offset o, with i the last variant whose out_pos[i] <= o and k = o - out_pos[i]: alt[alt_off[i] + k] while k < alt_len[i],
 * else ascii[pos0[i] + ref_len[i] + k - alt_len[i]]; in front of the first variant ascii[o].
 * iss_genome_upload_variants stages the letters and tables in HBM, compares every variant's REF letters with the record (case
 * ignored; a mismatch: ISS_E_INVALID, one line with the POS and both spellings), builds the haplotype into the new genome's ASCII
 * copy and packs it like iss_genome_upload does a large record: letters outside the alphabet -- ALT letters too -- are found there.
 * 1 <= L' <= 2^34 - 4096.  Tables that break a rule above: ISS_E_INVALID, nothing launched.  The call returns when the genome is
 * resident (the caller's buffers are free); it holds length + L' letters on the device while it runs.  The lift tables stay with the
 * genome until iss_genome_clear.
 * iss_genome_download: the resident ASCII copy of any genome (capacity >= its length; ascii NULL: *length alone).  Waits for the stream.
 * iss_variants_lift: d_out[t] = the record coordinate of haplotype coordinate d_in[t] (device arrays of n int64) of genome d_gid[t]
 * (device int32 [n]; NULL: `gid` for all).  With i the last variant whose out_pos[i] <= h and k = h - out_pos[i]: pos0[i] +
 * min(k, ref_len[i]) inside the ALT run (k < alt_len[i]), pos0[i] + ref_len[i] + k - alt_len[i] behind it, h in front of the first
 * variant.  Non-decreasing, L' -> length: valid for half-open interval ends.  A genome without tables, or an id that names none:
 * the identity.  Asynchronous on the context's stream, like iss_output_export (the first call after an upload waits for it once).
 * iss_variants_apply_tile: output bytes per workgroup of the splice kernel (tests straddle it).
 * iss_variants_host_apply / iss_variants_host_lift (host only, no GPU): the same mapping, compiled from the same source, on the
 * caller's tables; out takes out_pos[n] <= capacity letters.  The apply checks its tables like the upload; the lift reads only
 * entries [0, n) of them.
 */
int iss_genome_upload_variants(iss_ctx *ctx, const uint8_t *ascii, int64_t length, int64_t n, const int64_t *pos0,
                               const int32_t *ref_len, const int32_t *alt_len, const int64_t *alt_off, const uint8_t *alt, int64_t n_alt,
                               const int64_t *ref_off, const uint8_t *ref, int64_t n_ref, const int64_t *out_pos, int32_t *genome_id);
int iss_genome_download(iss_ctx *ctx, int32_t genome_id, uint8_t *ascii, int64_t capacity, int64_t *length);
int iss_variants_lift(iss_ctx *ctx, const int32_t *d_gid, int32_t gid, const int64_t *d_in, int64_t n, int64_t *d_out);
int iss_variants_apply_tile(void);
int iss_variants_host_apply(const uint8_t *ascii, int64_t length, int64_t n, const int64_t *pos0, const int32_t *ref_len,
                            const int32_t *alt_len, const int64_t *alt_off, const uint8_t *alt, int64_t n_alt, const int64_t *out_pos,
                            uint8_t *out, int64_t capacity);
int iss_variants_host_lift(int64_t n, const int64_t *pos0, const int32_t *ref_len, const int32_t *alt_len, const int64_t *out_pos,
                           const int64_t *in, int64_t n_coords, int64_t *out);

/*
 * `generate --device_fasta`: a genome FASTA indexed and its line ends removed ON THE DEVICE, in front of the pack kernels (additive in
 * ABI 8).  The host sends the bytes as they stand in the file.  The grammar over a text of n bytes:
 *   a HEADER starts at a '>' that is byte 0 or directly follows '\n'; bytes in front of the first header are ignored;
 *   header_off: that '>'; header_len: the bytes between it and the next '\n' (or the end of the text); the caller decodes and strips;
 *   the BODY runs from behind that '\n' (body_off, body_len bytes) to the next header or the end of the text;
 *   letters: the body's bytes other than '\r' and '\n';
 *   flags: ISS_FA_ODD when the body holds a byte outside 0x21 .. 0x7E other than '\r' and '\n' -- the caller takes such a record
 *   through its line-by-line parser.
 * Every offset is 64-bit and relative to the text.
 * iss_fa_create / iss_fa_destroy / iss_fa_last_error: a device session without a model, like iss_inflate.
 * iss_fa_index: `text` is host memory.  *n_records: the headers of the text.  With capacity < *n_records (0: always, unless the text
 * has no header) nothing else is written; otherwise the six arrays get one row per record.  The text must fit one device allocation.
 * iss_fasta_host_index (host only, no GPU): the same table from the same grammar source.
 * iss_fasta_tile: bytes per workgroup of the kernels; iss_fasta_scan_span: tiles per pass of the prefix scan (tests size by both).
 * iss_genome_upload_fasta: `text` is a host span of the file, n rows with offsets relative to it.  The table is checked on the host
 * first -- bodies inside the span, ascending, not overlapping, letters <= body_len -- and one that fails is ISS_E_INVALID with nothing
 * launched.  Records of at most 2^20 letters become ONE group with the arena layout, the ids and the -1 rule (no letters, too many, a
 * letter outside the rev_comp alphabet) of iss_genome_upload_group; a larger record comes alone (n = 1) and becomes a genome like a
 * large record of iss_genome_upload, its errors included.  A letter is stored only inside its record's place; a table that does not
 * fit the text (letters counted wrongly) is ISS_E_INVALID after the kernels ran, and no genome is made.  The call returns when the
 * genomes are resident; it holds the span on the device while it runs.  The resident ASCII copy is the stripped letters.
 */
#define ISS_FA_ODD 1
typedef struct iss_fa iss_fa;
int iss_fa_create(int device_ordinal, iss_fa **fa);
void iss_fa_destroy(iss_fa *fa);
const char *iss_fa_last_error(const iss_fa *fa);
int iss_fa_index(iss_fa *fa, const uint8_t *text, int64_t n_bytes, int64_t capacity, int64_t *header_off, int64_t *header_len,
                 int64_t *body_off, int64_t *body_len, int64_t *letters, int32_t *flags, int64_t *n_records);
int iss_fasta_host_index(const uint8_t *text, int64_t n_bytes, int64_t capacity, int64_t *header_off, int64_t *header_len, int64_t *body_off,
                         int64_t *body_len, int64_t *letters, int32_t *flags, int64_t *n_records);
int iss_fasta_tile(void);
int iss_fasta_scan_span(void);
int iss_genome_upload_fasta(iss_ctx *ctx, const uint8_t *text, int64_t n_bytes, int32_t n, const int64_t *body_off, const int64_t *body_len,
                            const int64_t *letters, int32_t *genome_ids);

#ifdef __cplusplus
}
#endif
#endif /* ISS_MI355X_H */
