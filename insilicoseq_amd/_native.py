"""ctypes binding of the C ABI in include/iss_mi355x.h (libiss_mi355x.so, built in-tree).

There is NO fallback: if the HIP library is missing or no MI355X is visible, the product
raises (``NativeLibraryError`` / ``EngineError``) instead of computing anything on the CPU."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libiss_mi355x.so"
LIB_PATH = os.environ.get("ISS_MI355X_LIB") or os.path.join(_HERE, LIB_NAME)  # override: A/B builds (tools/ab_bench.sh)

E_INVALID, E_HIP, E_NOMEM, E_SHORT_RECORD, E_IO = -1, -2, -3, -4, -5
SEQ_TYPES = {"metagenomics": 0, "amplicon": 1}
EXPORT_ENCODINGS = {"ascii": 0, "codes": 1}  # ISS_EXPORT_ASCII / ISS_EXPORT_CODES

# every symbol include/iss_mi355x.h declares (tests check the library exports all of them)
EXPORTS = (
    "iss_abi_version", "iss_ctx_create", "iss_ctx_destroy", "iss_last_error", "iss_ctx_set_stream",
    "iss_model_upload", "iss_genome_upload", "iss_genome_upload_packed", "iss_genome_upload_group", "iss_genome_clear", "iss_output_reserve", "iss_output_pitch",
    "iss_output_device_ptrs", "iss_output_row", "iss_generate", "iss_synchronize", "iss_output_download",
    "iss_output_download_coords", "iss_timing_enable", "iss_timing_read", "iss_stats_read", "iss_build_id", "iss_fastq_write",
    "iss_mt_seed", "iss_generate_mt", "iss_mt_peek", "iss_mt_mutations_reserve", "iss_mt_mutations_download",
    "iss_mt_set_fragment", "iss_set_fragment", "iss_mutations_reserve", "iss_mutations_download",
    "iss_mt_path_counts", "iss_fastq_emit", "iss_fastq_flush", "iss_fastq_compress", "iss_deflate_code_build",
    "iss_generate_batch", "iss_fastq_emit_batch", "iss_gen_phred_scores", "iss_mut_sequence", "iss_random_insert_size",
    "iss_introduce_indels", "iss_ev_step", "iss_mt_workers_seed", "iss_generate_mt_workers", "iss_mt_workers_peek",
    "iss_main_kernel", "iss_fastq_emit_scatter", "iss_vcf_emit", "iss_vcf_flush",
    "iss_mt_workers_mutations_reserve", "iss_mt_workers_mutations_download", "iss_vcf_emit_workers",
    "iss_bam_scan", "iss_bam_create", "iss_bam_destroy", "iss_bam_last_error", "iss_bam_reset", "iss_bam_feed",
    "iss_bam_tally_download", "iss_bam_kde",
    "iss_output_export", "iss_ctx_set_stream_ordered", "iss_mutations_export",
    "iss_tally_words", "iss_output_tally",
    "iss_depth_mark", "iss_depth_finish",
    "iss_ubam_emit_batch", "iss_ubam_flush", "iss_ubam_host_records",
    "iss_origins_emit_batch", "iss_origins_flush", "iss_origins_host_text",
    "iss_origins_compress", "iss_vcf_compress", "iss_bgzf_text_code_build",
    "iss_error_tally_words", "iss_mutations_tally",
    "iss_fq_create", "iss_fq_destroy", "iss_fq_last_error", "iss_fq_reset", "iss_fq_tally_words", "iss_fq_feed", "iss_fq_download",
    "iss_fq_kernel_ms",
    "iss_bgzf_scan", "iss_inflate_create", "iss_inflate_destroy", "iss_inflate_last_error", "iss_inflate_reset", "iss_inflate_feed",
    "iss_inflate_collect", "iss_inflate_first_bad", "iss_inflate_kernel_ms",
    "iss_br_create", "iss_br_destroy", "iss_br_last_error", "iss_br_reset", "iss_br_tally_words", "iss_br_feed", "iss_br_download",
    "iss_br_kernel_ms", "iss_br_errors_enable", "iss_br_error_words", "iss_br_errors_download",
    "iss_br_depth_enable", "iss_br_depth_download",
    "iss_mt_resolver_pick",
    "iss_genome_upload_variants", "iss_genome_download", "iss_variants_lift", "iss_variants_apply_tile", "iss_variants_host_apply",
    "iss_variants_host_lift",
)
# `generate --device_fasta` (a build from before them still loads; fasta.FastaIndexer and ReadEngine.add_genomes_fasta then raise)
FASTA_ENTRIES = ("iss_fa_create", "iss_fa_destroy", "iss_fa_last_error", "iss_fa_index", "iss_fasta_host_index", "iss_fasta_tile",
                 "iss_fasta_scan_span", "iss_genome_upload_fasta")
EXPORTS += FASTA_ENTRIES

# The stand-alone device contexts (class Session below): entry prefix -> the arguments of its create call between the device ordinal
# and the handle.  Each has create, destroy, last_error and reset; kernel_ms and tally_words where EXPORTS names them.
SESSIONS = {"iss_bam": (), "iss_fq": (C.c_int32,), "iss_inflate": (), "iss_br": (C.c_int32,)}

# `model` tallies (include/iss_mi355x.h: ISS_BAM_*)
BAM_MAX_LEN, BAM_NQ, BAM_NTLEN = 301, 94, 2000
BAM_OFF_INDEL, BAM_OFF_QHIST, BAM_OFF_TLEN, BAM_OFF_NREAD, BAM_OFF_MINLEN, BAM_OFF_TAKEN, BAM_TALLY_WORDS = (
    9632, 15050, 241402, 243402, 243410, 243418, 243426)
BAM_REC_ERRORS = {
    1: "malformed record", 2: "read longer than 301 bases", 3: "read without qualities", 4: "CIGAR operation other than M/I/D/S/H",
    5: "mapped read without an MD tag", 6: "MD tag does not match the CIGAR", 7: "indel position outside the read",
    8: "quality above 93", 9: "CIGAR length differs from the read length",
}


# `report` (include/iss_mi355x.h: ISS_FQ_*)
FQ_MAX_LEN = 1024
FQ_REC_ERRORS = {
    1: "line 1 of the record does not start with '@'", 2: "line 3 of the record does not start with '+'",
    3: "the bases and the quality line differ in length", 4: "read longer than --max_length",
    5: "quality character outside '!' .. '~'", 6: "truncated record (the file ends inside it)",
}

# `report --bam` (include/iss_mi355x.h: ISS_BR_*)
BR_MAX_LEN = 1024
BR_REC_ERRORS = {
    1: "malformed record (its fields do not fit its block_size)", 2: "read longer than --max_length", 3: "read without qualities",
    4: "quality above 93",
}
BR_ALN_ERRORS = {
    1: "CIGAR with an unknown operation, or one that does not add up to the read's length",
    2: "malformed optional fields", 3: "MD tag does not fit the CIGAR",
}
BR_DEPTH_ERRORS = {  # `report --bam --depth` (ISS_BR_DEPTH_*)
    1: "CIGAR with an unknown operation", 2: "reference index past the header's references",
    3: "alignment that starts before or ends past its reference",
}
BR_DEPTH_COUNT_DEL = 1


# the device inflate (include/iss_mi355x.h: ISS_BGZF_*)
BGZF_STATUS = ("OK", "BAD_BTYPE", "STORED_LEN", "BAD_CODE", "BAD_SYMBOL", "BAD_DISTANCE", "IN_OVERRUN", "OUT_OVERRUN", "SHORT", "TRAILING",
               "CRC")
BGZF_OK, BGZF_TRAILING = 0, 9


class NativeLibraryError(RuntimeError):
    pass


class EngineError(RuntimeError):
    def __init__(self, code, message):
        RuntimeError.__init__(self, "%s (iss error %d)" % (message, code))
        self.code = code
        self.message = message

    def __reduce__(self):
        # (a worker of `generate`'s process pool hands its exception to the parent pickled: one that cannot be rebuilt there
        #  kills the pool's result thread, and the command waits for ever instead of failing)
        return (EngineError, (self.code, self.message))


class ModelTables(C.Structure):
    _fields_ = [
        ("read_length", C.c_int32), ("n_isize", C.c_int32), ("n_q", C.c_int32),
        ("isize_thr", C.c_void_p), ("bin_thr", C.c_void_p), ("bin_nonempty", C.c_void_p), ("q_thr", C.c_void_p),
        ("subst_thr", C.c_void_p), ("subst_alt", C.c_void_p), ("ins_thr", C.c_void_p), ("ins_letter", C.c_void_p),
        ("del_thr", C.c_void_p), ("mut_thr", C.c_void_p),
        ("quality_mode", C.c_int32), ("basic_insert_size", C.c_int32), ("basic_mean", C.c_double),
        ("basic_sd", C.c_double), ("basic_cap", C.c_double),
    ]


_lib = None


def lib():
    """Load the HIP library (once).  Raises NativeLibraryError when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH)
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:
        raise NativeLibraryError("cannot load %s: %s" % (LIB_PATH, e))
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    L.iss_abi_version.restype = C.c_int
    L.iss_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.iss_ctx_destroy.argtypes = [vp]
    L.iss_ctx_destroy.restype = None
    L.iss_last_error.argtypes = [vp]
    L.iss_last_error.restype = C.c_char_p
    L.iss_ctx_set_stream.argtypes = [vp, vp]
    L.iss_model_upload.argtypes = [vp, C.POINTER(ModelTables)]
    L.iss_genome_upload.argtypes = [vp, vp, i64, C.POINTER(i32)]
    L.iss_genome_upload_packed.argtypes = [vp, vp, i64, i32, C.POINTER(i32)]
    L.iss_genome_upload_group.argtypes = [vp, i32, vp, vp, vp]
    L.iss_genome_clear.argtypes = [vp]
    L.iss_output_reserve.argtypes = [vp, i64]
    L.iss_output_pitch.argtypes = [vp]
    L.iss_output_row.argtypes = [vp]
    L.iss_output_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.iss_generate.argtypes = [vp, i32, i64, u64, u64, i32, i32, i64]
    L.iss_synchronize.argtypes = [vp]
    L.iss_output_download.argtypes = [vp, i64, i64, vp, vp, vp, vp]
    L.iss_output_download_coords.argtypes = [vp, i64, i64, vp]
    L.iss_timing_enable.argtypes = [vp, C.c_int]
    L.iss_timing_read.argtypes = [vp, C.POINTER(C.c_double * 4), C.POINTER(i64)]
    L.iss_stats_read.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.iss_build_id.restype = C.c_char_p
    L.iss_build_id.argtypes = []
    L.iss_mt_seed.argtypes = [vp, u64]
    L.iss_generate_mt.argtypes = [vp, i32, i64, i32, i32, i64, C.POINTER(i64)]
    L.iss_mt_peek.argtypes = [vp, vp, vp, i32]
    L.iss_mt_path_counts.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.iss_mt_workers_seed.argtypes = [vp, i32, vp]
    L.iss_generate_mt_workers.argtypes = [vp, i32, vp, vp, vp, i32, i32, vp, vp]
    L.iss_mt_workers_peek.argtypes = [vp, i32, vp, vp, i32]
    L.iss_mt_mutations_reserve.argtypes = [vp, i64]
    L.iss_mt_set_fragment.argtypes = [vp, i32, C.c_double, C.c_double]
    L.iss_set_fragment.argtypes = [vp, i32, C.c_double, C.c_double]
    L.iss_mutations_reserve.argtypes = [vp, i64]
    L.iss_mutations_download.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.iss_mt_mutations_download.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.iss_fastq_emit.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, i64, i32, i64, i64, i32]
    L.iss_fastq_emit_batch.argtypes = [vp, C.c_int, C.c_int, i32, vp, vp, vp, vp, i32]
    L.iss_fastq_emit_scatter.argtypes = [vp, C.c_int, C.c_int, i32, vp, vp, vp, vp, vp, vp, i32]
    # (the two entries a build from before them lacks: such a build still loads -- ISS_MI355X_LIB, A/B runs against an older
    #  library -- and ReadEngine.vcf_emit raises; build() and the tests check that the in-tree library exports every name)
    if hasattr(L, "iss_vcf_emit") and hasattr(L, "iss_vcf_flush"):
        L.iss_vcf_emit.argtypes = [vp, C.c_int, i32, i32, vp, vp, vp, vp, i32, C.POINTER(i64)]
        L.iss_vcf_flush.argtypes = [vp]
    # (additive to ABI 8 as well: --store_mutations for the workers of a set)
    if hasattr(L, "iss_vcf_emit_workers"):
        L.iss_mt_workers_mutations_reserve.argtypes = [vp, i64]
        L.iss_mt_workers_mutations_download.argtypes = [vp, i32, vp, i64, C.POINTER(i64)]
        L.iss_vcf_emit_workers.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    # (additive to ABI 8: the rows as dense device arrays; a build from before them still loads and ReadEngine.export raises)
    if hasattr(L, "iss_output_export"):
        L.iss_output_export.argtypes = [vp, i64, i64, i32, vp, vp, vp, vp]
        L.iss_ctx_set_stream_ordered.argtypes = [vp, vp]
    # (additive to ABI 8 again: the mutation rows as dense device arrays; without it ReadEngine.export_mutations raises)
    if hasattr(L, "iss_mutations_export"):
        L.iss_mutations_export.argtypes = [vp, i64, i64, i32, vp, vp, i64, vp]
    # (additive to ABI 8 once more: tallies of the rows built on the device; without them ReadEngine.tally raises)
    if hasattr(L, "iss_output_tally"):
        L.iss_tally_words.argtypes = [vp]
        L.iss_output_tally.argtypes = [vp, i64, i64, vp]
    # (and again: per-base coverage depth built on the device; without them ReadEngine.depth_mark / depth_finish raise)
    if hasattr(L, "iss_depth_mark"):
        L.iss_depth_mark.argtypes = [vp, i64, i64, vp, i32, vp]
        L.iss_depth_finish.argtypes = [vp, vp, i64, vp, vp, i32, i32, vp, vp]
    # (and once more: unaligned BAM built on the device; without them ReadEngine.ubam_emit_batch / ubam_flush raise)
    if hasattr(L, "iss_ubam_emit_batch"):
        L.iss_ubam_emit_batch.argtypes = [vp, C.c_int, i32, vp, vp, vp, vp, i32]
        L.iss_ubam_flush.argtypes = [vp]
        L.iss_ubam_host_records.argtypes = [C.c_int, C.c_char_p, i64, i32, i64, i32, i32, vp, vp, vp, vp]
    # (and the pairs' source intervals as BEDPE text built on the device; without them ReadEngine.origins_emit_batch / origins_flush raise)
    if hasattr(L, "iss_origins_emit_batch"):
        L.iss_origins_emit_batch.argtypes = [vp, C.c_int, i32, vp, vp, vp, vp, vp, i32]
        L.iss_origins_flush.argtypes = [vp]
        L.iss_origins_host_text.argtypes = [C.c_int, C.c_char_p, i64, i32, i64, i32, i64, vp]
    # (and the BGZF stage of the two text pipes; without them ReadEngine.origins_compress / vcf_compress raise)
    if hasattr(L, "iss_origins_compress"):
        L.iss_origins_compress.argtypes = [vp, i32]
        L.iss_vcf_compress.argtypes = [vp, i32]
        L.iss_bgzf_text_code_build.argtypes = [vp, vp, vp, vp, vp]
    # (and tallies of the mutation rows built on the device; without them ReadEngine.error_tally raises)
    if hasattr(L, "iss_mutations_tally"):
        L.iss_error_tally_words.argtypes = [vp]
        L.iss_mutations_tally.argtypes = [vp, i32, i64, i64, vp]
    # (and `report`, `report --bam` and the device inflate: their own entries here, what every session has in the loop over
    #  SESSIONS below; without them FastqTally, BamReadTally and BgzfInflater raise)
    if hasattr(L, "iss_fq_feed"):
        L.iss_fq_feed.argtypes = [vp, i32, vp, i64]
        L.iss_fq_download.argtypes = [vp, vp, vp, vp, vp]
    if hasattr(L, "iss_br_feed"):
        L.iss_br_feed.argtypes = [vp, vp, i64, vp, i64]
        L.iss_br_download.argtypes = [vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i32)]
    # (and the alignments' errors behind `report --bam`; without them BamReadTally(errors=True) raises)
    if hasattr(L, "iss_br_errors_enable"):
        L.iss_br_errors_enable.argtypes = [vp]
        L.iss_br_error_words.argtypes = [vp]
        L.iss_br_errors_download.argtypes = [vp, vp, vp, C.POINTER(i64), C.POINTER(i32)]
    # (and the alignments' reference intervals behind `report --bam`; without them BamReadTally(depth=True) raises)
    if hasattr(L, "iss_br_depth_enable"):
        L.iss_br_depth_enable.argtypes = [vp, vp, i32, vp, C.c_uint32, i32]
        L.iss_br_depth_download.argtypes = [vp, vp, C.POINTER(i64), C.POINTER(i32)]
    if hasattr(L, "iss_inflate_feed"):
        L.iss_bgzf_scan.argtypes = [vp, i64, vp, vp, vp, vp, vp, i64, C.POINTER(i64), C.POINTER(i64)]
        L.iss_inflate_feed.argtypes = [vp, vp, i64, vp, vp, vp, vp, i64]
        L.iss_inflate_collect.argtypes = [vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp), C.POINTER(i64)]
        L.iss_inflate_first_bad.argtypes = [vp, C.POINTER(i64), C.POINTER(i32)]
    # (and which resolver instantiation MT mode takes; without it ReadEngine.mt_resolver raises)
    if hasattr(L, "iss_mt_resolver_pick"):
        L.iss_mt_resolver_pick.argtypes = [vp, C.POINTER(i32 * 3)]
    # (and `generate --variants`: a record's haplotype spliced on the device; without them ReadEngine.add_genome_variants raises)
    if hasattr(L, "iss_genome_upload_variants"):
        L.iss_genome_upload_variants.argtypes = [vp, vp, i64, i64, vp, vp, vp, vp, vp, i64, vp, vp, i64, vp, C.POINTER(i32)]
        L.iss_genome_download.argtypes = [vp, i32, vp, i64, C.POINTER(i64)]
        L.iss_variants_lift.argtypes = [vp, vp, i32, vp, i64, vp]
        L.iss_variants_apply_tile.argtypes = []
        L.iss_variants_host_apply.argtypes = [vp, i64, i64, vp, vp, vp, vp, vp, i64, vp, vp, i64]
        L.iss_variants_host_lift.argtypes = [i64, vp, vp, vp, vp, vp, i64, vp]
    # (and `generate --device_fasta`: the genome FASTA indexed and stripped on the device -- a session without reset, so not one of
    #  SESSIONS; without them fasta.FastaIndexer and ReadEngine.add_genomes_fasta raise)
    if hasattr(L, "iss_fa_index"):
        L.iss_fa_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.iss_fa_destroy.argtypes = [vp]
        L.iss_fa_destroy.restype = None
        L.iss_fa_last_error.argtypes = [vp]
        L.iss_fa_last_error.restype = C.c_char_p
        L.iss_fa_index.argtypes = [vp, vp, i64, i64, vp, vp, vp, vp, vp, vp, C.POINTER(i64)]
        L.iss_fasta_host_index.argtypes = [vp, i64, i64, vp, vp, vp, vp, vp, vp, C.POINTER(i64)]
        L.iss_fasta_tile.argtypes = []
        L.iss_fasta_scan_span.argtypes = []
        L.iss_genome_upload_fasta.argtypes = [vp, vp, i64, i32, vp, vp, vp, vp]
    L.iss_main_kernel.argtypes = [vp, vp, C.c_int]
    L.iss_fastq_flush.argtypes = [vp]
    L.iss_generate_batch.argtypes = [vp, i32, vp, vp, C.c_uint64, C.c_uint64, i32, i32, i64]
    L.iss_fastq_compress.argtypes = [vp, i32]
    L.iss_deflate_code_build.argtypes = [vp, C.c_uint32, vp, vp, vp, vp]
    L.iss_gen_phred_scores.argtypes = [vp, i32, i64, u64, u64, vp]
    L.iss_mut_sequence.argtypes = [vp, i32, i64, u64, u64, vp, vp, vp]
    L.iss_random_insert_size.argtypes = [vp, i64, u64, u64, vp]
    L.iss_introduce_indels.argtypes = [vp, i32, i64, u64, u64, vp, vp, vp, i64, vp, vp, vp]
    L.iss_ev_step.argtypes = [vp, i32, i64, vp, vp, vp, vp, vp, vp]
    L.iss_fastq_write.argtypes = [C.c_int, C.c_int, C.c_char_p, i64, i32, i64, i32, i32, vp, vp, vp, vp, i32]
    L.iss_bam_scan.argtypes = [vp, i64, vp, i64, C.POINTER(i64), C.POINTER(i64)]
    L.iss_bam_feed.argtypes = [vp, vp, i64, vp, vp, i64]
    L.iss_bam_tally_download.argtypes = [vp, vp, C.POINTER(i64), C.POINTER(i32)]
    L.iss_bam_kde.argtypes = [vp, i32, i32, vp, vp]
    session_entries = tuple(prefix + "_" for prefix in SESSIONS)
    for name in EXPORTS:
        if (name.startswith(session_entries) or name in (
                "iss_vcf_emit", "iss_vcf_flush", "iss_mt_workers_mutations_reserve", "iss_mt_workers_mutations_download",
                "iss_vcf_emit_workers", "iss_output_export", "iss_ctx_set_stream_ordered", "iss_mutations_export", "iss_tally_words",
                "iss_output_tally", "iss_depth_mark", "iss_depth_finish", "iss_ubam_emit_batch", "iss_ubam_flush",
                "iss_ubam_host_records", "iss_origins_emit_batch", "iss_origins_flush", "iss_origins_host_text",
                "iss_origins_compress", "iss_vcf_compress", "iss_bgzf_text_code_build", "iss_error_tally_words",
                "iss_mutations_tally", "iss_bgzf_scan", "iss_mt_resolver_pick", "iss_genome_upload_variants", "iss_genome_download",
                "iss_variants_lift", "iss_variants_apply_tile", "iss_variants_host_apply", "iss_variants_host_lift") + FASTA_ENTRIES) and not hasattr(L, name):
            continue
        if name not in ("iss_ctx_destroy", "iss_last_error", "iss_build_id", "iss_fa_destroy", "iss_fa_last_error"):
            getattr(L, name).restype = C.c_int
    if hasattr(L, "iss_tally_words"):
        L.iss_tally_words.restype = i64
    if hasattr(L, "iss_error_tally_words"):
        L.iss_error_tally_words.restype = i64
    if hasattr(L, "iss_br_error_words"):
        L.iss_br_error_words.restype = i64
    # what every session has (a library from before a prefix still loads, and that prefix's Session raises); the entries whose
    # restype is not int are set here, behind the loop above
    for prefix, create_args in SESSIONS.items():
        if not hasattr(L, prefix + "_create"):
            continue
        getattr(L, prefix + "_create").argtypes = [C.c_int] + list(create_args) + [C.POINTER(vp)]
        getattr(L, prefix + "_destroy").argtypes = [vp]
        getattr(L, prefix + "_destroy").restype = None
        getattr(L, prefix + "_last_error").argtypes = [vp]
        getattr(L, prefix + "_last_error").restype = C.c_char_p
        getattr(L, prefix + "_reset").argtypes = [vp]
        if prefix + "_kernel_ms" in EXPORTS:
            getattr(L, prefix + "_kernel_ms").argtypes = [vp, C.POINTER(C.c_double)]
        if prefix + "_tally_words" in EXPORTS:
            getattr(L, prefix + "_tally_words").argtypes = [vp]
            getattr(L, prefix + "_tally_words").restype = i64
    _lib = L
    return L


def check(ctx, rc):
    if rc < 0:
        msg = lib().iss_last_error(ctx)
        raise EngineError(rc, msg.decode("utf-8", "replace") if msg else "unknown error")
    return rc


class Session(object):
    """A stand-alone device context of the library, one of SESSIONS: the handle, its errors and its life.  A subclass names its
    entry prefix and hands __init__ the arguments of its create call; ``_entry("feed")`` is the library's ``<prefix>_feed``."""

    PREFIX = None

    def __init__(self, device=0, *create_args):
        self._lib = lib()
        if not hasattr(self._lib, self.PREFIX + "_create"):
            raise NativeLibraryError("%s has no %s_* entries: rebuild it" % (LIB_PATH, self.PREFIX))
        self.device = int(device)
        self._h = C.c_void_p()
        try:  # (a create that fails may leave a handle: its error is read from it, then it goes)
            self._check(self._entry("create")(self.device, *create_args, C.byref(self._h)))
        except EngineError:
            self.close()
            raise

    def _entry(self, name):
        return getattr(self._lib, "%s_%s" % (self.PREFIX, name))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._entry("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc < 0:
            msg = self._entry("last_error")(self._h if self._h else None)
            raise EngineError(rc, msg.decode("utf-8", "replace") if msg else "unknown error")
        return rc

    def reset(self):
        self._check(self._entry("reset")(self._h))

    def kernel_ms(self):
        """Milliseconds the kernels of all feeds since the last reset took on the device (waits for them)."""
        ms = C.c_double()
        self._check(self._entry("kernel_ms")(self._h, C.byref(ms)))
        return ms.value
