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


# The binding, one row per declaration of include/iss_mi355x.h in the header's order: (name, restype, argtypes, group).  group None: every
# supported build has the entry.  A label: the entries that arrived together, additive to ABI 8 -- a build from before them still loads
# (ISS_MI355X_LIB, A/B runs against an older library) and need() raises where they are asked for.  To add an entry: its declaration in
# the header and its row here; tests/test_native_table_host.py holds the two to each other, type for type.
P, vp, str_, int_, i32, i64, u32, u64, f64 = C.POINTER, C.c_void_p, C.c_char_p, C.c_int, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_double
TABLE = (
    ("iss_abi_version", int_, (), None),
    ("iss_build_id", str_, (), None),
    ("iss_ctx_create", int_, (int_, P(vp)), None),
    ("iss_ctx_destroy", None, (vp,), None),
    ("iss_last_error", str_, (vp,), None),
    ("iss_ctx_set_stream", int_, (vp, vp), None),
    ("iss_model_upload", int_, (vp, P(ModelTables)), None),
    ("iss_genome_upload", int_, (vp, vp, i64, P(i32)), None),
    ("iss_genome_upload_packed", int_, (vp, vp, i64, i32, P(i32)), None),
    ("iss_genome_upload_group", int_, (vp, i32, vp, vp, vp), None),
    ("iss_genome_clear", int_, (vp,), None),
    ("iss_output_reserve", int_, (vp, i64), None),
    ("iss_output_pitch", int_, (vp,), None),
    ("iss_output_device_ptrs", int_, (vp, P(vp), P(vp), P(vp), P(vp)), None),
    ("iss_output_row", int_, (vp,), None),
    ("iss_generate", int_, (vp, i32, i64, u64, u64, i32, i32, i64), None),
    ("iss_generate_batch", int_, (vp, i32, vp, vp, u64, u64, i32, i32, i64), None),
    ("iss_set_fragment", int_, (vp, i32, f64, f64), None),
    ("iss_synchronize", int_, (vp,), None),
    ("iss_gen_phred_scores", int_, (vp, i32, i64, u64, u64, vp), None),
    ("iss_mut_sequence", int_, (vp, i32, i64, u64, u64, vp, vp, vp), None),
    ("iss_random_insert_size", int_, (vp, i64, u64, u64, vp), None),
    ("iss_introduce_indels", int_, (vp, i32, i64, u64, u64, vp, vp, vp, i64, vp, vp, vp), None),
    ("iss_ev_step", int_, (vp, i32, i64, vp, vp, vp, vp, vp, vp), None),
    ("iss_mutations_reserve", int_, (vp, i64), None),
    ("iss_mutations_download", int_, (vp, vp, i64, P(i64)), None),
    ("iss_output_download", int_, (vp, i64, i64, vp, vp, vp, vp), None),
    ("iss_output_download_coords", int_, (vp, i64, i64, vp), None),
    ("iss_output_export", int_, (vp, i64, i64, i32, vp, vp, vp, vp), "export"),
    ("iss_mutations_export", int_, (vp, i64, i64, i32, vp, vp, i64, vp), "mutations_export"),
    ("iss_tally_words", i64, (vp,), "tally"),
    ("iss_output_tally", int_, (vp, i64, i64, vp), "tally"),
    ("iss_depth_mark", int_, (vp, i64, i64, vp, i32, vp), "depth"),
    ("iss_depth_finish", int_, (vp, vp, i64, vp, vp, i32, i32, vp, vp), "depth"),
    ("iss_error_tally_words", i64, (vp,), "errtally"),
    ("iss_mutations_tally", int_, (vp, i32, i64, i64, vp), "errtally"),
    ("iss_ctx_set_stream_ordered", int_, (vp, vp), "export"),
    ("iss_timing_enable", int_, (vp, int_), None),
    ("iss_timing_read", int_, (vp, P(f64 * 4), P(i64)), None),
    ("iss_stats_read", int_, (vp, P(i64), P(i64)), None),
    ("iss_main_kernel", int_, (vp, vp, int_), None),
    ("iss_mt_seed", int_, (vp, u64), None),
    ("iss_generate_mt", int_, (vp, i32, i64, i32, i32, i64, P(i64)), None),
    ("iss_mt_peek", int_, (vp, vp, vp, i32), None),
    ("iss_mt_path_counts", int_, (vp, P(i64), P(i64)), None),
    ("iss_mt_resolver_pick", int_, (vp, P(i32 * 3)), "mt_resolver"),
    ("iss_mt_workers_seed", int_, (vp, i32, vp), None),
    ("iss_generate_mt_workers", int_, (vp, i32, vp, vp, vp, i32, i32, vp, vp), None),
    ("iss_mt_workers_peek", int_, (vp, i32, vp, vp, i32), None),
    ("iss_mt_set_fragment", int_, (vp, i32, f64, f64), None),
    ("iss_mt_mutations_reserve", int_, (vp, i64), None),
    ("iss_mt_mutations_download", int_, (vp, vp, i64, P(i64)), None),
    ("iss_mt_workers_mutations_reserve", int_, (vp, i64), "set_rows"),
    ("iss_mt_workers_mutations_download", int_, (vp, i32, vp, i64, P(i64)), "set_rows"),
    ("iss_fastq_emit", int_, (vp, int_, int_, str_, i64, i32, i64, i64, i32), None),
    ("iss_fastq_emit_batch", int_, (vp, int_, int_, i32, vp, vp, vp, vp, i32), None),
    ("iss_fastq_emit_scatter", int_, (vp, int_, int_, i32, vp, vp, vp, vp, vp, vp, i32), None),
    ("iss_fastq_flush", int_, (vp,), None),
    ("iss_vcf_emit", int_, (vp, int_, i32, i32, vp, vp, vp, vp, i32, P(i64)), "vcf"),
    ("iss_vcf_emit_workers", int_, (vp, i32, vp, vp, vp, vp, vp, vp), "set_rows"),
    ("iss_vcf_flush", int_, (vp,), "vcf"),
    ("iss_fastq_compress", int_, (vp, i32), None),
    ("iss_deflate_code_build", int_, (vp, u32, vp, vp, vp, vp), None),
    ("iss_fastq_write", int_, (int_, int_, str_, i64, i32, i64, i32, i32, vp, vp, vp, vp, i32), None),
    ("iss_ubam_emit_batch", int_, (vp, int_, i32, vp, vp, vp, vp, i32), "ubam"),
    ("iss_ubam_flush", int_, (vp,), "ubam"),
    ("iss_ubam_host_records", int_, (int_, str_, i64, i32, i64, i32, i32, vp, vp, vp, vp), "ubam"),
    ("iss_origins_emit_batch", int_, (vp, int_, i32, vp, vp, vp, vp, vp, i32), "origins"),
    ("iss_origins_flush", int_, (vp,), "origins"),
    ("iss_origins_host_text", int_, (int_, str_, i64, i32, i64, i32, i64, vp), "origins"),
    ("iss_origins_compress", int_, (vp, i32), "bgzip"),
    ("iss_vcf_compress", int_, (vp, i32), "bgzip"),
    ("iss_bgzf_text_code_build", int_, (vp, vp, vp, vp, vp), "bgzip"),
    ("iss_bam_scan", int_, (vp, i64, vp, i64, P(i64), P(i64)), None),
    ("iss_bam_create", int_, (int_, P(vp)), None),
    ("iss_bam_destroy", None, (vp,), None),
    ("iss_bam_last_error", str_, (vp,), None),
    ("iss_bam_reset", int_, (vp,), None),
    ("iss_bam_feed", int_, (vp, vp, i64, vp, vp, i64), None),
    ("iss_bam_tally_download", int_, (vp, vp, P(i64), P(i32)), None),
    ("iss_bam_kde", int_, (vp, i32, i32, vp, vp), None),
    ("iss_fq_create", int_, (int_, i32, P(vp)), "fq"),
    ("iss_fq_destroy", None, (vp,), "fq"),
    ("iss_fq_last_error", str_, (vp,), "fq"),
    ("iss_fq_reset", int_, (vp,), "fq"),
    ("iss_fq_tally_words", i64, (vp,), "fq"),
    ("iss_fq_feed", int_, (vp, i32, vp, i64), "fq"),
    ("iss_fq_download", int_, (vp, vp, vp, vp, vp), "fq"),
    ("iss_fq_kernel_ms", int_, (vp, P(f64)), "fq"),
    ("iss_bgzf_scan", int_, (vp, i64, vp, vp, vp, vp, vp, i64, P(i64), P(i64)), "inflate"),
    ("iss_inflate_create", int_, (int_, P(vp)), "inflate"),
    ("iss_inflate_destroy", None, (vp,), "inflate"),
    ("iss_inflate_last_error", str_, (vp,), "inflate"),
    ("iss_inflate_reset", int_, (vp,), "inflate"),
    ("iss_inflate_feed", int_, (vp, vp, i64, vp, vp, vp, vp, i64), "inflate"),
    ("iss_inflate_collect", int_, (vp, P(vp), P(i64), P(vp), P(i64)), "inflate"),
    ("iss_inflate_first_bad", int_, (vp, P(i64), P(i32)), "inflate"),
    ("iss_inflate_kernel_ms", int_, (vp, P(f64)), "inflate"),
    ("iss_br_create", int_, (int_, i32, P(vp)), "br"),
    ("iss_br_destroy", None, (vp,), "br"),
    ("iss_br_last_error", str_, (vp,), "br"),
    ("iss_br_reset", int_, (vp,), "br"),
    ("iss_br_tally_words", i64, (vp,), "br"),
    ("iss_br_feed", int_, (vp, vp, i64, vp, i64), "br"),
    ("iss_br_download", int_, (vp, vp, vp, vp, P(i64), P(i32)), "br"),
    ("iss_br_kernel_ms", int_, (vp, P(f64)), "br"),
    ("iss_br_errors_enable", int_, (vp,), "br_errors"),
    ("iss_br_error_words", i64, (vp,), "br_errors"),
    ("iss_br_errors_download", int_, (vp, vp, vp, P(i64), P(i32)), "br_errors"),
    ("iss_br_depth_enable", int_, (vp, vp, i32, vp, u32, i32), "br_depth"),
    ("iss_br_depth_download", int_, (vp, vp, P(i64), P(i32)), "br_depth"),
    ("iss_genome_upload_variants", int_, (vp, vp, i64, i64, vp, vp, vp, vp, vp, i64, vp, vp, i64, vp, P(i32)), "variants"),
    ("iss_genome_download", int_, (vp, i32, vp, i64, P(i64)), "variants"),
    ("iss_variants_lift", int_, (vp, vp, i32, vp, i64, vp), "variants"),
    ("iss_variants_apply_tile", int_, (), "variants"),
    ("iss_variants_host_apply", int_, (vp, i64, i64, vp, vp, vp, vp, vp, i64, vp, vp, i64), "variants"),
    ("iss_variants_host_lift", int_, (i64, vp, vp, vp, vp, vp, i64, vp), "variants"),
    ("iss_fa_create", int_, (int_, P(vp)), "fasta"),
    ("iss_fa_destroy", None, (vp,), "fasta"),
    ("iss_fa_last_error", str_, (vp,), "fasta"),
    ("iss_fa_index", int_, (vp, vp, i64, i64, vp, vp, vp, vp, vp, vp, P(i64)), "fasta"),
    ("iss_fasta_host_index", int_, (vp, i64, i64, vp, vp, vp, vp, vp, vp, P(i64)), "fasta"),
    ("iss_fasta_tile", int_, (), "fasta"),
    ("iss_fasta_scan_span", int_, (), "fasta"),
    ("iss_genome_upload_fasta", int_, (vp, vp, i64, i32, vp, vp, vp, vp), "fasta"),
)
EXPORTS = tuple(row[0] for row in TABLE)  # every symbol include/iss_mi355x.h declares (tests check the library exports all of them)
GROUPS = {g: tuple(row[0] for row in TABLE if row[3] == g) for g in dict.fromkeys(row[3] for row in TABLE if row[3])}  # label -> entries
GROUP_HINTS = {"vcf": ", or set ISS_HOST_VCF=1 for the rows-to-host route"}  # what need() adds to its message

# The stand-alone device contexts with a reset (class Session below), by entry prefix: each has create, destroy, last_error and reset
# in TABLE, kernel_ms and tally_words where TABLE has them.
SESSIONS = ("iss_bam", "iss_fq", "iss_inflate", "iss_br")

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
    for name, restype, argtypes, group in TABLE:
        if not hasattr(L, name):
            if group is None:
                raise NativeLibraryError("%s does not export %s: rebuild it" % (LIB_PATH, name))
            continue  # (a build from before the group: it still loads, and need() names what it lacks when that is asked for)
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, list(argtypes)
    _lib = L
    return L


def need(L, group):
    """Raise NativeLibraryError when the library ``L`` lacks an entry of ``group`` (there is no fall-back for a missing entry)."""
    missing = [name for name in GROUPS[group] if not hasattr(L, name)]
    if missing:
        raise NativeLibraryError("%s does not export %s: rebuild it%s" % (LIB_PATH, " / ".join(missing), GROUP_HINTS.get(group, "")))


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
