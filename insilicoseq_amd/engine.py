"""ReadEngine: one MI355X context = one reference worker (host-side driver over the C ABI).

Uploads the model tables and genomes once to HBM, launches the read-generation kernels for
(record, n_pairs) work items and brings the R1/R2 base + phred buffers back (or leaves them in
HBM for a device-side consumer).  Everything numeric happens in the HIP library; this file is
plumbing.  Reference counterparts: the body of ``worker_iterator`` / ``simulate_reads`` /
``reads_generator`` (iss/generator.py:223-251, 21-66, 69-95)."""
import ctypes as C

import numpy as np

from . import _native
from ._native import EngineError, SEQ_TYPES, check


MUT_DTYPE = np.dtype([("pair", "<i4"), ("mate", "i1"), ("type", "i1"), ("position", "<i2"), ("ref", "u1"),
                      ("alt", "u1"), ("quality", "<i2")], align=True)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _item_arrays(items, cols, id_col=0, bytes_ids=False):
    """What the emit entries take of a work list: [ids as (c_char_p * n) from column ``id_col``, an int64 array per column of ``cols``].
    The caller holds the list across the call.  ``bytes_ids``: an id may be bytes as well as str."""
    ids = [it[id_col] if bytes_ids and isinstance(it[id_col], bytes) else str(it[id_col]).encode() for it in items]
    return [(C.c_char_p * len(items))(*ids)] + [np.array([it[k] for it in items], dtype=np.int64) for k in cols]


class ReadEngine(object):
    def __init__(self, device=0):
        self._lib = _native.lib()
        self._ctx = C.c_void_p()
        check(None, self._lib.iss_ctx_create(int(device), C.byref(self._ctx)))
        self.device = int(device)
        self.read_length = None
        self.pitch = None
        self._capacity = 0
        self._genome_lengths = []
        self.stream_ptr = 0  # the hipStream_t set_stream() was given last (0: the context's own stream)

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx:
            self._lib.iss_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

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
        return check(self._ctx, rc)

    def _need(self, group):
        """No fall-back: a library from before the entries of ``group`` (_native.TABLE) cannot take this route."""
        _native.need(self._lib, group)

    # ------------------------------------------------------------------ uploads
    def load_model(self, dense):
        """Upload a DenseModel (insilicoseq_amd.model) -- replaces pickling the ErrorModel to the worker."""
        t = dense.device_tables()
        keep = {
            "isize_thr": _u64(t["isize_thr"]), "bin_thr": _u64(t["bin_thr"]), "q_thr": _u64(t["q_thr"]),
            "subst_thr": _u64(t["subst_thr"]), "ins_thr": _u64(t["ins_thr"]), "del_thr": _u64(t["del_thr"]),
            "mut_thr": _u64(t["mut_thr"]),
            "bin_nonempty": np.ascontiguousarray(dense.bin_nonempty, dtype=np.uint8),
            "subst_alt": np.ascontiguousarray(dense.subst_alt, dtype=np.uint8),
            "ins_letter": np.ascontiguousarray(dense.ins_letter, dtype=np.uint8),
        }
        mt = _native.ModelTables()
        mt.read_length = dense.read_length
        mt.n_isize = dense.n_isize
        mt.n_q = dense.n_q
        for k, v in keep.items():
            setattr(mt, k, v.ctypes.data)
        mt.quality_mode = int(getattr(dense, "quality_mode", 0))
        mt.basic_insert_size = int(getattr(dense, "basic_insert_size", 200))
        # np.random.normal(util.phred_to_prob(mean_quality), 0.01, read_length); min(q, 0.9999)  (basic.py:52)
        from .model import phred_to_prob
        mt.basic_mean = float(phred_to_prob(int(getattr(dense, "basic_mean_quality", 30))))
        mt.basic_sd = 0.01
        mt.basic_cap = 0.9999
        self._check(self._lib.iss_model_upload(self._ctx, C.byref(mt)))
        self.quality_mode = mt.quality_mode
        self.read_length = dense.read_length
        self.pitch = self._lib.iss_output_pitch(self._ctx)
        self._capacity = 0
        return self

    def add_genome(self, seq):
        """Upload one record's sequence (str / bytes / uint8 array); returns its genome id."""
        if isinstance(seq, str):
            seq = seq.encode("ascii")
        a = np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.ascontiguousarray(
            seq, dtype=np.uint8)
        gid = C.c_int32(-1)
        self._check(self._lib.iss_genome_upload(self._ctx, a.ctypes.data, a.size, C.byref(gid)))
        self._genome_lengths.append(int(a.size))
        return gid.value

    def add_genomes(self, seqs):
        """Upload several records in one group (iss_genome_upload_group: one copy, one pack kernel, one status read-back);
        returns their genome ids, -1 for a record the group does not take (no letters, letters outside the rev_comp
        alphabet): add_genome(seq) of that record raises the error."""
        arrs = []
        for seq in seqs:
            if isinstance(seq, str):
                seq = seq.encode("ascii")
            arrs.append(np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else
                        np.ascontiguousarray(seq, dtype=np.uint8))
        n = len(arrs)
        if not n:
            return []
        ptrs = np.array([a.ctypes.data if a.size else 0 for a in arrs], dtype=np.uint64)
        lengths = np.array([a.size for a in arrs], dtype=np.int64)
        ids = np.full(n, -1, dtype=np.int32)
        self._check(self._lib.iss_genome_upload_group(self._ctx, n, ptrs.ctypes.data, lengths.ctypes.data, ids.ctypes.data))
        # (ids are dense: the lengths of the records the group took, in order)
        for gid, a in zip(ids.tolist(), arrs):
            if gid >= 0:
                assert gid == len(self._genome_lengths)
                self._genome_lengths.append(int(a.size))
        return ids.tolist()

    def add_genomes_fasta(self, seqs):
        """Upload records as they stand in their FASTA file (``seqs``: fasta.FastaSeq): the bytes go to the device with their line
        ends, which are removed there (iss_genome_upload_fasta).  A call of the library takes a run of records of one file in file
        order (fasta.upload_runs) and sends the span from the first body to the last; its records of at most 2^20 letters become
        one group like add_genomes', a larger record is a call of its own.  Returns the genome ids, -1 like add_genomes."""
        from .fasta import upload_runs

        self._need("fasta")
        ids = []
        for first, last in [cut for run in upload_runs(seqs) for cut in self._cut_at_large(seqs, *run)]:
            run = seqs[first:last]
            base, end = run[0].body_off, run[-1].body_off + run[-1].body_len
            ids.extend(self.add_genomes_fasta_table(run[0].source.array[base:end], [s.body_off - base for s in run],
                                                    [s.body_len for s in run], [s.letters for s in run]))
        return ids

    @staticmethod
    def _cut_at_large(seqs, first, last):
        """[first, last) cut so that a record of more than 2^20 letters stands alone."""
        cuts, at = [], first
        for k in range(first, last):
            if seqs[k].letters > (1 << 20):
                if k > at:
                    cuts.append((at, k))
                cuts.append((k, k + 1))
                at = k + 1
        if last > at:
            cuts.append((at, last))
        return cuts

    def add_genomes_fasta_table(self, span, body_off, body_len, letters):
        """iss_genome_upload_fasta as it is: ``span`` (bytes or a uint8 array) and the table of its records, offsets relative to it."""
        a = span if isinstance(span, np.ndarray) else np.frombuffer(span, dtype=np.uint8)
        body_off, body_len, letters = (np.ascontiguousarray(x, dtype=np.int64) for x in (body_off, body_len, letters))
        n = body_off.size
        if not (body_len.size == letters.size == n):
            raise ValueError("the table's arrays differ in length")
        ids = np.full(n, -1, dtype=np.int32)
        self._check(self._lib.iss_genome_upload_fasta(self._ctx, a.ctypes.data if a.size else None, a.size, n, body_off.ctypes.data,
                                                      body_len.ctypes.data, letters.ctypes.data, ids.ctypes.data))
        for gid, length in zip(ids.tolist(), letters.tolist()):
            if gid >= 0:
                assert gid == len(self._genome_lengths)
                self._genome_lengths.append(int(length))
        return ids.tolist()

    def add_genome_packed(self, codes, length, device_ptr=None):
        """Upload a record of plain A/C/G/T given as 2-bit codes (see distributed.pack_2bit): ``codes`` a uint32 array
        on the host, or ``device_ptr`` the address of the words in this GPU's memory (a slice of the broadcast buffer)."""
        gid = C.c_int32(-1)
        if device_ptr is not None:
            self._check(self._lib.iss_genome_upload_packed(self._ctx, C.c_void_p(int(device_ptr)), int(length), 1, C.byref(gid)))
        else:
            a = np.ascontiguousarray(codes, dtype=np.uint32)
            assert a.size >= (int(length) + 15) // 16
            self._check(self._lib.iss_genome_upload_packed(self._ctx, a.ctypes.data, int(length), 0, C.byref(gid)))
        self._genome_lengths.append(int(length))
        return gid.value

    def add_genome_variants(self, seq, table, record_id=None):
        """Upload one record with the variants of ``table`` (variants.VariantTable) spliced in on the device: the genome is the
        haplotype, built in HBM from the record's letters and packed like any record (iss_genome_upload_variants).  Every variant's
        REF letters must be the record's (case ignored): a mismatch raises EngineError, one line with ``record_id``, the POS and both
        spellings.  Returns the genome id; genome_length() is the haplotype's length."""
        self._need("variants")
        if isinstance(seq, str):
            seq = seq.encode("ascii")
        a = np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.ascontiguousarray(seq, dtype=np.uint8)
        if a.size != table.record_length:
            raise EngineError(_native.E_INVALID, "add_genome_variants: the table is of a record of %d letters, not %d" % (
                table.record_length, a.size))
        gid = C.c_int32(-1)
        t = table
        try:
            self._check(self._lib.iss_genome_upload_variants(
                self._ctx, a.ctypes.data, a.size, len(t), t.pos0.ctypes.data, t.ref_len.ctypes.data, t.alt_len.ctypes.data,
                t.alt_off.ctypes.data, t.alt.ctypes.data, t.alt.size, t.ref_off.ctypes.data, t.ref.ctypes.data, t.ref.size,
                t.out_pos.ctypes.data, C.byref(gid)))
        except EngineError as e:
            if record_id is None:
                raise
            raise EngineError(e.code, "record %s: %s" % (record_id, e.message)) from None
        self._genome_lengths.append(int(t.out_pos[-1]))
        return gid.value

    def genome_letters(self, gid):
        """The resident ASCII copy of genome ``gid`` as a uint8 array (iss_genome_download; waits for the stream)."""
        self._need("variants")
        n = C.c_int64(0)
        self._check(self._lib.iss_genome_download(self._ctx, int(gid), None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.uint8)
        self._check(self._lib.iss_genome_download(self._ctx, int(gid), out.ctypes.data, out.size, C.byref(n)))
        return out

    def lift_ptr(self, in_ptr, n, out_ptr, gid=0, gids_ptr=None):
        """Haplotype coordinates -> record coordinates on the device: ``n`` int64 at the raw device address ``in_ptr`` to
        ``out_ptr`` (it may be ``in_ptr``), of genome ``gid``, or of the genome ids (int32 [n]) at ``gids_ptr``.  A genome
        uploaded without variants is the identity.  Asynchronous on the engine's current stream (iss_variants_lift)."""
        self._need("variants")
        self._check(self._lib.iss_variants_lift(self._ctx, C.c_void_p(int(gids_ptr)) if gids_ptr else None, int(gid),
                                                C.c_void_p(int(in_ptr)) if in_ptr else None, int(n),
                                                C.c_void_p(int(out_ptr)) if out_ptr else None))

    def lift(self, coords, gid=0, gids=None):
        """``coords`` (any shape) lifted on the device: a torch tensor on this GPU comes back as one (nothing waits on the host
        beyond torch's own stream hand-over); anything else goes through the device and comes back as a numpy int64 array.
        ``gids``: a genome id per element instead of ``gid``."""
        from .tensors import _torch

        torch = _torch()
        dev = torch.device("cuda", self.device)
        on_device = isinstance(coords, torch.Tensor) and coords.is_cuda
        with torch.cuda.device(self.device):
            x = (coords if on_device else torch.from_numpy(np.ascontiguousarray(coords, dtype=np.int64)).to(dev)).to(torch.int64).contiguous()
            g = None
            if gids is not None:
                g = (gids if isinstance(gids, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(gids, dtype=np.int32))).to(dev).to(torch.int32).contiguous()
                if g.numel() != x.numel():
                    raise ValueError("lift: one genome id per coordinate")
            out = torch.empty_like(x)
            torch.cuda.current_stream().synchronize()  # (made on torch's stream; the engine reads them on its own)
            self.lift_ptr(x.data_ptr(), x.numel(), out.data_ptr(), gid=gid, gids_ptr=g.data_ptr() if g is not None else None)
            self.synchronize()
        return out if on_device else out.cpu().numpy()

    def clear_genomes(self):
        self._check(self._lib.iss_genome_clear(self._ctx))
        self._genome_lengths = []

    def genome_length(self, gid):
        return self._genome_lengths[gid]

    def reserve(self, n_pairs):
        if n_pairs > self._capacity:
            self._check(self._lib.iss_output_reserve(self._ctx, int(n_pairs)))
            self._capacity = int(n_pairs)

    # ------------------------------------------------------------------ the hot path
    def generate(self, genome_id, n_pairs, first_ordinal=0, seed=0, sequence_type="metagenomics", gc_bias=False,
                 out_first_pair=0):
        """Asynchronously generate n_pairs pairs into rows [out_first_pair, +n_pairs).  Raises
        EngineError(code=E_SHORT_RECORD) when read_length >= len(record) (the reference's
        AssertionError, iss/generator.py:130)."""
        if sequence_type not in SEQ_TYPES:
            raise ValueError("Sequence type %s not known" % sequence_type)  # generator.py:171
        self.reserve(out_first_pair + n_pairs)
        self._check(self._lib.iss_generate(self._ctx, int(genome_id), int(n_pairs), int(first_ordinal) & (2**64 - 1),
                                           int(seed) & (2**64 - 1), SEQ_TYPES[sequence_type], int(bool(gc_bias)),
                                           int(out_first_pair)))

    def generate_batch(self, genome_ids, n_pairs, first_ordinal=0, seed=0, sequence_type="metagenomics", gc_bias=False,
                       out_first_pair=0):
        """A whole work list -- items (genome_ids[k], n_pairs[k]) -- in one set of launches; the rows equal those of
        consecutive generate() calls with running ordinals and rows.  No custom fragment lengths here."""
        if sequence_type not in SEQ_TYPES:
            raise ValueError("Sequence type %s not known" % sequence_type)
        ids = np.ascontiguousarray(genome_ids, dtype=np.int32)
        cnt = np.ascontiguousarray(n_pairs, dtype=np.int64)
        assert ids.ndim == 1 and ids.shape == cnt.shape
        self.reserve(out_first_pair + int(cnt.sum()))
        self._check(self._lib.iss_generate_batch(self._ctx, int(ids.size), ids.ctypes.data, cnt.ctypes.data,
                                                 int(first_ordinal) & (2**64 - 1), int(seed) & (2**64 - 1),
                                                 SEQ_TYPES[sequence_type], int(bool(gc_bias)), int(out_first_pair)))

    # ------------------------------------------------------------------ the ErrorModel methods, batched (inner plugin surface)
    def gen_phred_scores(self, orientation, n, first_ordinal=0, seed=0):
        """KDErrorModel.gen_phred_scores for n reads (iss/error_models/kde.py:52-86): uint8 [n, read_length]; read i draws
        at ordinal first_ordinal + i of the worker stream `seed` -- the phreds iss_generate gives that pair's mate."""
        out = np.empty((int(n), self.read_length), dtype=np.uint8)
        self._check(self._lib.iss_gen_phred_scores(self._ctx, int(orientation), int(n), int(first_ordinal) & (2**64 - 1),
                                                   int(seed) & (2**64 - 1), out.ctypes.data))
        return out

    def mut_sequence(self, orientation, seqs, quals, first_ordinal=0, seed=0):
        """ErrorModel.mut_sequence (iss/error_models/__init__.py:69-112) for uint8 [n, read_length] letters and phreds:
        (mutated letters, status per read -- 2: the reference's KeyError)."""
        s = np.array(seqs, dtype=np.uint8, order="C", copy=True).reshape(-1, self.read_length)
        q = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1, self.read_length)
        assert s.shape == q.shape
        st = np.zeros(s.shape[0], dtype=np.int32)
        self._check(self._lib.iss_mut_sequence(self._ctx, int(orientation), s.shape[0], int(first_ordinal) & (2**64 - 1),
                                               int(seed) & (2**64 - 1), s.ctypes.data, q.ctypes.data, st.ctypes.data))
        return s, st

    def random_insert_size(self, n, first_ordinal=0, seed=0):
        """KDErrorModel.random_insert_size (iss/error_models/kde.py:88-98) for n pairs: int64 [n]."""
        out = np.empty(int(n), dtype=np.int64)
        self._check(self._lib.iss_random_insert_size(self._ctx, int(n), int(first_ordinal) & (2**64 - 1), int(seed) & (2**64 - 1),
                                                     out.ctypes.data))
        return out

    def introduce_indels(self, orientation, seqs, lengths, full_seq, bounds, first_ordinal=0, seed=0):
        """ErrorModel.introduce_indels incl. adjust_seq_length (iss/error_models/__init__.py:158-228, 114-156): seqs uint8
        [n, read_length] holding lengths[i] letters each (read direction), bounds int64 [n, 2] = (read_start, read_end) in
        full_seq.  Returns (uint8 [n, read_length], status per read: 0, 2 KeyError, 3 IndexError)."""
        s = np.ascontiguousarray(seqs, dtype=np.uint8).reshape(-1, self.read_length)
        ln = np.ascontiguousarray(lengths, dtype=np.int32)
        b = np.ascontiguousarray(bounds, dtype=np.int64).reshape(-1, 2)
        g = np.frombuffer(full_seq.encode("ascii") if isinstance(full_seq, str) else bytes(full_seq), dtype=np.uint8)
        assert s.shape[0] == ln.size == b.shape[0]
        out = np.zeros_like(s)
        st = np.zeros(s.shape[0], dtype=np.int32)
        self._check(self._lib.iss_introduce_indels(self._ctx, int(orientation), s.shape[0], int(first_ordinal) & (2**64 - 1),
                                                   int(seed) & (2**64 - 1), s.ctypes.data, ln.ctypes.data, g.ctypes.data, g.size,
                                                   b.ctypes.data, out.ctypes.data, st.ctypes.data))
        return out, st

    def ev_step(self, orientation, cur, m53, v53=None):
        """One draw of the indel event process (the sampler behind the tests of introduce_indels,
        iss/error_models/__init__.py:193-196, :209) for arrays of (state, uniform numerator[, numerator of the deletion
        sub-draw]): (next state, slot that fires or -1, event mask).  A test hook (include/iss_mi355x.h: iss_ev_step)."""
        cur = np.ascontiguousarray(cur, dtype=np.int32)
        m53 = np.ascontiguousarray(m53, dtype=np.uint64)
        v53 = np.zeros_like(m53) if v53 is None else np.ascontiguousarray(v53, dtype=np.uint64)
        assert cur.shape == m53.shape == v53.shape
        nxt, slot, mask = np.zeros_like(cur), np.zeros_like(cur), np.zeros(cur.shape, dtype=np.uint8)
        self._check(self._lib.iss_ev_step(self._ctx, int(orientation), cur.size, cur.ctypes.data, m53.ctypes.data, v53.ctypes.data,
                                          nxt.ctypes.data, slot.ctypes.data, mask.ctypes.data))
        return nxt, slot, mask

    def set_fragment(self, fragment_length=None, fragment_sd=None):
        """Custom fragment length for generate() (None, None: the model's insert sizes)."""
        on = fragment_length is not None and fragment_sd is not None
        self._check(self._lib.iss_set_fragment(self._ctx, int(on), float(fragment_length or 0.0), float(fragment_sd or 0.0)))

    def mutations_reserve(self, capacity):
        """Enable (capacity > 0) / disable --store_mutations row capture of generate() (Philox path)."""
        self._check(self._lib.iss_mutations_reserve(self._ctx, int(capacity)))
        self._pmut_cap = int(capacity)

    def mutations(self):
        """Rows of the last generate() call, in the reference's order (structured array, see iss_mutation)."""
        cap = getattr(self, "_pmut_cap", 0)
        buf = getattr(self, "_pmut_buf", None)
        if buf is None or buf.size < cap:  # (one landing buffer per engine: tens of MB, not per call)
            buf = self._pmut_buf = np.empty(cap, dtype=MUT_DTYPE)
        n = C.c_int64(0)
        rc = self._lib.iss_mutations_download(self._ctx, buf.ctypes.data, cap, C.byref(n))
        self.mutation_slots_needed = n.value if rc == _native.E_NOMEM else 0  # (what a retry has to reserve)
        self._check(rc)
        return buf[: n.value].copy()

    @property
    def mutations_capacity(self):
        """Row slots reserved by mutations_reserve()."""
        return int(getattr(self, "_pmut_cap", 0))

    # ------------------------------------------------------------------ reference-compatible MT mode
    def seed_mt(self, seed):
        """random.seed(seed); np.random.seed(seed) -- on the device (iss/generator.py:234-236)."""
        self._check(self._lib.iss_mt_seed(self._ctx, int(seed)))

    def generate_mt(self, genome_id, n_pairs, sequence_type="metagenomics", gc_bias=False, out_first_pair=0):
        """Sequential, reference-identical generation; returns the number of pairs emitted."""
        if sequence_type not in SEQ_TYPES:
            raise ValueError("Sequence type %s not known" % sequence_type)
        self.reserve(out_first_pair + n_pairs)
        done = C.c_int64(0)
        self._check(self._lib.iss_generate_mt(self._ctx, int(genome_id), int(n_pairs), SEQ_TYPES[sequence_type],
                                              int(bool(gc_bias)), int(out_first_pair), C.byref(done)))
        return done.value

    def seed_mt_workers(self, seeds):
        """W reference workers side by side in this context: worker w == seed_mt(seeds[w]) in a context of its own
        (its two MT19937 streams; iss/generator.py:234-236 with seed + cpu_number)."""
        a = np.ascontiguousarray(seeds, dtype=np.uint64)
        self._check(self._lib.iss_mt_workers_seed(self._ctx, int(a.size), a.ctypes.data))
        self._mt_workers = int(a.size)

    def generate_mt_workers(self, genome_ids, n_pairs, out_first_pair, sequence_type="metagenomics", gc_bias=False):
        """One work item (or piece of one) per worker, every kernel of the path launched once for all workers: worker w
        generates n_pairs[w] pairs of genome genome_ids[w] into rows [out_first_pair[w], +n_pairs[w]) from ITS streams --
        the rows and stream positions of generate_mt per worker.  Returns (pairs emitted per worker, status per worker:
        0 or E_SHORT_RECORD)."""
        if sequence_type not in SEQ_TYPES:
            raise ValueError("Sequence type %s not known" % sequence_type)
        g = np.ascontiguousarray(genome_ids, dtype=np.int32)
        n = np.ascontiguousarray(n_pairs, dtype=np.int64)
        r = np.ascontiguousarray(out_first_pair, dtype=np.int64)
        if not (g.size == n.size == r.size == getattr(self, "_mt_workers", -1)):
            raise ValueError("generate_mt_workers: one genome id, pair count and first row per seeded worker")
        self.reserve(int((r + n).max()) if n.size else 0)
        done = np.zeros(n.size, dtype=np.int64)
        status = np.zeros(n.size, dtype=np.int32)
        self._check(self._lib.iss_generate_mt_workers(self._ctx, int(n.size), g.ctypes.data, n.ctypes.data, r.ctypes.data,
                                                      SEQ_TYPES[sequence_type], int(bool(gc_bias)), done.ctypes.data,
                                                      status.ctypes.data))
        return done, status

    def mt_workers_peek(self, worker, n=8):
        """mt_peek for worker ``worker`` of the set."""
        a = np.zeros(n, dtype=np.uint32)
        b = np.zeros(n, dtype=np.uint32)
        self._check(self._lib.iss_mt_workers_peek(self._ctx, int(worker), a.ctypes.data, b.ctypes.data, int(n)))
        return a, b

    def mt_set_fragment(self, fragment_length=None, fragment_sd=None):
        """Custom fragment length for generate_mt (None, None switches back to the model's insert sizes)."""
        on = fragment_length is not None and fragment_sd is not None
        self._check(self._lib.iss_mt_set_fragment(self._ctx, int(on), float(fragment_length or 0.0),
                                                  float(fragment_sd or 0.0)))

    def mt_mutations_reserve(self, capacity):
        """Enable (capacity > 0) / disable --store_mutations row capture of generate_mt."""
        self._check(self._lib.iss_mt_mutations_reserve(self._ctx, int(capacity)))
        self._mut_cap = int(capacity)

    def mt_mutations(self):
        """Rows of the last generate_mt call as a structured array (see iss_mutation in the C header)."""
        cap = getattr(self, "_mut_cap", 0)
        out = np.zeros(cap, dtype=MUT_DTYPE)
        n = C.c_int64(0)
        self._check(self._lib.iss_mt_mutations_download(self._ctx, out.ctypes.data, cap, C.byref(n)))
        if n.value > cap:
            raise EngineError(_native.E_INVALID, "mutation buffer too small: %d rows, capacity %d" % (n.value, cap))
        return out[: n.value]

    def mt_workers_mutations_reserve(self, rows_per_worker):
        """Enable (rows_per_worker > 0) / disable --store_mutations row capture of generate_mt_workers: every worker of the set
        owns a region of that many rows.  A worker that makes more rows fails the call with E_NOMEM (the set must be seeded
        again)."""
        self._need("set_rows")
        self._check(self._lib.iss_mt_workers_mutations_reserve(self._ctx, int(rows_per_worker)))
        self._set_mut_cap = int(rows_per_worker)

    def mt_workers_mutations(self, worker):
        """Rows of worker ``worker`` in the last generate_mt_workers call as a structured array (see mt_mutations)."""
        self._need("set_rows")
        cap = getattr(self, "_set_mut_cap", 0)
        out = np.zeros(cap, dtype=MUT_DTYPE)
        n = C.c_int64(0)
        self._check(self._lib.iss_mt_workers_mutations_download(self._ctx, int(worker), out.ctypes.data, cap, C.byref(n)))
        if n.value > cap:
            raise EngineError(_native.E_INVALID, "mutation buffer too small: %d rows, capacity %d" % (n.value, cap))
        return out[: n.value]

    def vcf_emit_workers(self, items):
        """The --store_mutations rows of the last generate_mt_workers call as VCF text built on the device in ONE job for all
        workers.  items: one entry per worker of the set, (fd, record id, first pair id, first output row, pairs, cpu number) --
        pairs 0: the worker sat the call out.  Worker k's text is appended to its fd (asynchronous; ``vcf_flush`` before the
        files are used)."""
        self._need("set_rows")
        fds, cpus = (np.array([it[k] for it in items], dtype=np.int32) for k in (0, 5))
        ids, first_i, first_pair, n_pairs = _item_arrays(items, (2, 3, 4), id_col=1)
        self._check(self._lib.iss_vcf_emit_workers(self._ctx, len(items), fds.ctypes.data, ids, first_i.ctypes.data, first_pair.ctypes.data,
                                                   n_pairs.ctypes.data, cpus.ctypes.data))

    def mt_peek(self, n=8):
        """The next n 32-bit words of (CPython random, numpy) -- not consumed."""
        a = np.zeros(n, dtype=np.uint32)
        b = np.zeros(n, dtype=np.uint32)
        self._check(self._lib.iss_mt_peek(self._ctx, a.ctypes.data, b.ctypes.data, int(n)))
        return a, b

    def fastq_emit(self, fd_r1, fd_r2, record_id, first_i, cpu_number, first_pair, n_pairs, n_threads=1):
        """Format rows [first_pair, +n_pairs) as FASTQ on the device and append them to the two file
        descriptors (asynchronous; ``fastq_flush`` before the files are used)."""
        self._check(self._lib.iss_fastq_emit(self._ctx, int(fd_r1), int(fd_r2), str(record_id).encode(), int(first_i),
                                             int(cpu_number), int(first_pair), int(n_pairs), int(n_threads)))

    def fastq_emit_batch(self, fd_r1, fd_r2, items, cpu_number):
        """items: (record id, first pair id, first output row, pairs) per work item -- one text job for all of them."""
        ids, first_i, first_pair, n_pairs = _item_arrays(items, (1, 2, 3))
        self._check(self._lib.iss_fastq_emit_batch(self._ctx, int(fd_r1), int(fd_r2), len(items), ids, first_i.ctypes.data,
                                                   first_pair.ctypes.data, n_pairs.ctypes.data, int(cpu_number)))

    def fastq_emit_scatter(self, fd_r1, fd_r2, items, n_threads=1):
        """items: (record id, first pair id, first output row, pairs, cpu number, byte offset in both files) -- one text job, every
        item's text written at its own place (the workers of a set straight into the final files; text mode only)."""
        if not items:
            return
        ids, first_i, first_pair, n_pairs, file_off = _item_arrays(items, (1, 2, 3, 5))
        cpus = np.array([it[4] for it in items], dtype=np.int32)
        self._check(self._lib.iss_fastq_emit_scatter(self._ctx, int(fd_r1), int(fd_r2), len(items), ids, first_i.ctypes.data,
                                                     first_pair.ctypes.data, n_pairs.ctypes.data, cpus.ctypes.data, file_off.ctypes.data,
                                                     int(n_threads)))

    def vcf_emit(self, fd, items, cpu_number, source="philox"):
        """The --store_mutations rows of the last generate() / generate_batch() call (``source="philox"``) or generate_mt() call
        (``"mt"``) as VCF text built on the device, appended to ``fd`` (asynchronous; ``vcf_flush`` before the file is used).
        items: the tuples of fastq_emit_batch -- (record id, first pair id, first output row, pairs), in ascending row order.  A
        Philox call that overflowed its row buffer raises E_NOMEM and leaves ``mutation_slots_needed`` like mutations()."""
        if source not in ("philox", "mt"):
            raise ValueError("source must be 'philox' or 'mt'")
        self._need("vcf")
        ids, first_i, first_pair, n_pairs = _item_arrays(items, (1, 2, 3))
        need = C.c_int64(0)
        rc = self._lib.iss_vcf_emit(self._ctx, int(fd), 0 if source == "philox" else 1, len(items), ids, first_i.ctypes.data,
                                    first_pair.ctypes.data, n_pairs.ctypes.data, int(cpu_number), C.byref(need))
        self.mutation_slots_needed = need.value if rc == _native.E_NOMEM else 0  # (what a retry has to reserve)
        self._check(rc)

    def vcf_flush(self):
        self._need("vcf")
        self._check(self._lib.iss_vcf_flush(self._ctx))

    def fastq_compress(self, on=True):
        """`--compress` on the device: every fastq_emit appends one gzip member per file instead of text."""
        self._check(self._lib.iss_fastq_compress(self._ctx, 1 if on else 0))

    def fastq_flush(self):
        self._check(self._lib.iss_fastq_flush(self._ctx))

    def ubam_emit_batch(self, fd, items, cpu_number):
        """The rows of the items of fastq_emit_batch -- (record id, first pair id, first output row, pairs) -- as unaligned BAM
        records (R1 then R2 of every pair: flags 77 / 141, names "{id}_{i}_{cpu}", lower-case bases as their capitals) in BGZF
        blocks built on the device, appended to ``fd`` (asynchronous; ``ubam_flush`` before the file is used).  Record blocks
        only: the BAM header and the EOF block are the caller's (ubam.py).  Ids may be str or bytes."""
        self._need("ubam")
        ids, first_i, first_pair, n_pairs = _item_arrays(items, (1, 2, 3), bytes_ids=True)
        self._check(self._lib.iss_ubam_emit_batch(self._ctx, int(fd), len(items), ids, first_i.ctypes.data, first_pair.ctypes.data,
                                                  n_pairs.ctypes.data, int(cpu_number)))

    def ubam_flush(self):
        self._need("ubam")
        self._check(self._lib.iss_ubam_flush(self._ctx))

    def origins_emit_batch(self, fd, items, record_lengths, cpu_number):
        """Where the pairs of the items of fastq_emit_batch -- (record id, first pair id, first output row, pairs), in ascending
        row order -- came from, as BEDPE text built on the device and appended to ``fd`` (asynchronous; ``origins_flush`` before
        the file is used): one line "{id} s1 e1 {id} s2 e2 {id}_{i}_{cpu} . + - isz" per pair, the two template intervals clamped
        against ``record_lengths[k]``, the length of item k's record (origins.py).  Ids may be str or bytes."""
        self._need("origins")
        n = len(items)
        if len(record_lengths) != n:
            raise ValueError("one record length per item")
        ids, first_i, first_pair, n_pairs = _item_arrays(items, (1, 2, 3), bytes_ids=True)
        lengths = np.array([int(x) for x in record_lengths], dtype=np.int64)
        self._check(self._lib.iss_origins_emit_batch(self._ctx, int(fd), n, ids, first_i.ctypes.data, first_pair.ctypes.data,
                                                     n_pairs.ctypes.data, lengths.ctypes.data, int(cpu_number)))

    def origins_flush(self):
        self._need("origins")
        self._check(self._lib.iss_origins_flush(self._ctx))

    def origins_compress(self, on=True):
        """Mode of ``origins_emit_batch``: False (default) appends the text, True the text's BGZF members built on the device
        (bgzf.py frames the file).  Switched only while nothing is queued (after ``origins_flush``)."""
        self._need("bgzip")
        self._check(self._lib.iss_origins_compress(self._ctx, 1 if on else 0))

    def vcf_compress(self, on=True):
        """The same for ``vcf_emit``; ``vcf_emit_workers`` raises in this mode."""
        self._need("bgzip")
        self._check(self._lib.iss_vcf_compress(self._ctx, 1 if on else 0))

    def mt_path_counts(self):
        """(pairs resolved in parallel, pairs walked sequentially) by generate_mt so far."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.iss_mt_path_counts(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def mt_resolver(self):
        """The resolver instantiation generate_mt / generate_mt_workers take for the loaded model and the current ISS_MT_PATH:
        (python ring half in K words, numpy ring half in K words, digit rows in LDS), or None when every pair is walked."""
        self._need("mt_resolver")
        out = (C.c_int32 * 3)()
        self._check(self._lib.iss_mt_resolver_pick(self._ctx, C.byref(out)))
        return (out[0], out[1], bool(out[2])) if out[0] else None

    def synchronize(self):
        self._check(self._lib.iss_synchronize(self._ctx))

    def download(self, first_pair, n_pairs):
        """Rows [first_pair, +n_pairs) as four uint8 arrays [n_pairs, read_length] (views on pitch-wide rows)."""
        outs = [np.empty((n_pairs, self.pitch), dtype=np.uint8) for _ in range(4)]
        self._check(self._lib.iss_output_download(self._ctx, int(first_pair), int(n_pairs),
                                                  *[o.ctypes.data for o in outs]))
        RL = self.read_length
        return {"r1_base": outs[0][:, :RL], "r1_qual": outs[1][:, :RL], "r2_base": outs[2][:, :RL],
                "r2_qual": outs[3][:, :RL], "_pitched": outs}

    def coords(self, first_pair, n_pairs):
        c = np.empty((n_pairs, 4), dtype=np.int64)
        self._check(self._lib.iss_output_download_coords(self._ctx, int(first_pair), int(n_pairs), c.ctypes.data))
        return c

    def device_ptrs(self):
        p = [C.c_void_p() for _ in range(4)]
        self._check(self._lib.iss_output_device_ptrs(self._ctx, *[C.byref(x) for x in p]))
        return [x.value for x in p]

    def set_stream(self, hip_stream_ptr, wait=True):
        """Launch on the caller's hipStream_t from now on (None / 0: the context's own stream again).  ``wait=False``: no wait on
        the host -- what the context has queued so far is ordered in front of the new stream's work by events."""
        if wait:
            self._check(self._lib.iss_ctx_set_stream(self._ctx, C.c_void_p(hip_stream_ptr or None)))
        else:
            self._need("export")
            self._check(self._lib.iss_ctx_set_stream_ordered(self._ctx, C.c_void_p(hip_stream_ptr or None)))
        self.stream_ptr = int(hip_stream_ptr or 0)

    def export(self, first_pair, n_pairs, bases_ptr=None, qual_ptr=None, coords_ptr=None, item_ptr=None, encoding="ascii"):
        """Rows [first_pair, +n_pairs) as dense arrays in device memory of the caller (raw device addresses, any array library's):
        bases / qual uint8 [n_pairs, 2, read_length], coords int64 [n_pairs, 4] (record coordinates), item int32 [n_pairs] (the
        pair's item of the last generate_batch(); 0 elsewhere); None: not wanted.  ``encoding``: "ascii" (the bytes of
        download()) or "codes" (A, C, G, T -> 0..3, anything else 4).  Asynchronous on the engine's current stream, behind the
        generation; nothing waits on the host (include/iss_mi355x.h: iss_output_export)."""
        if encoding not in _native.EXPORT_ENCODINGS:
            raise EngineError(_native.E_INVALID, "export: encoding must be 'ascii' or 'codes', not %r" % (encoding,))
        self._need("export")
        ptrs = [C.c_void_p(int(p)) if p else None for p in (bases_ptr, qual_ptr, coords_ptr, item_ptr)]
        self._check(self._lib.iss_output_export(self._ctx, int(first_pair), int(n_pairs), _native.EXPORT_ENCODINGS[encoding], *ptrs))

    def export_mutations(self, first_pair, n_pairs, truth_ptr=None, events_ptr=None, capacity=0, n_events_ptr=None, encoding="ascii"):
        """The mutation rows of the last generate() / generate_batch() (after mutations_reserve()) as dense arrays in device
        memory of the caller (raw device addresses), for output rows [first_pair, +n_pairs): truth uint8 [n_pairs, 2,
        read_length] -- the exported bases with every recorded substitution's ``ref`` letter put back, in ``encoding``; events
        int32 [capacity, 6] (pair - first_pair, mate, type, position, ref, alt) in the order of mutations(), with their number
        (int64, one word; -1: the call overflowed the reserved slots, truth is then the plain bases) at n_events_ptr; None: not
        wanted, events and n_events go together.  Asynchronous on the engine's current stream, behind the generation; nothing
        waits on the host (include/iss_mi355x.h: iss_mutations_export)."""
        if encoding not in _native.EXPORT_ENCODINGS:
            raise EngineError(_native.E_INVALID, "export_mutations: encoding must be 'ascii' or 'codes', not %r" % (encoding,))
        self._need("mutations_export")
        ptrs = [C.c_void_p(int(p)) if p else None for p in (truth_ptr, events_ptr, n_events_ptr)]
        self._check(self._lib.iss_mutations_export(self._ctx, int(first_pair), int(n_pairs), _native.EXPORT_ENCODINGS[encoding],
                                                   ptrs[0], ptrs[1], int(capacity), ptrs[2]))

    def tally_words(self):
        """uint64 words of a tally of this engine's model (include/iss_mi355x.h: iss_tally_words; tally.tally_layout)."""
        self._need("tally")
        n = self._lib.iss_tally_words(self._ctx)
        if n < 0:
            raise EngineError(_native.E_INVALID, "tally_words: upload a model first")
        return int(n)

    def tally(self, first_pair, n_pairs, tally_ptr):
        """Add the tallies of rows [first_pair, +n_pairs) -- per-position phreds and bases, GC and mean-quality histograms of the
        reads, insert sizes, pairs -- to the tally_words() uint64 words at ``tally_ptr`` (a raw device address; the caller's
        memory, zeroed by the caller).  Asynchronous on the engine's current stream, behind the generation; nothing waits on the
        host (include/iss_mi355x.h: iss_output_tally; tally.split_tally names the fields)."""
        self._need("tally")
        self._check(self._lib.iss_output_tally(self._ctx, int(first_pair), int(n_pairs), C.c_void_p(int(tally_ptr)) if tally_ptr else None))

    def error_tally_words(self):
        """uint64 words of an error tally of this engine's model (include/iss_mi355x.h: iss_error_tally_words; errtally.layout)."""
        self._need("errtally")
        n = self._lib.iss_error_tally_words(self._ctx)
        if n < 0:
            raise EngineError(_native.E_INVALID, "error_tally_words: upload a model first")
        return int(n)

    def error_tally(self, first_pair, n_pairs, tally_ptr, source="philox"):
        """Add the tallies of the mutation rows of the last generate() / generate_batch() call (``source="philox"``, after
        mutations_reserve()) or generate_mt() call (``"mt"``, after mt_mutations_reserve()) whose pair lies in output rows
        [first_pair, +n_pairs) -- substitutions by position, phred and letters, insertions, deletions, rows per read, pairs --
        to the error_tally_words() uint64 words at ``tally_ptr`` (a raw device address; the caller's memory, zeroed by the
        caller).  A Philox call that overflowed its reserved slots adds 1 to ``dropped`` and nothing else.  Asynchronous on
        the engine's current stream, behind the generation; nothing waits on the host (include/iss_mi355x.h:
        iss_mutations_tally; errtally.split names the fields)."""
        if source not in ("philox", "mt"):
            raise ValueError("source must be 'philox' or 'mt'")
        self._need("errtally")
        self._check(self._lib.iss_mutations_tally(self._ctx, 0 if source == "philox" else 1, int(first_pair), int(n_pairs),
                                                  C.c_void_p(int(tally_ptr)) if tally_ptr else None))

    def depth_mark(self, first_pair, n_pairs, table_ptr, n_table, diff_ptr):
        """Add the template intervals of rows [first_pair, +n_pairs) to the int32 difference array at ``diff_ptr``: +1 at the
        start, -1 at the end of each pair's forward and reverse interval, clamped to the record (depth.py has the definition).
        ``table_ptr``: int64 [n_table, 2] of (offset, length) on the device, row ``item`` the record of the pair's item in the
        last generate_batch() (row 0 for other rows); offset < 0: the pair is skipped.  Raw device addresses, the caller's memory.
        Asynchronous on the engine's current stream, behind the generation; nothing waits on the host.  The caller marks no more
        than 2^30 pairs into one accumulator (depth.count_marked) (include/iss_mi355x.h: iss_depth_mark)."""
        self._need("depth")
        self._check(self._lib.iss_depth_mark(self._ctx, int(first_pair), int(n_pairs), C.c_void_p(int(table_ptr)) if table_ptr else None,
                                             int(n_table), C.c_void_p(int(diff_ptr)) if diff_ptr else None))

    def depth_finish(self, diff_ptr, n_words, depth_ptr, table_ptr, n_table, bin=0, stats_ptr=None, bins_ptr=None):
        """The difference array of ``n_words`` int32 words at ``diff_ptr`` -> its inclusive prefix sum, the depth of every base
        (uint32 [n_words] at ``depth_ptr``; it may be ``diff_ptr`` itself), per-record statistics (uint64 [n_table, 4] at
        ``stats_ptr``: sum, sum of squares, covered bases, maximum) and, with ``bin`` > 0, the sums over ``bin``-base windows
        (uint64 [depth.n_windows(table, bin).sum()] at ``bins_ptr``); None: not wanted.  Works on an engine with no model.
        Asynchronous on the engine's current stream (include/iss_mi355x.h: iss_depth_finish; depth.finish_host is its twin)."""
        self._need("depth")
        ptrs = [C.c_void_p(int(p)) if p else None for p in (diff_ptr, depth_ptr, table_ptr, stats_ptr, bins_ptr)]
        self._check(self._lib.iss_depth_finish(self._ctx, ptrs[0], int(n_words), ptrs[1], ptrs[2], int(n_table), int(bin), ptrs[3], ptrs[4]))

    # ------------------------------------------------------------------ measurement
    def timing_enable(self, on=True):
        """False / 0: off; True / 1: HIP events around every kernel; 2: around k_main only (cheaper)."""
        self._check(self._lib.iss_timing_enable(self._ctx, int(on)))

    def timing_read(self):
        ms = (C.c_double * 4)()
        n = C.c_int64(0)
        self._check(self._lib.iss_timing_read(self._ctx, C.byref(ms), C.byref(n)))
        return {"setup_ms": ms[0], "main_ms": ms[1], "indel_scan_ms": ms[2], "indel_fixup_ms": ms[3],
                "launches": n.value}

    def main_kernel(self):
        """Name of the kernel the last generate() / generate_batch() launched for the hot path ("k_main<...>" / "k_main_g<NI, NP>")."""
        buf = C.create_string_buffer(64)
        self._check(self._lib.iss_main_kernel(self._ctx, buf, 64))
        return buf.value.decode()

    def stats_read(self):
        n, m = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.iss_stats_read(self._ctx, C.byref(n), C.byref(m)))
        return {"fixup_reads": n.value, "scripted_reads": m.value}


def fastq_write(fd_r1, fd_r2, record_id, first_i, cpu_number, n_pairs, read_length, pitch, r1_base, r1_qual, r2_base,
                r2_qual, n_threads=4):
    """FASTQ text for rows of pitched uint8 arrays (SeqIO.write(..., 'fastq-sanger'), generator.py:64-65)."""
    arrs = [np.ascontiguousarray(a, dtype=np.uint8) for a in (r1_base, r1_qual, r2_base, r2_qual)]
    rc = _native.lib().iss_fastq_write(int(fd_r1), int(fd_r2), str(record_id).encode(), int(first_i), int(cpu_number),
                                       int(n_pairs), int(read_length), int(pitch), *[a.ctypes.data for a in arrs],
                                       int(n_threads))
    check(None, rc)


__all__ = ["ReadEngine", "EngineError", "fastq_write"]


class BamTally(_native.Session):
    """Device tallies of `model` (include/iss_mi355x.h, iss_bam_*): feed record chunks, download the integer tallies, evaluate the
    quality and insert-size KDE CDFs from them.  Replaces the per-read loop of iss/bam.py:125-170 and the scipy KDEs of
    iss/modeller.py:12-38, 99-134."""

    PREFIX = "iss_bam"

    def feed(self, data, offsets, select):
        """Tally the selected records of one chunk (data: uint8 record bytes, offsets: int64 block_size offsets, select: uint8)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        select = np.ascontiguousarray(select, dtype=np.uint8)
        assert offsets.size == select.size
        self._check(self._lib.iss_bam_feed(self._h, data.ctypes.data, data.size, offsets.ctypes.data, select.ctypes.data, offsets.size))

    def tallies(self):
        """(flat u64 tally words, index of the first bad record or -1, its error code)."""
        out = np.zeros(_native.BAM_TALLY_WORDS, dtype=np.uint64)
        rec, code = C.c_int64(), C.c_int32()
        self._check(self._lib.iss_bam_tally_download(self._h, out.ctypes.data, C.byref(rec), C.byref(code)))
        return out, rec.value, code.value

    def kde(self, read_length, with_isize=True):
        """qcdf [2 mates][4 bins][301][41] (NaN rows where no CDF exists) and the 2000-point insert-size CDF (or None)."""
        q = np.empty((2, 4, _native.BAM_MAX_LEN, 41), dtype=np.float64)
        iz = np.empty(_native.BAM_NTLEN, dtype=np.float64)
        self._check(self._lib.iss_bam_kde(self._h, int(read_length), 1 if with_isize else 0, q.ctypes.data, iz.ctypes.data))
        return q, (iz if with_isize else None)
