"""Reads as PyTorch tensors on the GPU: the engine's output rows exported by k_rows_export (include/iss_mi355x.h:
iss_output_export) into tensors torch allocates -- for a consumer that stays on the device (a training or evaluation loop of a
read classifier, a quality model, a k-mer sketch).  Nothing here touches the host copy route (ReadEngine.download).

    for batch in ReadTensorStream(records, dense_model, work, batch_pairs=1 << 20, seed=7):
        loss = net(batch.bases, batch.qual, batch.record)     # uint8 [N, 2, L], uint8 [N, 2, L], int32 [N]

With ``truth=True`` every batch also carries per-base truth -- ``batch.truth``: the bases as they stood before the simulator's
substitutions -- and, with ``events_capacity``, the mutation rows themselves (``batch.events``, ``batch.n_events``): the engine's
--store_mutations rows exported on the device (iss_mutations_export).

torch is imported when a tensor is first needed (the package itself does not import it); the pure parts -- the cutting of a work
list into batches, the numpy twins of the export kernels, ``multinomial_work`` -- need numpy only."""
import collections
import logging

import numpy as np

from . import _native
from ._native import EXPORT_ENCODINGS, EngineError, E_INVALID, E_NOMEM

ReadBatch = collections.namedtuple("ReadBatch", ["bases", "qual", "coords", "record", "truth", "events", "n_events"],
                                   defaults=(None, None, None))
ReadBatch.ref_coords = None  # (not a field: a stream with ``variants`` hands out LiftedReadBatch, which has it as its eighth)
LiftedReadBatch = collections.namedtuple("LiftedReadBatch", ReadBatch._fields + ("ref_coords",), defaults=(None, None, None, None))
ReadBatch.__doc__ = """bases, qual: torch.uint8 [N, 2, L] (mate 1, mate 2; read length L, no padding); coords: torch.int64 [N, 4]
(forward_start, reverse_start, reverse_end, insert_size in the record's own coordinates); record: torch.int32 [N] (the index of
the pair's record in the list the stream was given; the work item for export_tensors).  Only when asked for (else None) --
truth: torch.uint8 [N, 2, L], ``bases`` with the ``ref`` letter of every recorded substitution put back, same encoding; events:
torch.int32 [capacity, 6], rows (pair within the batch, mate, type 0 substitution / 1 insertion / 2 deletion, position, ref,
alt -- ASCII) in the order of ReadEngine.mutations(); n_events: 0-dim torch.int64, the batch's rows (rows from ``capacity`` on
are not in ``events``; -1: the engine's row slots overflowed).  A stream with ``variants`` hands out LiftedReadBatch, the same
fields and an eighth -- ref_coords: torch.int64 [N, 4], ``coords`` with its three positions lifted from the haplotype to the
record on the device (ReadEngine.lift_ptr), the insert size copied; on a ReadBatch the attribute is None.  All on the engine's device, owned by the caller: the engine keeps
no reference and never writes to them again."""


def _torch():
    """torch, imported on first use.  A torch wheel carries its own HIP runtime and a process must hold ONE: when torch is
    imported first the engine's library binds to torch's copy (same soname); the other way round torch starts a second copy that
    finds no GPU -- said here instead of in torch's "No HIP GPUs are available"."""
    import sys

    late = "torch" not in sys.modules and _native._lib is not None
    import torch

    if late and not torch.cuda.is_available():
        raise RuntimeError("insilicoseq_amd.tensors: torch was imported after the engine's HIP library was loaded and sees no GPU "
                           "now (two HIP runtimes in one process); `import torch` before the first ReadEngine is created")
    return torch


# ---------------------------------------------------------------------------------------------------- the pure parts
def row_byte_index(p, k, pitch):
    """Byte of position ``p`` of array ``k`` (0 R1 bases, 1 R1 phred, 2 R2 bases, 3 R2 phred) inside a pair's device row (the
    formula of include/iss_mi355x.h, iss_output_reserve); the row is ``row_bytes(pitch)`` long."""
    p = np.asarray(p, dtype=np.int64)
    return 128 * (p // 32) + 64 * (k // 2) + 16 * ((p // 8) % 4) + 8 * (k % 2) + p % 8


def row_bytes(pitch):
    return 128 * ((int(pitch) + 31) // 32)


def pitch_of(read_length):
    return 8 * ((int(read_length) + 7) // 8)


_CODE_TABLE = np.full(256, 4, dtype=np.uint8)
for _k, _c in enumerate(b"ACGT"):
    _CODE_TABLE[_c] = _CODE_TABLE[_c | 0x20] = _k


def recode(ascii_bases):
    """ISS_EXPORT_CODES on the host: A, C, G, T -> 0, 1, 2, 3 in either case, every other byte 4."""
    return _CODE_TABLE[np.asarray(ascii_bases, dtype=np.uint8)]


def export_rows_host(rows, read_length, encoding="ascii"):
    """The numpy twin of k_rows_export's byte work: device rows uint8 [n, row_bytes] -> (bases, qual) uint8 [n, 2, read_length]."""
    if encoding not in EXPORT_ENCODINGS:
        raise ValueError("encoding must be 'ascii' or 'codes'")
    rows = np.asarray(rows, dtype=np.uint8)
    pos = np.arange(int(read_length))
    pitch = pitch_of(read_length)
    assert rows.ndim == 2 and rows.shape[1] == row_bytes(pitch)
    arrays = [rows[:, row_byte_index(pos, k, pitch)] for k in range(4)]
    bases = np.stack([arrays[0], arrays[2]], axis=1)
    qual = np.stack([arrays[1], arrays[3]], axis=1)
    return (recode(bases) if encoding == "codes" else bases), qual


def truth_host(bases, rows, encoding="ascii"):
    """The numpy twin of k_truth_scatter: ``bases`` uint8 [n, 2, L] as exported in ``encoding``, ``rows`` the structured array of
    ReadEngine.mutations() or any other with its fields (``pair`` counted from bases[0]; rows of other pairs are passed over) -> truth uint8
    [n, 2, L]: the ``ref`` letter (recoded under "codes", in either letter case) at every position with a substitution row
    (type 0), the base everywhere else.  Indel rows are not painted: their positions are positions of the sequence as it stood
    when the event fired."""
    if encoding not in EXPORT_ENCODINGS:
        raise ValueError("encoding must be 'ascii' or 'codes'")
    truth = np.array(bases, dtype=np.uint8, copy=True)
    assert truth.ndim == 3 and truth.shape[1] == 2
    rows = np.asarray(rows)
    sub = rows[(rows["type"] == 0) & (rows["pair"] >= 0) & (rows["pair"] < truth.shape[0])]
    ref = sub["ref"].astype(np.uint8)
    truth[sub["pair"].astype(np.int64), sub["mate"].astype(np.int64) & 1, sub["position"].astype(np.int64)] = \
        recode(ref) if encoding == "codes" else ref
    return truth


def events_host(rows, first_pair, n_pairs):
    """The numpy twin of k_truth_events: the rows of pairs [first_pair, first_pair + n_pairs), in the order they stand in
    (ReadEngine.mutations(): pair, mate, indel rows in loop order, substitution rows by position) -> int32 [k, 6]
    (pair - first_pair, mate, type, position, ref, alt)."""
    rows = np.asarray(rows)
    sel = rows[(rows["pair"] >= int(first_pair)) & (rows["pair"] < int(first_pair) + int(n_pairs))]
    out = np.empty((sel.shape[0], 6), dtype=np.int32)
    out[:, 0] = sel["pair"].astype(np.int64) - int(first_pair)
    for k, f in enumerate(("mate", "type", "position", "ref", "alt"), start=1):
        out[:, k] = sel[f]
    return out


MUT_CHUNK_SLOTS = 256         # slots a wavefront reserves at a time (iss_kernels.hip.h: MUT_CHUNK)
MAIN_LAUNCH_PAIRS = 12582912  # pairs of one launch of a generate call at most (iss_host_util.hip.h: MAIN_CHUNK_PAIRS)


def default_mutation_slots(error_model, batch_pairs, compute_units=256):
    """Row slots to reserve (ReadEngine.mutations_reserve) for generate calls of ``batch_pairs`` pairs, by the advice of
    include/iss_mi355x.h (iss_mutations_reserve): the kernels reserve slots in 256-slot chunks per wavefront, so

        slots = 256 * wavefronts + batch_pairs * (2 * expected rows of a pair + 4)

    * wavefronts: every wavefront that records a row leaves one chunk partly used.  Per launch the main kernel runs one
      16-wavefront workgroup per compute unit and the indel fix-up at most 8 four-wavefront workgroups per compute unit, one
      wavefront per read (2 * batch_pairs reads): 16 CU + min(32 CU, 2 * batch_pairs); a call of more than 12 582 912 pairs
      is several launches.
    * expected rows of a pair: DenseModel.expected_mutation_rows_per_pair() -- substitutions from the model's phred tables
      (sum over positions of P(phred) * 10 ** (-phred / 10), the quality bins weighted) plus its indel rates.  Twice that: a
      wavefront that needs n <= 64 slots when fewer are left in its chunk takes a new chunk (a chunk may end a quarter
      empty), and the reads the fix-up rebuilds leave their first rows behind as stale ones; + 4 per pair keeps small batches
      of a clean model above their own scatter (generator.py sizes the --store_mutations buffers the same way)."""
    n = max(int(batch_pairs), 1)
    cu = max(int(compute_units), 1)
    launches = -(-n // MAIN_LAUNCH_PAIRS)
    wavefronts = launches * (16 * cu + min(32 * cu, 2 * n))
    per_pair = 2.0 * float(error_model.expected_mutation_rows_per_pair()) + 4.0
    return int(MUT_CHUNK_SLOTS * wavefronts + np.ceil(n * per_pair))


def coords_from_descriptors(fs, re, meta, isz, read_length, arena_off=0):
    """The coordinates of iss_output_download_coords from the fields of the device's pair descriptors: 36-bit signed
    forward_start / reverse_end (low words ``fs`` / ``re``, bits 32-35 in ``meta`` bits 8-11 / 12-15), less the arena offset of
    the pair's record -> int64 [n, 4] (forward_start, reverse_start, reverse_end, insert_size)."""
    fs, re, meta = (np.asarray(a).astype(np.int64) for a in (fs, re, meta))

    def wide(lo, shift):
        hi = (meta >> shift) & 15
        hi = np.where(hi >= 8, hi - 16, hi)
        return (hi << 32) | (lo & 0xFFFFFFFF)

    off = np.asarray(arena_off, dtype=np.int64)
    f, r = wide(fs, 8) - off, wide(re, 12) - off
    return np.stack([f, r - int(read_length), r, np.broadcast_to(np.asarray(isz, dtype=np.int64), f.shape)], axis=-1)


def cut_batches(counts, batch_pairs):
    """Cut a work list -- ``counts[k]`` pairs of item k, in order -- into batches of ``batch_pairs`` pairs (the last one may be
    smaller).  -> [(first_ordinal, first_item, [pairs of items first_item, first_item + 1, ...])]: a batch takes consecutive
    items, the first and the last possibly in part; its pairs are the ordinals first_ordinal, first_ordinal + 1, ... of the whole
    list.  Every batch holds pairs and every pair is in one batch; items of no pairs may stand inside a batch."""
    batch_pairs = int(batch_pairs)
    if batch_pairs < 1:
        raise ValueError("batch_pairs must be positive")
    out = []
    ordinal, room, cur, first_item = 0, batch_pairs, [], 0
    for k, n in enumerate(counts):
        n = int(n)
        if n < 0:
            raise ValueError("negative pair count")
        if n == 0 and cur:
            cur.append(0)
        while n:
            if not cur:
                first_item = k
            take = min(n, room)
            cur.append(take)
            n -= take
            room -= take
            if not room:
                total = sum(cur)
                out.append((ordinal, first_item, cur))
                ordinal += total
                room, cur = batch_pairs, []
    if cur and sum(cur):
        out.append((ordinal, first_item, cur))
    return out


def multinomial_work(shares, n_pairs, seed):
    """One mixed work list from abundance shares: [(record_index, pairs)] with the pair counts drawn in ONE multinomial draw of
    numpy.random.Generator(Philox(seed)) -- deterministic in the seed, the counts sum to ``n_pairs``."""
    p = np.asarray(shares, dtype=np.float64)
    if p.ndim != 1 or not p.size or (p < 0).any() or not p.sum() > 0:
        raise ValueError("shares: a non-empty list of non-negative numbers, not all zero")
    rng = np.random.Generator(np.random.Philox(int(seed)))
    counts = rng.multinomial(int(n_pairs), p / p.sum())
    return [(k, int(c)) for k, c in enumerate(counts)]


# ---------------------------------------------------------------------------------------------------- tensors
_side_streams = {}


class _EngineOnCurrentStream(object):
    """Point the engine at torch's current stream, with no wait on the host (ReadEngine.set_stream(..., wait=False)).  The null
    stream has no handle the engine could take (NULL means "the engine's own stream"): the engine then works on a side stream
    of this module that waits for the current stream, and the current stream waits for it at the end."""

    def __init__(self, engine, restore):
        torch = _torch()
        self.engine, self.restore = engine, restore
        self.current = torch.cuda.current_stream(engine.device)
        self.side = None
        if not self.current.cuda_stream:
            if engine.device not in _side_streams:
                _side_streams[engine.device] = torch.cuda.Stream(engine.device)
            self.side = _side_streams[engine.device]

    def __enter__(self):
        self.previous = self.engine.stream_ptr
        work = self.side or self.current
        self.engine.set_stream(work.cuda_stream, wait=False)
        return self

    def join_inputs(self):
        """What the current stream has queued so far (the last use of memory the allocator hands out again, the caller's work on
        ``out``) comes before what the engine queues from here on."""
        if self.side is not None:
            self.side.wait_stream(self.current)

    def __exit__(self, *exc):
        if self.side is not None:
            self.current.wait_stream(self.side)
        if self.restore:
            self.engine.set_stream(self.previous, wait=False)


def _empty_batch(engine, n_pairs, truth=False, events_capacity=0):
    torch = _torch()
    dev = torch.device("cuda", engine.device)
    L = engine.read_length
    out = ReadBatch(torch.empty((n_pairs, 2, L), dtype=torch.uint8, device=dev), torch.empty((n_pairs, 2, L), dtype=torch.uint8, device=dev),
                    torch.empty((n_pairs, 4), dtype=torch.int64, device=dev), torch.empty((n_pairs,), dtype=torch.int32, device=dev))
    if truth:
        out = out._replace(truth=torch.empty((n_pairs, 2, L), dtype=torch.uint8, device=dev))
    if events_capacity > 0:
        out = out._replace(events=torch.empty((int(events_capacity), 6), dtype=torch.int32, device=dev),
                           n_events=torch.empty((), dtype=torch.int64, device=dev))
    return out


def _check_out(engine, out, n_pairs):
    torch = _torch()
    L = engine.read_length
    want = (((n_pairs, 2, L), torch.uint8), ((n_pairs, 2, L), torch.uint8), ((n_pairs, 4), torch.int64), ((n_pairs,), torch.int32),
            ((n_pairs, 2, L), torch.uint8), (("capacity >= 1", 6), torch.int32), ((), torch.int64))
    if (out.events is None) != (out.n_events is None):
        raise ValueError("out.events and out.n_events go together")
    for name, t, (shape, dtype) in zip(ReadBatch._fields, out, want):
        if t is None:
            continue
        if name == "events" and t.dim() == 2 and t.shape[0] >= 1:
            shape = (int(t.shape[0]), 6)
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != torch.device("cuda", engine.device):
            raise ValueError("out.%s: a contiguous %s tensor of shape %s on cuda:%d" % (name, dtype, shape, engine.device))


def _export_into(engine, first_pair, n_pairs, encoding, out):
    engine.export(first_pair, n_pairs, *[t.data_ptr() if t is not None and n_pairs else None for t in out[:4]], encoding=encoding)
    if out.truth is not None or out.events is not None:
        ev = out.events is not None
        engine.export_mutations(first_pair, n_pairs, truth_ptr=out.truth.data_ptr() if out.truth is not None and n_pairs else None,
                                events_ptr=out.events.data_ptr() if ev else None, capacity=out.events.shape[0] if ev else 0,
                                n_events_ptr=out.n_events.data_ptr() if ev else None, encoding=encoding)


def export_tensors(engine, first_pair, n_pairs, encoding="codes", out=None, truth=False, events_capacity=0):
    """Rows [first_pair, +n_pairs) of ``engine`` as a ReadBatch on its device; ``record`` holds the pair's item of the last
    generate_batch() (0 for other rows).  The tensors are allocated by torch, or ``out`` (a ReadBatch; a field may be None: not
    wanted) is written.  ``truth`` / ``events_capacity`` > 0: the fields ``truth`` / ``events`` and ``n_events`` as well, from
    the mutation rows of the last generate call -- the engine must hold a reservation (ReadEngine.mutations_reserve) made before
    that call, and the rows must be that call's; an ``out`` that carries these fields asks for them too.  Stream rule: the export runs on torch's current stream -- behind everything the engine has queued (its
    generation) and in front of whatever the caller queues on that stream next; afterwards the engine is back on the stream it
    had, ordered behind the export, so that generating into the same rows right away is safe.  Nothing waits on the host."""
    if encoding not in EXPORT_ENCODINGS:
        raise EngineError(E_INVALID, "export_tensors: encoding must be 'ascii' or 'codes', not %r" % (encoding,))
    n_pairs = int(n_pairs)
    torch = _torch()
    with torch.cuda.device(engine.device):
        if out is None:
            out = _empty_batch(engine, n_pairs, truth, int(events_capacity))
        else:
            out = ReadBatch(*out)
            _check_out(engine, out, n_pairs)
        with _EngineOnCurrentStream(engine, restore=True) as on:
            on.join_inputs()
            _export_into(engine, first_pair, n_pairs, encoding, out)
    return out


class ReadTensorStream(object):
    """Batches of reads as tensors: ``records`` (sequences: str / bytes) and the error model (a DenseModel) are uploaded once;
    iterating walks ``work`` -- [(record_index, pairs)] -- in order, ``batch_pairs`` pairs at a time (the last batch may be
    smaller, a batch may span several records): one generate_batch() and one export per batch, pair ordinals running on from
    batch to batch.  The concatenation of the batches does not depend on ``batch_pairs``: it is one generate_batch() of the
    whole list.  Records not longer than the read length are skipped with a warning, as the generator's work loop skips them.
    ``fragment_length`` / ``fragment_sd``: custom fragment lengths (both or none).

    Every batch is a new set of tensors that belongs to the caller.  A batch is generated and exported on torch's current
    stream at the time it is asked for; nothing waits on the host.

    ``truth=True``: the engine's mutation rows are reserved once, here (``mutation_slots`` row slots; default:
    default_mutation_slots() for the model, the batch size and the device's compute units), and every batch carries ``truth``;
    with ``events_capacity`` > 0 also ``events`` [events_capacity, 6] and ``n_events``, an event's pair counted from the batch's
    first pair.  The contract extends to them: concatenated over the batches (the pairs rebased by the batches' first
    ordinals), ``truth`` and the valid event rows do not depend on ``batch_pairs``.  ``truth=False`` (the default): no
    reservation, the same kernels and tensors as before, the three fields None.

    Overflow rule.  A batch whose generate call asked for more row slots than ``mutation_slots`` has no row that can be
    trusted: the device writes n_events = -1 and leaves ``truth`` equal to ``bases``.  The stream learns of it without a wait
    of its own: each batch's count is also copied, asynchronously, into a pinned host word with an event recorded behind the
    copy; the word of a batch is looked at when the NEXT batch is asked for (by then the event has normally passed; if not,
    that one event is waited for), the last batch's when the iteration ends.  On -1 the stream raises EngineError(E_NOMEM)
    naming the batch and ``mutation_slots`` -- so the batch in question has already been handed out when the error comes:
    do not keep results of an iteration that raised.

    ``tally=True``: the stream owns ``stream.tally``, one zeroed torch.int64 tensor of ReadEngine.tally_words() words on the
    device (zeroed on the current stream of the constructor), and adds every batch's tallies to it (ReadEngine.tally: quality
    profile, base composition, GC, mean quality, insert sizes; tally.split_tally names the fields) behind the batch's generation,
    on the same stream, with no wait on the host -- it is complete when the stream has passed the last batch, and does not
    depend on ``batch_pairs``.  The batches are unchanged.  ``tally=False`` (the default): ``stream.tally`` is None, no launch is
    added.

    ``depth=True``: per-base coverage depth (depth.py has the definition).  The stream owns
    ``stream.depth_diff``, one zeroed torch.int32 difference array over the records its work list names, and
    ``stream.depth_table``, torch.int64 [len(records), 2] of (offset, length) on the device, uploaded once -- row k is record k of
    the list the stream was given, offset -1 for a record the work list does not name (or that is too short).  Every batch's
    template intervals are added (ReadEngine.depth_mark) behind the batch's generation, on the same stream, with no wait on the
    host.  The contract extends to it: the array after the last batch does not depend on ``batch_pairs``.  ``stream.depth(bin=0)``
    -> (depth torch.uint32 [words], stats torch.uint64 [len(records), 4][, bins torch.uint64 with ``bin`` > 0]) computed on the
    device on torch's current stream (ReadEngine.depth_finish), not in place: iteration can go on, and a later call sees more.
    A stream refuses to mark more than 2^30 pairs (EngineError(E_INVALID)): a depth stays below 2^31.  ``depth=False`` (the
    default): both attributes are None, no launch is added.

    ``error_tally=True``: what the run did to the reads (errtally.py has the definition).  The stream owns
    ``stream.error_tally``, one zeroed torch.int64 tensor of ReadEngine.error_tally_words() words on the device, and adds the
    tallies of every batch's mutation rows to it (ReadEngine.error_tally; errtally.split names the fields) behind the batch's
    generation, on the same stream, with no wait on the host; it does not depend on ``batch_pairs``.  It needs the mutation rows:
    with ``truth=True`` it shares that reservation, without it the stream reserves ``mutation_slots`` slots of its own (default:
    default_mutation_slots()) and the batches stay without ``truth``.  The overflow rule above covers it: a batch that
    overflowed adds 1 to the tally's ``dropped`` and nothing else, and the stream raises when the next batch is asked for.
    ``error_tally=False`` (the default): the attribute is None, no launch is added.

    ``variants``: {record index: variants.VariantTable} -- those records are uploaded with their variants spliced in on the
    device (ReadEngine.add_genome_variants), every length and coordinate of the stream is the haplotype's, and every batch
    carries ``ref_coords``, its coordinates lifted back to the record on the device, behind the export, on the same stream.
    ``variants=None`` (the default): no launch is added, ``ref_coords`` is None."""

    def __init__(self, records, error_model, work, batch_pairs, seed=0, device=0, encoding="codes", sequence_type="metagenomics",
                 gc_bias=False, fragment_length=None, fragment_sd=None, truth=False, events_capacity=0, mutation_slots=None, tally=False, depth=False,
                 error_tally=False, variants=None):
        from .engine import ReadEngine

        if encoding not in EXPORT_ENCODINGS:
            raise EngineError(E_INVALID, "ReadTensorStream: encoding must be 'ascii' or 'codes', not %r" % (encoding,))
        self.truth, self.events_capacity = bool(truth), int(events_capacity)
        self._rows = self.truth or bool(error_tally)  # the mutation rows are reserved, every batch's overflow word is looked at
        if self.events_capacity < 0 or (self.events_capacity and not self.truth):
            raise EngineError(E_INVALID, "ReadTensorStream: events_capacity needs truth=True and must not be negative")
        torch = _torch()
        self.batch_pairs, self.seed, self.encoding = int(batch_pairs), int(seed), encoding
        self.sequence_type, self.gc_bias = sequence_type, bool(gc_bias)
        self.engine = ReadEngine(device)
        self.engine.load_model(error_model)
        if fragment_length is not None or fragment_sd is not None:
            self.engine.set_fragment(fragment_length, fragment_sd)
        records = list(records)
        self._variants = dict(variants) if variants else None
        if self._variants:  # (a record with a table counts with its haplotype's length everywhere below)
            from .variants import HaplotypeSeq

            records = [HaplotypeSeq(r, self._variants[k]) if k in self._variants else r for k, r in enumerate(records)]
        log = logging.getLogger(__name__)
        usable = [k for k, r in enumerate(records) if len(r) > self.engine.read_length]
        for k in sorted(set(range(len(records))) - set(usable)):
            log.warning("record %d shorter than read length for this ErrorModel" % k)
            log.warning("Skipping record %d. You will have less reads than specified" % k)
        plain = [k for k in usable if not (self._variants and k in self._variants)]
        ids = self.engine.add_genomes([records[k] for k in plain])
        gid = {}
        for k, g in zip(plain, ids):
            gid[k] = g if g >= 0 else self.engine.add_genome(records[k])  # (raises what the group could not say)
        for k in usable:
            if k not in gid:  # spliced on the device, alone
                gid[k] = self.engine.add_genome_variants(records[k].ref, records[k].table, record_id=k)
        self.work = [(int(k), int(n)) for k, n in work if int(k) in gid]
        for k, n in work:
            if not 0 <= int(k) < len(records):
                raise ValueError("work names record %d of %d" % (int(k), len(records)))
        self._gids = np.array([gid[k] for k, _ in self.work], dtype=np.int32)
        self._batches = cut_batches([n for _, n in self.work], self.batch_pairs)
        self.n_pairs = sum(n for _, n in self.work)
        self.engine.reserve(min(self.batch_pairs, max(self.n_pairs, 1)))
        self.mutation_slots = 0
        with torch.cuda.device(self.engine.device):
            dev = torch.device("cuda", self.engine.device)
            # the record of every work item, on the device once: a batch's labels are a gather from its slice
            self._work_record = torch.tensor([k for k, _ in self.work], dtype=torch.int32, device=dev)
            self._work_gid = torch.from_numpy(self._gids).to(dev) if self._variants else None  # (the lift's genome of every item)
            self.tally = torch.zeros(self.engine.tally_words(), dtype=torch.int64, device=dev) if tally else None
            self.depth_diff = self.depth_table = self._work_table = None
            self._marked = 0
            if depth:
                from .depth import depth_table

                named = sorted(set(k for k, _ in self.work))
                table = np.full((len(records), 2), -1, dtype=np.int64)
                table[:, 1] = [len(r) for r in records]
                packed, n_words = depth_table([len(records[k]) for k in named])
                table[named, 0] = packed[:, 0]
                self.depth_table = torch.from_numpy(table).to(dev)
                self.depth_diff = torch.zeros(n_words, dtype=torch.int32, device=dev)
                # the table row of every work item: a batch's items are a slice of it
                self._work_table = torch.index_select(self.depth_table, 0, self._work_record.long()).contiguous()
            self.error_tally = None
            if error_tally:
                self.error_tally = torch.zeros(self.engine.error_tally_words(), dtype=torch.int64, device=dev)
            if self._rows:
                if mutation_slots is None:
                    mutation_slots = default_mutation_slots(error_model, min(self.batch_pairs, max(self.n_pairs, 1)),
                                                            torch.cuda.get_device_properties(self.engine.device).multi_processor_count)
                self.mutation_slots = int(mutation_slots)
                self.engine.mutations_reserve(self.mutation_slots)
                self._words = torch.zeros(2, dtype=torch.int64).pin_memory()  # the counts of the last two batches, as they arrive
                self._no_events = torch.empty((1, 6), dtype=torch.int32, device=dev)  # (never written: capacity 0)

    def __len__(self):
        return len(self._batches)

    def close(self):
        self.engine.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def depth(self, bin=0):
        """(depth, stats[, bins]) of what has been marked so far -- see the class -- on the device, behind the marks, on
        torch's current stream; the accumulator is left as it is."""
        if self.depth_diff is None:
            raise EngineError(E_INVALID, "ReadTensorStream.depth: the stream was made without depth=True")
        from .depth import n_windows

        torch = _torch()
        eng = self.engine
        bin = int(bin)
        if bin < 0:
            raise EngineError(E_INVALID, "ReadTensorStream.depth: bin must not be negative")
        with torch.cuda.device(eng.device):
            dev = self.depth_diff.device
            n_words, n_table = int(self.depth_diff.shape[0]), int(self.depth_table.shape[0])
            depth = torch.empty(n_words, dtype=torch.int32, device=dev)
            stats = torch.empty((n_table, 4), dtype=torch.int64, device=dev)
            bins = torch.empty(int(n_windows(self._depth_lengths(), bin).sum()), dtype=torch.int64, device=dev) if bin else None
            with _EngineOnCurrentStream(eng, restore=True) as on:
                on.join_inputs()
                eng.depth_finish(self.depth_diff.data_ptr(), n_words, depth.data_ptr(), self.depth_table.data_ptr(), n_table, bin,
                                 stats.data_ptr(), bins.data_ptr() if bins is not None and bins.numel() else None)
        out = (depth.view(torch.uint32), stats.view(torch.uint64))
        return out + (bins.view(torch.uint64),) if bin else out

    def _depth_lengths(self):
        if getattr(self, "_depth_table_host", None) is None:
            self._depth_table_host = self.depth_table.cpu().numpy()
        return self._depth_table_host

    def _check_overflow(self, pending):
        """The pinned word of a batch handed out before: -1 says its generate call overflowed the reserved row slots."""
        index, event, word = pending
        event.synchronize()  # (normally passed long ago)
        if int(word.item()) < 0:
            raise EngineError(E_NOMEM, "ReadTensorStream: batch %d asked for more mutation row slots than mutation_slots=%d holds; "
                                       "its truth and events are not valid%s (pass a larger mutation_slots)"
                              % (index, self.mutation_slots, "" if self.error_tally is None else ", the error tally counts it as dropped"))

    def __iter__(self):
        torch = _torch()
        eng = self.engine
        pending = None
        for index, (first_ordinal, first_item, counts) in enumerate(self._batches):
            if pending is not None:
                self._check_overflow(pending)
                pending = None
            n = sum(counts)
            with torch.cuda.device(eng.device):
                out = _empty_batch(eng, n, self.truth, self.events_capacity)
                with _EngineOnCurrentStream(eng, restore=False) as on:
                    eng.generate_batch(self._gids[first_item:first_item + len(counts)], counts, first_ordinal=first_ordinal, seed=self.seed,
                                       sequence_type=self.sequence_type, gc_bias=self.gc_bias, out_first_pair=0)
                    on.join_inputs()
                    _export_into(eng, 0, n, self.encoding, out)
                    if self.tally is not None:
                        eng.tally(0, n, self.tally.data_ptr())
                    if self.depth_diff is not None:
                        from .depth import count_marked

                        self._marked = count_marked(self._marked, n)
                        eng.depth_mark(0, n, self._work_table[first_item:].data_ptr(), len(counts), self.depth_diff.data_ptr())
                    if self.error_tally is not None:
                        eng.error_tally(0, n, self.error_tally.data_ptr())
                    count = out.n_events
                    if self._rows and count is None:
                        # no events wanted: the overflow word alone, from an empty window (one small kernel, no row is ordered)
                        count = torch.empty((), dtype=torch.int64, device=out.bases.device)
                        eng.export_mutations(0, 0, events_ptr=self._no_events.data_ptr(), capacity=0, n_events_ptr=count.data_ptr())
                if self._variants:
                    # the three positions of every pair, lifted by the pair's genome; the insert size as it is.  The block above has
                    # ended: the current stream has the export behind it, so torch prepares the lift's inputs there, and the
                    # engine -- on its side stream when the current one is the null stream -- reads them behind join_inputs()
                    pair_gid = torch.index_select(self._work_gid[first_item:first_item + len(counts)], 0, out.record.long())
                    pos = out.coords[:, :3].contiguous()
                    gids3 = pair_gid.unsqueeze(1).expand(-1, 3).contiguous()
                    lifted = torch.empty_like(pos)
                    with _EngineOnCurrentStream(eng, restore=False) as on:
                        on.join_inputs()
                        eng.lift_ptr(pos.data_ptr(), pos.numel(), lifted.data_ptr(), gids_ptr=gids3.data_ptr())
                    out = LiftedReadBatch(*out, ref_coords=torch.cat((lifted, out.coords[:, 3:]), dim=1))
                if self._rows:
                    word = self._words[index & 1]
                    word.copy_(count, non_blocking=True)
                    event = torch.cuda.Event()
                    event.record()
                    pending = (index, event, word)
                # (item -> record on the device, in place: the slice of the work list's records this batch's items index)
                record = torch.index_select(self._work_record[first_item:first_item + len(counts)], 0, out.record.long())
            yield out._replace(record=record)
        if pending is not None:
            self._check_overflow(pending)


__all__ = ["ReadBatch", "LiftedReadBatch", "ReadTensorStream", "export_tensors", "multinomial_work", "cut_batches", "export_rows_host", "recode",
           "row_byte_index", "coords_from_descriptors", "truth_host", "events_host", "default_mutation_slots"]
