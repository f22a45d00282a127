"""Reads as PyTorch tensors on the GPU: the engine's output rows exported by k_rows_export (include/iss_mi355x.h:
iss_output_export) into tensors torch allocates -- for a consumer that stays on the device (a training or evaluation loop of a
read classifier, a quality model, a k-mer sketch).  Nothing here touches the host copy route (ReadEngine.download).

    for batch in ReadTensorStream(records, dense_model, work, batch_pairs=1 << 20, seed=7):
        loss = net(batch.bases, batch.qual, batch.record)     # uint8 [N, 2, L], uint8 [N, 2, L], int32 [N]

torch is imported when a tensor is first needed (the package itself does not import it); the pure parts -- the cutting of a work
list into batches, the numpy twin of the export kernel, ``multinomial_work`` -- need numpy only."""
import collections
import logging

import numpy as np

from . import _native
from ._native import EXPORT_ENCODINGS, EngineError, E_INVALID

ReadBatch = collections.namedtuple("ReadBatch", ["bases", "qual", "coords", "record"])
ReadBatch.__doc__ = """bases, qual: torch.uint8 [N, 2, L] (mate 1, mate 2; read length L, no padding); coords: torch.int64 [N, 4]
(forward_start, reverse_start, reverse_end, insert_size in the record's own coordinates); record: torch.int32 [N] (the index of
the pair's record in the list the stream was given; the work item for export_tensors).  All on the engine's device, owned by the
caller: the engine keeps no reference and never writes to them again."""


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


def _empty_batch(engine, n_pairs):
    torch = _torch()
    dev = torch.device("cuda", engine.device)
    L = engine.read_length
    return ReadBatch(torch.empty((n_pairs, 2, L), dtype=torch.uint8, device=dev), torch.empty((n_pairs, 2, L), dtype=torch.uint8, device=dev),
                     torch.empty((n_pairs, 4), dtype=torch.int64, device=dev), torch.empty((n_pairs,), dtype=torch.int32, device=dev))


def _check_out(engine, out, n_pairs):
    torch = _torch()
    L = engine.read_length
    want = ((n_pairs, 2, L), torch.uint8), ((n_pairs, 2, L), torch.uint8), ((n_pairs, 4), torch.int64), ((n_pairs,), torch.int32)
    for name, t, (shape, dtype) in zip(ReadBatch._fields, out, want):
        if t is None:
            continue
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != torch.device("cuda", engine.device):
            raise ValueError("out.%s: a contiguous %s tensor of shape %s on cuda:%d" % (name, dtype, shape, engine.device))


def _export_into(engine, first_pair, n_pairs, encoding, out):
    engine.export(first_pair, n_pairs, *[t.data_ptr() if t is not None and n_pairs else None for t in out], encoding=encoding)


def export_tensors(engine, first_pair, n_pairs, encoding="codes", out=None):
    """Rows [first_pair, +n_pairs) of ``engine`` as a ReadBatch on its device; ``record`` holds the pair's item of the last
    generate_batch() (0 for other rows).  The tensors are allocated by torch, or ``out`` (a ReadBatch; a field may be None: not
    wanted) is written.  Stream rule: the export runs on torch's current stream -- behind everything the engine has queued (its
    generation) and in front of whatever the caller queues on that stream next; afterwards the engine is back on the stream it
    had, ordered behind the export, so that generating into the same rows right away is safe.  Nothing waits on the host."""
    if encoding not in EXPORT_ENCODINGS:
        raise EngineError(E_INVALID, "export_tensors: encoding must be 'ascii' or 'codes', not %r" % (encoding,))
    n_pairs = int(n_pairs)
    torch = _torch()
    with torch.cuda.device(engine.device):
        if out is None:
            out = _empty_batch(engine, n_pairs)
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
    stream at the time it is asked for; nothing waits on the host."""

    def __init__(self, records, error_model, work, batch_pairs, seed=0, device=0, encoding="codes", sequence_type="metagenomics",
                 gc_bias=False, fragment_length=None, fragment_sd=None):
        from .engine import ReadEngine

        if encoding not in EXPORT_ENCODINGS:
            raise EngineError(E_INVALID, "ReadTensorStream: encoding must be 'ascii' or 'codes', not %r" % (encoding,))
        torch = _torch()
        self.batch_pairs, self.seed, self.encoding = int(batch_pairs), int(seed), encoding
        self.sequence_type, self.gc_bias = sequence_type, bool(gc_bias)
        self.engine = ReadEngine(device)
        self.engine.load_model(error_model)
        if fragment_length is not None or fragment_sd is not None:
            self.engine.set_fragment(fragment_length, fragment_sd)
        records = list(records)
        log = logging.getLogger(__name__)
        usable = [k for k, r in enumerate(records) if len(r) > self.engine.read_length]
        for k in sorted(set(range(len(records))) - set(usable)):
            log.warning("record %d shorter than read length for this ErrorModel" % k)
            log.warning("Skipping record %d. You will have less reads than specified" % k)
        ids = self.engine.add_genomes([records[k] for k in usable])
        gid = {}
        for k, g in zip(usable, ids):
            gid[k] = g if g >= 0 else self.engine.add_genome(records[k])  # (raises what the group could not say)
        self.work = [(int(k), int(n)) for k, n in work if int(k) in gid]
        for k, n in work:
            if not 0 <= int(k) < len(records):
                raise ValueError("work names record %d of %d" % (int(k), len(records)))
        self._gids = np.array([gid[k] for k, _ in self.work], dtype=np.int32)
        self._batches = cut_batches([n for _, n in self.work], self.batch_pairs)
        self.n_pairs = sum(n for _, n in self.work)
        self.engine.reserve(min(self.batch_pairs, max(self.n_pairs, 1)))
        with torch.cuda.device(self.engine.device):
            # the record of every work item, on the device once: a batch's labels are a gather from its slice
            self._work_record = torch.tensor([k for k, _ in self.work], dtype=torch.int32, device=torch.device("cuda", self.engine.device))

    def __len__(self):
        return len(self._batches)

    def close(self):
        self.engine.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __iter__(self):
        torch = _torch()
        eng = self.engine
        for first_ordinal, first_item, counts in self._batches:
            n = sum(counts)
            with torch.cuda.device(eng.device):
                out = _empty_batch(eng, n)
                with _EngineOnCurrentStream(eng, restore=False) as on:
                    eng.generate_batch(self._gids[first_item:first_item + len(counts)], counts, first_ordinal=first_ordinal, seed=self.seed,
                                       sequence_type=self.sequence_type, gc_bias=self.gc_bias, out_first_pair=0)
                    on.join_inputs()
                    _export_into(eng, 0, n, self.encoding, out)
                # (item -> record on the device, in place: the slice of the work list's records this batch's items index)
                record = torch.index_select(self._work_record[first_item:first_item + len(counts)], 0, out.record.long())
            yield out._replace(record=record)


__all__ = ["ReadBatch", "ReadTensorStream", "export_tensors", "multinomial_work", "cut_batches", "export_rows_host", "recode",
           "row_byte_index", "coords_from_descriptors"]
