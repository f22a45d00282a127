"""Host-side mirror of the reference's per-worker driver, on top of the HIP engine.

Same function names, argument order and error behaviour as iss/generator.py so the parity
tests read like the reference's:

* ``worker_iterator(work, error_model, cpu_number, worker_prefix, seed, sequence_type, gc_bias)``
  -- iss/generator.py:223-251: creates ``{prefix}_R1.fastq``, ``{prefix}_R2.fastq``,
  ``{prefix}.vcf``; worker seed = ``seed + cpu_number`` when ``seed is not None``; work items in
  order; pair ids restart at 0 for every work item (:72-75); read ids
  ``{record.id}_{i}_{cpu_number}/1|2`` (:150, 181).
* ``simulate_reads`` -- iss/generator.py:21-66.
* ``generate_work_divider`` -- iss/generator.py:254-356 (rounding correction :299-306, chunking
  :333-356); ``to_coverage`` -- iss/abundance.py:178-193.

One worker == one GPU (``cpu_number`` == rank).  The uniforms come from Philox addressed by
(worker seed, running pair ordinal within the worker), so the output is a pure function of
(seed, cpu_number, work list) -- independent of launch geometry.  It is bit-identical to the
CPU oracle in Philox mode, which in MT mode is bit-identical to the reference.
"""
import contextlib
import functools
import logging
import os
import sys
import time

import numpy as np

from . import _native
from .depth import count_marked, depth_table
from .engine import ReadEngine, fastq_write
from .model import DenseModel


class Record(object):
    """The two attributes of a Bio.SeqRecord the hot path reads: ``id`` and ``seq``."""

    def __init__(self, seq, id="<unknown id>", description=""):
        self.seq = seq
        self.id = id
        self.description = description

    def __len__(self):
        return len(self.seq)


def _parse_fasta_lines(fh):
    """Line by line (any text handle)."""
    header, chunks = None, []
    for line in fh:
        line = line.rstrip("\r\n")
        if line.startswith(">"):
            if header is not None:
                yield Record("".join(chunks), id=(header.split(None, 1) or [""])[0], description=header)
            header, chunks = line[1:], []
        elif header is not None:
            chunks.append(line.strip())
    if header is not None:
        yield Record("".join(chunks), id=(header.split(None, 1) or [""])[0], description=header)


def body_letters(body):
    """The sequence of a record's body (bytes): its line ends removed in one pass; a body with white space inside a line goes
    through the line-by-line form."""
    if b" " in body or b"\t" in body or b"\x0b" in body or b"\x0c" in body:
        return "".join(line.strip() for line in body.decode().splitlines())
    return body.translate(None, b"\r\n").decode()


def read_genome_bytes(path, device_inflate=None):
    """The bytes of a genome file; one that starts with the gzip magic is inflated.  A BGZF file goes through the device inflater
    (inflate.inflate_file) when ``device_inflate`` (None: ISS_DEVICE_INFLATE=1 in the environment); any other gzip file, and every
    file when ISS_HOST_INFLATE=1 is set, is inflated with ``gzip``."""
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:2] != b"\x1f\x8b":
        return data
    if device_inflate is None:
        device_inflate = os.environ.get("ISS_DEVICE_INFLATE", "") == "1"
    if device_inflate and os.environ.get("ISS_HOST_INFLATE", "") != "1":
        from . import inflate

        if inflate.is_bgzf(path):
            return b"".join(piece.tobytes() for piece in inflate.inflate_file(path))
    import gzip

    return gzip.decompress(data)


def parse_fasta(path_or_handle):
    """FASTA -> Records; id = first whitespace-separated token of the header, sequence case-preserved
    (what Bio.SeqIO.parse(..., 'fasta') yields; pinned by iss/test/test_util.py:41-45).  A file given by path is cut
    at its header lines and every record's line ends are removed in one pass (a few hundred Mbp: seconds line by
    line); records with unusual white space inside go through the line-by-line form."""
    if not isinstance(path_or_handle, (str, bytes, os.PathLike)):
        yield from _parse_fasta_lines(path_or_handle)
        return
    data = read_genome_bytes(path_or_handle)
    starts = []  # offsets of the '>' of every header line
    at = 0 if data.startswith(b">") else data.find(b"\n>") + 1
    while at > 0 or (at == 0 and data.startswith(b">") and not starts):
        starts.append(at)
        nxt = data.find(b"\n>", at)
        if nxt < 0:
            break
        at = nxt + 1
    for k, start in enumerate(starts):
        end = starts[k + 1] if k + 1 < len(starts) else len(data)
        eol = data.find(b"\n", start, end)
        if eol < 0:
            eol = end
        header = data[start + 1:eol].decode().rstrip("\r\n")
        yield Record(body_letters(data[eol + 1:end]), id=(header.split(None, 1) or [""])[0], description=header)


def to_coverage(total_n_reads, species_abundance, read_length, genome_size):
    """iss/abundance.py:178-193"""
    n_reads = total_n_reads * species_abundance
    coverage = (n_reads * read_length) / genome_size
    return coverage


def _pairs_per_record(records, readcount_dic, abundance_dic, n_reads, coverage_mode, read_length):
    """(record, read pairs) for every record that gets reads -- the arithmetic of iss/generator.py:288-311: pairs =
    round(reads / 2) per record, plus one whenever the running sum of the rounded counts falls behind the rounded
    running sum of the exact ones."""
    logger = logging.getLogger(__name__)
    if readcount_dic is None and abundance_dic is None:
        raise RuntimeError("No readcount or abundance file provided")
    table, what = (readcount_dic, "readcount") if readcount_dic is not None else (abundance_dic, "abundance")
    exact_sum, given = 0.0, 0
    for record in records:
        if record.id not in table:
            logger.warning("Record %s not found in %s file" % (record.id, what))
            continue
        if readcount_dic is not None:
            exact = table[record.id] / 2
        else:
            share, size = table[record.id], len(record.seq)
            cov = share if coverage_mode else to_coverage(n_reads, share, read_length, size)
            exact = ((cov * size) / read_length) / 2
        n_pairs = round(exact)
        exact_sum += exact
        given += n_pairs
        if round(exact_sum) > given:  # rounding correction
            n_pairs += 1
            given += 1
        logger.debug("%s: %s read pairs" % (record.id, n_pairs))
        if n_pairs:
            yield record, n_pairs


def generate_work_divider(fasta_file, readcount_dic, abundance_dic, n_reads, coverage, coverage_file, error_model,
                          output, chunk_size):
    """Lists of (record, n_pairs, mode), each list worth ``chunk_size`` pairs (the last one possibly less): the
    flattened (record, pairs) sequence cut into consecutive chunks, a record straddling a boundary being split --
    iss/generator.py:254-356.  ``mode`` is always "default": the > 2 GiB pickle spill (:313-331) is a transport
    workaround of the reference's process pool and has no counterpart here (genomes go to HBM, not through pickle)."""
    chunk, room = [], chunk_size
    for record, todo in _pairs_per_record(fasta_file, readcount_dic, abundance_dic, n_reads, bool(coverage or coverage_file),
                                          error_model.read_length):
        while todo:
            take = min(todo, room)
            chunk.append((record, take, "default"))
            todo -= take
            room -= take
            if room == 0:
                yield chunk
                chunk, room = [], chunk_size
    if chunk:
        yield chunk


def _dense_of(error_model):
    if isinstance(error_model, DenseModel):
        return error_model
    if hasattr(error_model, "dense"):
        return error_model.dense()
    raise TypeError("error_model must be an insilicoseq_amd KDErrorModel or DenseModel")


def worker_seed(seed, cpu_number):
    """``seed + cpu_number`` when seeded (iss/generator.py:234-236); OS entropy otherwise."""
    if seed is not None:
        return (int(seed) + int(cpu_number)) & (2**64 - 1)
    return int.from_bytes(os.urandom(8), "little")


SMALL_RECORD = 1 << 20  # records of at most this many letters go into grouped uploads (the engine's SMALL_RECORD)


def _seq_of(record):
    """str / bytes / uint8 array as they are; Bio.Seq and the like through str()"""
    seq = record.seq
    return seq if isinstance(seq, (str, bytes, bytearray, np.ndarray)) else str(seq)


def _in_file(record):
    """Is the record's ``seq`` a fasta.FastaSeq (--device_fasta): letters that stand in a file, uploaded as they stand there?"""
    return hasattr(record.seq, "body_off")


def _warn_short_record(eng, record):
    """True for a record not longer than the model's reads, with the reference's two warnings: its simulate_read fails an
    assertion and the record is skipped (iss/generator.py:77-80).  (An MT caller still consumes the reference's draw.)"""
    if eng.read_length < len(record.seq):
        return False
    logger = logging.getLogger(__name__)
    logger.warning("%s shorter than read length for this ErrorModel" % record.id)
    logger.warning("Skipping %s. You will have less reads than specified" % record.id)
    return True


class GenomeStore(object):
    """Which records are resident in one engine's HBM: id(record) -> (record, genome id), the letters they take, and the three
    operations of the work loops: gid() (look up, else upload), the grouped uploads (plan() / upload_groups()), drop().
    A record with variants -- its ``seq`` a variants.HaplotypeSeq, or its id in ``variants`` -- is uploaded alone, never in a group,
    and spliced on the device (ReadEngine.add_genome_variants); ``resident`` counts its haplotype's letters.

    ``limits`` has GENOME_BUDGET and GROUP_BASES (Worker, or a Worker: read at every call), the store keeps
    GENOME_BUDGET // ``budget_divisor`` letters.  ``drop_on_upload``: gid() drops the resident genomes itself before an upload that
    would pass the budget; otherwise it only notes it (``over``) and the caller drops at a point where nothing names them
    (drop_if_over()).  ``skip_short``: records not longer than the reads are left out of groups."""

    def __init__(self, engine, limits, budget_divisor, drop_on_upload, skip_short, variants=None):
        self.engine, self.limits, self.budget_divisor = engine, limits, budget_divisor
        self.drop_on_upload, self.skip_short = drop_on_upload, skip_short
        self.variants = variants  # --variants: {record id: variants.VariantTable} for records whose seq is the record's own letters
        self._gids = {}  # id(record) -> (record, genome id on the device; -1: the group did not take it)
        self.resident, self.over = 0, False
        self._plan, self._plan_at = [], {}  # the work list's records (plan()) and the first place of each

    @property
    def budget(self):
        return self.limits.GENOME_BUDGET // self.budget_divisor

    def _hit(self, record):
        hit = self._gids.get(id(record))
        return hit if hit is not None and hit[0] is record else None

    def _spliced(self, record):
        """(the record's own letters, its table) for a record with variants, else None."""
        table = getattr(record.seq, "table", None)
        if table is not None:
            return record.seq.ref, table
        table = self.variants.get(record.id) if self.variants else None
        return (_seq_of(record), table) if table is not None else None

    def plan(self, records):
        """Lazy grouping.  The records the work list will ask for, in order: a record's first gid() uploads it in one group
        with the small records after it that are not resident yet."""
        self._plan, self._plan_at = list(records), {}
        for i, record in enumerate(self._plan):
            self._plan_at.setdefault(id(record), i)

    def needs_room_for(self, record):
        """Would uploading this record pass the budget?"""
        return self._hit(record) is None and bool(self._gids) and self.resident + len(record.seq) > self.budget

    def gid(self, record):
        hit = self._hit(record)
        if hit is None:
            if self._gids and self.resident + len(record.seq) > self.budget:
                if self.drop_on_upload:
                    self.drop()
                else:
                    self.over = True
            spliced = self._spliced(record)
            if spliced is not None:
                gid = self.engine.add_genome_variants(spliced[0], spliced[1], record_id=record.id)
                hit = self._gids[id(record)] = (record, gid)
                self.resident += self.engine.genome_length(gid)
                return gid
            at = self._plan_at.get(id(record))
            if at is not None and self._plan[at] is record and len(record.seq) <= SMALL_RECORD:
                self.upload_groups(self._plan[at:], one_group=True)
                hit = self._hit(record)
        if hit is None and _in_file(record) and hasattr(self.engine, "add_genomes_fasta"):
            # --device_fasta: a large record, or one outside the groups, alone and as it stands in the file
            hit = (record, self.engine.add_genomes_fasta([record.seq])[0])
            if hit[1] >= 0:
                self._gids[id(record)] = hit
                self.resident += len(record.seq)
        if hit is None or hit[1] < 0:
            # a large record, one outside the groups, or one its group did not take (the upload raises its error here)
            seq = _seq_of(record)
            hit = self._gids[id(record)] = (record, self.engine.add_genome(seq))
            self.resident += len(seq)
        return hit[1]

    def upload_groups(self, records, one_group=False):
        """Eager grouping.  Upload those of ``records`` that are not resident and small (SMALL_RECORD) in groups of up to
        GROUP_BASES letters each (ReadEngine.add_genomes), in order, and no further than the budget: the record that would pass
        it comes through gid().  ``one_group``: stop where the first group is full."""
        if not hasattr(self.engine, "add_genomes"):
            return  # (an engine that takes records one at a time gets them from gid())
        picked, seqs, seen = [], [], set()
        size = group = 0  # letters picked by this call; letters of the group being filled

        def flush():
            # (--device_fasta: runs of records that stand in a file go as they stand there, each run a group of its own)
            at = 0
            while at < len(picked):
                end = at + 1
                while end < len(picked) and _in_file(picked[end]) == _in_file(picked[at]):
                    end += 1
                run = seqs[at:end]
                gids = self.engine.add_genomes_fasta(run) if _in_file(picked[at]) else self.engine.add_genomes(run)
                for record, seq, gid in zip(picked[at:end], run, gids):
                    self._gids[id(record)] = (record, gid)
                    if gid >= 0:
                        self.resident += len(seq)
                at = end
            del picked[:], seqs[:]

        for record in records:
            if self._hit(record) is not None or id(record) in seen:
                continue
            if self.skip_short and not (self.engine.read_length < len(record.seq)):
                continue  # (skipped by the work loop: never uploaded)
            if self._spliced(record) is not None:
                continue  # (spliced on the device, alone: through gid())
            seq = record.seq if _in_file(record) else _seq_of(record)
            if len(seq) > SMALL_RECORD:
                continue
            # (`resident` holds the groups flushed so far and `size` counts them again: a call that makes several groups stops
            # at about half the budget.  Kept as it was; what it leaves out is uploaded alone.)
            if self.resident + size + len(seq) > self.budget:
                break
            if picked and group + len(seq) > self.limits.GROUP_BASES:
                if one_group:
                    break
                flush()
                group = 0
            seen.add(id(record))
            picked.append(record)
            seqs.append(seq)
            size += len(seq)
            group += len(seq)
        flush()

    def drop(self):
        self.engine.clear_genomes()  # (waits for the device and the FASTQ pipeline first)
        self._gids.clear()
        self.resident, self.over = 0, False

    def drop_if_over(self):
        """For a caller without drop_on_upload, where nothing names an uploaded record."""
        if self.over or self.resident > self.budget:
            self.drop()


def _device_zeros(engine, n_words, dtype):
    """``n_words`` zeroed words (``dtype``: "int32" / "int64") as a torch tensor on the engine's device, for the engine to add to.
    torch zeroes them on its own stream and the engine adds on its own: torch is waited for here."""
    from .tensors import _torch

    torch = _torch()
    with torch.cuda.device(engine.device):
        words = torch.zeros(n_words, dtype=getattr(torch, dtype), device=torch.device("cuda", engine.device))
        torch.cuda.synchronize()
    return words


class _Consumer(object):
    """What reads a settled generate call -- _take_mutations has taken its rows and repeated the call if it had to, so a repeated
    call is read once -- before its rows are generated anew.  Worker.consumers holds those switched on, in
    the fixed order tally, error tally, depth, origins, reads; the work loops know nothing else about them.
    take(items, records): ``items`` are the text job's tuples (record id, id of the first pair, first output row, pairs), their
    rows contiguous from items[0][2], ``records`` the record of each item; asynchronous, like the text jobs.  flush(): drain its
    pipe before the handles close.  save(prefix): write the worker's temp file."""
    # False: it reads the OUTPUT ROWS -- once per batch (the arena fall-back's calls lay their rows side by side).
    # True: it reads what the next generate call overwrites (pair descriptors, mutation rows) -- behind every call.
    per_call = False

    def flush(self):
        pass

    def save(self, prefix):
        pass


class Tally(_Consumer):
    """Zeroed device words that ``add(first output row, rows, address of the words)`` adds the rows of a call to, written to
    ``{prefix}.{suffix}.npy`` as uint64 -- --report: ReadEngine.tally over the output rows (tally.tally_layout); --error_report:
    ReadEngine.error_tally over the call's mutation rows (errtally.layout), which the next call overwrites (``per_call``)."""

    def __init__(self, engine, n_words, add, suffix, per_call):
        self.engine, self.add, self.suffix, self.per_call = engine, add, suffix, per_call
        self.words = _device_zeros(engine, n_words, "int64")

    def take(self, items, records):
        self.add(items[0][2], sum(item[3] for item in items), self.words.data_ptr())

    def save(self, prefix):
        self.engine.synchronize()
        np.save("%s.%s.npy" % (prefix, self.suffix), self.words.cpu().numpy().view(np.uint64).copy())


class Depth(_Consumer):
    """--depth: the call's template intervals marked (ReadEngine.depth_mark) into one int32 difference array over the distinct
    ``records`` of the work list (in order of first appearance; ``ordinals``: their ordinals in the FASTA), whatever GenomeStore
    groups and arena offsets they come to stand in (depth.py) -> ``{prefix}.depth.npz``, for the parent's merge."""
    per_call = True

    def __init__(self, engine, records, ordinals):
        self.engine, self.row, self.ordinals, lengths = engine, {}, [], []
        for record, ordinal in zip(records, ordinals):
            if id(record) not in self.row:
                self.row[id(record)] = len(lengths)
                self.ordinals.append(int(ordinal))
                lengths.append(len(record.seq))
        self.table, n_words = depth_table(lengths)
        self.uploaded, self.pairs = [], 0  # the calls' tables the engine may still read; pairs taken so far
        self.diff = _device_zeros(engine, n_words, "int32")

    def take(self, items, records):  # (the call's table, item -> the record's words, is uploaded for it; asynchronous otherwise)
        from .tensors import _torch

        torch = _torch()
        n_pairs = sum(item[3] for item in items)
        self.pairs = count_marked(self.pairs, n_pairs)
        table = self.table[[self.row[id(r)] for r in records]]
        if len(self.uploaded) >= 8:  # (the marks that read the tables kept so far have run once the engine has been waited for)
            self.engine.synchronize()
            self.uploaded = []
        with torch.cuda.device(self.engine.device):
            dev_table = torch.from_numpy(np.ascontiguousarray(table)).to(torch.device("cuda", self.engine.device))
            torch.cuda.current_stream().synchronize()  # (uploaded on torch's stream; the engine reads it on its own)
        self.uploaded.append(dev_table)
        self.engine.depth_mark(items[0][2], n_pairs, dev_table.data_ptr(), len(records), self.diff.data_ptr())

    def save(self, prefix):
        self.engine.synchronize()
        with open("%s.depth.npz" % prefix, "wb") as fh:  # (a handle: numpy adds no suffix to the name)
            np.savez(fh, diff=self.diff.cpu().numpy(), table=self.table, ordinals=np.asarray(self.ordinals, dtype=np.int64))


class Origins(_Consumer):
    """--origins: the call's source intervals appended to ``handle``, the worker's BEDPE file, as text built on the device
    (ReadEngine.origins_emit_batch; origins.py)."""
    per_call = True

    def __init__(self, engine, handle, cpu_number):
        self.engine, self.handle, self.cpu_number = engine, handle, cpu_number

    def take(self, items, records):
        self.engine.origins_emit_batch(self.handle.fileno(), items, [len(r.seq) for r in records], self.cpu_number)

    def flush(self):
        self.engine.origins_flush()


class Reads(_Consumer):
    """The reads themselves, always the last consumer, in one ``form``: "device" (FASTQ text built on the device, copied and
    written behind the next batch's generation), "ubam" (unaligned BAM records in BGZF blocks instead, one stream: both handles
    are the .bam) or "host" (ISS_HOST_FASTQ=1: rows copied back and formatted by iss_fastq_write).  The work loop says where to
    before its first call: bind()."""

    def __init__(self, engine, cpu_number, form="device"):
        self.engine, self.cpu_number, self.form = engine, cpu_number, form

    def bind(self, forward_handle, reverse_handle, item_wise=False, writer_threads=4):
        """``item_wise``: one fastq_emit per item (one pwrite stream per file: tmpfs gets slower with concurrent writers to one
        file) instead of one text job for all.  The device's text follows what the handles have written: they are flushed."""
        for fh in (forward_handle, reverse_handle):
            fh.flush()
        self.handles, self.item_wise, self.writer_threads = (forward_handle, reverse_handle), item_wise, writer_threads

    def take(self, items, records):
        eng, fd1, fd2 = self.engine, self.handles[0].fileno(), self.handles[1].fileno()
        if self.form == "ubam":
            eng.ubam_emit_batch(fd1, items, self.cpu_number)  # one job of record blocks
        elif self.form == "device" and not self.item_wise:
            eng.fastq_emit_batch(fd1, fd2, items, self.cpu_number)  # one text job
        else:
            for rid, first_i, row, n in items:
                if self.form == "device":
                    eng.fastq_emit(fd1, fd2, rid, first_i, self.cpu_number, row, n, n_threads=1)
                else:
                    eng.synchronize()
                    rows = eng.download(row, n)["_pitched"]
                    fastq_write(fd1, fd2, rid, first_i, self.cpu_number, n, eng.read_length, eng.pitch, *rows[:4], n_threads=self.writer_threads)

    def flush(self):
        if self.form == "ubam":
            self.engine.ubam_flush()


class Worker(object):
    """State of one reference worker on one GPU: engine + uploaded genomes + running ordinal + the consumers of its calls."""

    # rows generated / formatted / written per step of the streaming loop (ISS_BATCH_PAIRS: tuning aid).  2^18: the
    # kernels still run at their full rate, the (pinned) buffers are allocated in a quarter of the time of 2^20
    BATCH_PAIRS = int(os.environ.get("ISS_BATCH_PAIRS", 1 << 18))
    GENOME_BUDGET = 96 << 30  # letters kept resident in HBM (1.4 B each incl. the packed copies) before all are dropped
    # records of at most SMALL_RECORD letters (draft contigs) are uploaded in groups of up to GROUP_BASES letters
    # (ReadEngine.add_genomes: one copy, one pack kernel; a batch whose records are of one group needs no arena copies)
    GROUP_BASES = 1 << 29

    @staticmethod
    def routes(compress=False, ubam=False, origins=False, bgzip=False, error_report=False, store_mutations=False):
        """(device_fastq, device_vcf): is the FASTQ, is the --store_mutations VCF text built on the device?  The one place that reads
        ISS_HOST_FASTQ=1 (rows to iss_fastq_write and to write_mutations) and ISS_HOST_VCF=1 (the latter alone), and that refuses
        what a route cannot do -- before anything is made."""
        device_fastq = os.environ.get("ISS_HOST_FASTQ", "") != "1"
        device_vcf = device_fastq and os.environ.get("ISS_HOST_VCF", "") != "1"
        if error_report and not store_mutations:
            raise ValueError("error_report=True needs a model that stores its mutations (--store_mutations)")
        if origins and not device_fastq:
            raise ValueError("origins=True needs the device path (unset ISS_HOST_FASTQ)")
        if bgzip and not device_vcf:
            raise ValueError("bgzip=True needs the device path (unset ISS_HOST_FASTQ and ISS_HOST_VCF)")
        if ubam and (compress or not device_fastq):
            raise ValueError("ubam=True needs the device path (unset ISS_HOST_FASTQ) and takes no compress=True: BGZF blocks are compressed")
        if compress and not device_fastq:
            raise ValueError("compress=True needs the device FASTQ path (unset ISS_HOST_FASTQ)")
        return device_fastq, device_vcf

    def __init__(self, error_model, cpu_number, seed, device=None, rng="philox", compress=False, store_mutations=False, ubam=False,
                 origins_handle=None, bgzip=False, report=False, error_report=False, depth=None):
        """(worker_iterator's switches; ``origins_handle``: the open BEDPE file, ``depth``: (the work list's records, their ordinals))"""
        if rng not in ("philox", "mt"):
            raise ValueError("rng must be 'philox' (parallel, default) or 'mt' (reference-identical, sequential)")
        self.device_fastq, self.device_vcf = self.routes(compress, ubam, origins_handle is not None, bgzip, error_report, store_mutations)
        self.rng = rng
        self.cpu_number = int(cpu_number)
        self.seed = worker_seed(seed, cpu_number)
        self.engine = ReadEngine(self.cpu_number if device is None else device)
        self.engine.load_model(_dense_of(error_model))
        self.store_mutations = bool(store_mutations)
        if compress:
            self.engine.fastq_compress(True)  # the FASTQ handles receive gzip members instead of text
        fragment = getattr(error_model, "fragment_length", None), getattr(error_model, "fragment_sd", None)
        if rng == "mt":
            # random.seed(seed + cpu_number); np.random.seed(seed + cpu_number)  (generator.py:234-236);
            # unseeded workers draw an OS-entropy seed (the reference is then not reproducible either)
            self.engine.seed_mt(self.seed & 0xFFFFFFFF if seed is None else self.seed)
            self.engine.mt_set_fragment(*fragment)
        else:
            self.engine.set_fragment(*fragment)
        self.ordinal = 0
        if bgzip and origins_handle is not None:
            self.engine.origins_compress(True)  # --bgzip: the two text files receive BGZF members instead of text
        if bgzip and self.store_mutations:
            self.engine.vcf_compress(True)
        eng = self.engine
        self.consumers = ([Tally(eng, eng.tally_words(), eng.tally, "tally", per_call=False)] if report else []) + \
            ([Tally(eng, eng.error_tally_words(), functools.partial(eng.error_tally, source=rng), "errtally", per_call=True)]
             if error_report else []) + \
            ([Depth(eng, *depth)] if depth is not None else []) + \
            ([Origins(eng, origins_handle, self.cpu_number)] if origins_handle is not None else []) + \
            [Reads(eng, self.cpu_number, "ubam" if ubam else "device" if self.device_fastq else "host")]
        self.genomes = GenomeStore(
            self.engine, self,
            budget_divisor=1,     # the whole GENOME_BUDGET: beside the genomes a worker holds one batch of rows and its text
            drop_on_upload=True,  # a work list visits a record in one or two consecutive items: nothing uploaded so far is needed again
            skip_short=rng == "philox")  # the Philox loops skip a short record before any upload; the MT engine needs it for its draw

    def plan(self, records):
        """The records the work list will ask for, in order (GenomeStore.plan: groups are made lazily, from a record's place
        in the list, so that a drop is followed by a new group and not by single uploads)."""
        self.genomes.plan(records)

    def close(self):
        self.consumers = []
        self.engine.close()

    def flush(self):
        """Drain every pipe before the handles close (the text is appended to their descriptors) and are the caller's again:
        the consumers' last to first (uBAM, origins), then the FASTQ pipe (with uBAM too) and the device-built VCF text's."""
        for consumer in reversed(self.consumers):
            consumer.flush()
        self.engine.fastq_flush()
        if _mutation_route(self) == "device":
            self.engine.vcf_flush()

    def needs_room_for(self, record):
        """Would uploading this record drop the resident genomes (GENOME_BUDGET)?"""
        return self.genomes.needs_room_for(record)

    def genome_id(self, record):
        return self.genomes.gid(record)

    def simulate_reads(self, record, n_pairs, forward_handle, reverse_handle, mutations_handle, sequence_type,
                       gc_bias=False, writer_threads=4, flush=True):
        """iss/generator.py:21-66 for one work item, streamed in batches of BATCH_PAIRS: generate on the GPU, then hand the rows
        to the device's text pipeline, which builds the FASTQ (and, with --store_mutations, the VCF) text and writes it behind
        the next batch's generation.  ISS_HOST_FASTQ=1 / ISS_HOST_VCF=1: rows copied back and formatted on the host instead."""
        logger = logging.getLogger(__name__)
        logger.debug("Cpu #%s: Generating %s read pairs" % (self.cpu_number, n_pairs))
        eng = self.engine
        if _warn_short_record(eng, record):
            if self.rng == "mt" and n_pairs > 0:
                # the reference has already drawn the insert size (or, with --fragment-length, its gaussian) when its assertion
                # fails (generator.py:121-130): the engine consumes the same draw and reports the short record
                gid = self.genome_id(record)  # (upload errors -- letters outside the alphabet, an empty record -- propagate)
                try:
                    eng.generate_mt(gid, 1)
                except _native.EngineError as e:
                    if e.code != _native.E_SHORT_RECORD:
                        raise
            return 0
        gid = self.genome_id(record)
        self.consumers[-1].bind(forward_handle, reverse_handle, item_wise=True, writer_threads=writer_threads)
        route = _mutation_route(self)
        if route == "device":
            mutations_handle.flush()  # (the device's text follows what the handle has written)
        done = 0
        while done < n_pairs:
            n = min(self.BATCH_PAIRS, n_pairs - done)

            def gen():
                if self.rng == "mt":
                    assert eng.generate_mt(gid, n, sequence_type=sequence_type, gc_bias=gc_bias, out_first_pair=0) == n
                else:
                    eng.generate(gid, n, first_ordinal=self.ordinal, seed=self.seed, sequence_type=sequence_type,
                                 gc_bias=gc_bias, out_first_pair=0)
            gen()
            items = [(record.id, done, 0, n)]
            _take_mutations(route, eng, gen, mutations_handle, items, self.cpu_number, self.rng)
            for consumer in self.consumers:
                consumer.take(items, [record])
            self.ordinal += n
            done += n
        if self.device_fastq and flush:
            self.flush()
        return done


def _retry_on_row_overflow(eng, regenerate, take):
    """``take()`` turns the --store_mutations rows of the generate call just made (Philox path) into what its caller wants:
    rows on the host, or text on the device.  The row buffer is sized from the model's expected rows; when a batch overflows it (ISS_E_NOMEM: a heavy-indel or edited model, rows written twice for reads
    the indel kernels rebuild) the reservation doubles and ``regenerate()`` repeats the call -- generation is a pure
    function of seed and ordinal, so the rows and the reads are the same ones."""
    while True:
        try:
            return take()
        except _native.EngineError as e:
            if e.code != _native.E_NOMEM:
                raise
            cap = eng.mutations_capacity
            if cap >= 0x7fffffff:
                raise
            # the call says how many slots it asked for: reserve them (+ 1/8, the kernels hand slots out in 256-row chunks
            # per wavefront) in ONE step and repeat the call once
            need = int(getattr(eng, "mutation_slots_needed", 0)) or 2 * max(cap, 1 << 16)
            new_cap = min(need + need // 8 + (1 << 16), 0x7fffffff)
            logging.getLogger(__name__).info("mutation rows: %d slots reserved, the call needs %d: reserving %d and repeating it" % (
                cap, need, new_cap))
            eng.mutations_reserve(new_cap)
            regenerate()


def mutation_rows(eng, regenerate):
    """--store_mutations rows of the generate call just made (Philox path), on the host; an overflowing call is repeated
    (_retry_on_row_overflow)."""
    return _retry_on_row_overflow(eng, regenerate, eng.mutations)


def emit_mutations(eng, regenerate, fd, items, cpu_number):
    """The same rows as VCF text built on the device and appended to ``fd`` (ReadEngine.vcf_emit; ``items`` as for
    fastq_emit_batch), with the same rule for a call that overflows its row buffer."""
    _retry_on_row_overflow(eng, regenerate, lambda: eng.vcf_emit(fd, items, cpu_number))


def _mutation_route(w):
    """Where a worker's --store_mutations rows go: "device" (VCF text built there), "host" (rows copied back), None."""
    return ("device" if w.device_vcf else "host") if w.store_mutations else None


def _take_mutations(route, eng, regenerate, handle, items, cpu_number, source):
    """The --store_mutations rows of the generate call just made -- ``source`` "philox" or "mt"; ``items`` as for
    fastq_emit_batch, the call's rows numbered from its first pair -- to the .vcf ``handle`` by ``route``: text built on the
    device, or rows fetched and written item by item.  A Philox call that overflows its row buffer is repeated with
    ``regenerate`` (_retry_on_row_overflow); an MT call cannot be (its streams have moved on) and never is."""
    if route == "device":
        if source == "mt":
            eng.vcf_emit(handle.fileno(), items, cpu_number, source="mt")
        else:
            emit_mutations(eng, regenerate, handle.fileno(), items, cpu_number)
    elif route == "host":
        rows = eng.mt_mutations() if source == "mt" else mutation_rows(eng, regenerate)
        if len(items) == 1:  # all rows are the item's, numbered from its first pair wherever its output rows start (no copy)
            write_mutations(rows, handle, items[0][0], items[0][1], cpu_number)
            return
        pairs = rows["pair"]  # ascending: the rows come back in (pair, mate, ...) order, so every item's rows are contiguous
        for rid, first_i, row, n in items:
            lo, hi = np.searchsorted(pairs, row, "left"), np.searchsorted(pairs, row + n, "left")
            sel = rows[lo:hi].copy()
            sel["pair"] -= row
            write_mutations(sel, handle, rid, first_i, cpu_number)


def _simulate_work_batched(w, work, forward_handle, reverse_handle, mutations_handle, sequence_type, gc_bias, timings=None):
    """The worker's loop over its work items (iss/generator.py:245-249) with the parallel path's batches cut across
    items: up to BATCH_PAIRS pairs of consecutive items go through ONE set of launches (engine.generate_batch; the
    rows are those of one call per item), then every item's rows are handed to the FASTQ pipeline under its own record
    id.  Same files as simulate_reads item by item.  ``timings``: worker_iterator's dict, for its ``batches``."""
    logger = logging.getLogger(__name__)
    eng = w.engine
    route = _mutation_route(w)
    pending, cur = [], 0  # (record, genome id, pairs, id of the item's first pair in this piece)

    def run():
        nonlocal pending, cur
        if not pending:
            return
        row, emit = 0, []  # one item per pending piece: (record id, first pair id, first output row, pairs)
        for record, _gid, n, first_i in pending:
            emit.append((record.id, first_i, row, n))
            row += n
        records = [p[0] for p in pending]
        rest = w.consumers  # those still to take the batch as a whole
        try:
            def gen():
                eng.generate_batch([p[1] for p in pending], [p[2] for p in pending], first_ordinal=w.ordinal, seed=w.seed,
                                   sequence_type=sequence_type, gc_bias=gc_bias, out_first_pair=0)
            gen()
            _take_mutations(route, eng, gen, mutations_handle, emit, w.cpu_number, "philox")
        except _native.EngineError as e:
            if e.code != _native.E_INVALID or "records of one call must stay below" not in str(e):
                raise
            # records too long to stand side by side in one arena: the same rows, the same call, one item at a time -- every item
            # a call of its own, which the per_call consumers take before the next one overwrites what they read
            eng.reserve(row)
            ordinal = w.ordinal
            for (record, gid, n, _first_i), item in zip(pending, emit):
                def gen1():
                    eng.generate(gid, n, first_ordinal=ordinal, seed=w.seed, sequence_type=sequence_type, gc_bias=gc_bias,
                                 out_first_pair=item[2])
                gen1()
                _take_mutations(route, eng, gen1, mutations_handle, [item], w.cpu_number, "philox")
                for consumer in w.consumers:
                    if consumer.per_call:
                        consumer.take([item], [record])
                ordinal += n
            rest = [consumer for consumer in w.consumers if not consumer.per_call]
        for consumer in rest:  # (every call of the batch has settled: a repeated one is not read twice)
            consumer.take(emit, records)
        w.ordinal += row
        if timings is not None:  # (measurement: when each batch was handed to the FASTQ pipeline, and how many pairs it held)
            timings.setdefault("batches", []).append((time.perf_counter(), row))
        pending, cur = [], 0

    w.consumers[-1].bind(forward_handle, reverse_handle)
    for record, n_pairs, _mode in work:
        logger.debug("Cpu #%s: Generating %s read pairs" % (w.cpu_number, n_pairs))
        if _warn_short_record(eng, record):
            continue
        if w.needs_room_for(record):
            run()  # (the genomes about to be dropped are still named by the pending items)
        gid = w.genome_id(record)
        done = 0
        while done < n_pairs:
            take = min(n_pairs - done, w.BATCH_PAIRS - cur)
            pending.append((record, gid, take, done))
            cur += take
            done += take
            if cur >= w.BATCH_PAIRS:
                run()
    run()


def write_mutations(rows, mutations_handle, record_id, first_i, cpu_number):
    """iss/generator.py:598-620 for the device's mutation records (columns converted once: the per-row cost matters
    at millions of rows per batch)."""
    if len(rows) == 0:
        return
    pair = (np.asarray(rows["pair"], dtype=np.int64) + int(first_i)).tolist()
    mate = (np.asarray(rows["mate"], dtype=np.int64) + 1).tolist()
    typ = np.asarray(rows["type"]).tolist()
    pos = (np.asarray(rows["position"], dtype=np.int64) + 1).tolist()
    ref = np.asarray(rows["ref"], dtype=np.uint8).tobytes().decode("latin-1")
    alt = np.asarray(rows["alt"], dtype=np.uint8).tobytes().decode("latin-1")
    qual = np.asarray(rows["quality"]).tolist()
    head = "%s_" % record_id
    tail = "_%d/" % cpu_number
    # insertion: alt = ref + inserted letter (__init__.py:203); only substitutions carry a quality
    mutations_handle.write("".join(
        "%s%d%s%d\t%d\t.\t%s\t%s\t%s\t\t\n" % (head, p, tail, m, x, r, r + a if t == 1 else a, q if t == 0 else ".")
        for p, m, t, x, r, a, q in zip(pair, mate, typ, pos, ref, alt, qual)))


def simulate_reads(record, error_model, n_pairs, cpu_number, forward_handle, reverse_handle, mutations_handle,
                   sequence_type, gc_bias=False, mode="default", seed=None):
    """Signature of iss/generator.py:21-32 (+ ``seed``: the reference reads the global RNG state)."""
    w = Worker(error_model, cpu_number, seed, device=0)
    try:
        return w.simulate_reads(record, n_pairs, forward_handle, reverse_handle, mutations_handle, sequence_type,
                                gc_bias)
    finally:
        w.close()


def worker_iterator(work, error_model, cpu_number, worker_prefix, seed, sequence_type, gc_bias, device=None,
                    rng="philox", compress=False, timings=None, report=False, depth=False, ordinals=None, ubam=False, origins=False,
                    bgzip=False, error_report=False):
    """iss/generator.py:223-251 on GPU ``device`` (default: ``cpu_number``).  ``rng="mt"`` consumes the
    reference's two Mersenne-Twister streams on the device: the files then equal the reference's byte for
    byte (sequential, ~1e5 pairs/s); ``rng="philox"`` is the parallel path.  ``compress=True``: the two FASTQ files
    (same names) hold gzip members built on the device instead of text -- `--compress` without the text ever leaving
    the GPU; gunzipped they are the files ``compress=False`` writes.  ``timings``: a dict that receives ``t_start``, ``t_ready``
    (engine created, model uploaded), ``batches`` [(time a batch was queued for the files, its pairs)] and ``t_end`` (files
    complete) -- bench.py's end-to-end legs report the steady state apart from the start-up.

    The other switches add consumers of the worker's generate calls (the classes above: what each reads, and when); without one
    no engine call is added.  ``report=True`` (`--report`): ``{prefix}.tally.npy``, uint64 words of tally.tally_layout.
    ``error_report=True`` (`--error_report`; the model must store its mutations): ``{prefix}.errtally.npy``, uint64 words of
    errtally.layout.  ``depth=True`` (`--depth`): ``{prefix}.depth.npz`` -- diff, table, ``ordinals``: the FASTA ordinal of each work
    item's record, default its position in ``work``.  ``origins=True`` (`--origins`): ``{prefix}_origins.bedpe``, one line per pair
    (origins.py).  ``ubam=True`` (`--ubam`): instead of the two FASTQ files ``{prefix}.bam``, the BGZF record blocks of the reads (R1
    then R2 of every pair) -- no BAM header, no EOF block: the parent frames the workers' blocks (ubam.assemble).  ``bgzip=True``
    (`--bgzip`): ``{prefix}.vcf`` and ``{prefix}_origins.bedpe`` hold the BGZF members of their text, compressed on the device
    (ReadEngine.vcf_compress / origins_compress) -- no header member, no EOF block: the parent frames them (bgzf.assemble)."""
    logger = logging.getLogger(__name__)
    store_mutations = bool(getattr(error_model, "store_mutations", False))
    Worker.routes(compress, ubam, origins, bgzip, error_report, store_mutations)  # (what the worker will refuse, before any file is made)
    if timings is not None:
        timings["t_start"] = time.perf_counter()
    if sequence_type not in _native.SEQ_TYPES:
        raise RuntimeError("sequence type '%s' is not supported" % sequence_type)  # generator.py:139
    try:
        if ubam:
            forward_handle = reverse_handle = open("%s.bam" % worker_prefix, "wb")  # (one stream for both mates)
        else:
            forward_handle = open("%s_R1.fastq" % worker_prefix, "w")
            reverse_handle = open("%s_R2.fastq" % worker_prefix, "w")
        mutation_handle = open("%s.vcf" % worker_prefix, "w")
        origins_handle = open("%s_origins.bedpe" % worker_prefix, "wb") if origins else None
    except PermissionError as e:
        logger.error("Failed to write temporary output file(s): %s" % e)
        sys.exit(1)
    records = [record for record, _n, _mode in work]
    w = Worker(error_model, cpu_number, seed, device=device, rng=rng, compress=compress, store_mutations=store_mutations, ubam=ubam,
               origins_handle=origins_handle, bgzip=bgzip, report=report, error_report=error_report,
               depth=(records, ordinals if ordinals is not None else range(len(work))) if depth else None)
    w.plan(records)
    if timings is not None:
        timings["t_ready"] = time.perf_counter()
    if store_mutations:
        # row buffers of a batch, from the model's own error rates (twice the expectation + slack; the Philox kernels
        # reserve 256-row chunks per wavefront on top)
        per_pair = 2.0 * _dense_of(error_model).expected_mutation_rows_per_pair() + 4.0
        if rng == "mt":
            w.engine.mt_mutations_reserve(int(Worker.BATCH_PAIRS * per_pair))
        else:
            w.engine.mutations_reserve(int(Worker.BATCH_PAIRS * per_pair) + (1 << 21))
    try:
        with forward_handle, reverse_handle, mutation_handle, origins_handle or contextlib.nullcontext():
            if store_mutations and w.device_vcf:
                mutation_handle.flush()  # the device's text goes to the descriptor, behind what the handle holds (nothing)
            if rng == "philox" and w.device_fastq and os.environ.get("ISS_ITEMWISE", "") != "1":
                _simulate_work_batched(w, work, forward_handle, reverse_handle, mutation_handle, sequence_type, gc_bias, timings)
            else:
                for record, n_pairs, _mode in work:
                    w.simulate_reads(record, n_pairs, forward_handle, reverse_handle, mutation_handle, sequence_type,
                                     gc_bias, flush=False)  # keep the text pipeline running across work items
            w.flush()
            for consumer in w.consumers:  # (behind the flushes: tally, error tally, depth)
                consumer.save(worker_prefix)
            if timings is not None:
                timings["t_end"] = time.perf_counter()
    finally:
        w.close()


def _digits_before(x):
    """Characters of the decimal numbers 0 .. x-1 written one after the other (iss_fastq.hip.h: digits_before)."""
    total, d, p = 0, 1, 1  # p = 10^(d-1): the numbers with d digits are p .. 10 p - 1 (and 0 has one)
    while x >= p * 10:
        total += d * (p * 10 - (p if d > 1 else 0))
        p *= 10
        d += 1
    return total + d * (x - (p if d > 1 else 0))


def fastq_text_bytes(record_id, n_pairs, cpu_number, read_length):
    """Bytes of the FASTQ text of pairs 0 .. n_pairs-1 of one work item in EITHER file: per record "@{id}_{i}_{cpu}/m\n" + SEQ +
    "\n+\n" + QUAL + "\n" (iss/generator.py:64-65, 150, 181) = len(id) + len(cpu) + 2 RL + 10 + digits(i)."""
    return n_pairs * (len(str(record_id).encode()) + len(str(int(cpu_number))) + 2 * read_length + 10) + _digits_before(n_pairs)


class WorkerSetNotSetUp(_native.EngineError):
    """The worker set could not be set up -- seeding failed, or there is no memory for the first call's stream buffers: nothing
    ran, and the caller may take the process pool instead.  Any other engine error is a failure of the set itself."""


def _open_set_files(worker_prefixes, final_prefix):
    """The set's handles: [(R1, R2)] of the final files, or (R1, R2, vcf) of every worker's temp files."""
    try:
        if final_prefix is not None:
            return [(open("%s_R1.fastq" % final_prefix, "w"), open("%s_R2.fastq" % final_prefix, "w"))]
        return [(open("%s_R1.fastq" % prefix, "w"), open("%s_R2.fastq" % prefix, "w"), open("%s.vcf" % prefix, "w"))
                for prefix in worker_prefixes]
    except PermissionError as e:
        logging.getLogger(__name__).error("Failed to write %s output file(s): %s" % (
            "the" if final_prefix is not None else "temporary", e))
        sys.exit(1)


def _final_offsets(works, cpu_numbers, read_length):
    """Where every worker's text starts and ends in either final file: worker k starts where workers 0 .. k-1 end, and a
    worker's text size is arithmetic (fastq_text_bytes; short records give no text)."""
    starts, ends, total = [], [], 0
    for work, cpu in zip(works, cpu_numbers):
        starts.append(total)
        total += sum(fastq_text_bytes(rec.id, n, cpu, read_length) for rec, n, _m in work if read_length < len(rec.seq))
        ends.append(total)
    return starts, ends


def _set_pieces(genomes, work, cpu, per):
    """One worker's work list as the pieces its rounds take, at most ``per`` pairs each: (record, genome id, pairs, id of the
    piece's first pair, short record?).  The genome id is looked up (or the record uploaded) when the piece's round comes."""
    for record, n_pairs, _mode in work:
        logging.getLogger(__name__).debug("Cpu #%s: Generating %s read pairs" % (cpu, n_pairs))
        if _warn_short_record(genomes.engine, record):
            # the reference has drawn the insert size (or its gaussian) by then (generator.py:121-130): a piece of one pair
            # makes the engine consume that draw
            if n_pairs > 0:
                yield record, genomes.gid(record), 1, 0, True
            continue
        done = 0
        while done < n_pairs:
            n = min(per, n_pairs - done)
            yield record, genomes.gid(record), n, done, False
            done += n


def _run_set_rounds(eng, genomes, its, cpu_numbers, handles, at, read_length, sequence_type, gc_bias, vcf=None):
    """Rounds of one piece per worker (``its``: _set_pieces of every worker) until every work list is done: one
    generate_mt_workers call, then the pieces' text -- one scattered job into the final files at the workers' places ``at``
    (moved on by what is written: fastq_text_bytes at the model's ``read_length``), or with ``at`` None one job per worker into
    its temp files.  ``vcf`` (--store_mutations): (route, the workers' .vcf handles) -- after every round the rows of all
    workers become ONE text job on the device (ReadEngine.vcf_emit_workers), worker k's bytes appended to handle k; route
    "host": the rows fetched worker by worker and written by write_mutations."""
    began = False
    while True:
        genomes.drop_if_over()  # between rounds nothing names an uploaded record (a round uploads what its pieces need again)
        cur = [next(it, None) for it in its]
        if all(c is None for c in cur):
            break
        g = [c[1] if c else 0 for c in cur]
        n = [c[2] if c else 0 for c in cur]
        row = np.concatenate(([0], np.cumsum(n)[:-1])).astype(np.int64)
        try:
            done, status = eng.generate_mt_workers(g, n, row, sequence_type=sequence_type, gc_bias=gc_bias)
        except _native.EngineError as e:
            if not began and e.code == _native.E_NOMEM:  # (the first call reserves the stream buffers)
                raise WorkerSetNotSetUp(e.code, e.message) from e
            raise
        began = True
        scattered = []
        for k, c in enumerate(cur):
            if c is None:
                continue
            if c[4]:
                assert status[k] == _native.E_SHORT_RECORD and done[k] == 0, (k, int(status[k]), int(done[k]))
                continue
            assert status[k] == 0 and done[k] == c[2], (k, int(status[k]), int(done[k]), c[2])
            if at is not None:  # (the piece's bytes: pairs c[3] .. c[3] + c[2] - 1 of the work item)
                scattered.append((c[0].id, c[3], int(row[k]), c[2], cpu_numbers[k], at[k]))
                at[k] += fastq_text_bytes(c[0].id, c[3] + c[2], cpu_numbers[k], read_length) - \
                    fastq_text_bytes(c[0].id, c[3], cpu_numbers[k], read_length)
            else:
                eng.fastq_emit(handles[k][0].fileno(), handles[k][1].fileno(), c[0].id, c[3], cpu_numbers[k], int(row[k]), c[2],
                               n_threads=1)
        if scattered:  # ONE text job per round: the next round's kernels run beside its copy and its writes
            eng.fastq_emit_scatter(handles[0][0].fileno(), handles[0][1].fileno(), scattered, n_threads=1)
        if vcf is not None:
            route, vcf_handles = vcf
            live = [c is not None and not c[4] for c in cur]  # (a short record makes no row: its worker sits the text out)
            if route == "device":
                eng.vcf_emit_workers([(vcf_handles[k].fileno(), c[0].id, c[3], int(row[k]), c[2], cpu_numbers[k]) if live[k]
                                      else (-1, "", 0, 0, 0, cpu_numbers[k]) for k, c in enumerate(cur)])
            else:
                for k, c in enumerate(cur):
                    if live[k]:
                        write_mutations(eng.mt_workers_mutations(k), vcf_handles[k], c[0].id, c[3], cpu_numbers[k])


def worker_set_iterator(works, error_model, cpu_numbers, worker_prefixes, seed, sequence_type, gc_bias, device=None,
                        compress=False, batch_pairs=None, final_prefix=None, vcf_files=False):
    """W reference workers (``rng="mt"``) on ONE GPU, side by side: the files of ``worker_iterator(works[k], error_model,
    cpu_numbers[k], worker_prefixes[k], seed, ..., rng="mt")`` for every k -- byte for byte the reference's
    ``iss generate --cpus W`` temp files (iss/app.py:99-106, iss/generator.py:223-251) -- but the workers' chains run in the
    same kernel launches, one workgroup per worker (ReadEngine.generate_mt_workers).  A worker is a sequential chain over its
    two MT19937 streams (seed + cpu_number, generator.py:234-236); W of them are what the reference itself runs in parallel.
    ``--store_mutations``: every worker owns a region of the engine's row pool (ReadEngine.mt_workers_mutations_reserve, sized
    by worker_iterator's rule at the set's pairs per round); after each round the rows of all workers become one VCF text job
    (vcf_emit_workers; ISS_HOST_VCF=1: rows to the host, write_mutations) appended to the workers' ``{prefix}.vcf`` files -- a
    VCF's size is not arithmetic, so those stay temp files in either mode and the caller concatenates them behind the header.
    ``vcf_files``: the command asked for --store_mutations, so the caller will concatenate the workers' ``.vcf`` files -- they
    are made with ``final_prefix`` too when the model records nothing (PerfectErrorModel: empty files, the header alone).

    ``final_prefix`` (text mode): the workers' text goes straight to ``{final_prefix}_R1.fastq`` / ``_R2.fastq`` -- what the
    parent's concatenation of the temp files in worker order would hold (iss/app.py:123-127, iss/util.py:213-234): a worker's
    text size is arithmetic (fastq_text_bytes), so worker k starts where workers 0 .. k-1 end, a round is ONE text job whose
    pieces are written at their places (ReadEngine.fastq_emit_scatter), and no temp file is made.  Returns True when the final
    files were written, False when the temp files were (the caller concatenates them).  Raises WorkerSetNotSetUp when the set
    could not be set up (nothing ran: seeding, no room for the stream buffers or for the row pool of --store_mutations)."""
    W = len(works)
    if not (W == len(cpu_numbers) == len(worker_prefixes)) or W < 1:
        raise ValueError("worker_set_iterator: one work list, cpu number and file prefix per worker")
    if sequence_type not in _native.SEQ_TYPES:
        raise RuntimeError("sequence type '%s' is not supported" % sequence_type)  # generator.py:139
    store_mutations = bool(getattr(error_model, "store_mutations", False))
    if seed is None:
        # (unseeded workers draw their seeds from the OS one by one, like the reference's processes)
        for work, cpu, prefix in zip(works, cpu_numbers, worker_prefixes):
            worker_iterator(work, error_model, cpu, prefix, seed, sequence_type, gc_bias, device=device, rng="mt", compress=compress)
        return False
    final = final_prefix is not None and not compress
    handles = _open_set_files(worker_prefixes, final_prefix if final else None)
    eng, finished, vcf_handles = None, False, None
    try:
        if store_mutations or vcf_files:  # (the temp-file layout opens a worker's .vcf beside its FASTQ files)
            vcf_handles = [open("%s.vcf" % prefix, "w") for prefix in worker_prefixes] if final else [h[2] for h in handles]
        eng = ReadEngine(0 if device is None else device)
        dense = _dense_of(error_model)
        eng.load_model(dense)
        at = ends = None  # final files: where worker k's next byte goes, and where its text has to end
        if final:
            at, ends = _final_offsets(works, cpu_numbers, dense.read_length)
            for fh in handles[0]:
                fh.flush()
                os.ftruncate(fh.fileno(), ends[-1])
        if compress:
            eng.fastq_compress(True)
        try:
            eng.seed_mt_workers([worker_seed(seed, c) for c in cpu_numbers])
        except _native.EngineError as e:
            raise WorkerSetNotSetUp(e.code, e.message) from e
        eng.mt_set_fragment(getattr(error_model, "fragment_length", None), getattr(error_model, "fragment_sd", None))
        # rows per worker and round (2^20 pairs per round for all workers together; 2^22 and 2^24 measured the same end to end:
        # 16 M pairs at W = 64 in 2.6-2.8 s incl. 0.5 s of engine start -- generation and text take turns)
        per = int(batch_pairs or max(1024, min(Worker.BATCH_PAIRS, (1 << 20) // W)))
        vcf = None
        if store_mutations:
            # a worker's rows of one round, by worker_iterator's rule (twice the model's expectation + slack per pair)
            try:
                eng.mt_workers_mutations_reserve(int(per * (2.0 * dense.expected_mutation_rows_per_pair() + 4.0)))
            except _native.EngineError as e:
                if e.code != _native.E_NOMEM:
                    raise
                raise WorkerSetNotSetUp(e.code, e.message) from e  # (no room for the row pool: nothing ran, like the stream buffers)
            vcf = ("device" if os.environ.get("ISS_HOST_VCF", "") != "1" else "host", vcf_handles)
        genomes = GenomeStore(
            eng, Worker,
            budget_divisor=2,      # Worker's budget less what the set itself holds on the device (stream buffers, rows of a round -- up to a third of the memory)
            drop_on_upload=False,  # a round's pieces name the resident records: they go between rounds (_run_set_rounds)
            skip_short=False)      # the engine consumes a short record's draw: it needs the record
        # eager grouping, once: the workers' lists advance side by side, so there is no one place in a plan to group from, and
        # after a drop the records still to come are uploaded alone as their pieces come up
        genomes.upload_groups(record for work in works for record, _n, _m in work)
        its = [_set_pieces(genomes, work, cpu, per) for work, cpu in zip(works, cpu_numbers)]
        for fh3 in handles:
            for fh in fh3[:2]:
                fh.flush()
        _run_set_rounds(eng, genomes, its, cpu_numbers, handles, at, dense.read_length, sequence_type, gc_bias, vcf)
        eng.fastq_flush()
        if vcf is not None and vcf[0] == "device":
            eng.vcf_flush()  # (before the handles close: the text is appended to their descriptors)
        if final and at != ends:  # every worker's text ends where the next one's starts
            raise RuntimeError("worker_set_iterator: a worker's text is not the size computed for it: %r / %r" % (at, ends))
        finished = True
        return final
    finally:
        if eng is not None:
            eng.close()  # (waits for the writer thread)
        for fh3 in handles:
            for fh in fh3:
                fh.close()
        for fh in (vcf_handles or []) if final else []:
            fh.close()
        if not finished:
            # the final files are full size from the start: a failed run must not leave them behind, nor the workers' .vcf files
            gone = ["%s%s" % (final_prefix, suffix) for suffix in ("_R1.fastq", "_R2.fastq")] if final else []
            for path in gone + (["%s.vcf" % prefix for prefix in worker_prefixes] if store_mutations or vcf_files else []):
                try:
                    os.remove(path)
                except FileNotFoundError:
                    pass


def lognormal_abundance(record_ids, rng):
    """iss/abundance.py:137-154 with an explicit RandomState."""
    dist = rng.lognormal(size=len(record_ids))
    dist_scaled = dist / sum(dist)
    return {r: a for r, a in zip(record_ids, dist_scaled)}
