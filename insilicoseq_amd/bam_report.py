"""`report --bam`: the --report tallies of the reads of a BAM file (include/iss_mi355x.h: iss_br_*; k_br_* of
csrc/iss_bamreads.hip.h), their numpy twin and the FASTQ text the twin stands for.  numpy only, besides the binding.

The words are fastq_report.py's at L = max_len, so that its relayout, longest_read and compare_tallies and tally.report_dict apply:

    pairs [1] | qual [2][L][94] | base [2][L][5] | gc [2][L + 1] | meanq [2][94] | insert [2048] | length [2][L + 1]

A record as read: its bases are "=ACMGRSVTWYHKDBN"[code], its phreds the quality bytes as stored; with flag 0x10 the read as
sequenced is the reverse complement of SEQ and the reversed QUAL, the complement of a 4-bit code being the code with its bits in
reverse order.  The letters then count as FASTQ letters do (tally._CODE_TABLE, tally._GC_TABLE), and every field but ``insert`` is
fastq_report's definition: the tally equals fastq_tally_host of the text bam_to_fastq writes.

Which records count: 0x100 or 0x800 set -- skipped (skipped[0]); else 0x1 clear -- mate 0; 0x1 set -- 0x40 alone mate 0, 0x80 alone
mate 1, both or neither skipped (skipped[1]).  Unmapped records count like any other.  A taken, good mate-0 record adds one to
insert[clip(|tlen| - 2 l_seq, 0, 2047)] when 0x1 is set, 0x4 and 0x8 are clear, refID == next_refID >= 0 and tlen != 0 -- the gap
between the mates, `generate --report`'s meaning of the word, exact where the mates have equal length.  A bad record (REC_*: the
first code that applies, checked before the skip rules) is not tallied, the records after it are, and the first bad one over all
records fed is reported.  DESIGN.md section 28."""
import ctypes as C

import numpy as np

from . import _native
from .bam import BamReader, Chunk
from .fastq_report import finish as _finish, fq_words, split_fq_words
from .tally import INSERT_BINS, PHREDS, _CODE_TABLE, _GC_TABLE

MAX_LEN = _native.BR_MAX_LEN
REC_SHORT, REC_TOO_LONG, REC_NO_QUAL, REC_QUAL_RANGE = 1, 2, 3, 4
SEQ_LETTERS = np.frombuffer(b"=ACMGRSVTWYHKDBN", dtype=np.uint8)
_COMPLEMENT = np.array([int("{:04b}".format(c)[::-1], 2) for c in range(16)], dtype=np.uint8)  # the four bits in reverse order
# CIGAR ops "MIDNSHP=X" (0 .. 8) by class: aligned columns (M = X: what MD describes); with I, S: consume the read; with D, N: the reference
_COLUMN_OPS, _QUERY_OPS, _REF_OPS = (0, 7, 8), (0, 7, 8, 1, 4), (0, 7, 8, 2, 3)


def _field(a, at, n_bytes, signed=False):
    """Little-endian integers of n_bytes at the byte offsets ``at`` of the uint8 array a, as int64."""
    v = np.zeros(at.shape, dtype=np.int64)
    for k in range(n_bytes):
        v |= a[at + k].astype(np.int64) << (8 * k)
    if signed:
        v -= (v >> (8 * n_bytes - 1)) << (8 * n_bytes)
    return v


def _classify(chunk, max_len):
    """Per record of a chunk: a dict of int64 / bool arrays -- ``code`` (0: good), ``mate`` (0, 1; -1: skipped as secondary or
    supplementary, -2: skipped for its mate flags; meaningful where code == 0), ``len``, ``seq`` and ``qual`` (byte offsets),
    ``reverse``, ``insert`` (the bin, or -1); and the header fields as read: ``block_size``, ``ref_id``, ``pos``, ``l_name``,
    ``mapq``, ``n_cigar``, ``flag``."""
    a = np.frombuffer(chunk.data, dtype=np.uint8)
    o = np.asarray(chunk.offsets, dtype=np.int64)
    block_size, ref_id, ref_pos = _field(a, o, 4, True), _field(a, o + 4, 4, True), _field(a, o + 8, 4, True)
    l_name, mapq, n_cigar, flag = _field(a, o + 12, 1), _field(a, o + 13, 1), _field(a, o + 16, 2), _field(a, o + 18, 2)
    l_seq, next_ref, tlen = _field(a, o + 20, 4, True), _field(a, o + 24, 4, True), _field(a, o + 32, 4, True)
    seq = o + 36 + l_name + 4 * n_cigar
    code = np.zeros(o.size, dtype=np.int64)
    short = (l_name == 0) | (l_seq < 0) | (32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq > block_size)
    code[short] = REC_SHORT
    code[~short & (l_seq > max_len)] = REC_TOO_LONG
    length = np.where(code == 0, l_seq, 0)
    qual = seq + (length + 1) // 2
    first_q = a[np.minimum(qual, a.size - 1)]
    code[(code == 0) & (length > 0) & (first_q == 0xFF)] = REC_NO_QUAL
    length[code != 0] = 0
    ok = np.flatnonzero(code == 0)
    rec = np.repeat(ok, length[ok])
    pos = np.arange(rec.size) - np.repeat(np.cumsum(length[ok]) - length[ok], length[ok])
    over = np.bincount(rec, weights=a[qual[rec] + pos] > PHREDS - 1, minlength=o.size) > 0
    code[over] = REC_QUAL_RANGE
    paired = (flag & 1) != 0
    first, last = (flag & 0x40) != 0, (flag & 0x80) != 0
    mate = np.where(paired & last, 1, 0)
    mate[paired & (first == last)] = -2
    mate[(flag & 0x900) != 0] = -1
    gap = np.clip(np.abs(tlen) - 2 * length, 0, INSERT_BINS - 1)  # (int64: |INT32_MIN| does not wrap)
    has_insert = paired & ((flag & 0xC) == 0) & (ref_id == next_ref) & (ref_id >= 0) & (tlen != 0) & (mate == 0) & (code == 0)
    return {"code": code, "mate": mate, "len": length, "seq": seq, "qual": qual, "reverse": (flag & 0x10) != 0,
            "insert": np.where(has_insert, gap, -1), "block_size": block_size, "ref_id": ref_id, "pos": ref_pos, "l_name": l_name,
            "mapq": mapq, "n_cigar": n_cigar, "flag": flag}


def _cigar(a, offset, l_name, n_cigar):
    """The CIGAR of the record at byte ``offset`` of the chunk's bytes a -> [(op, length)]."""
    at = int(offset) + 36 + int(l_name)
    words = np.frombuffer(bytes(a[at:at + 4 * int(n_cigar)]), dtype="<u4").astype(np.int64)
    return list(zip((words & 15).tolist(), (words >> 4).tolist()))


def _tally_chunk(chunk, max_len, t):
    """One feed of the twin: adds the chunk's taken records to the views t; (good records taken [2], skipped [2], first bad
    (index in the chunk, code) or None)."""
    a = np.frombuffer(chunk.data, dtype=np.uint8)
    c = _classify(chunk, max_len)
    good = c["code"] == 0
    skipped = [int((good & (c["mate"] == -1)).sum()), int((good & (c["mate"] == -2)).sum())]
    bad = np.flatnonzero(~good)
    bad = (int(bad[0]), int(c["code"][bad[0]])) if bad.size else None
    taken = np.flatnonzero(good & (c["mate"] >= 0))
    length, mate, reverse = c["len"][taken], c["mate"][taken], c["reverse"][taken]
    rec = np.repeat(np.arange(taken.size), length)                               # every base of the taken records: its record
    pos = np.arange(rec.size) - np.repeat(np.cumsum(length) - length, length)  # (index into taken) and position as sequenced
    src = np.where(reverse[rec], length[rec] - 1 - pos, pos)                    # its position in SEQ and QUAL
    byte = a[c["seq"][taken][rec] + src // 2]
    nib = np.where(src & 1, byte & 15, byte >> 4)
    b = SEQ_LETTERS[np.where(reverse[rec], _COMPLEMENT[nib], nib)]
    q = a[c["qual"][taken][rec] + src].astype(np.int64)
    L = int(max_len)
    m_of = mate[rec]
    gc = np.bincount(rec, weights=_GC_TABLE[b], minlength=taken.size).astype(np.int64)
    qsum = np.bincount(rec, weights=q, minlength=taken.size).astype(np.int64)  # (float64 sums of small integers: exact)
    for m in range(2):
        at, of = m_of == m, mate == m
        t["qual"][m] += np.bincount(pos[at] * PHREDS + q[at], minlength=L * PHREDS).reshape(L, PHREDS).astype(np.uint64)
        t["base"][m] += np.bincount(pos[at] * 5 + _CODE_TABLE[b[at]], minlength=L * 5).reshape(L, 5).astype(np.uint64)
        t["gc"][m] += np.bincount(gc[of], minlength=L + 1).astype(np.uint64)
        some = of & (length > 0)
        t["meanq"][m] += np.bincount(np.minimum(qsum[some] // length[some], PHREDS - 1), minlength=PHREDS).astype(np.uint64)
        t["length"][m] += np.bincount(length[of], minlength=L + 1).astype(np.uint64)
    t["pairs"][0] += np.uint64((mate == 0).sum())
    ins = c["insert"][taken]
    t["insert"] += np.bincount(ins[ins >= 0], minlength=INSERT_BINS).astype(np.uint64)
    return [int((mate == 0).sum()), int((mate == 1).sum())], skipped, bad


def _as_chunks(chunks):
    return [chunks] if isinstance(chunks, Chunk) else chunks


def bam_reads_host(chunks, max_len=MAX_LEN):
    """The numpy twin of the device path (iss_br_feed / iss_br_download): the same words and the same bad-record rules.  chunks: a
    bam.Chunk (data: the bytes of whole records, offsets: their block_size fields) or an iterable of them -- the feeds.  Returns a
    dict: ``tally`` (the flat uint64 device words at max_len), ``records`` (good records taken, [2]), ``skipped`` [2],
    ``bad_record`` (index over all records fed; -1: none), ``bad_code``."""
    max_len = int(max_len)
    if not 1 <= max_len <= MAX_LEN:
        raise ValueError("max_len outside 1 .. %d" % MAX_LEN)
    words = np.zeros(fq_words(max_len), dtype=np.uint64)
    t = split_fq_words(words, max_len)
    records, skipped, bad_record, bad_code, fed = [0, 0], [0, 0], -1, 0, 0
    for chunk in _as_chunks(chunks):
        if not len(chunk.offsets):
            continue
        n, s, bad = _tally_chunk(chunk, max_len, t)
        records = [records[0] + n[0], records[1] + n[1]]
        skipped = [skipped[0] + s[0], skipped[1] + s[1]]
        if bad is not None and bad_record < 0:
            bad_record, bad_code = fed + bad[0], bad[1]
        fed += len(chunk.offsets)
    return {"tally": words, "records": records, "skipped": skipped, "bad_record": bad_record, "bad_code": bad_code}


def bam_to_fastq(chunks, max_len=MAX_LEN):
    """(R1 text, R2 text): the taken, good records of the chunks as FASTQ, each read as sequenced -- mate 0 in the first text, mate
    1 in the second.  fastq_tally_host of the two texts is the twin's tally in every field but ``insert``.  One record at a time, in
    plain Python: what the words mean, written a second way."""
    comp = bytes.maketrans(b"=ACMGRSVTWYHKDBN", bytes(SEQ_LETTERS[_COMPLEMENT]))
    out = ([], [])
    for chunk in _as_chunks(chunks):
        if not len(chunk.offsets):
            continue
        data = bytes(chunk.data)
        c = _classify(chunk, int(max_len))
        for r in np.flatnonzero((c["code"] == 0) & (c["mate"] >= 0)):
            o, n, seq, qual = int(chunk.offsets[r]), int(c["len"][r]), int(c["seq"][r]), int(c["qual"][r])
            name = data[o + 36:seq].split(b"\0", 1)[0]
            letters = "".join("=ACMGRSVTWYHKDBN"[(data[seq + k // 2] >> (0 if k & 1 else 4)) & 15] for k in range(n)).encode()
            quals = bytes(x + 33 for x in data[qual:qual + n])
            if c["reverse"][r]:
                letters, quals = letters.translate(comp)[::-1], quals[::-1]
            out[int(c["mate"][r])].append(b"@" + name + b"\n" + letters + b"\n+\n" + quals + b"\n")
    return b"".join(out[0]), b"".join(out[1])


def finish(raw, max_len):
    """A download (or the twin's dict) as BamReadTally.result() returns it: fastq_report.finish's keys and ``skipped``."""
    res = _finish(dict(raw, records=list(raw["records"]), bad_record=[raw["bad_record"]], bad_code=[raw["bad_code"]]), max_len)
    res.update(bad_record=int(raw["bad_record"]), bad_code=int(raw["bad_code"]), skipped=list(raw["skipped"]))
    return res


class BamReadTally(_native.Session):
    """Device tallies of the reads of BAM files (iss_br_*): feed chunks or files, download the result."""

    PREFIX = "iss_br"

    def __init__(self, device=0, max_len=MAX_LEN, errors=False, depth=False, depth_flags=0, min_mapq=0):
        """``errors``: also tally the alignments' errors (bam_errors.py; iss_br_errors_enable) -- download() and result() then
        hold ``errors``, ``error_counts``, ``bad_alignment`` and ``bad_alignment_code`` as well.  ``depth``: also mark the
        alignments' reference intervals into a difference array on the device (bam_depth.py; iss_br_depth_enable) with
        ``depth_flags`` (bam_depth.COUNT_DEL) and ``min_mapq`` -- feed_file() takes the references from the file's header, feed()
        needs set_depth_table() first, and depth_result() finishes.  download() and result() do not change with it."""
        self.max_len = int(max_len)
        self.errors = bool(errors)
        self.depth = bool(depth)
        self.depth_flags, self.min_mapq = int(depth_flags), int(min_mapq)
        self.references = None  # the (name, length) list the accumulator was laid out for
        self._depth_table = self._d_table = self._d_diff = None
        if self.depth:
            from .tensors import _torch

            self._torch = _torch()  # (the accumulator is torch tensors: torch's HIP runtime has to be the process's first)
        _native.Session.__init__(self, device, self.max_len)
        try:
            if self.depth:
                _native.need(self._lib, "br_depth")
            if self.errors:
                _native.need(self._lib, "br_errors")
                self._check(self._lib.iss_br_errors_enable(self._h))
        except (_native.NativeLibraryError, _native.EngineError):
            self.close()
            raise

    def feed(self, chunk):
        """One bam.Chunk of whole records; its arrays are free again when the call returns."""
        data = np.ascontiguousarray(np.frombuffer(chunk.data, dtype=np.uint8))
        offs = np.ascontiguousarray(chunk.offsets, dtype=np.int64)
        self._check(self._lib.iss_br_feed(self._h, data.ctypes.data if data.size else None, data.size,
                                          offs.ctypes.data if offs.size else None, offs.size))

    def feed_file(self, path, inflater=None, chunk_bytes=64 << 20, threads=None):
        """Every record of a BAM file; ``inflater``: an inflate.BgzfInflater for its BGZF blocks (None: the host pool).  With
        ``depth`` the file's references lay out the accumulator (a file without records too); a further file has to carry the
        same references."""
        reader = BamReader(path, chunk_bytes, threads, inflater)
        first = self.depth
        for chunk in reader.chunks():
            if first:
                self.set_depth_table(reader.references)
                first = False
            self.feed(chunk)
        if first:
            self.set_depth_table(reader.references)

    def set_depth_table(self, references):
        """The (name, length) list of the references the records' refID index: lays out depth.depth_table of the lengths, allocates
        and zeroes the accumulator on the device and enables the stage.  Before the first feed; the same list again changes
        nothing, another one is an EngineError."""
        if not self.depth:
            raise _native.EngineError(_native.E_INVALID, "set_depth_table: the context was made without depth=True")
        references = [(str(name), int(length)) for name, length in references]
        if self.references is not None:
            if references != self.references:
                raise _native.EngineError(_native.E_INVALID, "the BAM files fed into one depth accumulator differ in their references")
            return
        if not references:
            raise _native.EngineError(_native.E_INVALID, "no references in the BAM header: nothing to lay the depth out on")
        from .depth import depth_table

        torch = self._torch
        table, n_words = depth_table([length for _name, length in references])
        with torch.cuda.device(self.device):
            dev = torch.device("cuda", self.device)
            self._d_table = torch.from_numpy(table).to(dev)
            self._d_diff = torch.zeros(n_words, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()  # (made on torch's stream; the context works on its own)
        self._check(self._lib.iss_br_depth_enable(self._h, C.c_void_p(self._d_table.data_ptr()), table.shape[0],
                                                  C.c_void_p(self._d_diff.data_ptr()), self.depth_flags, self.min_mapq))
        self.references, self._depth_table = references, table

    def reset(self):
        """iss_br_reset; with ``depth`` the accumulator (this object's) is zeroed too, the table and the stage stay."""
        _native.Session.reset(self)
        if self._d_diff is not None:
            with self._torch.cuda.device(self.device):
                self._d_diff.zero_()
                self._torch.cuda.synchronize()

    def depth_download(self):
        """Waits for everything fed -> ``depth_counts`` (bam_depth.COUNT_NAMES), ``bad_depth_record`` (-1: none), ``bad_depth_code``."""
        if self.references is None:
            raise _native.EngineError(_native.E_INVALID, "depth: no table yet (feed_file or set_depth_table first)")
        counts, bad, code = (C.c_int64 * 6)(), C.c_int64(), C.c_int32()
        self._check(self._lib.iss_br_depth_download(self._h, C.addressof(counts), C.byref(bad), C.byref(code)))
        return {"depth_counts": list(counts), "bad_depth_record": bad.value, "bad_depth_code": code.value}

    def depth_diff(self):
        """The difference array as it stands, downloaded (int32; waits for everything fed)."""
        self.depth_download()
        return self._d_diff.cpu().numpy()

    def depth_result(self, bin=0):
        """The stage downloaded, then its accumulator finished on the device through a bare ReadEngine (depth_finish): ``stats``
        uint64 [n, 4] (depth.STATS_FIELDS), ``bins`` (uint64 window sums, None without ``bin``), ``table``, ``ids``,
        ``depth_counts``, ``bad_depth_record``, ``bad_depth_code``.  The accumulator stays as it is: more may be fed."""
        from .depth import n_windows
        from .engine import ReadEngine

        out = self.depth_download()  # (the wait that orders the engine's stream behind the feeds)
        torch, table, n = self._torch, self._depth_table, len(self.references)
        n_bins = int(n_windows(table, bin).sum())
        with ReadEngine(self.device) as eng, torch.cuda.device(self.device):
            dev = torch.device("cuda", self.device)
            d_stats = torch.empty((n, 4), dtype=torch.int64, device=dev)
            d_bins = torch.empty(max(n_bins, 1), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            eng.depth_finish(self._d_diff.data_ptr(), self._d_diff.numel(), None, self._d_table.data_ptr(), n, int(bin), d_stats.data_ptr(),
                             d_bins.data_ptr() if n_bins else None)
            eng.synchronize()
            stats = d_stats.cpu().numpy().view(np.uint64)
            bins = d_bins.cpu().numpy().view(np.uint64)[:n_bins] if int(bin) > 0 else None
        out.update(stats=stats, bins=bins, table=table.copy(), ids=[name for name, _length in self.references])
        return out

    def download(self):
        """The twin's dict from the device: ``tally`` at max_len, ``records``, ``skipped``, ``bad_record``, ``bad_code``."""
        words = np.zeros(fq_words(self.max_len), dtype=np.uint64)
        assert self._lib.iss_br_tally_words(self._h) == words.size
        rec, skip, bad, code = (C.c_int64 * 2)(), (C.c_int64 * 2)(), C.c_int64(), C.c_int32()
        self._check(self._lib.iss_br_download(self._h, words.ctypes.data, C.addressof(rec), C.addressof(skip), C.byref(bad), C.byref(code)))
        out = {"tally": words, "records": list(rec), "skipped": list(skip), "bad_record": bad.value, "bad_code": code.value}
        if self.errors:
            from .bam_errors import words as error_words

            err = np.zeros(error_words(self.max_len), dtype=np.uint64)
            assert self._lib.iss_br_error_words(self._h) == err.size
            counts = (C.c_int64 * 4)()
            self._check(self._lib.iss_br_errors_download(self._h, err.ctypes.data, C.addressof(counts), C.byref(bad), C.byref(code)))
            out.update(errors=err, error_counts=list(counts), bad_alignment=bad.value, bad_alignment_code=code.value)
        return out

    def result(self):
        """``tally``: tally.py's flat words re-laid to L = the longest read seen (interchangeable with `generate --report`'s
        _tally.npy), ``read_length`` L, ``lengths`` [2][L + 1], ``records`` [2], ``skipped`` [2], ``bad_record``, ``bad_code``;
        with errors enabled also ``errors`` (bam_errors.layout's words re-laid to L), ``error_counts`` [4], ``bad_alignment`` and
        ``bad_alignment_code``."""
        raw = self.download()
        res = finish(raw, self.max_len)
        if self.errors:
            from .bam_errors import relayout

            res.update(errors=relayout(raw["errors"], self.max_len, res["read_length"]), error_counts=list(raw["error_counts"]),
                       bad_alignment=int(raw["bad_alignment"]), bad_alignment_code=int(raw["bad_alignment_code"]))
        return res


__all__ = ["MAX_LEN", "REC_SHORT", "REC_TOO_LONG", "REC_NO_QUAL", "REC_QUAL_RANGE", "bam_reads_host", "bam_to_fastq", "finish",
           "BamReadTally"]
