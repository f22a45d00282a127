"""`report`: the --report tallies of existing FASTQ files (include/iss_mi355x.h: iss_fq_*; k_fq_* of csrc/iss_fqtally.hip.h), their
numpy twin, the host side of the chunk contract and the comparison of two tallies.  numpy only, besides the binding.

The device words are tally.py's layout at L = max_len and one field behind it:

    pairs [1] | qual [2][L][94] | base [2][L][5] | gc [2][L + 1] | meanq [2][94] | insert [2048] | length [2][L + 1]

R1's file is mate 0, R2's mate 1; the phred is the quality byte - 33; qual and base count positions 0 .. len - 1 of a read of length
len, meanq is floor(sum of phreds / len) of the read's own length, a read of length 0 counts in length[mate][0] and gc[mate][0] alone,
pairs counts the good records of mate 0 and insert stays zero.  A record is four lines found by line number; a bad record (REC_*:
the smallest code that applies) is not tallied, the records after it are, and the first bad one per mate is reported.
DESIGN.md section 24."""
import ctypes as C
import gzip
import os

import numpy as np

from . import _native
from .tally import FIELDS, INSERT_BINS, PHREDS, _CODE_TABLE, _GC_TABLE, split_tally, tally_layout, tally_words

MAX_LEN = _native.FQ_MAX_LEN
REC_NO_AT, REC_NO_PLUS, REC_LENGTHS, REC_TOO_LONG, REC_QUAL_RANGE, REC_TRUNCATED = 1, 2, 3, 4, 5, 6
GC_BINS = 101  # compare_tallies: GC as a fraction of the read length, floor(100 * gc / L)


def fq_words(max_len):
    """Words of the device tally (iss_fq_tally_words)."""
    return tally_words(max_len) + 2 * (int(max_len) + 1)


def split_fq_words(words, max_len):
    """The flat device words as a dict of views: tally.py's fields and ``length`` [2][max_len + 1]."""
    words = np.asarray(words)
    n = tally_words(max_len)
    if words.ndim != 1 or words.shape[0] != fq_words(max_len):
        raise ValueError("a FASTQ tally of max_len %d has %d words, not %r" % (int(max_len), fq_words(max_len), words.shape))
    out = split_tally(words[:n], max_len)
    out["length"] = words[n:].reshape(2, int(max_len) + 1)
    return out


def relayout(words, max_len, L):
    """The device words at max_len -> (tally.py's flat words at read length L, lengths [2][L + 1]); L: at least the longest read
    counted, so that nothing is cut off."""
    src = split_fq_words(words, max_len)
    L = int(L)
    if not 1 <= L <= int(max_len):
        raise ValueError("read length %d outside 1 .. %d" % (L, int(max_len)))
    if src["length"][:, L + 1:].any():
        raise ValueError("reads longer than %d were counted" % L)
    out = np.zeros(tally_words(L), dtype=np.uint64)
    dst = split_tally(out, L)
    dst["pairs"][:] = src["pairs"]
    dst["qual"][:] = src["qual"][:, :L]
    dst["base"][:] = src["base"][:, :L]
    dst["gc"][:] = src["gc"][:, :L + 1]
    dst["meanq"][:] = src["meanq"]
    dst["insert"][:] = src["insert"]
    return out, np.array(src["length"][:, :L + 1], dtype=np.uint64)


def longest_read(words, max_len):
    """The longest read counted in either mate (1 at least: a layout needs a position)."""
    nz = np.flatnonzero(split_fq_words(words, max_len)["length"].sum(axis=0))
    return max(1, int(nz[-1])) if nz.size else 1


def _tally_chunk(chunk, mate, max_len, t, first_rec):
    """One feed of the twin: adds the chunk's good records to the views t; (whole records, first bad (index, code) or None)."""
    a = np.frombuffer(chunk, dtype=np.uint8)
    nl = np.flatnonzero(a == 10)
    n_rec = nl.size // 4
    bad = None
    if nl.size % 4 or (a.size and a[-1] != 10):
        bad = (first_rec + n_rec, REC_TRUNCATED)
    if not n_rec:
        return 0, bad
    start = np.concatenate(([0], nl[:4 * n_rec - 1] + 1)).reshape(n_rec, 4)
    end = nl[:4 * n_rec].reshape(n_rec, 4).copy()  # the '\n'; one '\r' directly before it is the terminator's
    end -= (end > start) & (a[np.maximum(end, 1) - 1] == 13)
    ln = end - start
    code = np.zeros(n_rec, dtype=np.int64)
    code[ln[:, 1] > max_len] = REC_TOO_LONG
    code[ln[:, 1] != ln[:, 3]] = REC_LENGTHS
    code[(ln[:, 2] == 0) | (a[np.minimum(start[:, 2], a.size - 1)] != ord("+"))] = REC_NO_PLUS
    code[(ln[:, 0] == 0) | (a[np.minimum(start[:, 0], a.size - 1)] != ord("@"))] = REC_NO_AT
    ok = np.flatnonzero(code == 0)
    length = ln[ok, 1]
    rec = np.repeat(np.arange(ok.size), length)                      # every base of the records that stand so far:
    pos = np.arange(rec.size) - np.repeat(np.cumsum(length) - length, length)  # its record (index into ok) and position
    q = a[start[ok, 3][rec] + pos].astype(np.int64)
    out_of_range = np.bincount(rec, weights=(q < 33) | (q > 126), minlength=ok.size) > 0
    code[ok[out_of_range]] = REC_QUAL_RANGE
    first_bad = np.flatnonzero(code)
    if first_bad.size:  # (within a chunk it stands before the TRUNCATED record)
        bad = (first_rec + int(first_bad[0]), int(code[first_bad[0]]))
    keep = ~out_of_range[rec]
    rec, pos, q = rec[keep], pos[keep], q[keep] - 33
    b = a[start[ok, 1][rec] + pos]
    good = np.flatnonzero(~out_of_range)
    length = length[good]
    L = int(max_len)
    t["qual"][mate] += np.bincount(pos * PHREDS + q, minlength=L * PHREDS).reshape(L, PHREDS).astype(np.uint64)
    t["base"][mate] += np.bincount(pos * 5 + _CODE_TABLE[b], minlength=L * 5).reshape(L, 5).astype(np.uint64)
    gc = np.bincount(rec, weights=_GC_TABLE[b], minlength=ok.size).astype(np.int64)[good]
    t["gc"][mate] += np.bincount(gc, minlength=L + 1).astype(np.uint64)
    qsum = np.bincount(rec, weights=q, minlength=ok.size).astype(np.int64)[good]  # (float64 sums of small integers: exact)
    some = length > 0
    t["meanq"][mate] += np.bincount(np.minimum(qsum[some] // length[some], PHREDS - 1), minlength=PHREDS).astype(np.uint64)
    t["length"][mate] += np.bincount(length, minlength=L + 1).astype(np.uint64)
    if mate == 0:
        t["pairs"][0] += np.uint64(good.size)
    return n_rec, bad


def fastq_tally_host(text_r1, text_r2=None, max_len=MAX_LEN):
    """The numpy twin of the device path (iss_fq_feed / iss_fq_download): the same words and the same bad-record rules.  text_r1,
    text_r2: the FASTQ text of a mate as bytes, or a sequence of bytes -- the feeds, each holding whole records (split_chunks makes
    them; what is not whole is TRUNCATED as on the device).  Returns a dict: ``tally`` (the flat uint64 device words at max_len),
    ``records``, ``bad_record`` (-1: none), ``bad_code``, each [2]."""
    max_len = int(max_len)
    if not 1 <= max_len <= MAX_LEN:
        raise ValueError("max_len outside 1 .. %d" % MAX_LEN)
    words = np.zeros(fq_words(max_len), dtype=np.uint64)
    t = split_fq_words(words, max_len)
    records, bad_record, bad_code = [0, 0], [-1, -1], [0, 0]
    for mate, text in enumerate((text_r1, text_r2)):
        if text is None:
            continue
        for chunk in ([text] if isinstance(text, (bytes, bytearray, memoryview)) else text):
            if not len(chunk):
                continue
            n, bad = _tally_chunk(chunk, mate, max_len, t, records[mate])
            records[mate] += n
            # (the smallest (index, code): a TRUNCATED record and record 0 of the next feed have the same index)
            if bad is not None and (bad_record[mate] < 0 or bad < (bad_record[mate], bad_code[mate])):
                bad_record[mate], bad_code[mate] = bad
    return {"tally": words, "records": records, "bad_record": bad_record, "bad_code": bad_code}


def _cut(buf, end):
    """Bytes of buf[:end] up to and with the last line whose number (from 1) is a multiple of 4."""
    n = buf.count(b"\n", 0, end)
    if n < 4:
        return 0
    p = buf.rfind(b"\n", 0, end)
    for _ in range(n % 4):
        p = buf.rfind(b"\n", 0, p)
    return p + 1


def _split_views(fh, chunk_bytes):
    """split_chunks without its copies: the chunks as memoryviews of one buffer that is filled again behind each of them -- a view
    is good until the next one is asked for (FastqTally.feed has copied the bytes by then)."""
    chunk_bytes = max(1, int(chunk_bytes))
    buf, have, eof = bytearray(2 * chunk_bytes + 1), 0, False
    while not eof:
        want = have + chunk_bytes
        if want + 1 > len(buf):  # (a tail longer than a chunk: records longer than chunk_bytes)
            buf = buf[:have] + bytearray(want + chunk_bytes + 1 - have)
        with memoryview(buf) as view:
            while have < want:
                n = fh.readinto(view[have:want])
                if not n:
                    eof = True
                    break
                have += n
        if eof and have and buf[have - 1] != 10:  # the missing '\n' at the end of the file
            buf[have] = 10
            have += 1
        cut = _cut(buf, have)
        if cut:
            yield memoryview(buf)[:cut]
        if eof and cut < have:
            yield memoryview(buf)[cut:have]
        buf[:have - cut] = buf[cut:have]  # the tail, carried into the next chunk
        have -= cut


def split_chunks(fh, chunk_bytes):
    """The host side of the chunk contract: reads fh (binary) chunk_bytes at a time and yields bytes that hold whole four-line
    records -- each chunk cut behind its last line whose number is a multiple of 4, the tail carried into the next one, the missing
    '\\n' appended at the end of the file.  What remains after that is yielded last: a TRUNCATED record.  No device round trip: a
    count of the '\\n' bytes and a few searches from the end."""
    for view in _split_views(fh, chunk_bytes):
        yield bytes(view)


def open_fastq(path, device=None):
    """Binary reader of a FASTQ file.  ``.gz``: a file whose first member carries the BGZF ``BC`` subfield (bgzip's) is inflated on the
    GPU ``device`` (inflate.BgzfReader; None, or ISS_HOST_INFLATE=1: on the host); any other gzip goes through gzip.open (many members
    per file, as `generate --compress` writes, read through)."""
    if not str(path).endswith(".gz"):
        return open(path, "rb")
    if device is not None and os.environ.get("ISS_HOST_INFLATE", "") != "1":
        from . import inflate

        if inflate.is_bgzf(path):
            return inflate.BgzfReader(path, device)
    return gzip.open(path, "rb")


class FastqTally(_native.Session):
    """Device tallies of FASTQ files (iss_fq_*): feed files, download the result."""

    PREFIX = "iss_fq"

    def __init__(self, device=0, max_len=MAX_LEN):
        self.max_len = int(max_len)
        _native.Session.__init__(self, device, self.max_len)

    def feed(self, text, mate):
        """One chunk of whole records (bytes, or any buffer) of mate 0 or 1; the bytes are free again when the call returns."""
        a = np.frombuffer(text, dtype=np.uint8)
        self._check(self._lib.iss_fq_feed(self._h, int(mate), a.ctypes.data if a.size else None, a.size))

    def feed_file(self, path, mate, chunk_bytes=64 << 20):
        with open_fastq(path, self.device) as fh:
            for view in _split_views(fh, chunk_bytes):
                self.feed(view, mate)

    def download(self):
        """The twin's dict from the device: ``tally`` at max_len, ``records``, ``bad_record``, ``bad_code``."""
        words = np.zeros(fq_words(self.max_len), dtype=np.uint64)
        assert self._lib.iss_fq_tally_words(self._h) == words.size
        rec, bad, code = (C.c_int64 * 2)(), (C.c_int64 * 2)(), (C.c_int32 * 2)()
        self._check(self._lib.iss_fq_download(self._h, words.ctypes.data, C.addressof(rec), C.addressof(bad), C.addressof(code)))
        return {"tally": words, "records": list(rec), "bad_record": list(bad), "bad_code": list(code)}

    def result(self):
        """``tally``: tally.py's flat words re-laid to L = the longest read seen (interchangeable with `generate --report`'s
        _tally.npy), ``read_length`` L, ``lengths`` [2][L + 1], ``records``, ``bad_record``, ``bad_code`` [2] each."""
        return finish(self.download(), self.max_len)


def finish(raw, max_len):
    """A download (or the twin's dict) as FastqTally.result() returns it."""
    L = longest_read(raw["tally"], max_len)
    words, lengths = relayout(raw["tally"], max_len, L)
    return {"tally": words, "read_length": L, "lengths": lengths, "records": list(raw["records"]),
            "bad_record": list(raw["bad_record"]), "bad_code": list(raw["bad_code"])}


def read_length_of_words(n_words):
    """The read length of a tally.py tally from its word count (None: the count fits no length)."""
    per, const = 2 * PHREDS + 2 * 5 + 2, 1 + 2 + 2 * PHREDS + INSERT_BINS
    L, rest = divmod(int(n_words) - const, per)
    return L if rest == 0 and L >= 1 and tally_layout(L)["words"] == int(n_words) else None


def _tv(a, b):
    """Total-variation distance of two histograms as distributions (None: one of them is empty)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not a.sum() or not b.sum():
        return None
    n = max(a.size, b.size)
    a, b = np.pad(a, (0, n - a.size)), np.pad(b, (0, n - b.size))
    return float(0.5 * np.abs(a / a.sum() - b / b.sum()).sum())


def _gc_fraction_hist(gc, L):
    """Reads by GC count at read length L -> reads by floor(100 * gc / L), 101 bins."""
    return np.bincount(np.arange(L + 1) * 100 // L, weights=np.asarray(gc, dtype=np.float64), minlength=GC_BINS)


def _max_abs(values):
    values = [abs(v) for v in values if v is not None]
    return max(values) if values else None


def compare_tallies(a, La, b, Lb):
    """Two tally.py tallies (flat words, read lengths) side by side, JSON-serialisable: over the first min(La, Lb) positions, per
    mate, ``mean_phred_diff`` (a - b) and ``base_l1`` (L1 distance of the five base fractions), None where either side has no
    read at the position; per mate ``gc_tv`` (total-variation distance of the reads' GC fraction in 101 bins, so that different
    read lengths compare) and ``meanq_tv``; ``insert_tv`` when both have any count, else None; the maxima as ``summary``."""
    ta, tb = split_tally(np.asarray(a, dtype=np.uint64), La), split_tally(np.asarray(b, dtype=np.uint64), Lb)
    P = min(int(La), int(Lb))
    phred = np.arange(PHREDS, dtype=np.float64)
    mates = []
    for m in range(2):
        qa, qb = ta["qual"][m, :P].astype(np.float64), tb["qual"][m, :P].astype(np.float64)
        ba, bb = ta["base"][m, :P].astype(np.float64), tb["base"][m, :P].astype(np.float64)
        diff, l1 = [], []
        for p in range(P):
            na, nb = qa[p].sum(), qb[p].sum()
            diff.append(float((qa[p] * phred).sum() / na - (qb[p] * phred).sum() / nb) if na and nb else None)
            sa, sb = ba[p].sum(), bb[p].sum()
            l1.append(float(np.abs(ba[p] / sa - bb[p] / sb).sum()) if sa and sb else None)
        mates.append({"mean_phred_diff": diff, "base_l1": l1,
                      "gc_tv": _tv(_gc_fraction_hist(ta["gc"][m], int(La)), _gc_fraction_hist(tb["gc"][m], int(Lb))),
                      "meanq_tv": _tv(ta["meanq"][m], tb["meanq"][m])})
    insert_tv = _tv(ta["insert"], tb["insert"])
    summary = {"max_abs_mean_phred_diff": _max_abs([x for m in mates for x in m["mean_phred_diff"]]),
               "max_base_l1": _max_abs([x for m in mates for x in m["base_l1"]]),
               "max_gc_tv": _max_abs([m["gc_tv"] for m in mates]),
               "max_meanq_tv": _max_abs([m["meanq_tv"] for m in mates]),
               "insert_tv": insert_tv}
    return {"positions": P, "read_lengths": [int(La), int(Lb)], "pairs": [int(ta["pairs"][0]), int(tb["pairs"][0])],
            "mates": mates, "insert_tv": insert_tv, "summary": summary}


__all__ = ["MAX_LEN", "GC_BINS", "FIELDS", "fq_words", "split_fq_words", "relayout", "longest_read", "fastq_tally_host", "split_chunks",
           "open_fastq", "FastqTally", "finish", "read_length_of_words", "compare_tallies"]
