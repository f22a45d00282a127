"""`model`: a KDE error model from a BAM file, the reference's `iss model` (iss/app.py:147-169 -> iss/bam.py:103-227, iss/modeller.py).

The per-read work runs on the GPU (engine.BamTally: integer tallies of substitutions, indels, qualities per (mate, mean-quality bin,
position) and template lengths; the quality and insert-size KDE CDFs from those tallies).  This module drives it over the chunks of
bam.BamReader and finishes on the host with the reference's own numpy operations: the substitution and indel choices, the read
length, the ``.npz`` in the reference's schema (bam.py:49-100), readable by the reference's ``iss generate -m`` and by this
project's KDErrorModel / DenseModel.from_reference_npz.

Parity: read counts per bin, read_length, the substitution and indel tables are exact; the quality and
insert-size CDFs agree with scipy's gaussian_kde within 1e-12; with more than ``n_reads`` mapped records the subsample equals the
reference's in distribution only (bam.Subsample).
"""
import contextlib
import os
import time

import numpy as np

from . import _native
from .bam import DEFAULT_N_READS, BamError, BamReader, Subsample, mapped_mask

N_BINS = 4
SUBST_GROUPS = (("A", 1, ["T", "C", "G"]), ("T", 5, ["A", "C", "G"]), ("C", 9, ["A", "T", "G"]), ("G", 13, ["A", "T", "C"]))


def unpack_tallies(t):
    """The flat u64 tally words of iss_bam_tally_download as named arrays."""
    M = _native.BAM_MAX_LEN
    return dict(
        subst=t[:_native.BAM_OFF_INDEL].reshape(2, M, 16),
        indel=t[_native.BAM_OFF_INDEL:_native.BAM_OFF_QHIST].reshape(2, M, 9),
        qhist=t[_native.BAM_OFF_QHIST:_native.BAM_OFF_TLEN].reshape(2, N_BINS, M, _native.BAM_NQ),
        tlen=t[_native.BAM_OFF_TLEN:_native.BAM_OFF_NREAD],
        nread=t[_native.BAM_OFF_NREAD:_native.BAM_OFF_MINLEN].reshape(2, N_BINS),
        minlen=t[_native.BAM_OFF_MINLEN:_native.BAM_OFF_TAKEN].reshape(2, N_BINS),
        taken=int(t[_native.BAM_OFF_TAKEN]),
    )


def subst_matrix_to_choices(matrix, read_length):
    """Per position, for each reference base: (the three other letters, their probabilities).  A base never seen substituted at a
    position gets 1/3 each -- the division 0/0 raises under np.errstate(all="raise") like in iss/modeller.py:183-259."""
    out = []
    for pos in range(read_length):
        row = matrix[pos]
        choice = {}
        for base, col, letters in SUBST_GROUPS:
            counts = row[col:col + 3]
            total = np.sum(counts)
            with np.errstate(all="raise"):
                try:
                    probs = [c / total for c in counts]
                except FloatingPointError:
                    probs = [1 / 3, 1 / 3, 1 / 3]
            choice[base] = (letters, probs)
        out.append(choice)
    return out


def indel_matrix_to_choices(matrix, read_length):
    """Insertion and deletion rates per position: counts over column 0 (the bases seen there), NaN and inf kept (modeller.py:318-358)."""
    ins, dele = [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for pos in range(read_length):
            row = matrix[pos]
            ins.append({b: row[k] / row[0] for b, k in zip("ATCG", (1, 2, 3, 4))})
            dele.append({b: row[k] / row[0] for b, k in zip("ATCG", (5, 6, 7, 8))})
    return ins, dele


def read_length_of(nread, minlen):
    """min over both mates of the per-mate read length: the shortest read of each bin holding more than one read (its CDF list is
    that long, zip(*) truncates), counting lists longer than one position (bam.py:184-189)."""
    lengths = []
    for mate in range(2):
        ls = [int(minlen[mate][b]) for b in range(N_BINS) if nread[mate][b] > 1 and int(minlen[mate][b]) > 1]
        if not ls:
            raise BamError("no mean-quality bin of read%d holds two reads or more" % (mate + 1))
        lengths.append(min(ls))
    return min(lengths)


def insert_size_ok(tlen, read_length):
    """The reference's insert_size() needs two template lengths or more in (0, 2000) with a spread (else scipy fails)."""
    nz = np.flatnonzero(tlen)
    if nz.size == 0:
        raise BamError("no paired reads with 0 < |template length| < 2000")
    if int(tlen.sum()) < 2 or nz.size < 2:
        raise BamError("the template lengths of the paired reads have no spread")


def finish(t, qcdf, isize_cdf, read_length):
    """The model's fields (bam.py:172-227) from the tallies and the device CDFs."""
    hists, means = [], []
    for mate in range(2):
        means.append([int(n) for n in t["nread"][mate]])
        hists.append([[qcdf[mate, b, p].copy() for p in range(int(t["minlen"][mate][b]))] if t["nread"][mate][b] > 1 else []
                      for b in range(N_BINS)])
    fields = dict(read_length=read_length, insert_size=isize_cdf, mean_f=means[0], mean_r=means[1], hist_f=hists[0], hist_r=hists[1])
    for mate, tag in ((0, "f"), (1, "r")):
        subst = t["subst"][mate].astype(np.float64)
        indel = t["indel"][mate].astype(np.float64)
        subst.resize([read_length, 16], refcheck=False)  # rows past read_length go, incl. the wrapped rows of negative positions
        indel.resize([read_length, 9], refcheck=False)
        for pos in range(read_length):
            indel[pos][0] = sum(subst[pos][::4])
        fields["sub_" + tag] = subst_matrix_to_choices(subst, read_length)
        fields["ins_" + tag], fields["del_" + tag] = indel_matrix_to_choices(indel, read_length)
    return fields


def write_npz(path, f):
    """np.savez_compressed with the reference's keys, in its order (bam.py:82-98)."""
    np.savez_compressed(
        path, model="kde", read_length=f["read_length"], insert_size=f["insert_size"], mean_count_forward=f["mean_f"],
        mean_count_reverse=f["mean_r"], quality_hist_forward=np.array(f["hist_f"], dtype=object),
        quality_hist_reverse=np.array(f["hist_r"], dtype=object), subst_choices_forward=f["sub_f"], subst_choices_reverse=f["sub_r"],
        ins_forward=f["ins_f"], ins_reverse=f["ins_r"], del_forward=f["del_f"], del_reverse=f["del_r"])


def tally_bam(dev, bam_path, n_reads=DEFAULT_N_READS, seed=0, chunk_bytes=64 << 20, threads=None, timings=None, inflater=None):
    """Tally the records read_bam(bam_path, n_reads) would yield (iss/bam.py:14-46) on the BamTally `dev`.

    One pass tallies every mapped record while counting them: that is the result whenever n_reads >= the mapped count (a fraction
    of 1 or more takes every mapped record).  Otherwise a second pass tallies the subsample.  Returns the mapped count.
    ``inflater``: an inflate.BgzfInflater for the BGZF blocks (None: the host pool)."""
    timings = timings if timings is not None else {}

    def run(select_of, stopped=lambda: False):
        reader = BamReader(bam_path, chunk_bytes, threads, inflater)
        for ch in reader.chunks():
            sel = select_of(mapped_mask(ch))
            t0 = time.perf_counter()
            dev.feed(ch.data, ch.offsets, sel)
            timings["tally"] = timings.get("tally", 0.0) + time.perf_counter() - t0
            if stopped():  # the reference's `break`: nothing after this record is read
                break
        for k, v in reader.timings.items():
            timings[k] = timings.get(k, 0.0) + v

    total = [0]

    def count_all(mapped):
        total[0] += int(mapped.sum())
        return mapped.astype(np.uint8)

    dev.reset()
    run(count_all)
    if total[0] == 0:
        raise BamError("no mapped reads in the BAM file")
    if n_reads < total[0]:
        dev.reset()
        sub = Subsample(total[0], n_reads, seed)
        run(sub.select, lambda: sub.stopped)
    return total[0]


def device_inflater(device, wanted=None):
    """What inflates the BGZF blocks of `model`, as a context manager: None -- the host pool of zlib threads, the default, because
    end to end it is the faster route for `model` (Measured) -- or a BgzfInflater on the device when
    ``wanted`` (None: ISS_DEVICE_INFLATE=1 in the environment).  ISS_HOST_INFLATE=1 keeps the host route whatever else is said."""
    if wanted is None:
        wanted = os.environ.get("ISS_DEVICE_INFLATE", "") == "1"
    if not wanted or os.environ.get("ISS_HOST_INFLATE", "") == "1":
        return contextlib.nullcontext(None)
    from .inflate import BgzfInflater

    return BgzfInflater(device)


def to_model(bam_path, output, n_reads=DEFAULT_N_READS, seed=0, device=0, dense=False, chunk_bytes=64 << 20, threads=None,
             timings=None, device_inflate=None):
    """Write ``output + ".npz"`` (and ``output + ".dense.npz"`` when dense) from bam_path.  Raises BamError on input the reference
    fails on; returns the output path.  ``device_inflate``: inflate the BGZF blocks on the GPU (None: ISS_DEVICE_INFLATE=1)."""
    from .engine import BamTally

    timings = timings if timings is not None else {}
    next(iter(BamReader(bam_path, 1 << 16, 1).chunks()), None)  # not a BAM file: fail before the GPU is opened
    with BamTally(device) as dev, device_inflater(device, device_inflate) as inflater:
        tally_bam(dev, bam_path, n_reads, seed, chunk_bytes, threads, timings, inflater)
        words, bad, code = dev.tallies()
        if bad >= 0:
            raise BamError("record %d: %s" % (bad + 1, _native.BAM_REC_ERRORS.get(code, "error %d" % code)))
        t = unpack_tallies(words)
        read_length = read_length_of(t["nread"], t["minlen"])
        insert_size_ok(t["tlen"], read_length)
        t0 = time.perf_counter()
        qcdf, isize_cdf = dev.kde(read_length)
        timings["kde"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    path = output + ".npz"
    write_npz(path, finish(t, qcdf, isize_cdf, read_length))
    if dense:
        from .model import DenseModel

        DenseModel.from_reference_npz(path).save(output + ".dense.npz")
    timings["write"] = time.perf_counter() - t0
    return path
