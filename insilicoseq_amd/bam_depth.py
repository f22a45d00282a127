"""`report --bam --depth`: where the reads of an aligned BAM fall on its references, as their CIGARs tell it (include/iss_mi355x.h:
iss_br_depth_enable, iss_br_depth_download; k_bd_records of csrc/iss_bamdepth.hip.h) -- the numpy twin of the
device stage, the coverage file `generate --coverage_file` reads, and the comparison of two ``_depth.txt`` tables.  numpy only;
importable without the HIP library.

Definition.  The accumulator is depth.py's: a table int64 [n, 2] of (offset, length), row = refID, and an int32 difference array in
which reference k owns the length + 1 words from its offset on.  A record the read tally took (bam_report: good, mate 0 or 1,
neither secondary nor supplementary) counts once, the first that applies:

    counts[1]  not aligned: 0x4 set, n_cigar_op == 0 or refID < 0
    counts[2]  filtered: 0x200 or 0x400 set
    counts[3]  mapq < min_mapq

-- `samtools depth`'s default filter minus the supplementary records, which the context skips anyway.  Every other record is
validated completely before any word is touched, the first code deciding: DEPTH_CIGAR (an op code above 8), DEPTH_REF (refID >=
the table's rows), DEPTH_SPAN (pos < 0, or pos plus the lengths of M, D, N, =, X past the row's length); between DEPTH_REF and
DEPTH_SPAN a record whose row has offset < 0 adds 1 to counts[4] and marks nothing.  A bad record adds nothing, and the smallest
record index over all records fed is kept with its code.  A valid record adds 1 to counts[0] and is walked with a reference
cursor that starts at pos: M, = and X cover [cursor, cursor + len) and advance; D advances and covers only with COUNT_DEL; N
advances and never covers; I, S, H and P do nothing.  A covered run adds +1 at offset + start, -1 at offset + end and its length
to counts[5]."""
import numpy as np

from .bam_report import MAX_LEN, _COLUMN_OPS, _REF_OPS, _as_chunks, _cigar, _classify

COUNT_DEL = 1
DEPTH_CIGAR, DEPTH_REF, DEPTH_SPAN = 1, 2, 3
COUNT_NAMES = ("marked", "not_aligned", "filtered", "below_min_mapq", "on_skipped_row", "covered_bases")
MAX_RECORDS = (1 << 31) - 1  # records fed into one accumulator at most: a record adds at most 1 to a base


def mark_chunk_host(diff, chunk, table, flags=0, min_mapq=0, max_len=MAX_LEN):
    """The numpy twin of one feed of k_bd_records: the records of ``chunk`` (a bam.Chunk) marked into the int32 difference array
    ``diff``, in place -> (counts int64 [6], index in the chunk of the first bad record or -1, its code or 0).  One record at a
    time, in plain Python: the definition above, nothing of the kernel's shape."""
    table = np.asarray(table, dtype=np.int64).reshape(-1, 2)
    if int(flags) & ~COUNT_DEL:
        raise ValueError("unknown flag bits")
    if not 0 <= int(min_mapq) <= 255:
        raise ValueError("min_mapq outside 0 .. 255")
    counts, bad_record, bad_code = np.zeros(6, dtype=np.int64), -1, 0
    if not len(chunk.offsets):
        return counts, bad_record, bad_code
    a = np.frombuffer(chunk.data, dtype=np.uint8)
    o = np.asarray(chunk.offsets, dtype=np.int64)
    c = _classify(chunk, int(max_len))
    taken = (c["code"] == 0) & (c["mate"] >= 0)
    ref_id, pos, mapq, n_cigar, flag = c["ref_id"], c["pos"], c["mapq"], c["n_cigar"], c["flag"]
    for r in np.flatnonzero(taken).tolist():
        if flag[r] & 4 or not n_cigar[r] or ref_id[r] < 0:
            counts[1] += 1
            continue
        if flag[r] & 0x600:
            counts[2] += 1
            continue
        if mapq[r] < int(min_mapq):
            counts[3] += 1
            continue
        cigar = _cigar(a, o[r], c["l_name"][r], n_cigar[r])
        code = 0
        if any(op > 8 for op, _ in cigar):
            code = DEPTH_CIGAR
        elif ref_id[r] >= table.shape[0]:
            code = DEPTH_REF
        else:
            off, length = table[ref_id[r]].tolist()
            if off < 0:
                counts[4] += 1
                continue
            if pos[r] < 0 or int(pos[r]) + sum(ln for op, ln in cigar if op in _REF_OPS) > length:
                code = DEPTH_SPAN
        if code:
            if bad_record < 0:
                bad_record, bad_code = r, code
            continue
        counts[0] += 1
        cursor = int(pos[r])
        for op, ln in cigar:
            if op in _COLUMN_OPS or (op == 2 and int(flags) & COUNT_DEL):
                diff[off + cursor] += 1
                diff[off + cursor + ln] -= 1
                counts[5] += ln
            if op in _REF_OPS:
                cursor += ln
    return counts, bad_record, bad_code


def mark_host(diff, chunks, table, flags=0, min_mapq=0, max_len=MAX_LEN):
    """mark_chunk_host over the feeds ``chunks`` (a bam.Chunk or an iterable of them) -> a dict: ``depth_counts`` (list of 6),
    ``bad_depth_record`` (index over all records fed; -1: none), ``bad_depth_code``."""
    counts, bad_record, bad_code, fed = np.zeros(6, dtype=np.int64), -1, 0, 0
    for chunk in _as_chunks(chunks):
        n, bad, code = mark_chunk_host(diff, chunk, table, flags, min_mapq, max_len)
        counts += n
        if bad >= 0 and bad_record < 0:
            bad_record, bad_code = fed + bad, code
        fed += len(chunk.offsets)
    return {"depth_counts": [int(x) for x in counts], "bad_depth_record": bad_record, "bad_depth_code": bad_code}


def counts_dict(counts):
    """The six counts under their names: the ``depth`` key of <prefix>_report.json."""
    return {name: int(n) for name, n in zip(COUNT_NAMES, counts)}


# ---------------------------------------------------------------------------------------------------- the coverage file
def coverage_rows(stats, table, ids):
    """(id, mean depth) per row of the table: sum / length, a record of no bases 0.0 (depth.depth_rows' mean)."""
    from .depth import depth_rows

    return [(row[0], row[2]) for row in depth_rows(stats, table, ids)]


def write_coverage_file(path, rows):
    """``<prefix>_coverage.txt``: id<TAB>mean depth per line (floats as repr), what `generate --coverage_file` reads."""
    with open(path, "w") as fh:
        for rid, mean in rows:
            fh.write("%s\t%r\n" % (rid, mean))


# ---------------------------------------------------------------------------------------------------- two depth tables
def read_depth_table(path):
    """``_depth.txt`` as depth.write_depth_table writes it -> {id: (length, mean depth, variance, covered fraction, max)} in file
    order.  ValueError: another header, a line that does not parse, an id twice."""
    from .depth import DEPTH_HEADER

    rows = {}
    with open(path) as fh:
        if fh.readline() != DEPTH_HEADER:
            raise ValueError("not a _depth.txt table (its first line is not the header)")
        for n, line in enumerate(fh, 2):
            f = line.rstrip("\n").split("\t")
            if len(f) != 6:
                raise ValueError("line %d: %d fields, not 6" % (n, len(f)))
            if f[0] in rows:
                raise ValueError("line %d: id %s twice" % (n, f[0]))
            rows[f[0]] = (int(f[1]), float(f[2]), float(f[3]), float(f[4]), int(f[5]))
    return rows


def compare_depth_tables(mine, other):
    """Two read_depth_table dicts -> the dict of <prefix>_depth_compare.json: per id present in both the differences (mine - other)
    of mean depth and of covered fraction, their largest absolute values, the total-variation distance between the two mean-depth
    vectors over the shared ids, each normalised to sum 1 (None when either sums to 0), and the ids only one table holds."""
    shared = [rid for rid in mine if rid in other]
    records = {rid: {"mean_depth": mine[rid][1] - other[rid][1], "covered_fraction": mine[rid][3] - other[rid][3]} for rid in shared}
    a = np.array([mine[rid][1] for rid in shared], dtype=np.float64)
    b = np.array([other[rid][1] for rid in shared], dtype=np.float64)
    tv = None
    if shared and a.sum() > 0 and b.sum() > 0:
        tv = float(0.5 * np.abs(a / a.sum() - b / b.sum()).sum())
    return {
        "records": records,
        "summary": {"max_abs_mean_depth": max([abs(v["mean_depth"]) for v in records.values()] or [0.0]),
                    "max_abs_covered_fraction": max([abs(v["covered_fraction"]) for v in records.values()] or [0.0]),
                    "total_variation_mean_depth": tv},
        "only_here": [rid for rid in mine if rid not in other],
        "only_there": [rid for rid in other if rid not in mine],
    }


__all__ = ["COUNT_DEL", "DEPTH_CIGAR", "DEPTH_REF", "DEPTH_SPAN", "COUNT_NAMES", "MAX_RECORDS", "mark_chunk_host", "mark_host",
           "counts_dict", "coverage_rows", "write_coverage_file", "read_depth_table", "compare_depth_tables"]
