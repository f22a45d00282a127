"""Per-base coverage depth of the generated reads (include/iss_mi355x.h: iss_depth_mark, iss_depth_finish; DESIGN.md section
19): the layout of the accumulator, numpy twins of the device kernels, the merge of the workers' accumulators and the tables
`generate --depth` writes.  numpy only; importable without the HIP library.

Definition.  A pair with coordinates (fs, rs, re, isz) -- ReadEngine.coords -- on a record of ``length`` bases covers the
half-open intervals [fs, fs + read_length) and [rs, re), each clamped to [0, length] (a clamp, not Python's negative-index wrap;
it only bites with custom fragment lengths) and empty when that leaves start >= end.  The depth of a base is the number of such
intervals over it: the nominal depth of the template intervals, whatever indels did to the reads cut from them.

Accumulator.  A record table is int64 [n, 2] of (offset, length); record k owns the length + 1 int32 words [offset, offset +
length] of a difference array, the last one its sink.  An interval adds +1 at offset + start and -1 at offset + end.  Every
record's words sum to zero, so one plain inclusive prefix sum over the whole array is the depth of all records at once, and the
array is additive over calls, batches, workers and GPUs."""
import numpy as np

MAX_MARKED_PAIRS = 1 << 30  # pairs marked into one accumulator at most: a pair adds at most 2 to a base, a depth stays below 2^31
STATS_FIELDS = ("sum", "sum_squares", "covered", "max")


def depth_table(lengths):
    """Records of ``lengths`` bases back to back, each followed by its sink -> (table int64 [n, 2] of (offset, length), n_words)."""
    lengths = np.asarray(list(lengths), dtype=np.int64).reshape(-1)
    if (lengths < 0).any():
        raise ValueError("negative record length")
    table = np.zeros((lengths.shape[0], 2), dtype=np.int64)
    table[:, 1] = lengths
    table[1:, 0] = np.cumsum(lengths[:-1] + 1)
    return table, int((lengths + 1).sum())


def count_marked(marked, n_pairs):
    """The host's count of the pairs marked into one accumulator, with the bound that keeps a depth below 2^31."""
    from ._native import EngineError, E_INVALID

    total = int(marked) + int(n_pairs)
    if total > MAX_MARKED_PAIRS:
        raise EngineError(E_INVALID, "depth: more than 2^30 pairs marked into one accumulator (a base's depth has to stay below 2^31)")
    return total


def clamped_intervals(coords, lengths, read_length):
    """(start, end) int64 [n, 2] each -- column 0 the forward, column 1 the reverse interval -- of pairs with ``coords`` [n, 4]
    on records of ``lengths`` [n] bases, clamped; an empty interval has start >= end."""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 4)
    ln = np.broadcast_to(np.asarray(lengths, dtype=np.int64), (c.shape[0],))
    start = np.stack([c[:, 0], c[:, 1]], axis=1)
    end = np.stack([c[:, 0] + int(read_length), c[:, 2]], axis=1)
    return np.minimum(np.maximum(start, 0), ln[:, None]), np.minimum(np.maximum(end, 0), ln[:, None])


def mark_host(diff, coords, item, table, read_length):
    """The numpy twin of k_depth_mark: add the intervals of pairs with ``coords`` [n, 4] and work items ``item`` [n] (an index
    into ``table``; a scalar serves all pairs) to the int32 difference array ``diff``, in place.  Rows of the table with offset
    < 0: their pairs are skipped."""
    table = np.asarray(table, dtype=np.int64).reshape(-1, 2)
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 4)
    it = np.broadcast_to(np.asarray(item, dtype=np.int64), (c.shape[0],))
    off, ln = table[it, 0], table[it, 1]
    s, e = clamped_intervals(c, ln, read_length)
    keep = (s < e) & (off >= 0)[:, None]
    np.add.at(diff, (off[:, None] + s)[keep], 1)
    np.subtract.at(diff, (off[:, None] + e)[keep], 1)
    return diff


def n_windows(table, bin):
    """Windows of ``bin`` bases each row of the table owns in the ``bins`` array of finish (a record's last window may be short)."""
    ln = np.maximum(np.asarray(table, dtype=np.int64).reshape(-1, 2)[:, 1], 0)
    return -(-ln // int(bin)) if int(bin) > 0 else np.zeros_like(ln)


def finish_host(diff, table, bin=0):
    """The numpy twin of iss_depth_finish -> (depth uint32 [n_words], stats uint64 [n, 4], bins uint64 [windows] or None):
    depth is the inclusive prefix sum of ``diff``; stats per row of the table over its bases (the sink left out) -- sum, sum of
    squares, bases with depth > 0, maximum; bins the sum of depth over every ``bin``-base window of every row, rows in table
    order.  A row with offset < 0 is skipped: zero statistics, zero windows (it keeps its windows in the layout)."""
    diff = np.asarray(diff)
    table = np.asarray(table, dtype=np.int64).reshape(-1, 2)
    total = np.cumsum(diff.astype(np.int64))
    if total.size and (total.min() < 0 or total.max() >= 1 << 31):
        raise ValueError("a prefix of the difference array lies outside [0, 2^31)")
    depth = total.astype(np.uint32)
    stats = np.zeros((table.shape[0], 4), dtype=np.uint64)
    wins = n_windows(table, bin)
    first = np.concatenate([[0], np.cumsum(wins)])
    bins = np.zeros(int(first[-1]), dtype=np.uint64) if int(bin) > 0 else None
    for k, (off, ln) in enumerate(table.tolist()):
        if off < 0 or ln < 1:
            continue
        d = depth[off:off + ln].astype(np.uint64)
        stats[k] = (d.sum(dtype=np.uint64), (d * d).sum(dtype=np.uint64), np.count_nonzero(d), d.max())
        if bins is not None:
            bins[first[k]:first[k + 1]] = np.add.reduceat(d, np.arange(0, ln, int(bin)))
    return depth, stats, bins


def merge_into(diff, table, other_diff, other_table, ordinals):
    """Add a worker's accumulator into a global one, in place: row j of ``other_table`` is record ``ordinals[j]`` of ``table``
    (equal lengths); its length + 1 words are added to that record's."""
    table = np.asarray(table, dtype=np.int64).reshape(-1, 2)
    other_table = np.asarray(other_table, dtype=np.int64).reshape(-1, 2)
    ordinals = np.asarray(ordinals, dtype=np.int64).reshape(-1)
    if ordinals.shape[0] != other_table.shape[0]:
        raise ValueError("one ordinal per row of the worker's table")
    for (o_off, o_len), k in zip(other_table.tolist(), ordinals.tolist()):
        off, ln = table[k].tolist()
        if o_off < 0:
            continue
        if ln != o_len or off < 0:
            raise ValueError("record %d: the worker's row has %d bases, the table's %d" % (k, o_len, ln))
        diff[off:off + ln + 1] += other_diff[o_off:o_off + o_len + 1]
    return diff


def depth_rows(stats, table, ids):
    """Per record (id, length, mean depth, depth variance, covered fraction, max depth).  Mean = sum / length; variance is the
    population variance sum_squares / length - mean^2, worked out exactly from the integers (fractions) and rounded to float64
    once; covered fraction = bases with depth > 0 / length.  A record of no bases: zeros."""
    from fractions import Fraction

    table = np.asarray(table, dtype=np.int64).reshape(-1, 2)
    rows = []
    for rid, (_off, ln), st in zip(ids, table.tolist(), np.asarray(stats, dtype=np.uint64).tolist()):
        if ln < 1:
            rows.append((rid, int(ln), 0.0, 0.0, 0.0, 0))
            continue
        mean = Fraction(int(st[0]), ln)
        rows.append((rid, int(ln), float(mean), float(Fraction(int(st[1]), ln) - mean * mean), float(Fraction(int(st[2]), ln)), int(st[3])))
    return rows


DEPTH_HEADER = "id\tlength\tmean_depth\tdepth_variance\tcovered_fraction\tmax_depth\n"


def write_depth_table(path, rows):
    """``<output>_depth.txt``: a header line, then depth_rows() tab separated (floats as repr: the shortest text that reads back)."""
    with open(path, "w") as fh:
        fh.write(DEPTH_HEADER)
        for rid, ln, mean, var, cov, mx in rows:
            fh.write("%s\t%d\t%r\t%r\t%r\t%d\n" % (rid, ln, mean, var, cov, mx))


def bin_means(bins, table, bin):
    """(record index, start, end, mean depth) of every window of ``bins``: the window's sum over the bases it holds."""
    table = np.asarray(table, dtype=np.int64).reshape(-1, 2)
    out, g = [], 0
    for k, w in enumerate(n_windows(table, bin).tolist()):
        ln = int(table[k, 1])
        for i in range(w):
            start, end = i * int(bin), min((i + 1) * int(bin), ln)
            out.append((k, start, end, int(bins[g]) / float(end - start)))
            g += 1
    return out


def write_bedgraph(path, bins, table, ids, bin):
    """``<output>_depth.bedgraph``: id, start, end, mean depth of the window, tab separated, records in table order."""
    ids = list(ids)
    with open(path, "w") as fh:
        for k, start, end, mean in bin_means(bins, table, bin):
            fh.write("%s\t%d\t%d\t%r\n" % (ids[k], start, end, mean))


__all__ = ["depth_table", "mark_host", "finish_host", "merge_into", "depth_rows", "write_depth_table", "write_bedgraph", "bin_means",
           "n_windows", "clamped_intervals", "count_marked", "MAX_MARKED_PAIRS", "STATS_FIELDS", "DEPTH_HEADER"]
