"""`generate --origins`: where every pair came from, as BEDPE (``<output>_origins.bedpe``).  numpy only.

One line per pair, tab separated, no header, workers in worker order and pairs in FASTQ order::

    {id}  s1  e1  {id}  s2  e2  {id}_{i}_{cpu}  .  +  -  isz

With ``(fs, rs, re, isz)`` the row's coordinates (ReadEngine.coords), RL the read length and len the record's length, ``[s1, e1)``
is ``[fs, fs + RL)`` and ``[s2, e2)`` is ``[rs, re)`` -- the template intervals the two reads were cut from
(iss/generator.py:135-147, 165-177) -- each clamped by the rule of the depth (depth.clamped_intervals): ``s' = min(max(s, 0), len)``,
``e' = max(min(max(e, 0), len), s')``; an interval that is empty after the clamp reads ``s' s'``.  Read 1 is always ``+`` and read 2
always ``-`` (generator.py:149, 180), the score is ``.``, the name is the FASTQ read name without ``/1``, ``/2`` and ``isz`` the
insert size as drawn.  The device builds the text (ReadEngine.origins_emit_batch); ``lines_host`` is its twin, written from this
definition."""
import numpy as np

SUFFIX = "_origins.bedpe"


def clamp(start, end, length):
    """The rule above on arrays -> (s', e')."""
    start, end, length = (np.asarray(a, dtype=np.int64) for a in (start, end, length))
    s = np.minimum(np.maximum(start, 0), length)
    return s, np.maximum(np.minimum(np.maximum(end, 0), length), s)


def lines_host(items, record_lengths, cpu_number, coords, read_length):
    """The text of ``items`` -- (record id, first pair id, first output row, pairs), the tuples of ReadEngine.origins_emit_batch --
    on records of ``record_lengths`` bases, from ``coords`` [pairs of all items, 4]: the rows' (fs, rs, re, isz), item after item."""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 4)
    if len(record_lengths) != len(items) or c.shape[0] != sum(int(it[3]) for it in items):
        raise ValueError("one record length per item and one row of coords per pair")
    out, at = [], 0
    for (rid, first_i, _row, n), length in zip(items, record_lengths):
        n = int(n)
        rid = rid.decode() if isinstance(rid, bytes) else str(rid)
        part = c[at:at + n]
        at += n
        s1, e1 = clamp(part[:, 0], part[:, 0] + int(read_length), int(length))
        s2, e2 = clamp(part[:, 1], part[:, 2], int(length))
        cols = [a.tolist() for a in (s1, e1, s2, e2, part[:, 3])]
        tail = "_%d\t.\t+\t-\t" % int(cpu_number)
        out.extend("\t".join((rid, str(a), str(b), rid, str(x), str(y), rid + "_" + str(int(first_i) + j) + tail + str(z))) + "\n"
                   for j, (a, b, x, y, z) in enumerate(zip(*cols)))
    return "".join(out).encode()


def parse(path, lift=None):
    """``<output>_origins.bedpe`` (or its ``.gz``) -> dict of arrays, one entry per line: ``id`` and ``name`` (object arrays of
    str), ``s1`` ``e1`` ``s2`` ``e2`` ``isz`` (int64).  A line that is not a line of this file raises ValueError.
    ``lift`` (a run with --variants: the file is in haplotype coordinates): ``{record id: f}``, f mapping an int64 array of
    haplotype coordinates to the record's -- VariantTable.lift_host, or ``lambda h: variants.lift_chain(chain, h)`` for a chain
    of ``<output>_haplotype.chain``; the four interval ends of the records it names are lifted, ``isz`` stays."""
    import gzip

    opener = gzip.open if str(path).endswith(".gz") else open
    ids, names, nums = [], [], []
    with opener(path, "rb") as fh:
        for k, line in enumerate(fh.read().decode().split("\n")[:-1]):
            f = line.split("\t")
            if len(f) != 11 or f[0] != f[3] or f[7:10] != [".", "+", "-"] or not f[6].startswith(f[0] + "_"):
                raise ValueError("%s: line %d is not an origins line" % (path, k + 1))
            ids.append(f[0])
            names.append(f[6])
            nums.append((int(f[1]), int(f[2]), int(f[4]), int(f[5]), int(f[10])))
    nums = np.asarray(nums, dtype=np.int64).reshape(-1, 5)
    out = {"id": np.asarray(ids, dtype=object), "name": np.asarray(names, dtype=object)}
    out.update({k: nums[:, j].copy() for j, k in enumerate(("s1", "e1", "s2", "e2", "isz"))})
    for rid, f in (lift or {}).items():
        rows = out["id"] == rid
        for k in ("s1", "e1", "s2", "e2"):
            out[k][rows] = f(out[k][rows])
    return out


def intervals_for_depth(parsed, ids=None):
    """The parsed intervals in the form depth.mark_host takes -> (coords int64 [2 n, 4], item int64 [2 n], ids): one row
    (0, s, e, 0) per interval, to be marked with ``read_length=0`` -- mark_host's first interval [fs, fs + 0) is then empty and
    its second is [s, e) -- and the row of ``ids`` (default: the file's record ids in order of first appearance) the line names:
    ``mark_host(diff, coords, item, depth_table(lengths of ids), 0)``.  Records are told apart by id here."""
    if ids is None:
        ids = list(dict.fromkeys(parsed["id"].tolist()))
    row = {rid: k for k, rid in enumerate(ids)}
    item = np.asarray([row[rid] for rid in parsed["id"].tolist()], dtype=np.int64)
    n = item.shape[0]
    coords = np.zeros((2 * n, 4), dtype=np.int64)
    coords[0::2, 1], coords[0::2, 2] = parsed["s1"], parsed["e1"]
    coords[1::2, 1], coords[1::2, 2] = parsed["s2"], parsed["e2"]
    return coords, np.repeat(item, 2), list(ids)


__all__ = ["SUFFIX", "clamp", "lines_host", "parse", "intervals_for_depth"]
