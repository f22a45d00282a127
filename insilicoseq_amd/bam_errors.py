"""`report --bam --errors`: the errors of an aligned BAM's reads as CIGAR and MD tell them (include/iss_mi355x.h:
iss_br_errors_*; k_be_records and k_be_bases of csrc/iss_bamerrors.hip.h), their Python twin, the report made from them and the
comparison with another error tally.  numpy only.

For max_len L the words are errtally.layout(L) unchanged, followed by the aligned bases (2 + 446 L + 384 words):

    dropped [1] | pairs [1] | sub_q [2][L][94] | sub_mat [2][L][5][5] | ins [2][L][5] | del [2][L][5] | per_read [2][3][64]
    | bases [2][L][94]

``bases`` has the shape of the --report tally's ``qual``: a `generate --report` tally gives the simulator's denominators in the
same form.  Which records count, how they are validated (ALN_*) and what a valid one adds: bam_errors_host below is the
definition, the device equals it word for word.  DESIGN.md section 29."""
import collections

import numpy as np

from . import errtally
from .bam_report import MAX_LEN, _COLUMN_OPS, _QUERY_OPS, _as_chunks, _cigar, _classify
from .errtally import FIELDS as _ERR_FIELDS, LETTERS, PHREDS, READ_BINS, TYPES, _CODE_TABLE, _trim

ALN_CIGAR, ALN_TAGS, ALN_MD = 1, 2, 3
FIELDS = _ERR_FIELDS + ("bases",)
_SCALAR_SIZE = {ord(c): n for c, n in (("A", 1), ("c", 1), ("C", 1), ("s", 2), ("S", 2), ("i", 4), ("I", 4), ("f", 4))}
_ELEMENT_SIZE = {ord(c): n for c, n in (("c", 1), ("C", 1), ("s", 2), ("S", 2), ("i", 4), ("I", 4), ("f", 4))}
_NIBBLE_CODE = [4, 0, 1, 4, 2, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4]  # "=ACMGRSVTWYHKDBN"


def layout(L):
    """max_len -> OrderedDict field -> (word offset, shape), plus "words": errtally.layout(L) and ``bases`` behind it."""
    err = errtally.layout(L)
    out = collections.OrderedDict((name, err[name]) for name in _ERR_FIELDS)
    out["bases"] = (err["words"], (2, int(L), PHREDS))
    out["words"] = err["words"] + 2 * int(L) * PHREDS
    return out


def words(L):
    return layout(L)["words"]


def split(flat, L):
    """The flat words as a dict of views, one per field, in the shapes of layout."""
    flat = np.asarray(flat)
    lay = layout(L)
    if flat.ndim != 1 or flat.shape[0] != lay["words"]:
        raise ValueError("a BAM error tally of max_len %d has %d words, not %r" % (int(L), lay["words"], flat.shape))
    return {name: flat[lay[name][0]:lay[name][0] + int(np.prod(lay[name][1]))].reshape(lay[name][1]) for name in FIELDS}


def relayout(flat, max_len, L):
    """The words at max_len -> the words at L (same layout).  L: at least the longest read tallied -- no position at or past a
    read's length ever counts, so nothing is cut off."""
    src = split(flat, max_len)
    L = int(L)
    if not 1 <= L <= int(max_len):
        raise ValueError("read length %d outside 1 .. %d" % (L, int(max_len)))
    if any(src[name][:, L:].any() for name in ("sub_q", "sub_mat", "ins", "del", "bases")):
        raise ValueError("positions at or past %d were counted" % L)
    out = np.zeros(words(L), dtype=np.uint64)
    dst = split(out, L)
    for name in ("dropped", "pairs", "per_read"):
        dst[name][...] = src[name]
    for name in ("sub_q", "sub_mat", "ins", "del", "bases"):
        dst[name][...] = src[name][:, :L]
    return out


def errors_and_bases(flat, L):
    """The words -> (errtally.layout(L)'s words: `generate --error_report`'s file, bases [2][L][94])."""
    flat = np.asarray(flat, dtype=np.uint64)
    n = errtally.words(L)
    return flat[:n].copy(), split(flat, L)["bases"].copy()


# ------------------------------------------------------------------------------------------------------------ the twin
def _tag_walk(a, at, end):
    """The optional fields a[at:end]: ("md", start, stop) at the first MD:Z, ("none",) when the walk ends cleanly without one,
    ("bad",) on an unknown type byte, a value past the end, a Z / H without its NUL, a B with an unknown subtype or a negative
    count.  Fewer than three bytes left end the walk cleanly."""
    while at + 3 <= end:
        t0, t1, ty = a[at], a[at + 1], a[at + 2]
        at += 3
        if ty in _SCALAR_SIZE:
            size = _SCALAR_SIZE[ty]
        elif ty in (ord("Z"), ord("H")):
            z = at
            while z < end and a[z]:
                z += 1
            if z >= end:
                return ("bad",)
            if (t0, t1, ty) == (ord("M"), ord("D"), ord("Z")):
                return ("md", at, z)
            size = z - at + 1
        elif ty == ord("B"):
            if at + 5 > end:
                return ("bad",)
            count = int.from_bytes(a[at + 1:at + 5], "little", signed=True)
            if a[at] not in _ELEMENT_SIZE or count < 0:
                return ("bad",)
            size = 5 + count * _ELEMENT_SIZE[a[at]]
        else:
            return ("bad",)
        if at + size > end:
            return ("bad",)
        at += size
    return ("none",)


def _is_letter(ch):
    return 65 <= (ch & ~0x20) <= 90


def _md_walk(cigar, md):
    """The MD bytes against the CIGAR [(op, length)]: (mismatches [(SEQ index, letter)], deletions [(query bases in front of the
    gap, letter)]), or None when the string does not fit."""
    k, num, q = 0, 0, 0
    mism, dels = [], []
    for op, n in cigar:
        if op in _COLUMN_OPS:
            while n:
                if num:
                    t = min(num, n)
                    num, n, q = num - t, n - t, q + t
                elif k >= len(md):
                    return None  # too short
                elif 48 <= md[k] <= 57:
                    stop = k
                    while stop < len(md) and 48 <= md[stop] <= 57:
                        stop += 1
                    num, k = int(md[k:stop]), stop
                elif _is_letter(md[k]):
                    mism.append((q, md[k]))
                    q, n, k = q + 1, n - 1, k + 1
                else:
                    return None  # '^' inside aligned columns, or a stray byte
        elif op in (1, 4):
            q += n
        elif op == 2:
            if num:
                return None  # a number that runs into the gap
            while k < len(md) and md[k] == 48:
                k += 1
            if k >= len(md) or md[k] != 94:
                return None
            k += 1
            stop = k
            while stop < len(md) and _is_letter(md[stop]):
                stop += 1
            if stop == k or stop - k != n:
                return None
            dels.extend((q, ch) for ch in md[k:stop])
            k = stop
    if num or md[k:].strip(b"0"):
        return None  # too long
    return mism, dels


def _complement(code):
    return 3 - code if code < 4 else 4


def _tally_record(a, o, c, r, L, t):
    """One taken record -- r of the chunk's bytes a at offset o, c the chunk's _classify: adds what it adds to the views t;
    "tallied", "unaligned", "no_md" or the ALN_* code."""
    length, seq, qual, reverse, mate = int(c["len"][r]), int(c["seq"][r]), int(c["qual"][r]), bool(c["reverse"][r]), int(c["mate"][r])
    if c["flag"][r] & 4 or not c["n_cigar"][r] or not length:
        return "unaligned"
    cigar = _cigar(a, o, c["l_name"][r], c["n_cigar"][r])
    if any(op > 8 for op, _ in cigar) or sum(n for op, n in cigar if op in _QUERY_OPS) != length:
        return ALN_CIGAR
    tags = _tag_walk(a, qual + length, o + 4 + int(c["block_size"][r]))
    if tags[0] != "md":
        return "no_md" if tags[0] == "none" else ALN_TAGS
    walk = _md_walk(cigar, a[tags[1]:tags[2]])
    if walk is None:
        return ALN_MD
    turn = (lambda q: length - 1 - q) if reverse else (lambda q: q)
    strand = _complement if reverse else (lambda c: c)
    letter = lambda q: strand(_NIBBLE_CODE[(a[seq + q // 2] >> (0 if q & 1 else 4)) & 15])
    q = 0
    n_ins = 0
    for op, n in cigar:
        for i in range(q, q + n if op in _COLUMN_OPS or op == 1 else q):
            if op == 1:
                t["ins"][mate, turn(i), letter(i)] += 1
                n_ins += 1
            else:
                t["bases"][mate, turn(i), a[qual + i]] += 1
        if op in _QUERY_OPS:
            q += n
    for q, ch in walk[0]:
        t["sub_q"][mate, turn(q), a[qual + q]] += 1
        t["sub_mat"][mate, turn(q), strand(int(_CODE_TABLE[ch])), letter(q)] += 1
    for q, ch in walk[1]:
        t["del"][mate, min(length - q if reverse else q, length - 1), strand(int(_CODE_TABLE[ch]))] += 1
    for k, rows in enumerate((len(walk[0]), n_ins, len(walk[1]))):
        t["per_read"][mate, k, min(rows, READ_BINS - 1)] += 1
    if mate == 0:
        t["pairs"][0] += 1
    return "tallied"


def bam_errors_host(chunks, max_len=MAX_LEN):
    """The twin of the device path (iss_br_feed with errors enabled / iss_br_errors_download), one record at a time in plain
    Python.  chunks: a bam.Chunk or an iterable of them -- the feeds.  Returns a dict: ``errors`` (the flat uint64 words at
    max_len), ``error_counts`` (records tallied per mate [2], taken but not aligned, aligned without an MD tag),
    ``bad_alignment`` (index over all records fed; -1: none) and ``bad_alignment_code``."""
    L = int(max_len)
    if not 1 <= L <= MAX_LEN:
        raise ValueError("max_len outside 1 .. %d" % MAX_LEN)
    flat = np.zeros(words(L), dtype=np.uint64)
    t = split(flat, L)
    counts, bad, fed = [0, 0, 0, 0], None, 0
    for chunk in _as_chunks(chunks):
        if not len(chunk.offsets):
            continue
        a = bytes(np.frombuffer(chunk.data, dtype=np.uint8))
        c = _classify(chunk, L)
        for r in np.flatnonzero((c["code"] == 0) & (c["mate"] >= 0)):
            mate = int(c["mate"][r])
            what = _tally_record(a, int(chunk.offsets[r]), c, r, L, t)
            if what == "tallied":
                counts[mate] += 1
            elif what == "unaligned":
                counts[2] += 1
            elif what == "no_md":
                counts[3] += 1
            else:
                t["dropped"][0] += 1
                if bad is None:
                    bad = (fed + int(r), what)
        fed += len(chunk.offsets)
    return {"errors": flat, "error_counts": counts, "bad_alignment": bad[0] if bad else -1, "bad_alignment_code": bad[1] if bad else 0}


# ------------------------------------------------------------------------------------------------------------ reports
def _rate(rows, bases):
    return [int(x) / int(n) if n else None for x, n in zip(rows, bases)]


def report_dict(flat, L, counts=None):
    """errtally.report_dict's content for an aligned BAM (JSON-serialisable): the rates are per aligned base at the position
    (``bases`` summed over phreds), None where there is none; ``calibration`` comes from ``bases``; ``aligned_bases`` per mate
    and position; ``counts`` (with ``counts``: the download's four) and ``dropped``."""
    t = split(np.asarray(flat, dtype=np.uint64), L)
    mates, calibration = [], []
    for m in range(2):
        at_pos = t["bases"][m].astype(np.int64).sum(axis=1)
        per_pos = {"substitution": t["sub_q"][m].astype(np.int64).sum(axis=1), "insertion": t["ins"][m].astype(np.int64).sum(axis=1),
                   "deletion": t["del"][m].astype(np.int64).sum(axis=1)}
        mat = t["sub_mat"][m].astype(np.int64).sum(axis=0)
        mates.append({
            "rates": {name: _rate(per_pos[name], at_pos) for name in TYPES},
            "aligned_bases": [int(x) for x in at_pos],
            "substitution_matrix": {LETTERS[r]: {LETTERS[a]: int(mat[r, a]) for a in range(5)} for r in range(5)},
            "substitutions_by_phred": _trim(t["sub_q"][m].astype(np.int64).sum(axis=0)),
            "per_read": {name: _trim(t["per_read"][m, k]) for k, name in enumerate(TYPES)},
        })
        bases = t["bases"][m].astype(np.int64).sum(axis=0)
        subs = t["sub_q"][m].astype(np.int64).sum(axis=0)
        calibration.append([{"phred": q, "bases": int(bases[q]), "substitutions": int(subs[q]), "nominal": 10.0 ** (-q / 10.0),
                             "empirical": int(subs[q]) / int(bases[q])} for q in range(PHREDS) if bases[q]])
    out = {"pairs": int(t["pairs"][0]), "dropped": int(t["dropped"][0]), "read_length": int(L), "mates": mates, "calibration": calibration}
    if counts is not None:
        out["counts"] = {"tallied": [int(counts[0]), int(counts[1])], "unaligned": int(counts[2]), "no_md": int(counts[3])}
    return out


def _tv(a, b):
    """Total-variation distance of two histograms as distributions (None: one of them is empty)."""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    if not a.sum() or not b.sum():
        return None
    return float(0.5 * np.abs(a / a.sum() - b / b.sum()).sum())


def _max_abs(values):
    values = [abs(v) for v in values if v is not None]
    return max(values) if values else None


def compare_errors(a_err, a_bases, La, b_err, b_bases, Lb):
    """Two error tallies side by side (a - b), JSON-serialisable.  x_err: errtally.layout(Lx)'s words; x_bases: [2][Lx][94]
    aligned (or emitted) bases, or None -- that side then takes ``pairs`` as its denominator at every position.  Over the first
    min(La, Lb) positions, per mate and position ``rate_diff`` of the three types (None where a side has no denominator); per mate
    ``substitution_matrix_tv`` (normalised matrices summed over all positions of each side) and ``per_read_tv`` of the three
    rows-per-read distributions; per phred ``calibration_diff`` of the empirical rates where both sides have bases; the maxima as
    ``summary``."""
    ta, tb = errtally.split(np.asarray(a_err, dtype=np.uint64), La), errtally.split(np.asarray(b_err, dtype=np.uint64), Lb)
    P = min(int(La), int(Lb))

    def denominators(t, bases, L):
        if bases is None:
            return np.full((2, int(L)), int(t["pairs"][0]), dtype=np.int64)
        bases = np.asarray(bases)
        if bases.shape != (2, int(L), PHREDS):
            raise ValueError("bases of read length %d have the shape (2, %d, %d), not %r" % (int(L), int(L), PHREDS, bases.shape))
        return bases.astype(np.int64).sum(axis=2)

    da, db = denominators(ta, a_bases, La), denominators(tb, b_bases, Lb)
    mates = []
    for m in range(2):
        diffs = {}
        for name, field in zip(TYPES, ("sub_q", "ins", "del")):
            ra, rb = ta[field][m, :P].astype(np.int64).sum(axis=1), tb[field][m, :P].astype(np.int64).sum(axis=1)
            diffs[name] = [int(ra[p]) / int(da[m, p]) - int(rb[p]) / int(db[m, p]) if da[m, p] and db[m, p] else None for p in range(P)]
        mates.append({"rate_diff": diffs,
                      "substitution_matrix_tv": _tv(ta["sub_mat"][m].astype(np.int64).sum(axis=0), tb["sub_mat"][m].astype(np.int64).sum(axis=0)),
                      "per_read_tv": {name: _tv(ta["per_read"][m, k], tb["per_read"][m, k]) for k, name in enumerate(TYPES)}})
    calibration = None
    if a_bases is not None and b_bases is not None:
        calibration = []
        for m in range(2):
            na, nb = np.asarray(a_bases)[m].astype(np.int64).sum(axis=0), np.asarray(b_bases)[m].astype(np.int64).sum(axis=0)
            sa, sb = ta["sub_q"][m].astype(np.int64).sum(axis=0), tb["sub_q"][m].astype(np.int64).sum(axis=0)
            calibration.append([{"phred": q, "diff": int(sa[q]) / int(na[q]) - int(sb[q]) / int(nb[q])} for q in range(PHREDS) if na[q] and nb[q]])
    summary = {"max_abs_%s_rate_diff" % name: _max_abs([x for m in mates for x in m["rate_diff"][name]]) for name in TYPES}
    summary["max_substitution_matrix_tv"] = _max_abs([m["substitution_matrix_tv"] for m in mates])
    summary["max_per_read_tv"] = _max_abs([x for m in mates for x in m["per_read_tv"].values()])
    summary["max_abs_calibration_diff"] = _max_abs([x["diff"] for c in calibration or [] for x in c])
    return {"positions": P, "read_lengths": [int(La), int(Lb)], "mates": mates, "calibration_diff": calibration, "summary": summary}


__all__ = ["ALN_CIGAR", "ALN_TAGS", "ALN_MD", "FIELDS", "layout", "words", "split", "relayout", "errors_and_bases", "bam_errors_host",
           "report_dict", "compare_errors"]
