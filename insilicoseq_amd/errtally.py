"""Tallies of the simulator's own errors: the layout of the device's counters (include/iss_mi355x.h: iss_mutations_tally;
k_errtally_rows and k_errtally_reads of csrc/iss_errtally.hip.h), their numpy twin, and the report made from them.  numpy only.

For read length L the tally is one flat uint64 array, the fields in this order with no padding (2 + 258 L + 384 words):

    dropped [1] | pairs [1] | sub_q [2][L][94] | sub_mat [2][L][5][5] | ins [2][L][5] | del [2][L][5] | per_read [2][3][64]

calls whose rows could not be trusted (they add nothing else); pairs of the windows tallied; substitution rows by (mate,
position, quality -- above 93 counts in bin 93); substitution rows by (mate, position, code of ref, code of alt: A, C, G, T ->
0..3 in either case, every other byte 4); insertion rows by (mate, position, code of alt); deletion rows by (mate, position,
code of ref); reads of a mate by their number of rows of a type (0 substitution, 1 insertion, 2 deletion) clamped to 63.  A
position outside [0, L - 1] counts in the nearest end bin.  Every count is an exact integer sum.

The rows are the ``iss_mutation`` rows of ReadEngine.mutations() / mt_mutations().  Two things they do not say (DESIGN.md
section 17): a substitution back to the original letter is no row, and an indel's position is the position at the time of the
event."""
import collections

import numpy as np

PHREDS = 94     # ISS_ERRTALLY_PHREDS
READ_BINS = 64  # ISS_ERRTALLY_READ_BINS
FIELDS = ("dropped", "pairs", "sub_q", "sub_mat", "ins", "del", "per_read")
TYPES = ("substitution", "insertion", "deletion")
LETTERS = ("A", "C", "G", "T", "other")

_CODE_TABLE = np.full(256, 4, dtype=np.int64)
for _k, _c in enumerate(b"ACGT"):
    _CODE_TABLE[_c] = _CODE_TABLE[_c | 0x20] = _k


def layout(L):
    """Read length -> OrderedDict field -> (word offset, shape), plus "words": the size of the whole tally."""
    L = int(L)
    if L < 1:
        raise ValueError("read length must be positive")
    shapes = (("dropped", (1,)), ("pairs", (1,)), ("sub_q", (2, L, PHREDS)), ("sub_mat", (2, L, 5, 5)), ("ins", (2, L, 5)),
              ("del", (2, L, 5)), ("per_read", (2, 3, READ_BINS)))
    out, at = collections.OrderedDict(), 0
    for name, shape in shapes:
        out[name] = (at, shape)
        at += int(np.prod(shape))
    out["words"] = at
    return out


def words(L):
    return layout(L)["words"]


def split(flat, L):
    """The flat words as a dict of views, one per field, in the shapes of layout."""
    flat = np.asarray(flat)
    lay = layout(L)
    if flat.ndim != 1 or flat.shape[0] != lay["words"]:
        raise ValueError("an error tally of read length %d has %d words, not %r" % (int(L), lay["words"], flat.shape))
    return {name: flat[lay[name][0]:lay[name][0] + int(np.prod(lay[name][1]))].reshape(lay[name][1]) for name in FIELDS}


def errors_host(rows, first_pair, n_pairs, L):
    """The numpy twin of iss_mutations_tally for one call that did not overflow: ``rows`` a structured iss_mutation array
    (engine.MUT_DTYPE: pair, mate, type, position, ref, alt, quality -- ``pair`` counted from the call's first pair), the window
    the pairs [first_pair, first_pair + n_pairs) of the call -> the flat uint64 tally."""
    L, first_pair, n_pairs = int(L), int(first_pair), int(n_pairs)
    if n_pairs < 0:
        raise ValueError("n_pairs must not be negative")
    flat = np.zeros(words(L), dtype=np.uint64)
    t = split(flat, L)
    t["pairs"][0] = n_pairs
    rows = np.asarray(rows)
    w = rows["pair"].astype(np.int64) - first_pair
    typ = rows["type"].astype(np.int64) & 3
    keep = (rows["pair"] >= 0) & (w >= 0) & (w < n_pairs) & (typ < 3)
    rows, w, typ = rows[keep], w[keep], typ[keep]
    mate = rows["mate"].astype(np.int64) & 1
    pos = np.clip(rows["position"].astype(np.int64), 0, L - 1)
    ref, alt = _CODE_TABLE[rows["ref"]], _CODE_TABLE[rows["alt"]]
    qual = np.clip(rows["quality"].astype(np.int64), 0, PHREDS - 1)
    mp = mate * L + pos
    sub, ins, dele = typ == 0, typ == 1, typ == 2
    t["sub_q"][...] = np.bincount(mp[sub] * PHREDS + qual[sub], minlength=2 * L * PHREDS).reshape(2, L, PHREDS)
    t["sub_mat"][...] = np.bincount((mp[sub] * 5 + ref[sub]) * 5 + alt[sub], minlength=2 * L * 25).reshape(2, L, 5, 5)
    t["ins"][...] = np.bincount(mp[ins] * 5 + alt[ins], minlength=2 * L * 5).reshape(2, L, 5)
    t["del"][...] = np.bincount(mp[dele] * 5 + ref[dele], minlength=2 * L * 5).reshape(2, L, 5)
    per_read = np.bincount((w * 2 + mate) * 3 + typ, minlength=n_pairs * 6).reshape(n_pairs, 2, 3)
    per_read = np.minimum(per_read, READ_BINS - 1)
    for m in range(2):
        for k in range(3):
            t["per_read"][m, k] = np.bincount(per_read[:, m, k], minlength=READ_BINS)
    return flat


def merge(tallies):
    """The tally of several calls, batches or workers: a plain sum."""
    tallies = [np.asarray(t, dtype=np.uint64) for t in tallies]
    if not tallies:
        raise ValueError("no tally to merge")
    if any(t.shape != tallies[0].shape or t.ndim != 1 for t in tallies):
        raise ValueError("tallies of different read lengths")
    out = tallies[0].copy()
    for t in tallies[1:]:
        out += t
    return out


def _trim(hist):
    """A histogram as a list, trailing zeros left out."""
    hist = np.asarray(hist)
    nz = np.flatnonzero(hist)
    return [int(x) for x in hist[:nz[-1] + 1]] if nz.size else []


def report_dict(flat, L, tally=None):
    """What the run did to the reads, from the tally alone (JSON-serialisable): ``pairs``, ``dropped``; per mate and position
    the substitution, insertion and deletion rows per read (None without a pair); the substitution matrix (ref letter -> alt
    letter -> count) and the substitutions by phred, both summed over positions; the per-read histograms of each type with
    trailing zeros trimmed (63 stands for 63 and more).  With ``tally``, the words of the --report tally of the same run
    (tally.py), also ``calibration``: per mate, for every phred that has bases, the bases emitted at it, the substitutions
    recorded at it, the nominal error probability 10^(-q/10) and the empirical rate substitutions / bases."""
    t = split(np.asarray(flat, dtype=np.uint64), L)
    pairs = int(t["pairs"][0])
    mates = []
    for m in range(2):
        per_pos = {"substitution": t["sub_q"][m].astype(np.int64).sum(axis=1), "insertion": t["ins"][m].astype(np.int64).sum(axis=1),
                   "deletion": t["del"][m].astype(np.int64).sum(axis=1)}
        mat = t["sub_mat"][m].astype(np.int64).sum(axis=0)
        mates.append({
            "rates": {name: [int(x) / pairs if pairs else None for x in per_pos[name]] for name in TYPES},
            "substitution_matrix": {LETTERS[r]: {LETTERS[a]: int(mat[r, a]) for a in range(5)} for r in range(5)},
            "substitutions_by_phred": _trim(t["sub_q"][m].astype(np.int64).sum(axis=0)),
            "per_read": {name: _trim(t["per_read"][m, k]) for k, name in enumerate(TYPES)},
        })
    out = {"pairs": pairs, "dropped": int(t["dropped"][0]), "read_length": int(L), "mates": mates}
    if tally is not None:
        from .tally import split_tally

        qual = split_tally(np.asarray(tally, dtype=np.uint64), L)["qual"]
        out["calibration"] = []
        for m in range(2):
            bases = qual[m].astype(np.int64).sum(axis=0)
            subs = t["sub_q"][m].astype(np.int64).sum(axis=0)
            out["calibration"].append([
                {"phred": q, "bases": int(bases[q]), "substitutions": int(subs[q]), "nominal": 10.0 ** (-q / 10.0),
                 "empirical": int(subs[q]) / int(bases[q])}
                for q in range(PHREDS) if bases[q]])
    return out


__all__ = ["PHREDS", "READ_BINS", "FIELDS", "TYPES", "LETTERS", "layout", "words", "split", "errors_host", "merge", "report_dict"]
