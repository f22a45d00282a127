"""Tallies of generated reads: the layout of the device's counters (include/iss_mi355x.h: iss_output_tally; k_tally_lines and
k_tally_reads of csrc/iss_tally.hip.h), their numpy twin, and the report made from them.  numpy only.

For read length L the tally is one flat uint64 array, the fields in this order with no padding:

    pairs [1] | qual [2][L][94] | base [2][L][5] | gc [2][L + 1] | meanq [2][94] | insert [2048]

(mate, position, phred -- a byte above 93 counts in bin 93), (mate, position, base code: A, C, G, T -> 0..3 in either case, every
other letter 4), reads of a mate by their number of G / C letters, reads of a mate by floor(sum of phreds / L), pairs by insert
size clamped to [0, 2047].  Every count is an exact integer sum."""
import collections

import numpy as np

PHREDS = 94         # ISS_TALLY_PHREDS
INSERT_BINS = 2048  # ISS_TALLY_INSERT_BINS
FIELDS = ("pairs", "qual", "base", "gc", "meanq", "insert")

_CODE_TABLE = np.full(256, 4, dtype=np.uint8)
for _k, _c in enumerate(b"ACGT"):
    _CODE_TABLE[_c] = _CODE_TABLE[_c | 0x20] = _k
_GC_TABLE = np.zeros(256, dtype=np.int64)
_GC_TABLE[[ord(c) for c in "GCgc"]] = 1


def tally_layout(L):
    """Read length -> OrderedDict field -> (word offset, shape), plus "words": the size of the whole tally."""
    L = int(L)
    if L < 1:
        raise ValueError("read length must be positive")
    shapes = (("pairs", (1,)), ("qual", (2, L, PHREDS)), ("base", (2, L, 5)), ("gc", (2, L + 1)), ("meanq", (2, PHREDS)),
              ("insert", (INSERT_BINS,)))
    out, at = collections.OrderedDict(), 0
    for name, shape in shapes:
        out[name] = (at, shape)
        at += int(np.prod(shape))
    out["words"] = at
    return out


def tally_words(L):
    return tally_layout(L)["words"]


def split_tally(words, L):
    """The flat words as a dict of views, one per field, in the shapes of tally_layout."""
    words = np.asarray(words)
    lay = tally_layout(L)
    if words.ndim != 1 or words.shape[0] != lay["words"]:
        raise ValueError("a tally of read length %d has %d words, not %r" % (int(L), lay["words"], words.shape))
    return {name: words[lay[name][0]:lay[name][0] + int(np.prod(lay[name][1]))].reshape(lay[name][1]) for name in FIELDS}


def tally_host(bases_ascii, qual, insert_sizes, L):
    """The numpy twin of iss_output_tally: bases_ascii, qual uint8 [n, 2, L] (mate 1, mate 2; the bytes of ReadEngine.download /
    an "ascii" export), insert_sizes [n] (coords[:, 3]) -> the flat uint64 tally."""
    L = int(L)
    bases = np.asarray(bases_ascii, dtype=np.uint8)
    qual = np.asarray(qual, dtype=np.uint8)
    isz = np.asarray(insert_sizes, dtype=np.int64).reshape(-1)
    n = bases.shape[0]
    if bases.shape != (n, 2, L) or qual.shape != (n, 2, L) or isz.shape != (n,):
        raise ValueError("bases and qual [n, 2, %d], insert sizes [n]" % L)
    words = np.zeros(tally_words(L), dtype=np.uint64)
    t = split_tally(words, L)
    t["pairs"][0] = n
    pos = np.arange(L)
    for m in range(2):
        q = np.minimum(qual[:, m, :].astype(np.int64), PHREDS - 1)
        t["qual"][m] = np.bincount((pos[None, :] * PHREDS + q).reshape(-1), minlength=L * PHREDS).reshape(L, PHREDS)
        c = _CODE_TABLE[bases[:, m, :]].astype(np.int64)
        t["base"][m] = np.bincount((pos[None, :] * 5 + c).reshape(-1), minlength=L * 5).reshape(L, 5)
        t["gc"][m] = np.bincount(_GC_TABLE[bases[:, m, :]].sum(axis=1), minlength=L + 1)
        mean = np.minimum(qual[:, m, :].astype(np.int64).sum(axis=1) // L, PHREDS - 1)
        t["meanq"][m] = np.bincount(mean, minlength=PHREDS)
    t["insert"][:] = np.bincount(np.clip(isz, 0, INSERT_BINS - 1), minlength=INSERT_BINS)
    return words


def merge_tallies(tallies):
    """The tally of several runs, batches or workers: a plain sum."""
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


def _quantile(hist, frac):
    """The smallest value v with cumulative count >= frac * total (None for an empty histogram)."""
    total = int(hist.sum())
    if not total:
        return None
    return int(np.searchsorted(np.cumsum(hist.astype(np.int64)), frac * total, side="left"))


def report_dict(words, L):
    """What a QC tool would say about the reads, from the tally alone (JSON-serialisable): ``pairs``; per mate and position the
    mean phred, the phred quartiles (q25, median, q75) and the fractions of A, C, G, T and other letters; per mate the GC-count
    and mean-quality histograms of the reads; the insert-size histogram -- histograms as lists with trailing zeros trimmed
    (insert sizes below 0 count in bin 0, from 2047 on in bin 2047)."""
    t = split_tally(np.asarray(words, dtype=np.uint64), L)
    phred = np.arange(PHREDS, dtype=np.float64)
    mates = []
    for m in range(2):
        q = t["qual"][m].astype(np.int64)
        n = q.sum(axis=1)
        safe = np.maximum(n, 1)
        b = t["base"][m].astype(np.int64)
        bn = np.maximum(b.sum(axis=1), 1)
        mates.append({
            "mean_phred": [float(x) if k else None for x, k in zip((q * phred).sum(axis=1) / safe, n)],
            "phred_q25": [_quantile(row, 0.25) for row in q],
            "phred_median": [_quantile(row, 0.5) for row in q],
            "phred_q75": [_quantile(row, 0.75) for row in q],
            "base_fractions": {name: [float(x) for x in b[:, k] / bn] for k, name in enumerate(("A", "C", "G", "T", "other"))},
            "gc_histogram": _trim(t["gc"][m]),
            "mean_quality_histogram": _trim(t["meanq"][m]),
        })
    return {"pairs": int(t["pairs"][0]), "read_length": int(L), "mates": mates, "insert_size_histogram": _trim(t["insert"])}


__all__ = ["PHREDS", "INSERT_BINS", "FIELDS", "tally_layout", "tally_words", "split_tally", "tally_host", "merge_tallies", "report_dict"]
