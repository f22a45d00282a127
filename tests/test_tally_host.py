"""insilicoseq_amd.tally without a GPU: the layout of the tally words, the numpy twin against a plain Python loop, the sums that
tie the fields together, merge_tallies and report_dict."""
import json

import numpy as np
import pytest

from insilicoseq_amd import tally as T


@pytest.mark.parametrize("L", [1, 32, 33, 125, 151, 301])
def test_layout(L):
    lay = T.tally_layout(L)
    assert list(lay) == ["pairs", "qual", "base", "gc", "meanq", "insert", "words"]
    assert lay["pairs"] == (0, (1,))
    assert lay["qual"] == (1, (2, L, 94))
    assert lay["base"] == (1 + 2 * L * 94, (2, L, 5))
    assert lay["gc"] == (1 + 2 * L * 94 + 2 * L * 5, (2, L + 1))
    assert lay["meanq"] == (1 + 2 * L * 94 + 2 * L * 5 + 2 * (L + 1), (2, 94))
    assert lay["insert"] == (1 + 2 * L * 94 + 2 * L * 5 + 2 * (L + 1) + 2 * 94, (2048,))
    assert lay["words"] == T.tally_words(L) == 1 + 2 * L * 94 + 2 * L * 5 + 2 * (L + 1) + 2 * 94 + 2048
    words = np.arange(lay["words"], dtype=np.uint64)
    parts = T.split_tally(words, L)
    assert set(parts) == set(T.FIELDS)
    for name in T.FIELDS:  # views on the flat words, at the offsets of the layout, no gap and no overlap
        assert parts[name].shape == lay[name][1] and parts[name].base is not None
        assert int(parts[name].reshape(-1)[0]) == lay[name][0]
    assert sum(p.size for p in parts.values()) == lay["words"]
    with pytest.raises(ValueError):
        T.split_tally(words[:-1], L)


def _case(L=37, n=50, seed=3):
    rng = np.random.RandomState(seed)
    letters = np.frombuffer(b"ACGTacgtNRYnry", dtype=np.uint8)
    bases = letters[rng.randint(0, letters.size, (n, 2, L))]
    qual = rng.randint(0, 42, (n, 2, L)).astype(np.uint8)
    qual[0, 0, 0], qual[1, 1, L - 1], qual[2, 0, 5] = 94, 255, 93  # above the range FASTQ can print: bin 93
    qual[3, 1, :] = 200                                            # a mean above 93 too
    isz = rng.randint(0, 600, n).astype(np.int64)
    isz[:5] = [0, -7, 2048, 2047, 100000]
    return bases, qual, isz, L


def _loop_tally(bases, qual, isz, L):
    t = {"pairs": [0], "qual": np.zeros((2, L, 94), int), "base": np.zeros((2, L, 5), int), "gc": np.zeros((2, L + 1), int),
         "meanq": np.zeros((2, 94), int), "insert": np.zeros(2048, int)}
    for i in range(bases.shape[0]):
        t["pairs"][0] += 1
        t["insert"][min(max(int(isz[i]), 0), 2047)] += 1
        for m in range(2):
            gc = total = 0
            for p in range(L):
                ch, q = chr(bases[i, m, p]), int(qual[i, m, p])
                t["qual"][m, p, min(q, 93)] += 1
                t["base"][m, p, "ACGT".index(ch.upper()) if ch.upper() in "ACGT" else 4] += 1
                gc += ch in "GCgc"
                total += q
            t["gc"][m, gc] += 1
            t["meanq"][m, min(total // L, 93)] += 1
    return t


def test_twin_equals_a_plain_loop():
    bases, qual, isz, L = _case()
    words = T.tally_host(bases, qual, isz, L)
    assert words.dtype == np.uint64 and words.shape == (T.tally_words(L),)
    got, exp = T.split_tally(words, L), _loop_tally(bases, qual, isz, L)
    for name in T.FIELDS:
        assert np.array_equal(got[name], np.asarray(exp[name], dtype=np.uint64)), name
    # the case holds what it is meant to hold
    assert got["qual"][:, :, 93].sum() >= 3 + L and got["base"][:, :, 4].sum() > 0
    assert got["insert"][0] >= 2 and got["insert"][2047] == 3 and got["meanq"][1, 93] >= 1
    with pytest.raises(ValueError):
        T.tally_host(bases, qual[:, :, :-1], isz, L)


def test_sums():
    bases, qual, isz, L = _case(L=33, n=77, seed=9)
    t = T.split_tally(T.tally_host(bases, qual, isz, L), L)
    pairs = int(t["pairs"][0])
    assert pairs == 77
    assert (t["qual"].sum(-1) == pairs).all() and t["qual"].sum(-1).shape == (2, L)
    assert (t["base"].sum(-1) == pairs).all()
    assert (t["gc"].sum(-1) == pairs).all() and (t["meanq"].sum(-1) == pairs).all()
    assert t["insert"].sum() == pairs
    empty = T.split_tally(T.tally_host(bases[:0], qual[:0], isz[:0], L), L)
    assert not any(v.any() for v in empty.values())


def _hand_made(L=3):
    words = np.zeros(T.tally_words(L), dtype=np.uint64)
    t = T.split_tally(words, L)
    t["pairs"][0] = 4
    for m in range(2):
        t["qual"][m, :, 10] = 1
        t["qual"][m, :, 20] = 2
        t["qual"][m, :, 40] = 1          # phreds 10, 20, 20, 40 at every position: mean 22.5, quartiles 10 / 20 / 20
        t["base"][m, :, :] = [1, 1, 1, 0, 1]
        t["gc"][m, 2] = 4
        t["meanq"][m, 22] = 4
    t["insert"][[0, 7]] = [1, 3]
    return words, L


def test_merge_and_report():
    words, L = _hand_made()
    both = T.merge_tallies([words, words, words])
    assert both.dtype == np.uint64 and np.array_equal(both, 3 * words) and both is not words
    assert np.array_equal(T.merge_tallies([words]), words)
    with pytest.raises(ValueError):
        T.merge_tallies([words, words[:-1]])
    with pytest.raises(ValueError):
        T.merge_tallies([])
    rep = json.loads(json.dumps(T.report_dict(words, L)))  # (serialisable as it is)
    assert rep["pairs"] == 4 and rep["read_length"] == L and len(rep["mates"]) == 2
    for mate in rep["mates"]:
        assert mate["mean_phred"] == [22.5] * L
        assert mate["phred_q25"] == [10] * L and mate["phred_median"] == [20] * L and mate["phred_q75"] == [20] * L
        assert mate["base_fractions"] == {"A": [0.25] * L, "C": [0.25] * L, "G": [0.25] * L, "T": [0.0] * L, "other": [0.25] * L}
        assert mate["gc_histogram"] == [0, 0, 4] and mate["mean_quality_histogram"] == [0] * 22 + [4]
    assert rep["insert_size_histogram"] == [1, 0, 0, 0, 0, 0, 0, 3]
    blank = T.report_dict(np.zeros(T.tally_words(L), dtype=np.uint64), L)
    assert blank["pairs"] == 0 and blank["insert_size_histogram"] == [] and blank["mates"][0]["mean_phred"] == [None] * L
    assert blank["mates"][1]["phred_median"] == [None] * L
