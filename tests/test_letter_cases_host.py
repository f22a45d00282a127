"""The records, the ledger and the cases of tests/letter_cases.py, on the CPU.

* The ledger on a hand-built example of ten pairs where the class of every mate is written out.
* Every class a case names counts FLOOR hits per mate in the oracle's sample of the case, and the sample shows every placed
  letter on both strands: the GPU legs of tests/test_gpu_letter_cases.py compare what the ledger says they compare.
* The templates without the oracle's own letter rules: a read without a mutation row (and without padding) equals the genome
  slice, or its reverse complement through the thirty-entry table written out below -- case kept, W / S / N onto themselves,
  R <-> Y, K <-> M, B <-> V, D <-> H (util.py:57-88).
* Under the model whose every substitution test fires, every A/C/G/T/a/c/g/t of a template is substituted and every ambiguous
  letter is left alone (__init__.py:94, :190-192)."""
import numpy as np
import pytest

import letter_cases as LC

# util.rev_comp's table, written out
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "R": "Y", "Y": "R", "K": "M", "M": "K", "B": "V", "V": "B", "D": "H", "H": "D",
              "W": "W", "S": "S", "N": "N",
              "a": "t", "c": "g", "g": "c", "t": "a", "r": "y", "y": "r", "k": "m", "m": "k", "b": "v", "v": "b", "d": "h", "h": "d",
              "w": "w", "s": "s", "n": "n"}
assert len(COMPLEMENT) == 30
COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in COMPLEMENT.items():
    COMP[ord(_a)] = ord(_b)
AMBIGUOUS = np.zeros(256, dtype=bool)
AMBIGUOUS[list(b"RYWSMKHBVDNrywsmkhbvdn")] = True
ROW_DTYPE = np.dtype([("pair", "<i4"), ("mate", "i1"), ("type", "i1"), ("position", "<i2"), ("ref", "u1"), ("alt", "u1"), ("quality", "<i2")])


def _total(counts, k):
    return counts[k] if isinstance(counts[k], int) else min(counts[k])


# ------------------------------------------------------------------ the ledger, by hand
def test_ledger_on_ten_pairs_written_out():
    """Reads of 10 bases on 160 letters with exceptions at 32 (N: bit 0 of mask word 1), 63 (r: bit 31 of word 1), 90 .. 104 (a run
    of n) and 120 (a)."""
    RL = 10
    g = np.frombuffer(b"ACGT" * 40, dtype=np.uint8).copy()
    g[32], g[63], g[120] = ord("N"), ord("r"), ord("a")
    g[90:105] = ord("n")
    #         fs   rs     forward window                      reverse window
    pairs = [(0, 22),    # [0, 10)    none                     [22, 32)   none, 32 just above
             (32, 54),   # [32, 42)   lo_only                  [54, 64)   hi_only (63): 32 and 63 within 8 bases of the other window
             (33, 64),   # [33, 43)   none, 32 just below      [64, 74)   none, 63 just below
             (28, 58),   # [28, 38)   32 inside; group [28, 36) straddles 32 with its exception above: group_upper_word
             #                                                 [58, 68)   63 inside; group [60, 68) has it in the LOWER word
             (92, 105),  # [92, 102)  all                      [105, 115) none, 104 just below
             (80, 95),   # [80, 90)   none, 90 just above      [95, 105)  all
             (53, 120),  # [53, 63)   none, 63 just above      [120, 130) lo_only (120); 63 is 8 bases from the forward window
             (63, 130),  # [63, 73)   lo_only, lo_alone        [130, 140) none
             (23, 130),  # [23, 33)   hi_only, hi_alone; group [31, 33) straddles 32: group_upper_word
             #                                                 [130, 140) none
             (0, 26)]    # [0, 10)    none                     [26, 36)   32 inside; group [28, 36): group_upper_word
    coords = np.array([(fs, rs, rs + RL, rs - fs - RL) for fs, rs in pairs], dtype=np.int64)
    counts, masks = LC.ledger(g.tobytes().decode(), coords, RL, alone=8)
    assert counts == {"none": [5, 5], "lo_only": [2, 1], "hi_only": [1, 1], "below": [1, 2], "above": [2, 1], "all": [1, 1],
                      "group_upper_word": [2, 1], "lo_alone": [1, 0], "hi_alone": [1, 0], "one_mate_only": 6}
    assert np.flatnonzero(masks["none"][:, 0]).tolist() == [0, 2, 5, 6, 9] and np.flatnonzero(masks["none"][:, 1]).tolist() == [0, 2, 4, 7, 8]
    assert np.flatnonzero(masks["lo_only"][:, 0]).tolist() == [1, 7] and np.flatnonzero(masks["lo_only"][:, 1]).tolist() == [6]
    assert np.flatnonzero(masks["hi_only"][:, 0]).tolist() == [8] and np.flatnonzero(masks["hi_only"][:, 1]).tolist() == [1]
    assert np.flatnonzero(masks["below"][:, 0]).tolist() == [2] and np.flatnonzero(masks["below"][:, 1]).tolist() == [2, 4]
    assert np.flatnonzero(masks["above"][:, 0]).tolist() == [5, 6] and np.flatnonzero(masks["above"][:, 1]).tolist() == [0]
    assert np.flatnonzero(masks["all"][:, 0]).tolist() == [4] and np.flatnonzero(masks["all"][:, 1]).tolist() == [5]
    assert np.flatnonzero(masks["group_upper_word"][:, 0]).tolist() == [3, 8] and np.flatnonzero(masks["group_upper_word"][:, 1]).tolist() == [9]
    assert np.argwhere(masks["lo_alone"]).tolist() == [[7, 0]] and np.argwhere(masks["hi_alone"]).tolist() == [[8, 0]]
    assert np.flatnonzero(masks["one_mate_only"]).tolist() == [4, 5, 6, 7, 8, 9]
    assert masks["count"].tolist() == [[0, 0], [1, 1], [0, 0], [1, 1], [10, 0], [0, 10], [0, 1], [1, 0], [1, 0], [0, 1]]
    # within 64 bases (the default) nothing of this record is alone
    assert LC.ledger(g.tobytes().decode(), coords, RL)[0]["lo_alone"] == [0, 0]
    # mutation rows: (pair, mate, type 0 substitution / 1 insertion / 2 deletion, position, ref, alt, quality)
    rows = np.array([(0, 0, 2, 1, 65, 46, -1), (0, 0, 2, 4, 65, 46, -1), (0, 0, 1, 6, 65, 67, -1),  # net 1: pads with 10, plain
                     (1, 0, 0, 3, ord("A"), ord("C"), 30),                                          # an upper-case ref
                     (2, 1, 2, 3, 65, 46, -1),                                                      # net 1: pads with 63
                     (4, 1, 2, 3, 65, 46, -1), (4, 1, 2, 5, 65, 46, -1),                            # net 2: pads with 103, 104
                     (5, 0, 1, 2, 65, 71, -1),                                                      # an insertion: no padding
                     (6, 0, 2, 7, 65, 46, -1),                                                      # net 1: pads with 63
                     (6, 1, 0, 9, ord("t"), ord("G"), 12),                                          # the complement of the a at 120
                     (9, 1, 2, 0, 65, 46, -1)],                                                     # net 1: pads with 25, plain
                    dtype=ROW_DTYPE)
    counts, masks = LC.ledger(g.tobytes().decode(), coords, RL, rows)
    assert counts["pad_takes_exception"] == [1, 2] and counts["lower_substituted"] == [0, 1]
    assert np.argwhere(masks["pad_takes_exception"]).tolist() == [[2, 1], [4, 1], [6, 0]]
    assert np.argwhere(masks["has_rows"]).tolist() == [[0, 0], [1, 0], [2, 1], [4, 1], [5, 0], [6, 0], [6, 1], [9, 1]]


# ------------------------------------------------------------------ the records
@pytest.mark.parametrize("RL", [33, 126, 151, 301])
def test_records_are_what_they_say(RL):
    P = LC.period(RL)
    assert P % 32 == 0 and RL + 9 <= P < RL + 9 + 32
    for kind, bit in (("bit0", 0), ("bit31", 31)):
        g = LC._bytes(LC.record(kind, RL))
        at = np.flatnonzero(~LC.PLAIN[g])
        assert len(g) == 40 * P and at.tolist() == list(range(bit, len(g), P))
        assert g[at].tobytes() == (LC.LETTERS * 2)[:len(at)]
    Q = LC.sparse_period(RL)
    assert Q % 32 == 0 and 4 * RL <= Q < 4 * RL + 32
    for kind, bit in (("sparse0", 0), ("sparse31", 31)):
        g = LC._bytes(LC.record(kind, RL))
        assert len(g) == 48 * Q and np.flatnonzero(~LC.PLAIN[g]).tolist() == list(range(bit, len(g), Q))
    g = LC._bytes(LC.record("odd", RL))
    at = np.flatnonzero(~LC.PLAIN[g])
    assert at[0] == 5 and len(set(np.diff(at))) == 1 and np.diff(at)[0] in (RL + 10, RL + 11) and np.diff(at)[0] % 2 == 1
    assert set(at % 32) == set(range(32))
    runs, soft, base = (LC._bytes(LC.record(k, RL)) for k in ("runs", "soft", "plain"))
    at = np.flatnonzero(runs == ord("N"))
    starts = at[np.concatenate([[True], np.diff(at) > 1])]
    assert len(at) == len(starts) * (2 * RL + 7) and set(np.diff(starts)) == {6 * RL + 13} and len(starts) >= 5
    assert np.array_equal(np.flatnonzero(~LC.PLAIN[soft]), at) and set(soft[at].tolist()) == set(b"acgt")
    assert LC.PLAIN[base].all()


@pytest.mark.parametrize("RL", [33, 151])
def test_ends_are_what_they_say(RL):
    recs, counts, where = LC.ends(RL)
    assert sum(counts) == LC.ENDS_PAIRS and where[0] is None and where[-1] is None
    assert all((a is None) != (b is None) for a, b in zip(where, where[1:]))  # a plain record before, between and behind
    seen = set()
    for seq, p in zip(recs, where):
        g, L = LC._bytes(seq), len(seq)
        assert np.flatnonzero(~LC.PLAIN[g]).tolist() == ([] if p is None else [p])
        if p is not None:
            seen.add((L, p))
    assert seen == {(L, p) for L in [RL + 1] + [2 * RL + k for k in (0, 1, 31, 32, 33)] for p in (0, RL - 1, RL, L - RL - 1, L - RL, L - 1)}


# ------------------------------------------------------------------ the floor
@pytest.mark.parametrize("cid", [c.id for c in LC.CASES])
def test_every_named_class_meets_the_floor(cid):
    c = LC.case(cid)
    counts, _ = LC.case_ledger(cid)
    print(cid, dict(counts))
    for k in c.named:
        assert _total(counts, k) >= LC.FLOOR, (cid, k, counts[k])
    if c.record in ("bit0", "bit31", "odd", "sparse0", "sparse31"):  # every placed letter, on both strands
        fwd, rev = LC.letters_met(LC.case_record(c), LC.oracle_rows(cid)["coords"], LC.model(c.model).read_length)
        assert fwd == rev == set(LC.LETTERS)
    if c.rng == "mt":  # about half the pairs touch a letter: the walker's; the rest are the resolver's
        touched = (LC.case_ledger(cid)[1]["count"] > 0).any(axis=1).mean()
        assert 0.35 < touched < 0.6, touched


@pytest.mark.parametrize("name", LC.ENDS_MODELS)
def test_ends_batch_meets_the_floor(name):
    total = LC.ends_ledger(name)
    print(name, dict(total))
    for o in range(2):
        for k in LC.ENDS_NAMED[o]:
            assert total[k, o] >= LC.FLOOR, (name, k, o, total[k, o])
    # every pair of a record is the same pair in amplicon mode
    RL = LC.model(name).read_length
    for seq, res in zip(LC.ends(RL)[0], LC.ends_oracle(name)):
        assert (res["coords"][:, 0] == 0).all() and (res["coords"][:, 2] == len(seq)).all() and (res["coords"][:, 1] == len(seq) - RL).all()


def test_worker_set_case_meets_the_floor():
    RL = LC.model(LC.WORKER_MODEL).read_length
    total = {k: [0, 0] for k in LC.BOUNDARY}
    for w in range(len(LC.WORKER_SEEDS)):
        counts, _ = LC.ledger(LC.record(LC.WORKER_RECORD, RL), LC.worker_oracle(w)["coords"], RL)
        for k in LC.BOUNDARY:
            total[k] = [a + b for a, b in zip(total[k], counts[k])]
    print(total)
    assert all(min(v) >= LC.FLOOR for v in total.values()), total


def test_batch_middle_item_meets_the_floor():
    counts, _ = LC.ledger(LC.batch_records(151)[1], LC.batch_oracle()[1]["coords"], 151)
    print(dict(counts))
    for k in LC.BOUNDARY:
        assert min(counts[k]) >= LC.FLOOR, (k, counts[k])
    for k in (0, 2):
        assert LC.ledger(LC.batch_records(151)[k], LC.batch_oracle()[k]["coords"], 151)[0]["none"] == [LC.BATCH_COUNTS[k]] * 2


# ------------------------------------------------------------------ the templates, without the oracle's letter rules
def _templates(c, coords):
    g = LC._bytes(LC.case_record(c))
    ar = np.arange(LC.model(c.model).read_length)
    return g[coords[:, 0:1] + ar], COMP[g[coords[:, 2:3] - 1 - ar]]


@pytest.mark.parametrize("cid", ["novaseq-odd-vcf", "novaseq-soft-vcf", "novaseq-runs", "novaseq-bit0", "miseq-bit31", "perfect33-bit0"])
def test_untouched_reads_are_the_genome_slice_or_its_reverse_complement(cid):
    """(Not the models with raised indel rates or phreds below 9: no read of theirs is without a row.)"""
    c = LC.case(cid)
    res = LC.oracle_rows(cid, mutations=True)
    _, masks = LC.case_ledger(cid, mutations=True)
    fwd, rev = _templates(c, res["coords"])
    assert (rev != 0).all()  # (every letter of the records has an entry in the table)
    for o, (tmpl, key) in enumerate(((fwd, "r1_base"), (rev, "r2_base"))):
        keep = ~masks["has_rows"][:, o] & ~masks["pad_takes_exception"][:, o]
        assert keep.sum() > 256 and (masks["count"][keep, o] > 0).sum() > 100, (keep.sum(), (masks["count"][keep, o] > 0).sum())
        assert np.array_equal(res[key][keep], tmpl[keep]), (cid, o)


@pytest.mark.parametrize("cid", ["hiseq-fires-odd", "hiseq-fires-runs"])
def test_every_test_fires_on_acgt_and_never_on_an_ambiguous_letter(cid):
    c = LC.case(cid)
    res = LC.oracle_rows(cid, mutations=True)
    for k in ("r1_base", "r2_base", "r1_qual", "r2_qual"):  # (the rows' bookkeeping changes no read)
        assert np.array_equal(res[k], LC.oracle_rows(cid)[k])
    rows = res["mutations"]
    indel = np.zeros((c.pairs, 2), dtype=bool)
    indel[rows["pair"][rows["type"] != 0], rows["mate"][rows["type"] != 0]] = True
    fwd, rev = _templates(c, res["coords"])
    seen = 0
    for o, (tmpl, key) in enumerate(((fwd, "r1_base"), (rev, "r2_base"))):
        keep = ~indel[:, o]
        assert keep.sum() > c.pairs // 2
        t, b = tmpl[keep], res[key][keep]
        amb = AMBIGUOUS[t]
        assert (b[amb] == t[amb]).all() and (b[~amb] != t[~amb]).all(), (cid, o)
        seen += int(amb.sum())
    assert seen >= LC.FLOOR
