"""Every reader of genome letters against the oracle on the records of tests/letter_cases.py: IUPAC codes and lower-case letters
placed on the mask-word boundaries, whole reads inside runs of N and of soft-masked bases, records whose only exception is the
first or last base of a window or the base just outside it.

tests/test_letter_cases_host.py proves from the oracle's coordinates alone that the pairs of every case meet what the case
names (FLOOR windows per mate whose single exception is their first / last base, clean windows beside an exception, windows
inside a run, lane groups with their exceptions in the upper mask word only, pairs with one flagged mate).  Here the device runs
the same calls: rows, phreds and coordinates equal the oracle's bit for bit, and the kernel that ran is the one the leg names.

  1  k_main<false, false, false> on NovaSeq, MiSeq (five position tiles) and a 33-base model; few workgroups on one case each
  2  --store_mutations (k_main<true, false, false>): every row field by field, `ref` of lower-case and complemented letters
  3  indels: edit scripts and k_indel_fixup on records with exceptions (padding from beyond the template), and the light route
  4  every substitution test fires: main_slow_base's "leave it alone" for every ambiguous letter of a read
  5  k_perfect, and the `ends` batch
  6  batches: `ends` in amplicon mode; plain, bit31, plain under an indel-heavy model -- scripted reads and fix-up in one launch
  7  rng="mt": generate_mt and generate_mt_workers where half the pairs touch a letter -- walked == touched exactly

Tried once each against a scratch build with one planted defect (never committed; each changes which mask words are consulted
or which letter is written, none an address); the tests each turns red:

* k_setup scanning the forward window to `(fs + RL - 2) >> 5`: test_plain_path_matches_the_oracle[novaseq-sparse0],
  test_every_test_fires_matches_the_oracle[hiseq-fires-runs], test_perfect_matches_the_oracle[perfect33-bit0] and
  [perfect151-sparse0], test_ends_batch_matches_the_oracle[perfect33].  Not the bit0 / bit31 / odd legs of NovaSeq and MiSeq,
  whose hi_only count is a hundred: k_setup ORs whole mask words, and k_main's branch reads both masks when EITHER mate is
  flagged -- at a period of RL + 9 .. RL + 40 the next letter always lies in a word scanned for the other mate.  Hence the
  sparse records on the Philox path and the ledger's lo_alone / hi_alone.
* k_setup scanning the reverse window from `(rs + 1) >> 5`: test_plain_path_matches_the_oracle[novaseq-sparse31],
  test_perfect_matches_the_oracle[perfect33-bit31], [perfect33-runs] and [perfect151-sparse31].
* k_main's forward mask from one word (`funnel_r(mw[0], 0, ..)`): every leg of test_plain_path_matches_the_oracle,
  test_store_mutations_rows_match_the_oracle, test_light_route_matches_the_oracle and test_every_test_fires_matches_the_oracle
  on bit0, odd, runs, soft and sparse0 -- the records that name group_upper_word -- and none on bit31 / sparse31.
* exceptions_in's last-word mask shifted by `32 - ..`: test_mt_case_matches_the_oracle[RL159-NB4-noisy-sparse31] and
  [RL246-NB1-noisy-sparse31], test_mt_worker_set_matches_the_oracle (on sparse0 the shift is by 32 bits, which the hardware
  takes as 0: the mask stays whole).
* complement_ascii mapping B to B: every leg on bit0, bit31, odd and the MT legs on sparse0 / sparse31, the batch and the worker
  set (26 of the 42 tests tried; the Philox legs on the sparse records came later).  Not the legs on runs / soft (no B) nor
  the `ends` batches (the two records with a B or b have it at position 0: the forward window only)."""
import numpy as np
import pytest

import letter_cases as LC
from helpers import model_geometry

pytestmark = pytest.mark.gpu

KEYS = ("r1_qual", "r2_qual", "r1_base", "r2_base")
MUT_FIELDS = ("pair", "mate", "type", "position", "ref", "alt", "quality")
SWITCHES = ("ISS_TILES", "ISS_GUIDE_BITS", "ISS_MAIN_GROUP", "ISS_MAIN_GROUP_MIN", "ISS_LIGHT_INDELS", "ISS_MAIN_WGS", "ISS_CHUNK_PAIRS",
            "ISS_PERFECT_KERNEL", "ISS_SETUP_AHEAD", "ISS_MT_PATH", "ISS_MT_GUARD", "ISS_MT_SET_TURN", "ISS_MT_SET_BUF_TURNS")
N_TILES = {"novaseq": 1, "miseq": 5, "syn33": 1}


@pytest.fixture(scope="module")
def engine():
    from insilicoseq_amd.engine import ReadEngine

    eng = ReadEngine(0)
    yield eng
    eng.close()


def _load(engine, monkeypatch, name, env=None, capfd=None):
    """Upload the model `name` with none of the library's switches set but `env`; the engine holds no record afterwards."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if capfd is not None:
        monkeypatch.setenv("ISS_DEBUG_MODEL", "1")
        capfd.readouterr()
    engine.load_model(LC.model(name))
    engine.clear_genomes()
    engine.stats_read()
    return model_geometry(capfd.readouterr().err) if capfd is not None else None


def _assert_rows(got, coords, exp, what):
    assert np.array_equal(coords, exp["coords"]), (what, "pair coordinates differ", np.flatnonzero((coords != exp["coords"]).any(axis=1))[:5])
    for k in KEYS:
        bad = np.argwhere(got[k] != exp[k])
        assert bad.size == 0, "%s: %s differs at (pair, pos) %s ... (%d cells)" % (what, k, bad[:5].tolist(), len(bad))


def _assert_mutations(got, exp, what):
    assert len(got) == len(exp) and len(exp) > 0, (what, len(got), len(exp))
    for f in MUT_FIELDS:
        bad = np.flatnonzero(got[f] != exp[f])
        assert bad.size == 0, (what, f, bad[:5], got[bad[:3]], exp[bad[:3]])


def _run(engine, c, exp, kernel, mutations=False):
    """One generate call of the case on the loaded model against the oracle's rows `exp`."""
    gid = engine.add_genome(LC.case_record(c))
    engine.mutations_reserve(4_000_000 if mutations else 0)
    try:
        engine.generate(gid, c.pairs, first_ordinal=LC.FIRST_ORDINAL, seed=LC.SEED)
        engine.synchronize()
        assert engine.main_kernel() == kernel, (c.id, engine.main_kernel())
        _assert_rows(engine.download(0, c.pairs), engine.coords(0, c.pairs), exp, c.id)
        if mutations:
            _assert_mutations(engine.mutations(), exp["mutations"], c.id)
    finally:
        engine.mutations_reserve(0)
    return engine.stats_read()


# ------------------------------------------------------------------ 1: the plain Philox path
FEW_WORKGROUPS = ("novaseq-odd", "miseq-bit0", "syn33-runs")  # ISS_MAIN_WGS=3: a workgroup makes many passes
PLAIN_LEGS = ([("%s-%s" % (mo, rec), None) for mo in LC.PLAIN_MODELS for rec in LC.PLAIN_RECORDS]
              + [("novaseq-sparse0", None), ("novaseq-sparse31", None)] + [(cid, "3") for cid in FEW_WORKGROUPS])


@pytest.mark.parametrize("cid,wgs", PLAIN_LEGS, ids=[cid + ("-wgs" + w if w else "") for cid, w in PLAIN_LEGS])
def test_plain_path_matches_the_oracle(engine, cid, wgs, capfd, monkeypatch):
    c = LC.case(cid)
    geo = _load(engine, monkeypatch, c.model, {"ISS_MAIN_WGS": wgs} if wgs else None, capfd)
    assert geo.n_tiles == N_TILES[c.model], geo
    _run(engine, c, LC.oracle_rows(cid), "k_main<false, false, false>")


def test_a_record_without_exceptions_keeps_the_plain_kernel(engine, monkeypatch):
    """(What the legs above are not: the same model on the plain record launches a PLAIN kernel.)"""
    _load(engine, monkeypatch, "novaseq")
    gid = engine.add_genome(LC.record("plain", 151))
    engine.generate(gid, 256, first_ordinal=LC.FIRST_ORDINAL, seed=LC.SEED)
    engine.synchronize()
    assert engine.main_kernel() in ("k_main<false, true, false>", "k_main_g<5, 1>"), engine.main_kernel()


# ------------------------------------------------------------------ 2: --store_mutations
@pytest.mark.parametrize("cid", ["novaseq-odd-vcf", "novaseq-soft-vcf"])
def test_store_mutations_rows_match_the_oracle(engine, cid, monkeypatch):
    c = LC.case(cid)
    exp = LC.oracle_rows(cid)
    rows = exp["mutations"]
    lower = rows[(rows["type"] == 0) & (rows["ref"] >= 97)]
    assert len(lower) > 0 and set(lower["mate"].tolist()) == {0, 1}  # lower-case refs of both mates (the reverse one: complemented)
    _load(engine, monkeypatch, c.model)
    _run(engine, c, exp, "k_main<true, false, false>", mutations=True)


# ------------------------------------------------------------------ 3: indels on records with exceptions
@pytest.mark.parametrize("cid,mutations", [("novaseq-indel-odd", True), ("novaseq-indel-runs", False)])
def test_indel_heavy_model_matches_the_oracle(engine, cid, mutations, monkeypatch):
    """NovaSeq with indel rates (0.01, 0.03): k_main<.., false, true>; the reads of a record with exceptions are k_indel_fixup's,
    and a deletion's padding pulls letters in from beyond the template (pad_takes_exception of the ledger)."""
    c = LC.case(cid)
    _load(engine, monkeypatch, c.model)
    stats = _run(engine, c, LC.oracle_rows(cid, mutations), "k_main<%s, false, true>" % ("true" if mutations else "false"), mutations)
    assert stats["fixup_reads"] > 0, stats


@pytest.mark.parametrize("cid", ["novaseq-odd", "miseq-odd"])
def test_light_route_matches_the_oracle(engine, cid, monkeypatch):
    """The models as shipped: few reads have an indel event (NovaSeq: 2 in 10^5, none in this sample; MiSeq: 1.4 in 10^3), k_setup
    finds them and each goes to k_indel_fixup behind k_main as it is -- on a record where nineteen windows in twenty are flagged."""
    c = LC.case(cid)
    rows = LC.oracle_rows(cid, mutations=True)["mutations"]
    events = rows[rows["type"] != 0]
    reads = len(set(zip(events["pair"].tolist(), events["mate"].tolist())))
    assert reads >= LC.FLOOR or c.model == "novaseq", reads
    _load(engine, monkeypatch, c.model)
    stats = _run(engine, c, LC.oracle_rows(cid), "k_main<false, false, false>")
    assert stats["fixup_reads"] >= reads and stats["scripted_reads"] == 0, (stats, reads)


# ------------------------------------------------------------------ 4: every test fires
@pytest.mark.parametrize("cid", ["hiseq-fires-odd", "hiseq-fires-runs"])
def test_every_test_fires_matches_the_oracle(engine, cid, monkeypatch):
    c = LC.case(cid)
    _load(engine, monkeypatch, c.model)
    _run(engine, c, LC.oracle_rows(cid), "k_main<false, false, false>")


# ------------------------------------------------------------------ 5: k_perfect
@pytest.mark.parametrize("cid", ["perfect%d-%s" % (RL, rec) for RL in (151, 33) for rec in ("bit0", "bit31", "runs")] + ["perfect151-sparse0", "perfect151-sparse31"])
def test_perfect_matches_the_oracle(engine, cid, monkeypatch):
    c = LC.case(cid)
    _load(engine, monkeypatch, c.model)
    _run(engine, c, LC.oracle_rows(cid), "k_perfect")


# ------------------------------------------------------------------ 5, 6: the batches
def _run_batch(engine, recs, counts, exp, sequence_type, kernel, what):
    gids = [engine.add_genome(seq) for seq in recs]
    engine.generate_batch(gids, list(counts), first_ordinal=LC.FIRST_ORDINAL, seed=LC.SEED, sequence_type=sequence_type, out_first_pair=0)
    engine.synchronize()
    assert engine.main_kernel() == kernel, (what, engine.main_kernel())
    row = 0
    for k, (n, res) in enumerate(zip(counts, exp)):
        _assert_rows(engine.download(row, n), engine.coords(row, n), res, (what, "item", k))
        row += n
    return engine.stats_read()


@pytest.mark.parametrize("name", LC.ENDS_MODELS)
def test_ends_batch_matches_the_oracle(engine, name, monkeypatch):
    """Amplicon mode, one launch over the small records: every pair of a record has its exception on the first or last base of a
    window or just outside one; plain records before, between and behind."""
    _load(engine, monkeypatch, name)
    recs, counts, _ = LC.ends(LC.model(name).read_length)
    _run_batch(engine, recs, counts, LC.ends_oracle(name), "amplicon", "k_perfect" if name.startswith("perfect") else "k_main<false, false, false>",
               "ends, " + name)


def test_batch_of_plain_and_exception_records_matches_the_oracle(engine, monkeypatch):
    """plain, bit31, plain under NovaSeq with indel rates (0.001, 0.003): the plain items' reads with events are built from edit
    scripts, the middle item's by k_indel_fixup, in one launch; each item equals its own oracle run, ordinals running on."""
    _load(engine, monkeypatch, "novaseq-batch")
    stats = _run_batch(engine, LC.batch_records(151), LC.BATCH_COUNTS, LC.batch_oracle(), "metagenomics", "k_main<false, false, true>", "batch")
    assert stats["scripted_reads"] > 0 and stats["fixup_reads"] > 0, stats


# ------------------------------------------------------------------ 7: MT mode
def _res53(words):
    w = words.astype(np.uint64)
    return ((w[0::2] >> np.uint64(5)) * np.uint64(67108864) + (w[1::2] >> np.uint64(6))).astype(np.float64) / 9007199254740992.0


def _load_mt(engine, monkeypatch, name):
    import mt_resolver_cases as M

    _load(engine, monkeypatch, name)
    assert engine.mt_resolver() == M.case(name).pick, (name, engine.mt_resolver())


def _touched(rec, coords, RL):
    return int((LC.ledger(rec, coords, RL)[1]["count"] > 0).any(axis=1).sum())


@pytest.mark.parametrize("cid", [c.id for c in LC.CASES if c.rng == "mt"])
def test_mt_case_matches_the_oracle(engine, cid, monkeypatch):
    c = LC.case(cid)
    exp = LC.oracle_rows(cid)
    _load_mt(engine, monkeypatch, c.model)
    gid = engine.add_genome(LC.case_record(c))
    engine.seed_mt(LC.MT_SEED)
    r0, w0 = engine.mt_path_counts()
    assert engine.generate_mt(gid, c.pairs) == c.pairs
    resolved, walked = (a - b for a, b in zip(engine.mt_path_counts(), (r0, w0)))
    _assert_rows(engine.download(0, c.pairs), engine.coords(0, c.pairs), exp, cid)
    py, npw = engine.mt_peek(8)
    assert (list(_res53(py)), list(_res53(npw))) == exp["next_words"], cid  # both streams stand where the oracle's stand
    touched = _touched(LC.case_record(c), exp["coords"], LC.model(c.model).read_length)
    assert resolved + walked == c.pairs and walked == touched, (resolved, walked, touched)


def test_mt_worker_set_matches_the_oracle(monkeypatch):
    """Three workers side by side (k_mt_resolve_w, k_mt_emit_w) with pair counts of their own: each worker's rows, coordinates and
    next stream words equal those of an oracle run of its seed."""
    from insilicoseq_amd.engine import ReadEngine

    W = len(LC.WORKER_SEEDS)
    RL = LC.model(LC.WORKER_MODEL).read_length
    rec = LC.record(LC.WORKER_RECORD, RL)
    first = [sum(LC.WORKER_PAIRS[:w]) for w in range(W)]
    with ReadEngine(0) as eng:
        _load_mt(eng, monkeypatch, LC.WORKER_MODEL)
        gid = eng.add_genome(rec)
        eng.seed_mt_workers(list(LC.WORKER_SEEDS))
        eng.reserve(sum(LC.WORKER_PAIRS))
        r0, w0 = eng.mt_path_counts()
        done, status = eng.generate_mt_workers([gid] * W, list(LC.WORKER_PAIRS), first)
        assert list(done) == list(LC.WORKER_PAIRS) and list(status) == [0] * W
        resolved, walked = (a - b for a, b in zip(eng.mt_path_counts(), (r0, w0)))
        touched = 0
        for w in range(W):
            exp = LC.worker_oracle(w)
            n = LC.WORKER_PAIRS[w]
            _assert_rows(eng.download(first[w], n), eng.coords(first[w], n), exp, ("worker", w))
            py, npw = eng.mt_workers_peek(w, 8)
            assert (list(_res53(py)), list(_res53(npw))) == exp["next_words"], w
            touched += _touched(rec, exp["coords"], RL)
        assert resolved + walked == sum(LC.WORKER_PAIRS) and walked == touched, (resolved, walked, touched)
