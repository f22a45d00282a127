"""The Philox path's indel events on the device, held to the model's tables (tests/philox_indel_stats.py; DESIGN section 4, "What
holds the map to the model").  tests/test_gpu_philox_stats.py stops where indels begin; here the --store_mutations rows of a
generate call are replayed into the state of every step of the reference's loop, exactly (I0), and the events are held to the
tables (I1) and to their independence of the phreds (I2), of the error path (I3, and S5 .. S7 with the replayed sequence as
template), of each other -- earlier steps, the other mate, neighbouring pairs, another seed, another call (I4) -- and of the
coordinates (I5), at the sizes at which tests/test_philox_indel_stats_host.py shows every kept planted defect rejected.
Cases: `flat` (NovaSeq, indel rates 0.001 / 0.003, plain genome: the scripted route), `patterned` (MiSeq, tables that differ by
mate, position and letter, mixed genome: the fix-up route), the same tables on the plain genome (both routes), the first steps
of `flat` at the cap of 2^20 pairs, two seeds, two calls, the shipped NovaSeq tables, the device's MT path -- and the rows
themselves against the oracle's at a size where a wavefront records many reads, which is what the replay found broken.

A case is generated and replayed once (slices over host threads) and its statistics are shared by the test functions; all
hypotheses of a test function share philox_stats.ALPHA (Bonferroni); seeds are fixed."""
import os
import time

import numpy as np
import pytest

import philox_indel_stats as IS
import philox_stats as PS
from helpers import dense_model, random_genome
from philox_indel_stats import GENOME, all_stats, assert_accepted, case_model

pytestmark = pytest.mark.gpu

SEED = 2024
KERNEL = {"flat": "k_main<true, true, true>", "patterned": "k_main<true, false, true>", "patterned-plain": "k_main<true, true, true>",
          "shipped": "k_main<true, true, false>"}
CASES = ["flat", "patterned", "patterned-plain"]
THREADS = max(1, min(16, os.cpu_count() or 1))
STEP = 1 << 13
_DONE = {}


class LazySlice(dict):
    """A slice that is replayed by the host thread that first looks at it."""

    def __init__(self, build):
        dict.__init__(self)
        self._build = build

    def __missing__(self, key):
        if self._build is None:
            raise KeyError(key)
        build, self._build = self._build, None
        self.update(build())
        return self[key]


@pytest.fixture(scope="module")
def engine():
    from insilicoseq_amd.engine import ReadEngine

    eng = ReadEngine(0)
    yield eng
    eng.mutations_reserve(0)
    eng.close()


@pytest.fixture(autouse=True)
def _host_picks_the_kernel(monkeypatch):
    for k in ("ISS_MAIN_GROUP", "ISS_MAIN_GROUP_MIN", "ISS_MAIN_WGS", "ISS_TILES", "ISS_CHUNK_PAIRS", "ISS_LIGHT_INDELS"):
        monkeypatch.delenv(k, raising=False)


def _load(engine, dense, genome):
    engine.load_model(dense)
    engine.clear_genomes()
    return engine.add_genome(genome)


def _generate(engine, dense, gid, n, seed, first_ordinal, row, kernel):
    """One generate call with row capture: its rows in the order of iss_mutations_download."""
    from insilicoseq_amd.tensors import default_mutation_slots

    engine.mutations_reserve(default_mutation_slots(dense, n))
    engine.generate(gid, n, first_ordinal=first_ordinal, seed=seed, out_first_pair=row)
    engine.synchronize()
    assert engine.main_kernel() == kernel
    return engine.mutations()


def _slices(engine, t, genome, row, n, rows, step=STEP):
    """Lazy slices of output rows [row, row + n) of the call whose mutation rows are ``rows``."""
    for a in range(0, n, step):
        m = min(step, n - a)
        got, coords, part = engine.download(row + a, m), engine.coords(row + a, m), IS.rows_of(rows, a, m)
        bases, quals = PS.stack_mates(got["r1_base"], got["r2_base"]), PS.stack_mates(got["r1_qual"], got["r2_qual"])
        yield LazySlice(lambda coords=coords, bases=bases, quals=quals, part=part: IS.indel_slice(t, genome, coords, bases, quals, part))


def _verdict(what, results):
    ok, text = PS.accept(results)
    print("\n[philox-indel-stats] %s: %s" % (what, text))
    assert ok, text


def _case(engine, case):
    """The statistics of a case, from one generation and one replay."""
    if case not in _DONE:
        t0 = time.time()
        dense, genome, mixed = case_model(case)
        t, x, n = IS.Tables(dense), PS.Expect(dense), IS.N_PAIRS[case]
        gid = _load(engine, dense, genome)
        engine.reserve(n)
        engine.stats_read()  # (the counters run on until they are read)
        rows = _generate(engine, dense, gid, n, SEED, 0, 0, KERNEL[case])
        shares = engine.stats_read()
        stats = PS.run_stats(lambda: all_stats(dense, t, x, mixed), _slices(engine, t, genome, 0, n, rows), THREADS)
        if case == "flat":  # the variants without rows make the same reads
            first = engine.download(0, STEP)
            first = {k: v.copy() for k, v in first.items() if k != "_pitched"}
            engine.mutations_reserve(0)
            engine.generate(gid, STEP, first_ordinal=0, seed=SEED)
            engine.synchronize()
            assert engine.main_kernel() == "k_main<false, true, true>"
            again = engine.download(0, STEP)
            for k, v in first.items():
                assert np.array_equal(v, again[k]), k
        indel_rows = int((rows["type"] != 0).sum())
        print("\n[philox-indel-stats] %s: %d pairs, %s, %d rows, %.2f indel rows per read, fix-up reads %.4f, scripted reads %.4f of the "
              "reads, excluded steps %.4f %%, I0 %s, %.2f s" % (case, n, KERNEL[case], len(rows), indel_rows / (2.0 * n), shares["fixup_reads"] / (2.0 * n),
                                                               shares["scripted_reads"] / (2.0 * n), 100 * stats[1].excluded_share(), dict(stats[0].i0),
                                                               time.time() - t0))
        _DONE[case] = (stats, shares, indel_rows / (2.0 * n))
    return _DONE[case]


def _of(stats, *classes):
    return [r for st in stats if isinstance(st, classes) for r in st.results()]


@pytest.mark.parametrize("case", CASES)
def test_the_rows_replay_exactly_and_the_rates_are_the_tables(engine, case):
    """I0 and I1; the hidden deletion tests are at most 0.5 % of the live steps.  The routes: on the mixed genome every read with
    an event is k_indel_fixup's (k_indel_script works on records of plain A, C, G, T only), so the patterned tables run on the
    plain genome as well, where the reads are scripted but for those with more events than a list holds: both routes."""
    stats, shares, per_read = _case(engine, case)
    assert not stats[0].failures(), stats[0].i0
    assert stats[1].live > 0 and stats[1].excluded_share() <= IS.EXCLUDED_SHARE
    assert 0.9 < per_read < 1.2 if case == "flat" else 1.6 < per_read < 2.0
    if case == "patterned":
        assert shares["fixup_reads"] > 0 and shares["scripted_reads"] == 0, shares
    else:
        assert shares["scripted_reads"] > 0, shares
    if case == "patterned-plain":
        assert shares["fixup_reads"] > 0, shares
    _verdict("%s I1" % case, _of(stats, IS.I1))


@pytest.mark.parametrize("case", CASES)
def test_events_against_phreds(engine, case):
    """I2: `K_EV` against `K_QM` / `K_QM_LO`."""
    _verdict("%s I2" % case, _of(_case(engine, case)[0], IS.I2))


@pytest.mark.parametrize("case", CASES)
def test_events_against_the_error_path(engine, case):
    """S5, S6, S7 with the replayed sequence as template (a table indexed before the shift), and I3: `K_EV` against `K_SUB` and
    the error-test digit."""
    _verdict("%s S5-S7 I3" % case, _of(_case(engine, case)[0], PS.S5, PS.S6, PS.S7, IS.I3))


@pytest.mark.parametrize("case", CASES)
def test_events_against_events(engine, case):
    """I4: earlier steps of the mate (draw j against draw j + 1), the other mate, pair i + k."""
    _verdict("%s I4" % case, _of(_case(engine, case)[0], IS.I4))


@pytest.mark.parametrize("case", CASES)
def test_events_against_coordinates(engine, case):
    """I5: `K_EV` against `K_PAIR` / `K_FS`."""
    _verdict("%s I5" % case, _of(_case(engine, case)[0], IS.I5))


def test_the_rows_are_the_oracles_when_a_wavefront_records_many_reads(engine):
    """Parity of the rows themselves, at a size the row tests of small samples do not reach: more fix-up reads than the fix-up's
    grid has wavefronts (8 workgroups of 4 per compute unit), so that a wavefront records read after read into its chunk of row
    slots, at a read length that is no multiple of 64, and k_main's short exact-path rounds on a noisy model.  The replay found
    it: 8 % of the rows were missing (a lane that sat out a trip kept a stale chunk state and placed its next rows onto slots in
    use), the reads themselves were right."""
    from oracle import oracle as O

    dense, genome, _ = case_model("patterned")
    n = 1 << 14
    gid = _load(engine, dense, genome)
    engine.reserve(n)
    engine.stats_read()
    rows = _generate(engine, dense, gid, n, SEED, 0, 0, KERNEL["patterned"])
    assert engine.stats_read()["fixup_reads"] > 2 * 8 * 4 * 256
    exp = O.Oracle(dense).simulate(O.Rng().seed_philox(SEED), genome, n, store_mutations=True)
    assert exp["status"] == 0 and exp["n_done"] == n
    got = engine.download(0, n)
    for k in ("r1_base", "r1_qual", "r2_base", "r2_qual"):
        assert np.array_equal(got[k], exp[k][:, :dense.read_length]), k
    assert len(rows) == len(exp["mutations"]), (len(rows), len(exp["mutations"]))
    assert np.array_equal(rows, exp["mutations"])


def test_adjacent_draws_at_the_cap(engine):
    """I1 and I4 over the first CAP_STEPS steps of both mates at 2^20 pairs of the flat case: the size at which one read in a
    hundred drawing step n + 1 from step n's block is rejected.  Cut by positions, and said so: the state of a step needs
    nothing behind it, so the case reads coordinates and the early indel rows, no bases."""
    dense, genome, _ = case_model("flat")
    t, n = IS.Tables(dense, steps=IS.CAP_STEPS), IS.N_PAIRS["flat-cap"]
    gid = _load(engine, dense, genome)
    engine.reserve(n)
    rows = _generate(engine, dense, gid, n, SEED, 0, 0, KERNEL["flat"])
    early = rows[(rows["type"] != 0) & (rows["position"] < IS.CAP_STEPS)]

    def slices(step=1 << 16):
        for a in range(0, n, step):
            coords, part = engine.coords(a, step), IS.rows_of(early, a, step)
            yield LazySlice(lambda coords=coords, part=part: IS.indel_slice(t, genome, coords, None, None, part))

    stats = PS.run_stats(lambda: [IS.I0(), IS.I1(t), IS.I4(t)], slices(), THREADS)
    assert not stats[0].failures(), stats[0].i0
    assert stats[1].n == n and len(early) > 0
    _verdict("flat-cap I1, %d pairs, first %d steps" % (n, IS.CAP_STEPS), stats[1].results())
    _verdict("flat-cap I4, %d pairs, first %d steps" % (n, IS.CAP_STEPS), stats[2].results())


class _TwoSets(object):
    """I4 between two sets of rows, slice by slice, with I0 and I1 over both (rows that are not what they should be would pass
    a test of independence); ``seam``: the last slice of the first set and the first of the second touch."""

    def __init__(self, t, key):
        self.key, self.i4, self.i1, self.i0 = key, IS.I4(t, lags=(), within=False), IS.I1(t), IS.I0()

    def add(self, s):
        self.i4.add_cross(self.key, s["a"], s["b"])
        if s.get("seam"):
            a, b = s["seam"]
            for k in PS.LAGS:  # pair n - k + i of the first call against pair i of the second
                self.i4._acc("seam lag %d" % k, a["E2"][-k:], b["E2"][:k], b["P2"][:k])
        for x in (s["a"], s["b"]):
            self.i1.add(x)
            self.i0.add(x)

    def merge(self, other):
        for a, b in ((self.i4, other.i4), (self.i1, other.i1), (self.i0, other.i0)):
            a.merge(b)

    def results(self):
        return self.i4.results() + self.i1.results()


def _two(engine, t, genome, n, rows_a, rows_b, seam):
    sa, sb = list(_slices(engine, t, genome, 0, n, rows_a)), list(_slices(engine, t, genome, n, n, rows_b))
    for i, (a, b) in enumerate(zip(sa, sb)):
        s = {"a": a, "b": b}
        if seam and i == 0:
            s["seam"] = (sa[-1], sb[0])
        yield s


@pytest.mark.parametrize("legs", ["seeds", "calls"])
def test_two_workers_and_two_calls(engine, legs):
    """I4, flat case.  seeds: keys `seed + cpu_number` of two workers at equal ordinals; calls: first_ordinal 0 and n into
    adjacent rows -- pair i of one call against pair i of the other, and the pair lags across the seam."""
    dense, genome, _ = case_model("flat")
    t, n = IS.Tables(dense), IS.N_PAIRS["flat"]
    gid = _load(engine, dense, genome)
    engine.reserve(2 * n)
    rows_a = _generate(engine, dense, gid, n, SEED, 0, 0, KERNEL["flat"])
    rows_b = _generate(engine, dense, gid, n, SEED + 1 if legs == "seeds" else SEED, 0 if legs == "seeds" else n, n, KERNEL["flat"])
    two = PS.run_stats(lambda: [_TwoSets(t, legs)], _two(engine, t, genome, n, rows_a, rows_b, legs == "calls"), THREADS)[0]
    assert not two.i0.failures(), two.i0.i0
    _verdict("flat I4 %s, 2 x %d pairs" % (legs, n), two.results())


def test_the_shipped_indel_tables(engine):
    """NovaSeq as shipped (nine insertion entries of 2e-6, the light route): I0, and I1 over the non-zero cells -- an event in any
    other cell rejects by itself."""
    dense, genome = dense_model("novaseq"), random_genome(99, GENOME)
    t, n = IS.Tables(dense), PS.N_PAIRS["novaseq"]
    gid = _load(engine, dense, genome)
    engine.reserve(n)
    rows = _generate(engine, dense, gid, n, SEED, 0, 0, KERNEL["shipped"])
    stats = PS.run_stats(lambda: [IS.I0(), IS.I1(t)], _slices(engine, t, genome, 0, n, rows, step=1 << 14), THREADS)
    assert not stats[0].failures(), stats[0].i0
    assert int((rows["type"] != 0).sum()) > 0
    print("\n[philox-indel-stats] shipped: %d indel rows, I0 %s" % (int((rows["type"] != 0).sum()), dict(stats[0].i0)))
    _verdict("shipped I1, %d pairs, %s" % (n, KERNEL["shipped"]), stats[1].results())


def test_the_reference_compatible_path(engine):
    """The device's MT path (seed_mt, generate_mt, mt_mutations) on the flat case through I0 .. I3 and S5 .. S7: it equals the
    reference byte for byte, so it anchors the replay and the expectations on the device."""
    dense, genome, mixed = case_model("flat")
    t, x, n = IS.Tables(dense), PS.Expect(dense), 1 << 17
    gid = _load(engine, dense, genome)
    engine.seed_mt(77)
    engine.reserve(n)
    engine.mt_mutations_reserve(int(n * (2 * dense.expected_mutation_rows_per_pair() + 4)))
    t0 = time.time()
    try:
        assert engine.generate_mt(gid, n) == n
        rows = engine.mt_mutations()
    finally:
        engine.mt_mutations_reserve(0)
    print("\n[philox-indel-stats] MT path: generate_mt and its rows %.2f s" % (time.time() - t0))
    stats = PS.run_stats(lambda: [s for s in all_stats(dense, t, x, mixed) if not isinstance(s, (IS.I4, IS.I5))],
                         _slices(engine, t, genome, 0, n, rows), THREADS)
    print("\n[philox-indel-stats] MT path: I0 %s, excluded steps %.4f %%" % (dict(stats[0].i0), 100 * stats[1].excluded_share()))
    assert_accepted(stats)
    _verdict("flat MT path I1-I3 S5-S7, %d pairs" % n, [r for st in stats[1:] for r in st.results()])
