"""The Philox path's joint distribution on the device, held to the model (tests/philox_stats.py; DESIGN section 4, "What holds
the map to the model").  The parity tests compare the device with an oracle that restates the same address map; these compare
what the device generates with the model's own distribution: every (mate, position) marginal, every pair of positions of a pair
of reads, the full joint tables of the map's structurally distinct pairs, pair lags, two worker seeds, two calls whose ordinals
touch, the error test given the phred and its independence of every quality draw, the choice of the alternative, the
coordinates -- at the sizes at which tests/test_philox_stats_host.py shows every planted defect rejected.  The device's
reference-compatible (MT) path, which equals the reference byte for byte, goes through the same statistics.

Samples are downloaded in slices and accumulated; every case asserts the kernel that made it.  All hypotheses of a test function
share philox_stats.ALPHA (Bonferroni); seeds are fixed."""
import os

import pytest

import philox_stats as PS
from helpers import dense_model, mixed_genome, random_genome

pytestmark = pytest.mark.gpu

GENOME = 400_000
SEED = 2024
# case -> (model, mixed genome, the kernel that must have run)
CASES = {"novaseq": ("novaseq", False, "k_main<false, true, false>"), "hiseq": ("hiseq", False, "k_main_g<2, 2>"),
         "miseq": ("miseq", False, "k_main_g<2, 1>"), "nextseq": ("nextseq", False, "k_main_g<4, 1>"),
         "miseq-mixed": ("miseq", True, "k_main<false, false, false>")}
_GENOMES = {}
THREADS = max(1, min(16, os.cpu_count() or 1))  # host threads over the slices of a sample


@pytest.fixture(scope="module")
def engine():
    from insilicoseq_amd.engine import ReadEngine

    eng = ReadEngine(0)
    yield eng
    eng.close()


@pytest.fixture(autouse=True)
def _host_picks_the_kernel(monkeypatch):
    for k in ("ISS_MAIN_GROUP", "ISS_MAIN_GROUP_MIN", "ISS_MAIN_WGS", "ISS_TILES", "ISS_CHUNK_PAIRS", "ISS_LIGHT_INDELS"):
        monkeypatch.delenv(k, raising=False)


def _genome(mixed):
    if mixed not in _GENOMES:
        _GENOMES[mixed] = mixed_genome(98, GENOME) if mixed else random_genome(99, GENOME)
    return _GENOMES[mixed]


def _slice_pairs(RL):
    """Pairs of a download: the largest power of two with at most 2^21 cells -- some 70 MB of work arrays a slice, THREADS
    slices alive at once."""
    return 1 << (((1 << 21) // (2 * RL)).bit_length() - 1)


def _generate(engine, dense, genome, calls, kernel, gc_bias=False):
    """calls: (n, seed, first_ordinal, first row) each; the rows stay on the device."""
    engine.load_model(dense)
    engine.clear_genomes()
    gid = engine.add_genome(genome)
    engine.reserve(max(row + n for n, _, _, row in calls))  # (a reservation that grows drops the rows it held)
    for n, seed, first_ordinal, row in calls:
        engine.generate(gid, n, first_ordinal=first_ordinal, seed=seed, gc_bias=gc_bias, out_first_pair=row)
        engine.synchronize()
        if kernel is None:
            assert engine.main_kernel().startswith("k_main")
        else:
            assert engine.main_kernel() == kernel


def _slices(engine, dense, genome, first, n, step=None, rows_only=False):
    RL = dense.read_length
    step = step or _slice_pairs(RL)
    for a in range(first, first + n, step):
        m = min(step, first + n - a)
        rows = engine.download(a, m)
        if rows_only:
            yield {"Q": PS.stack_mates(rows["r1_qual"], rows["r2_qual"])}
        else:
            yield PS.slice_of(rows, engine.coords(a, m), genome, RL)


def _verdict(what, results):
    ok, text = PS.accept(results)
    print("\n[philox-stats] %s: %s" % (what, text))
    assert ok, text


def _case(case, indel=None):
    model, mixed, kernel = CASES[case]
    return model, dense_model(model, indel), _genome(mixed), mixed, kernel


@pytest.mark.parametrize("case", list(CASES))
def test_marginals_and_every_pair_of_positions(engine, case):
    """S1, S2, S3: the phred PMF of every (mate, position), the score covariance of every pair of columns against the bin
    mixture's, the full joint tables of the structural pairs."""
    model, dense, genome, _, kernel = _case(case)
    n = PS.N_PAIRS[model]
    _generate(engine, dense, genome, [(n, SEED, 0, 0)], kernel)
    x = PS.Expect(dense)
    pairs = PS.structural_pairs(model, dense.read_length)
    _verdict("%s S1-S3, %d pairs, %s" % (case, n, kernel),
             PS.run(lambda: [PS.S1(dense, None, x), PS.S2(dense, None, x), PS.S3(dense, pairs, None, x)],
                    _slices(engine, dense, genome, 0, n, rows_only=True), THREADS))


@pytest.mark.parametrize("case", list(CASES))
def test_neighbouring_pairs_draw_independently(engine, case):
    """S4: the cross matrix of the scores of pair i and pair i + k, k = 1, 63, 64, 256 -- every entry 0."""
    model, dense, genome, _, kernel = _case(case)
    n = PS.N_PAIRS[model]
    _generate(engine, dense, genome, [(n, SEED, 0, 0)], kernel)
    x = PS.Expect(dense)
    _verdict("%s S4 lags, %d pairs, %s" % (case, n, kernel),
             PS.run(lambda: [PS.S4(dense, None, x)], _slices(engine, dense, genome, 0, n, rows_only=True), THREADS))


@pytest.mark.parametrize("case", list(CASES))
def test_error_test_and_alternative(engine, case):
    """S5, S6, S7 on the model without indels: errors given the phred, the residuals err - pe[q] against every quality score
    (their own position's first of all), double errors of every pair of columns, the alternatives against subst_cdf.  On the
    mixed genome only upper-case A, C, G, T templates count, and an ambiguous letter never changes."""
    model, dense, genome, mixed, kernel = _case(case, indel=(0.0, 0.0))
    n = PS.N_PAIRS[model]
    _generate(engine, dense, genome, [(n, SEED, 0, 0)], kernel)
    x = PS.Expect(dense)
    _verdict("%s S5-S7, %d pairs, %s" % (case, n, kernel),
             PS.run(lambda: [PS.S5(dense, None, x, letters_only=mixed), PS.S6(dense, None, x, letters_only=mixed), PS.S7(dense, None, x)],
                    _slices(engine, dense, genome, 0, n), THREADS))


@pytest.mark.parametrize("case", list(CASES))
def test_coordinates(engine, case):
    """S8: insert sizes, forward starts, the two against each other, forward starts of neighbouring pairs."""
    model, dense, genome, _, kernel = _case(case)
    n = PS.N_PAIRS[model]
    _generate(engine, dense, genome, [(n, SEED, 0, 0)], kernel)
    st = PS.S8(dense, GENOME)
    for a in range(0, n, PS.SLICE):
        st.add({"coords": engine.coords(a, min(PS.SLICE, n - a))})
    _verdict("%s S8, %d pairs, %s" % (case, n, kernel), st.results())


def test_custom_fragment_length(engine):
    """S8 with set_fragment(450, 30): the insert size is int(normal(450, 30)) - 2 RL, truncated toward zero."""
    model, dense, genome, _, _ = _case("novaseq")
    n = PS.N_PAIRS[model]
    engine.load_model(dense)
    engine.clear_genomes()
    gid = engine.add_genome(genome)
    engine.set_fragment(450, 30)
    try:
        engine.generate(gid, n, first_ordinal=0, seed=SEED)
        engine.synchronize()
        assert engine.main_kernel() == "k_main<false, false, false>"
        st = PS.S8(dense, GENOME, fragment=(450.0, 30.0))
        for a in range(0, n, PS.SLICE):
            st.add({"coords": engine.coords(a, min(PS.SLICE, n - a))})
    finally:
        engine.set_fragment(None, None)
    _verdict("novaseq fragment 450/30 S8, %d pairs, k_main<false, false, false>" % n, st.results())


def test_gc_bias_fills_the_attempt_field(engine):
    """S1, S2, S4 with gc_bias: rejected candidates redraw at the same ordinal with the next `attempt` of the counter; the phreds
    do not depend on the letters, so the accepted pairs keep the model's phred distribution."""
    model, dense, genome, _, _ = _case("hiseq")
    n = PS.N_PAIRS[model]
    _generate(engine, dense, genome, [(n, SEED, 0, 0)], None, gc_bias=True)
    kernel = engine.main_kernel()
    x = PS.Expect(dense)
    _verdict("hiseq gc_bias S1 S2 S4, %d pairs, %s" % (n, kernel),
             PS.run(lambda: [PS.S1(dense, None, x), PS.S2(dense, None, x), PS.S4(dense, None, x)],
                    _slices(engine, dense, genome, 0, n, rows_only=True), THREADS))


class _TwoSets(object):
    """S4 between two sets of rows, slice by slice, with S1 over both (rows that are not what they should be -- stale, empty --
    would pass a test of independence)."""

    def __init__(self, dense, x, key):
        self.key, self.s4, self.s1 = key, PS.S4(dense, None, x), PS.S1(dense, None, x)

    def add(self, s):
        self.s4.add_cross(self.key, s["a"], s["b"])
        self.s1.add(s["a"])
        self.s1.add(s["b"])

    def merge(self, other):
        self.s4.merge(other.s4)
        self.s1.merge(other.s1)

    def results(self):
        return self.s4.results() + self.s1.results()


def _two(engine, dense, genome, n):
    for sa, sb in zip(_slices(engine, dense, genome, 0, n, rows_only=True), _slices(engine, dense, genome, n, n, rows_only=True)):
        yield {"a": sa, "b": sb}


@pytest.mark.parametrize("case", ["novaseq", "hiseq"])
def test_two_workers_draw_independently(engine, case):
    """S4, seed leg: keys `seed + cpu_number` of two workers, equal ordinals."""
    model, dense, genome, _, kernel = _case(case)
    n = PS.N_PAIRS[model]
    _generate(engine, dense, genome, [(n, SEED, 0, 0), (n, SEED + 1, 0, n)], kernel)
    x = PS.Expect(dense)
    _verdict("%s S4 seeds, 2 x %d pairs, %s" % (case, n, kernel),
             PS.run(lambda: [_TwoSets(dense, x, "seeds %d, %d" % (SEED, SEED + 1))], _two(engine, dense, genome, n), THREADS))


@pytest.mark.parametrize("case", ["novaseq", "hiseq"])
def test_two_calls_whose_ordinals_touch(engine, case):
    """S4, call leg: first_ordinal 0 and n into adjacent rows.  Pair i of one call against pair i of the other, and the pair lags
    over the n / 2 rows around the seam, in slices that straddle it."""
    model, dense, genome, _, kernel = _case(case)
    n = PS.N_PAIRS[model]
    _generate(engine, dense, genome, [(n, SEED, 0, 0), (n, SEED, n, n)], kernel)
    x = PS.Expect(dense)
    step = _slice_pairs(dense.read_length)
    results = PS.run(lambda: [_TwoSets(dense, x, "calls at 0, n")], _two(engine, dense, genome, n), THREADS)
    results += PS.run(lambda: [PS.S4(dense, None, x)], _slices(engine, dense, genome, n - n // 4 + step // 2, n // 2, rows_only=True), THREADS)
    _verdict("%s S4 calls, 2 x %d pairs, %s" % (case, n, kernel), results)


@pytest.mark.parametrize("model", ["hiseq", "miseq"])
def test_the_reference_compatible_path(engine, model):
    """The device's MT path (seed_mt, generate_mt) through S1, S2, S5, S7: it equals the reference byte for byte, so it anchors
    the expectations themselves on the device."""
    dense, genome = dense_model(model, indel=(0.0, 0.0)), _genome(False)
    n = 1 << 17
    engine.load_model(dense)
    engine.clear_genomes()
    gid = engine.add_genome(genome)
    engine.seed_mt(77)
    engine.reserve(n)
    assert engine.generate_mt(gid, n) == n
    x = PS.Expect(dense)
    _verdict("%s MT path S1 S2 S5 S7, %d pairs" % (model, n),
             PS.run(lambda: [PS.S1(dense, None, x), PS.S2(dense, None, x), PS.S5(dense, None, x), PS.S7(dense, None, x)],
                    _slices(engine, dense, genome, 0, n), THREADS))
