"""The Philox path's pair setup on the device, held to the model on short records (tests/philox_setup_stats.py; DESIGN section 4,
"What holds the pair setup to the model").  tests/test_gpu_philox_stats.py sees the coordinates of long records only; here the
records are a few bases longer than a read, about as long as a fragment, or cut by a custom fragment length, so that every
branch of simulate_read is taken: the fallback start, the reverse-end fallback (`K_RS`), randbelow's rejection loop where it
rejects half of all candidates, negative inserts and irregular pairs, gc_bias with its `attempt` field, a batch call over short
records, two seeds, two calls, amplicons -- and the setup draws against the per-base draws.  Every pair of every case goes
through the exact rule C0; the sizes are those at which tests/test_philox_setup_stats_host.py shows every planted defect
rejected.

Before its statistics every case holds `engine.coords` of its first 2 000 pairs to the oracle's, so that the statistics read the
convention the parity tests read.  All hypotheses of a test function share philox_stats.ALPHA (Bonferroni); seeds are fixed."""
import os
import time

import numpy as np
import pytest

import philox_setup_stats as SS
import philox_stats as PS
from helpers import random_genome

pytestmark = pytest.mark.gpu

SEED = 2024
PARITY_PAIRS = 2000
KERNEL = {"fallback-pow2": "k_main<false, true, false>", "fallback-3q": "k_main<false, true, false>", "mixed-hiseq": "k_main_g<2, 2>",
          "mixed-miseq": "k_main<false, false, false>", "fragment-overlap": "k_main<false, false, false>",
          "fragment-cut": "k_main<false, false, false>", "long": "k_main<false, true, false>", "gc": "k_main_g<2, 2>", "gc-fallback": "k_main_g<2, 2>"}
THREADS = max(1, min(16, os.cpu_count() or 1))  # host threads over the slices of a sample


@pytest.fixture(scope="module")
def engine():
    from insilicoseq_amd.engine import ReadEngine

    eng = ReadEngine(0)
    yield eng
    eng.set_fragment(None, None)
    eng.close()


@pytest.fixture(autouse=True)
def _host_picks_the_kernel(monkeypatch):
    for k in ("ISS_MAIN_GROUP", "ISS_MAIN_GROUP_MIN", "ISS_MAIN_WGS", "ISS_TILES", "ISS_CHUNK_PAIRS", "ISS_LIGHT_INDELS"):
        monkeypatch.delenv(k, raising=False)


def _slice_pairs(RL):
    """Pairs of a download of rows: the largest power of two with at most 2^21 cells."""
    return 1 << (((1 << 21) // (2 * RL)).bit_length() - 1)


def _load(engine, dense, genomes):
    engine.load_model(dense)
    engine.clear_genomes()
    return [engine.add_genome(g) for g in genomes]


def _generate(engine, gid, n, kernel, seed=SEED, first_ordinal=0, row=0, **kw):
    engine.generate(gid, n, first_ordinal=first_ordinal, seed=seed, out_first_pair=row, **kw)
    engine.synchronize()
    assert engine.main_kernel() == kernel, engine.main_kernel()


def _coords_are_the_oracles(engine, dense, genome, row, n, first_ordinal=0, seed=SEED, **kw):
    """The first pairs of a call against the oracle's Philox provider, irregular pairs included."""
    from oracle import oracle as O

    n = min(n, PARITY_PAIRS)
    exp = O.Oracle(dense).simulate(O.Rng().seed_philox(seed), genome, n, first_ordinal=first_ordinal, want_coords=True, **kw)
    assert exp["status"] == 0 and exp["n_done"] == n
    got = engine.coords(row, n)
    assert np.array_equal(got, exp["coords"]), np.flatnonzero((got != exp["coords"]).any(axis=1))[:5]


def _slices(engine, dense, genome, first, n, rows):
    """Coordinates alone in slices of philox_stats.SLICE, or rows with them in slices of 2^21 cells."""
    step = _slice_pairs(dense.read_length) if rows else PS.SLICE
    for a in range(first, first + n, step):
        m = min(step, first + n - a)
        coords = engine.coords(a, m)
        yield PS.slice_of(engine.download(a, m), coords, genome, dense.read_length) if rows else {"coords": coords}


def _verdict(what, results):
    ok, text = PS.accept(results)
    print("\n[philox-setup-stats] %s: %s" % (what, text))
    assert ok, text


def _shares(geo, coords):
    return "regular %.4f, fell back %.4f, irregular %.4f" % SS.shares(geo, coords)


@pytest.mark.parametrize("case", ["fallback-pow2", "fallback-3q", "mixed-hiseq", "mixed-miseq", "fragment-overlap", "fragment-cut", "long"])
def test_the_setup_on_a_record(engine, case):
    """C0 on every pair, and the statistics of the case (philox_setup_stats.CASES): C1 .. C5 from coordinates alone; C6, where
    the case has it, from rows as well.  With a fragment length that cuts templates at the record's ends the fix-up builds the
    irregular pairs, both reads of each and nothing else (the model has no indels)."""
    t0 = time.time()
    c = SS.CASES[case]
    dense, genome, geo = SS.case_setup(case)
    n, rows = SS.N_PAIRS[case], "C6" in c.stats
    gid, = _load(engine, dense, [genome])
    kw = dict(fragment_length=c.fragment[0], fragment_sd=c.fragment[1]) if c.fragment else {}
    if c.fragment:
        engine.set_fragment(*c.fragment)
    try:
        engine.reserve(n)
        engine.stats_read()  # (the counters run on until they are read)
        _generate(engine, gid, n, KERNEL[case])
        fixup = engine.stats_read()["fixup_reads"]
        _coords_are_the_oracles(engine, dense, genome, 0, n, **kw)
        stats = PS.run_stats(lambda: SS.case_stats(case, dense, geo, None, c.mixed), _slices(engine, dense, genome, 0, n, rows), THREADS)
        coords = np.concatenate([engine.coords(a, min(PS.SLICE, n - a)) for a in range(0, n, PS.SLICE)])
    finally:
        if c.fragment:
            engine.set_fragment(None, None)
    irregular = int(SS.pair_rule(coords, geo.L, geo.RL).irregular.sum())
    assert fixup == 2 * irregular, (fixup, irregular)
    if case == "fragment-cut":
        assert 0.25 * n < irregular < 0.45 * n
    print("\n[philox-setup-stats] %s: L %d, %s, negative inserts %.4f, fix-up reads %d" % (case, geo.L, _shares(geo, coords), float((coords[:, 3] < 0).mean()), fixup))
    _verdict("%s %s, %d pairs, %s, %.2f s" % (case, c.stats, n, KERNEL[case], time.time() - t0), [r for st in stats for r in st.results()])


@pytest.mark.parametrize("case", ["gc", "gc-fallback"])
def test_gc_bias_against_the_plain_run(engine, case):
    """G1: the plain run and the gc_bias run of one seed, ordinals and record, side by side in the rows."""
    t0 = time.time()
    dense, genome, geo = SS.case_setup(case)
    n = SS.N_PAIRS[case]
    gid, = _load(engine, dense, [genome])
    engine.reserve(2 * n)
    _generate(engine, gid, n, KERNEL[case])
    _generate(engine, gid, n, KERNEL[case], row=n, gc_bias=True)
    _coords_are_the_oracles(engine, dense, genome, n, n, gc_bias=True)

    def both():
        for a, b in zip(_slices(engine, dense, genome, 0, n, True), _slices(engine, dense, genome, n, n, True)):
            yield {"a": a, "b": b}

    g1, = PS.run_stats(lambda: [SS.G1(dense, geo)], both(), THREADS)
    print("\n[philox-setup-stats] %s: L %d, %s, redrawn by gc_bias %.4f" % (case, geo.L, _shares(geo, engine.coords(n, n)), 1.0 - g1.k / float(g1.n)))
    assert g1.n == n
    _verdict("%s G1, 2 x %d pairs, %s, %.2f s" % (case, n, KERNEL[case], time.time() - t0), g1.results())


BATCH_COUNTS = (12345, 23457, 34567, 12347)  # no multiples of 64
SEAM = 4096  # rows on either side of a seam


def test_a_batch_call_over_short_records(engine):
    """One generate_batch over [a record of RL + 64 bases, one of 768, one of 400 kb, the first again] under NovaSeq: ordinals
    run on across the items and coordinates are arena coordinates underneath.  C0 per item with its own length, C1 .. C3 per
    item, C5 over the rows around each seam."""
    t0 = time.time()
    dense, first, _ = SS.case_setup("fallback-pow2")
    genomes = [first, random_genome(99, 2 * 126 + 516), random_genome(99, 400_000)]
    gids = _load(engine, dense, genomes)
    items = [0, 1, 2, 0]
    engine.reserve(sum(BATCH_COUNTS))
    engine.generate_batch([gids[k] for k in items], list(BATCH_COUNTS), first_ordinal=0, seed=SEED)
    engine.synchronize()
    assert engine.main_kernel() == "k_main<false, true, false>", engine.main_kernel()
    results, row, pits, said = [], 0, [], []
    for k, cnt in zip(items, BATCH_COUNTS):
        geo = SS.Geo(dense, len(genomes[k]))
        _coords_are_the_oracles(engine, dense, genomes[k], row, cnt, first_ordinal=row)
        s = {"coords": engine.coords(row, cnt)}
        stats = [SS.C1(geo), SS.C2(geo), SS.C3(geo)]
        for st in stats:
            st.add(s)
        results += [r._replace(stat="item %d %s" % (len(pits), r.stat)) for st in stats for r in st.results()]
        pits.append(geo.of(s)["P"])
        said.append("item %d L %d %s" % (len(pits) - 1, geo.L, _shares(geo, s["coords"])))
        row += cnt
    c5 = SS.C5(None)
    for k in range(len(pits) - 1):
        c5.add_rows(np.concatenate([pits[k][-SEAM:], pits[k + 1][:SEAM]]), "seam %d " % k)
    print("\n[philox-setup-stats] batch: %s" % "; ".join(said))
    _verdict("batch C0-C3 per item, C5 across the seams, %d pairs, %.2f s" % (row, time.time() - t0), results + c5.results())


@pytest.mark.parametrize("legs", ["seeds", "calls"])
def test_two_workers_and_two_calls(engine, legs):
    """C5's cross legs on the mixed HiSeq record.  seeds: keys `seed + cpu_number` of two workers at equal ordinals; calls:
    first_ordinal 0 and n into adjacent rows -- pair i of one call against pair i of the other, and the pair lags over the rows
    around the seam.  C0 and C1 run over both sets: stale or empty rows must not pass for independent ones."""
    t0 = time.time()
    case = "mixed-hiseq"
    dense, genome, geo = SS.case_setup(case)
    n = SS.N_PAIRS[case]
    gid, = _load(engine, dense, [genome])
    engine.reserve(2 * n)
    _generate(engine, gid, n, KERNEL[case])
    second = dict(seed=SEED + 1, first_ordinal=0) if legs == "seeds" else dict(seed=SEED, first_ordinal=n)
    _generate(engine, gid, n, KERNEL[case], row=n, **second)
    _coords_are_the_oracles(engine, dense, genome, n, n, **second)
    a, b = {"coords": engine.coords(0, n)}, {"coords": engine.coords(n, n)}
    assert not np.array_equal(a["coords"], b["coords"])
    c1, c5 = SS.C1(geo), SS.C5(geo)
    c1.add(a)
    c1.add(b)
    c5.add_cross(legs, a, b)
    if legs == "calls":
        c5.add_rows(geo.of({"coords": engine.coords(n - n // 4, n // 2)})["P"], "seam ")
    _verdict("%s C0 C1 C5 %s, 2 x %d pairs, %s, %.2f s" % (case, legs, n, KERNEL[case], time.time() - t0), c1.results() + c5.results())


def test_amplicons(engine):
    """sequence_type "amplicon" on the mixed HiSeq record: fs = 0 and re = L in every pair (C0), the phreds through S1."""
    t0 = time.time()
    case = "mixed-hiseq"
    dense, genome, geo = SS.case_setup(case, "amplicon")
    n = SS.N_PAIRS[case]
    gid, = _load(engine, dense, [genome])
    engine.reserve(n)
    _generate(engine, gid, n, KERNEL[case], sequence_type="amplicon")
    _coords_are_the_oracles(engine, dense, genome, 0, n, sequence_type="amplicon")
    coords = engine.coords(0, n)
    rule = SS.pair_rule(coords, geo.L, geo.RL, "amplicon")
    assert not rule.fell.any() and (coords[:, 0] == 0).all() and (coords[:, 2] == geo.L).all()
    s1 = PS.S1(dense)
    rows = engine.download(0, n)
    s1.add({"Q": PS.stack_mates(rows["r1_qual"], rows["r2_qual"])})
    _verdict("amplicon C0 S1, %d pairs, %s, %.2f s" % (n, KERNEL[case], time.time() - t0), s1.results())
