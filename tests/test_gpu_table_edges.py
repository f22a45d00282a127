"""Every table lookup of the device against the oracle on the edge-built tables of tests/table_edges.py.

iss_model_upload compresses the model's tables with hand-made edge rules (merged leading digits, clamps to 0xffff / 255 / 0x1fff,
closing sentinels with phred n_q, padding to s_max, guide bytes, the un-merged digits of the MT resolver).  The cases of
table_edges put thresholds on those edges, and tests/test_table_edges_host.py proves -- from a restatement of the draws, without
the library -- that the draws of each case land on them (the ledger).  Here the device runs the same calls: bases, phreds and
coordinates equal the oracle's for the whole call, on every route of the hot loop (k_main, k_main_g, two position tiles, a
batch, --store_mutations) at 6, 7 and 8 guide bits, and the kernel that ran is the one the route names.

The MT legs run the same tables through generate_mt (resolver and walker) for mt_rows' un-clamped digits and padding.  The MT
streams are not the Philox address map: the ledger does not describe their draws, and their hits on the edges are not counted.

Plus the refusal of a bin CDF that ends below 1.0 over an empty last bin at the C ABI (an upload launches nothing)."""
import numpy as np
import pytest

import table_edges as E
from helpers import TILE_GEOMETRY_ENV, model_geometry, synthetic_model

pytestmark = pytest.mark.gpu

KEYS = ("r1_qual", "r2_qual", "r1_base", "r2_base")
MUT_FIELDS = ("pair", "mate", "type", "position", "ref", "alt", "quality")
# (n_tiles, TS, ni) the upload must report: the tables of Q33 (four bin slots, rows of up to 44 entries) fit one tile with 6 and
# 7 guide bits and need two with 8; Q65 (two slots, 63 entries) likewise
GEOMETRY = {"Q33-6": (1, 5, 2), "Q33-7": (1, 5, 2), "Q33-8": (2, 4, 1), "Q33-6-mixed": (1, 5, 2), "Q65-6": (1, 9, 3),
            "Q65-7": (1, 9, 3), "Q65-8": (2, 8, 2), "Q9": (1, 2, 1), "S33": (1, 5, 2)}
GROUPED = {5: (1,), 4: (1,), 3: (1,), 2: (2, 1), 1: (2,)}  # ni -> passes per group the library holds (ISS_MAIN_G_LIST)


def _geometry(cid):
    return GEOMETRY.get(cid, (1, 5, 2))  # (I33-*, B33-*: Q33's shape with at most four slots at 6 guide bits)


def _kernel(cid, group):
    """The kernel a route must launch.  group None: as the host picks -- these tables send far more than one base in sixty out of
    the hot loop, so main_group_passes groups, with the fewest passes a group the library holds for ni."""
    ni = _geometry(cid)[2]
    if cid.endswith("mixed"):
        return "k_main<false, false, false>"
    if group == 0:
        return "k_main<false, true, false>"
    return "k_main_g<%d, %d>" % (ni, min(GROUPED[ni]) if group is None else group)


ROUTES = [(cid, g) for cid in E.PHILOX_CASES
          for g in ([None] + ([0] + [g for g in (1, 2) if g in GROUPED[_geometry(cid)[2]]] if cid[:3] in ("Q33", "Q65") and not cid.endswith("mixed") else []))]


@pytest.fixture(scope="module")
def engine():
    from insilicoseq_amd.engine import ReadEngine

    eng = ReadEngine(0)
    yield eng
    eng.close()


def _load(engine, capfd, monkeypatch, c, env, geometry=None):
    """Upload the case's model with its guide bits pinned and the switches `env` (read at upload); the geometry the library
    reports is the one expected."""
    for k, v in dict(TILE_GEOMETRY_ENV, ISS_GUIDE_BITS=str(c.guide_bits), **env).items():
        monkeypatch.setenv(k, v)
    for k in ("ISS_TILES", "ISS_MAIN_GROUP", "ISS_MAIN_GROUP_MIN", "ISS_LIGHT_INDELS", "ISS_MAIN_WGS", "ISS_CHUNK_PAIRS", "ISS_MT_PATH"):
        if k not in env:
            monkeypatch.delenv(k, raising=False)
    capfd.readouterr()
    engine.load_model(c.dense)
    got = model_geometry(capfd.readouterr().err)
    assert (got.RL, got.GB) == (c.RL, c.guide_bits)
    assert (got.n_tiles, got.TS, got.ni) == (geometry or _geometry(c.id)), (c.id, got)
    return got


def _assert_rows(got, exp, what, coords=None):
    if coords is not None:
        assert np.array_equal(coords, exp["coords"]), (what, "pair coordinates differ")
    for k in KEYS:
        bad = np.argwhere(got[k] != exp[k])
        assert bad.size == 0, "%s: %s differs at (pair, pos) %s ... (%d cells)" % (what, k, bad[:5].tolist(), len(bad))


def _generate(engine, c):
    engine.clear_genomes()
    gid = engine.add_genome(c.genome)
    engine.generate(gid, c.pairs, first_ordinal=E.FIRST_ORDINAL, seed=E.SEED)
    engine.synchronize()
    return engine.download(0, c.pairs), engine.coords(0, c.pairs)


# ------------------------------------------------------------------ the Philox legs
@pytest.mark.parametrize("cid,group", ROUTES, ids=["%s-%s" % (c, "host" if g is None else "group%d" % g) for c, g in ROUTES])
def test_case_matches_the_oracle(engine, cid, group, capfd, monkeypatch):
    """One model, one record, one call: the whole call equals the oracle's, and the kernel that ran is the route's."""
    c = E.case(cid)
    _load(engine, capfd, monkeypatch, c, {} if group is None else {"ISS_MAIN_GROUP": str(group)})
    got, coords = _generate(engine, c)
    assert engine.main_kernel() == _kernel(cid, group), (cid, group)
    _assert_rows(got, E.oracle_rows(cid), (cid, group), coords)


def test_q33_on_two_position_tiles(engine, capfd, monkeypatch):
    """Q33 cut into two position tiles (ISS_TILES=2: four superitems, then one with one valid position) with groups of two
    passes: k_main_g<1, 2>, geometry E of helpers.TILE_GEOMETRIES."""
    c = E.case("Q33-6")
    _load(engine, capfd, monkeypatch, c, {"ISS_TILES": "2", "ISS_MAIN_GROUP": "2"}, geometry=(2, 4, 1))
    got, coords = _generate(engine, c)
    assert engine.main_kernel() == "k_main_g<1, 2>"
    _assert_rows(got, E.oracle_rows("Q33-6"), "Q33-6 on two tiles", coords)


def test_q33_as_a_batch_of_three_copies(engine, capfd, monkeypatch):
    """generate_batch over three copies of Q33's record, the seams (pairs 5003 and 5014) inside a wavefront's 16 pairs: the
    ordinals run on over the work list and the copies hold the same letters, so the rows are those of the single call."""
    c = E.case("Q33-6")
    _load(engine, capfd, monkeypatch, c, {})
    counts = [5003, 11, c.pairs - 5014]
    engine.clear_genomes()
    gids = [engine.add_genome(c.genome) for _ in counts]
    engine.generate_batch(gids, counts, first_ordinal=E.FIRST_ORDINAL, seed=E.SEED, out_first_pair=0)
    engine.synchronize()
    assert engine.main_kernel() == _kernel("Q33-6", None)
    _assert_rows(engine.download(0, c.pairs), E.oracle_rows("Q33-6"), "Q33-6 as a batch", engine.coords(0, c.pairs))


def test_q33_store_mutations_rows(engine, capfd, monkeypatch):
    """--store_mutations on Q33: every row of the call, field by field (the phred of a substitution is the table lookup's)."""
    c = E.case("Q33-6")
    exp = E.oracle_rows("Q33-6", store_mutations=True)
    engine.mutations_reserve(8_000_000)
    try:
        _load(engine, capfd, monkeypatch, c, {})
        got, coords = _generate(engine, c)
        assert engine.main_kernel() == "k_main<true, true, false>"
        _assert_rows(got, exp, "Q33-6 with mutation rows", coords)
        rows, exp_rows = engine.mutations(), exp["mutations"]
        assert len(rows) == len(exp_rows) and len(exp_rows) > 100_000
        for f in MUT_FIELDS:
            bad = np.flatnonzero(rows[f] != exp_rows[f])
            assert bad.size == 0, (f, bad[:5], rows[bad[:3]], exp_rows[bad[:3]])
    finally:
        engine.mutations_reserve(0)


# ------------------------------------------------------------------ the MT legs
MT_CASES = ["Q33-6", "S33"] + ["I33-%d" % k for k in range(4)] + ["B33-%d" % k for k in range(4)]
MT_PAIRS, MT_SEED = 1 << 13, 4321


@pytest.mark.parametrize("cid", MT_CASES)
def test_mt_case_matches_the_oracle(engine, cid, capfd, monkeypatch):
    """The case's tables through generate_mt against the oracle's MT sample, on a record with an N every thousand letters: the
    resolver (mt_rows: un-merged, un-clamped-but-for-2^53 digits, 0xffff padding) hands the pairs that touch one to the walker.
    Both must have run -- but for insert-size tables of more than 4096 entries, which are the walker's alone.  (What these draws
    hit is not counted: the ledger describes the Philox draws.)"""
    from oracle import oracle as O

    c = E.case(cid)
    genome = E.sprinkled_genome(c.RL)
    exp = O.Oracle(c.dense).simulate(O.Rng().seed_mt(MT_SEED), genome, MT_PAIRS)
    assert exp["status"] == 0 and exp["n_done"] == MT_PAIRS
    _load(engine, capfd, monkeypatch, c, {})
    engine.clear_genomes()
    gid = engine.add_genome(genome)
    engine.seed_mt(MT_SEED)
    r0, w0 = engine.mt_path_counts()
    assert engine.generate_mt(gid, MT_PAIRS) == MT_PAIRS
    resolved, walked = (a - b for a, b in zip(engine.mt_path_counts(), (r0, w0)))
    _assert_rows(engine.download(0, MT_PAIRS), exp, cid + " (MT)")
    assert resolved + walked == MT_PAIRS
    if c.dense.n_isize > 4096:
        assert walked == MT_PAIRS
    else:
        assert resolved > MT_PAIRS // 2 and walked >= E.FLOOR, (resolved, walked)


# ------------------------------------------------------------------ the refusal
def test_upload_refuses_a_short_bin_cdf_over_an_empty_last_bin():
    """bin_cdf = [0.5, 0.9, 0.9, 0.9] over histograms in bins 0 and 1 only: a tenth of the draws would be clamped to bin 3, which
    has none.  The tables go to iss_model_upload as they are (load_model does not validate); the error comes back as a code and a
    message, nothing is launched, and the context takes a valid model afterwards.  No read is generated with such a model."""
    from insilicoseq_amd import _native
    from insilicoseq_amd.engine import ReadEngine

    d = synthetic_model(20, 5, 7, seed=1, nonempty=((1, 1, 0, 0), (1, 1, 1, 1)))
    good_cdf = d.bin_cdf.copy()
    with ReadEngine(0) as eng:
        for o in range(2):
            d.bin_cdf[:] = good_cdf
            d.bin_nonempty[:] = ((1, 1, 0, 0), (1, 1, 1, 1)) if o == 0 else ((1, 1, 1, 1), (1, 1, 0, 0))
            d.bin_cdf[o] = [0.5, 0.9, 0.9, 0.9]
            d.bin_cdf[1 - o] = [0.25, 0.5, 0.75, 1.0]
            with pytest.raises(_native.EngineError, match="last bin has no histograms") as e:
                eng.load_model(d)
            assert e.value.code == _native.E_INVALID
        d.bin_cdf[1] = [0.5, 1.0, 1.0, 1.0]  # a full CDF over an empty last bin is a valid model
        eng.load_model(d)
        d.bin_nonempty[1] = (1, 1, 0, 1)
        d.bin_cdf[1] = [0.5, 0.9, 0.9, 0.9]  # ... and so is a short one over a last bin with histograms (the clamp proper)
        eng.load_model(d)
