"""k_main and k_main_g over the position-tile geometry.

What the two kernels execute is fixed at model upload by the position tiling: TS superitems per tile, n_tiles, ni = ceil(TS / 4)
iterations per pass, how short the last tile is; from ni follow it_bits (the iteration field of a deferred entry's tag),
sc_gpt = ceil(ni / 8) (64-byte script rows per tile and read) and the k_main_g<NI, NP> instantiation.  The shipped profiles reach
ni 1, 2, 4 and 5; helpers.TILE_GEOMETRIES reaches ni 3 (k_main_g<3, 1>), 9 to 20 (the reload of the script rows every eight
iterations, sc_gpt 2 and 3, it_bits 4 and 5), last tiles of one superitem with one position, the scripts' pitch limit and the
first pitch above it.  Everything is byte-exact against the CPU oracle: rows, coordinates, --store_mutations rows.  Every case
first asserts that the library reports the geometry of its row (ISS_DEBUG_MODEL's `[model]` line) and, after the launch, the
kernel that ran."""
import collections

import numpy as np
import pytest

from helpers import (TILE_GEOMETRIES, TILE_GEOMETRY_ENV, TILE_GROUPED, dense_model, mixed_genome, model_geometry, random_genome,
                     tag_iteration_bits, tile_geometry, tile_geometry_genome_length, tile_geometry_model)

pytestmark = pytest.mark.gpu

KEYS = ("r1_qual", "r2_qual", "r1_base", "r2_base")
MUT_FIELDS = ("pair", "mate", "type", "position", "ref", "alt", "quality")
N_SWEEP = 256 * 13 + 37  # thirteen full passes and a partial block: 5 to 14 passes of a workgroup, a partial last group
SEED = 20240
IDS = [g.id for g in TILE_GEOMETRIES]

# route -> (mixed-letter genome, indels, --store_mutations rows, geometries, the kernel that must run (None: TILE_GROUPED's))
ROUTES = {
    "plain": (False, False, False, IDS, "k_main<false, true, false>"),
    "grouped": (False, False, False, sorted(TILE_GROUPED), None),
    "mixed": (True, False, False, IDS, "k_main<false, false, false>"),
    "indel": (False, True, False, IDS, "k_main<false, true, true>"),
    "mut": (True, True, True, ["C", "F", "H"], "k_main<true, false, true>"),
    # (a record with IUPAC letters sends every read with an event to k_indel_fixup: the rows k_indel_script appends for scripted
    #  reads at sc_gpt == 2 need a plain record)
    "mut-plain": (False, True, True, ["F", "H"], "k_main<true, true, true>"),
}
SWEEP = [(route, gid) for route in ROUTES for gid in ROUTES[route][3]]


@pytest.fixture(scope="module")
def engine():
    from insilicoseq_amd.engine import ReadEngine

    eng = ReadEngine(0)
    yield eng
    eng.close()


_memo = collections.OrderedDict()


def _memoized(key, make):
    """(the cases that share a value follow each other: the few latest are kept)"""
    if key not in _memo:
        _memo[key] = make()
        while len(_memo) > 6:
            _memo.popitem(last=False)
    _memo.move_to_end(key)
    return _memo[key]


def _genome(geo, mixed):
    n = tile_geometry_genome_length(geo)
    return _memoized(("genome", geo.id, mixed), lambda: mixed_genome(900 + geo.RL, n) if mixed else random_genome(900 + geo.RL, n))


def _oracle(key, dense, genome, n_pairs, seed, first_ordinal, store_mutations=False):
    """The oracle's reads of a case, computed once (the cases of a geometry and route differ in the switches only) and never
    written to."""
    def make():
        from oracle import oracle as O

        exp = O.Oracle(dense).simulate(O.Rng().seed_philox(seed), genome, n_pairs, first_ordinal=first_ordinal, want_coords=True,
                                       store_mutations=store_mutations)
        assert exp["status"] == 0 and exp["n_done"] == n_pairs
        for k in KEYS + ("coords",):
            exp[k].setflags(write=False)
        return exp

    return _memoized(("oracle",) + key + (n_pairs, seed, first_ordinal, store_mutations), make)


def _load(engine, capfd, monkeypatch, dense, env, geo=None):
    """Upload `dense` under the switches `env` (they are read at upload) and return the geometry the library reports; with
    `geo`, that is asserted to be the row's -- a case that silently ran another geometry is a failed case."""
    for k, v in dict(TILE_GEOMETRY_ENV, **env).items():
        monkeypatch.setenv(k, v)
    for k in ("ISS_TILES", "ISS_MAIN_GROUP", "ISS_MAIN_GROUP_MIN", "ISS_LIGHT_INDELS", "ISS_MAIN_WGS", "ISS_CHUNK_PAIRS"):
        if k not in env:
            monkeypatch.delenv(k, raising=False)
    capfd.readouterr()
    engine.load_model(dense)
    got = model_geometry(capfd.readouterr().err)
    assert got.RL == dense.read_length and got.GB == 6
    if geo is not None:
        assert (got.n_tiles, got.TS, got.ni) == (geo.n_tiles, geo.TS, geo.ni), (geo.id, got)
        assert got.NB == max(sum(geo.nonempty[0]), sum(geo.nonempty[1]))
    return got


def _run(engine, genome, n_pairs, seed, first_ordinal):
    engine.clear_genomes()
    gid = engine.add_genome(genome)
    engine.stats_read()
    engine.generate(gid, n_pairs, first_ordinal=first_ordinal, seed=seed)
    engine.synchronize()
    return engine.download(0, n_pairs), engine.coords(0, n_pairs)


def _assert_rows(got, exp, what, coords=None):
    if coords is not None:
        assert np.array_equal(coords, exp["coords"]), (what, "pair coordinates differ")
    for k in KEYS:
        bad = np.argwhere(got[k] != exp[k])
        assert bad.size == 0, "%s: %s differs at (pair, pos) %s ... (%d cells)" % (what, k, bad[:5].tolist(), len(bad))


def _env(geo, route, wgs, group_min=None):
    env = {"ISS_MAIN_WGS": wgs}
    if geo.tiles:
        env["ISS_TILES"] = str(geo.tiles)
    if route == "plain":
        env["ISS_MAIN_GROUP"] = "0"
    if route == "grouped":
        env["ISS_MAIN_GROUP"] = str(TILE_GROUPED[geo.id][0])
        env["ISS_MAIN_GROUP_MIN"] = group_min
    if ROUTES[route][1]:
        env["ISS_LIGHT_INDELS"] = "0"  # never the light path: k_indel_scan, k_indel_script, k_main<.., true>
    return env


# ------------------------------------------------------------------ 1. the sweep
@pytest.mark.parametrize("wgs", ["1", "3"])
@pytest.mark.parametrize("route,gid", SWEEP, ids=["%s-%s" % c for c in SWEEP])
def test_geometry_matches_oracle(engine, route, gid, wgs, capfd, monkeypatch):
    """Every geometry on every route it can take, with one and with three workgroups (5 to 14 passes each), half of the
    geometries of a route far beyond 2^32 in the ordinals; the plain route once more with five pairs.  Grouped: closing rounds of
    any size and full ones only (ISS_MAIN_GROUP_MIN 1 / 64); F has no instantiation and keeps k_main.  Indel: reads up to
    AP_MAX_PITCH are built from their scripts by k_main<.., true>, longer ones all go to k_indel_fixup while k_main walks idle
    scripts."""
    geo = tile_geometry(gid)
    mixed, indel, mut, _, kernel = ROUTES[route]
    kernel = kernel or TILE_GROUPED[gid][1]
    dense = tile_geometry_model(geo, indel)
    genome = _genome(geo, mixed)
    first_ordinal = 2**33 + 11 if (IDS.index(gid) + list(ROUTES).index(route)) % 2 else 0
    shapes = [(gm, N_SWEEP) for gm in (("1", "64") if route == "grouped" else (None,))]
    if route == "plain" and wgs == "1":
        shapes.append((None, 5))
    if mut:
        engine.mutations_reserve(8_000_000)  # (few phreds: most bases are substituted, and a read rebuilt by the fix-up leaves stale rows)
    try:
        for group_min, n in shapes:
            what = (route, gid, "wgs " + wgs, "group_min %s" % group_min, n)
            _load(engine, capfd, monkeypatch, dense, _env(geo, route, wgs, group_min), geo)
            got, coords = _run(engine, genome, n, SEED, first_ordinal)
            assert engine.main_kernel() == kernel, what
            stats = engine.stats_read()
            with capfd.disabled():  # (pytest -s: what ran, per case)
                print("%s %s wgs %s group_min %s, %d pairs: n_tiles %d TS %d ni %d -> %s %s"
                      % (route, gid, wgs, group_min, n, geo.n_tiles, geo.TS, geo.ni, kernel, stats))
            exp = _oracle((gid, mixed, indel), dense, genome, n, SEED, first_ordinal, mut)
            _assert_rows(got, exp, what, coords)
            if route == "indel" and gid in "IJK":
                assert stats["fixup_reads"] > 0 and stats["scripted_reads"] == 0, what
            elif route in ("indel", "mut-plain"):
                assert stats["scripted_reads"] > 0, what
            if mut:
                rows, exp_rows = engine.mutations(), exp["mutations"]
                assert len(rows) == len(exp_rows) and len(exp_rows) > 0, what
                for f in MUT_FIELDS:
                    bad = np.flatnonzero(rows[f] != exp_rows[f])
                    assert bad.size == 0, (what, f, bad[:5], rows[bad[:3]], exp_rows[bad[:3]])
    finally:
        if mut:
            engine.mutations_reserve(0)


# ------------------------------------------------------------------ 2. the pass limit
# (shipped profile or geometry, ISS_MAIN_GROUP, iterations per pass, the kernel that must run)
PASS_LIMIT = [("ecoli", None, "0", 1, "k_main<false, true, false>"), ("ecoli", None, "2", 1, "k_main_g<1, 2>"),
              ("novaseq", None, "0", 5, "k_main<false, true, false>"), (None, "F", "0", 10, "k_main<false, true, false>"),
              (None, "J", "0", 17, "k_main<false, true, false>"), (None, "C", "0", 3, "k_main<false, true, false>")]


@pytest.mark.parametrize("model,gid,group,ni,kernel", PASS_LIMIT, ids=["%s-group%s" % (m or g, grp) for m, g, grp, _, _ in PASS_LIMIT])
def test_a_workgroup_makes_every_pass_the_tag_allows(engine, model, gid, group, ni, kernel, capfd, monkeypatch):
    """A deferred entry's tag holds (pass of the workgroup, iteration) in 13 bits, so generate_core cuts a call into chunks of
    max_passes * 256 * (workgroups of the tile that has the fewest) pairs, max_passes = 2^(13 - it_bits) - 1.  With one workgroup
    per tile (ISS_MAIN_WGS=1) and max_passes * 256 + 300 pairs, the workgroup makes exactly max_passes passes in the first chunk,
    then a short second chunk.  The boundary is derived from generate_core's formula: the test cannot observe the cut itself, it
    observes that nothing aliases -- an entry whose pass number wrapped is settled for a pair at the front of the launch, with
    the letters of its own pair (wrong substitutions in the first window), and its own pair stays as the hot loop left it
    (the last window).
    Oracle windows by ordinal: the first 512 pairs, the 512 in front of the boundary, the pairs behind it -- the last 300."""
    from oracle import oracle as O

    geo = tile_geometry(gid) if gid else None
    dense = tile_geometry_model(geo) if geo else dense_model(model)
    env = {"ISS_MAIN_WGS": "1", "ISS_MAIN_GROUP": group}
    if geo is not None and geo.tiles:
        env["ISS_TILES"] = str(geo.tiles)
    reported = _load(engine, capfd, monkeypatch, dense, env, geo)
    assert reported.ni == ni
    max_passes = 2 ** (13 - tag_iteration_bits(reported.ni)) - 1
    boundary = max_passes * 256
    n = boundary + 300
    genome = random_genome(431, max(8 * dense.read_length + 7, 64) + 100000)
    first_ordinal = 2**33 + 11
    engine.clear_genomes()
    g = engine.add_genome(genome)
    engine.generate(g, n, first_ordinal=first_ordinal, seed=SEED + 1)
    engine.synchronize()
    assert engine.main_kernel() == kernel
    orc = O.Oracle(dense)
    for a, m in ((0, 512), (boundary - 512, 512), (boundary, n - boundary)):
        exp = orc.simulate(O.Rng().seed_philox(SEED + 1), genome, m, first_ordinal=first_ordinal + a, want_coords=True)
        assert exp["status"] == 0 and exp["n_done"] == m
        _assert_rows(engine.download(a, m), exp, (model or gid, "pairs %d + %d of %d, boundary %d" % (a, m, n, boundary)),
                     engine.coords(a, m))


# ------------------------------------------------------------------ 3. ring pressure at the new iteration counts
@pytest.mark.parametrize("gid,route,group_min", [("A", "grouped", "1"), ("A", "grouped", "64"), ("F", "plain", None), ("F", "indel", None)])
def test_every_base_deferred(engine, gid, route, group_min, capfd, monkeypatch):
    """Every phred's substitution test fires (threshold 0: `u > 0`): every lane-item pushes 16 bases, 64 entries per wavefront
    and iteration, and an entry comes back sixteen times -- with three iterations per group (k_main_g<3, 1>: the ring fills
    inside a group), and with ten iterations per pass, where the iteration field of the tag is four bits wide."""
    geo = tile_geometry(gid)
    mixed, indel, _, _, kernel = ROUTES[route]
    dense = tile_geometry_model(geo, indel)
    dense.phred_thr[:] = 0.0
    genome = _genome(geo, mixed)
    _load(engine, capfd, monkeypatch, dense, _env(geo, route, "2", group_min), geo)
    got, coords = _run(engine, genome, 2600, SEED + 2, 5)
    assert engine.main_kernel() == (kernel or TILE_GROUPED[gid][1])
    _assert_rows(got, _oracle((gid, mixed, indel, "thr0"), dense, genome, 2600, SEED + 2, 5), (gid, route, group_min), coords)
