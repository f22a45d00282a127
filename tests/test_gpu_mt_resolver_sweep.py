"""rng="mt" through the resolver and the emitter over the read lengths of tests/mt_resolver_cases.py, against the oracle.

k_mt_resolve / k_mt_resolve_w find every pair's stream offsets from two-half rings refilled one half ahead, the two mates side by
side and the second again when the first had a substitution; k_mt_emit / k_mt_emit_w build the reads from the offsets.  Which
of the five instantiations runs, how much slack the rings have, where the spare wavefront and the second trip of the position
loop come in all follow from the read length and the bin layout.  tests/test_mt_resolver_sweep_host.py proves from the oracle
alone that the cases are what they say (noisy: every pair re-runs its second mate; clean: most do not; worst: a pair takes the
most numpy words a pair can) and derives the pick each case carries.

Here, per case on one engine: a call of 2048 pairs and a second work item of 300 on the same streams.  Bases, phreds and
coordinates of all of them equal the oracle's MT sample byte for byte, the --store_mutations rows field by field where they are
on, both streams stand where the oracle's stand, the library reports the instantiation the case names, and the path counts show
that the resolver did the work: every pair that touches an N was walked, and -- without gc_bias, from mt_chain_generate: the
resolver stops at such a pair, the walker takes exactly that one -- no other was (the two cases with indel rates: every read with
an indel was walked as well).  Everything is exact.

Tried once against scratch builds with one planted defect each: `8 RL + 72` for mt_res_need_np turns the four RL 247 cases red
(the pick's literal); `onp1 = onp1_guess + nev0` every case but the walker-only one.  Two defects change nothing the reads could
show, and no case here or elsewhere turns red on them: `spare_wave = RL <= 193` makes a group's fourth wavefront check the indel
draws and take position 192 as well (the same result), and without the python ring's mirror store only the indel-candidate words
(limits of zero in these models) and the low 26 bits of one error-test numerator per wrap are read from stale LDS."""
import numpy as np
import pytest

import mt_resolver_cases as M
from helpers import model_geometry

pytestmark = pytest.mark.gpu

KEYS = ("r1_qual", "r2_qual", "r1_base", "r2_base")
MUT_FIELDS = ("pair", "mate", "type", "position", "ref", "alt", "quality")


@pytest.fixture(scope="module")
def engine():
    from insilicoseq_amd.engine import ReadEngine

    eng = ReadEngine(0)
    yield eng
    eng.close()


def _res53(words):
    w = words.astype(np.uint64)
    return ((w[0::2] >> np.uint64(5)) * np.uint64(67108864) + (w[1::2] >> np.uint64(6))).astype(np.float64) / 9007199254740992.0


def _load(engine, c, capfd, monkeypatch):
    """Upload the case's model with none of the MT switches set; the bin slots and the resolver the library reports are the case's."""
    for k in ("ISS_MT_PATH", "ISS_MT_GUARD", "ISS_MT_SET_TURN", "ISS_MT_SET_BUF_TURNS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ISS_DEBUG_MODEL", "1")
    capfd.readouterr()
    engine.load_model(M.model(c))
    geo = model_geometry(capfd.readouterr().err)
    assert (geo.RL, geo.NB) == (c.RL, c.NB), geo
    assert engine.mt_resolver() == c.pick, c.id
    engine.clear_genomes()
    return engine.add_genome(M.genome(c.RL))


def _assert_rows(got, exp, lo, hi, what, coords=None):
    if coords is not None:
        assert np.array_equal(coords, exp["coords"][lo:hi]), (what, "pair coordinates differ")
    for k in KEYS:
        bad = np.argwhere(got[k] != exp[k][lo:hi])
        assert bad.size == 0, "%s: %s differs at (pair, pos) %s ... (%d cells)" % (what, k, bad[:5].tolist(), len(bad))


def _assert_mutations(got, exp, what):
    assert len(got) == len(exp) and len(exp) > 0, (what, len(got), len(exp))
    for f in MUT_FIELDS:
        bad = np.flatnonzero(got[f] != exp[f])
        assert bad.size == 0, (what, f, bad[:5], got[bad[:3]], exp[bad[:3]])


@pytest.mark.parametrize("cid", [c.id for c in M.CASES])
def test_case_matches_the_oracle(engine, cid, capfd, monkeypatch):
    c = M.case(cid)
    n, m = M.PAIRS, M.PAIRS_SECOND
    exp, rng = M.oracle_sample(c)
    assert exp["status"] == 0 and exp["n_done"] == n + m
    gid = _load(engine, c, capfd, monkeypatch)
    engine.seed_mt(M.MT_SEED)
    engine.reserve(n + m)
    engine.mt_set_fragment(*M.fragment(c))
    engine.mt_mutations_reserve(2 * c.RL * n + 16 if c.mutations else 0)
    try:
        r0, w0 = engine.mt_path_counts()
        assert engine.generate_mt(gid, n, gc_bias=c.gc_frag) == n
        rows_a = engine.mt_mutations().copy() if c.mutations else None
        # a second work item on the same streams: its offsets start in the middle of the buffers
        assert engine.generate_mt(gid, m, gc_bias=c.gc_frag, out_first_pair=n) == m
        rows_b = engine.mt_mutations().copy() if c.mutations else None
        resolved, walked = (a - b for a, b in zip(engine.mt_path_counts(), (r0, w0)))
        got, coords = engine.download(0, n + m), engine.coords(0, n + m)
        py, npw = engine.mt_peek(8)
    finally:
        engine.mt_set_fragment(None, None)
        engine.mt_mutations_reserve(0)
    _assert_rows(got, exp, 0, n + m, cid, coords)
    if c.mutations:
        rows = exp["mutations"]
        second = rows[rows["pair"] >= n].copy()
        second["pair"] -= n  # (the rows of a call count its pairs from 0)
        _assert_mutations(rows_a, rows[rows["pair"] < n], cid + ", first item")
        _assert_mutations(rows_b, second, cid + ", second item")
    # both streams stand where the oracle's stand
    assert list(_res53(py)) == [rng.py_random() for _ in range(4)], cid
    assert list(_res53(npw)) == [rng.np_random() for _ in range(4)], cid
    touched = int(M.touches_n(c, exp["coords"]).sum())
    assert resolved + walked == n + m and touched <= M.TOUCH_CAP * (n + m)
    if c.pick is None:
        assert (resolved, walked) == (0, n + m)
    else:
        assert walked >= touched and resolved >= 0.75 * (n + m), (resolved, walked, touched)
        if c.indels:  # every read with an indel is the walker's too (and the candidates that came to nothing)
            other = np.setdiff1d(M.indel_pairs(exp["mutations"]), np.flatnonzero(M.touches_n(c, exp["coords"])))
            assert walked >= touched + len(other) > touched, (resolved, walked, touched, len(other))
            # ... and no more than the candidates the model's own rates allow: each of a position's five tests is one when the 27
            # leading bits of its draw are below its limit (the rate, rounded up), so their number over the call is a sum of
            # independent rare events of mean lam; six standard deviations above it is out of reach of any sample
            d = M.model(c)
            lam = (n + m) * float((d.ins + 2.0 ** -26).sum() + (d.dele.max(axis=2) + 2.0 ** -26).sum())
            assert 40 < lam and walked - touched <= lam + 6.0 * lam ** 0.5, (walked, touched, lam)
        elif not c.gc_frag:  # (with gc_bias the walker's turn goes on to the next pair that is kept)
            assert walked == touched, (resolved, walked, touched)


@pytest.mark.parametrize("cid", M.WORKER_CASES)
def test_worker_set_matches_the_oracle(cid, capfd, monkeypatch):
    """Three workers side by side (k_mt_resolve_w, k_mt_emit_w: one workgroup, one grid row a worker) on the case's model: each
    worker's rows, coordinates and next stream words equal those of an oracle run of its own seed."""
    from insilicoseq_amd.engine import ReadEngine

    c = M.case(cid)
    n, W = M.WORKER_PAIRS, len(M.WORKER_SEEDS)
    first = [w * n for w in range(W)]
    with ReadEngine(0) as eng:
        gid = _load(eng, c, capfd, monkeypatch)
        eng.seed_mt_workers(list(M.WORKER_SEEDS))
        eng.reserve(W * n)
        r0, w0 = eng.mt_path_counts()
        done, status = eng.generate_mt_workers([gid] * W, [n] * W, first)
        assert list(done) == [n] * W and list(status) == [0] * W
        resolved, walked = (a - b for a, b in zip(eng.mt_path_counts(), (r0, w0)))
        assert eng.mt_resolver() == c.pick
        touched = 0
        for w, seed in enumerate(M.WORKER_SEEDS):
            exp, rng = M.oracle_sample(c, n=n, seed=seed)
            assert exp["status"] == 0 and exp["n_done"] == n
            _assert_rows(eng.download(first[w], n), exp, 0, n, (cid, "worker", w), eng.coords(first[w], n))
            py, npw = eng.mt_workers_peek(w, 8)
            assert list(_res53(py)) == [rng.py_random() for _ in range(4)], (cid, w)
            assert list(_res53(npw)) == [rng.np_random() for _ in range(4)], (cid, w)
            touched += int(M.touches_n(c, exp["coords"]).sum())
        assert resolved + walked == W * n
        assert walked >= touched > 0 and resolved >= 0.75 * W * n, (resolved, walked, touched)
