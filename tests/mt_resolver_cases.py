"""The cases of the MT resolver sweep: rng="mt" through k_mt_resolve / k_mt_resolve_w and k_mt_emit / k_mt_emit_w over the read
lengths at which their hand arithmetic changes.

The resolver is eligible only for a model without indel candidates to speak of (mt_bounce_rate < 0.05), so the models here have
indel tables of exact zeros (all but two: see the end of CASES): mt_lim is all zero, no pair is bounced for a candidate, and what
goes to the walker is exactly the pairs that touch a letter outside ACGT.  The record is random ACGT with an N at every 4001st letter: 2 to 8 % of the mates touch
one over the sweep, so the hand-over to the walker and the resume at an arbitrary ring offset run a hundred times a case.

Three flavours of the quality tables:
  noisy  the tables as generated: 0.12 substitutions a base, no mate without one -- every pair takes the resolver's "the guess
         was wrong, the second mate again from its true numpy offset" branch
  clean  qcdf[..., :30] = 0: phreds of 30 and more, most first mates without a substitution -- the first guess mostly holds
  worst  qcdf[...] = 1.0: every phred 0, every ACGT base substituted -- a pair consumes the most numpy words a pair can, the case
         mt_res_need_np is sized for

The read lengths: 113/114, 159/160/161, 214/215, 246/247, 308/309, 331/332 are where mt_pick_resolver changes its pick for one,
two and four bin slots (CASES below); 246 is where the numpy ring has no slack (8 * 246 + 80 = 2048 words = one half), 331 where
the python ring has 12 words (8180 of 8192); 192/193 is spare_wave, 256/257 the second trip of the position loop.

Each case carries the instantiation mt_pick_resolver must pick for it as a literal; test_mt_resolver_sweep_host.py derives the
literals from a restatement of the rule, the GPU test asserts what the library reports against them."""
import collections
import functools

import numpy as np

from helpers import random_genome, synthetic_model

SLOTS = {1: ((1, 0, 0, 0), (0, 0, 1, 0)), 2: ((1, 1, 0, 0), (0, 1, 1, 0)), 4: ((1, 1, 1, 1), (1, 0, 1, 1))}  # NB -> nonempty
N_ISIZE = 50
PAIRS, PAIRS_SECOND, MT_SEED = 2048, 300, 4321  # a call of PAIRS pairs, then a second item on the same streams
N_SPACING = 4001
TOUCH_CAP = 0.20  # share of a case's pairs that may touch an N (the GPU test demands a resolver share of 0.75)
WORKER_SEEDS, WORKER_PAIRS = (40, 41, 42), 700

ROWS, NO_ROWS = True, False
Case = collections.namedtuple("Case", "id RL NB n_q flavour pick gc_frag mutations indels")


def _case(RL, NB, flavour, pick, n_q=41, gc_frag=False, mutations=False, indels=False):
    cid = ("RL%d-NB%d-%s" % (RL, NB, flavour) + ("" if n_q == 41 else "-q%d" % n_q) + ("-gc" if gc_frag else "") + ("-vcf" if mutations else "")
           + ("-indels" if indels else ""))
    return Case(cid, RL, NB, n_q, flavour, pick, gc_frag, mutations, indels)


def _rows(table, flavours, **kw):
    return [_case(RL, NB, f, pick, **kw) for (RL, NB, pick) in table for f in flavours]


# (python ring half in K words, numpy ring half in K words, digit rows in LDS); None: the walker only
CASES = tuple(
    # one bin slot: the rows fit the LDS up to 308 positions; the numpy ring doubles from 247 on
    _rows([(246, 1, (8, 2, ROWS)), (247, 1, (8, 4, ROWS)), (331, 1, (8, 4, NO_ROWS))], ("noisy", "clean", "worst"))
    + _rows([(308, 1, (8, 4, ROWS)), (309, 1, (8, 4, NO_ROWS))], ("noisy", "clean"))
    + _rows([(332, 1, None)], ("noisy",))
    # two bin slots: the rows leave the LDS at 215
    + _rows([(214, 2, (8, 2, ROWS)), (215, 2, (8, 2, NO_ROWS))], ("noisy", "clean"))
    # four bin slots: 8 K python words with rows up to 113, 4 K with rows up to 159 (need_py <= 4096 ends at 160, where the rows
    # no longer fit either), then rows from memory
    + _rows([(113, 4, (8, 2, ROWS)), (114, 4, (4, 2, ROWS)), (159, 4, (4, 2, ROWS)), (160, 4, (8, 2, NO_ROWS)), (161, 4, (8, 2, NO_ROWS)),
             (192, 4, (8, 2, NO_ROWS)), (193, 4, (8, 2, NO_ROWS)), (256, 4, (8, 4, NO_ROWS)), (257, 4, (8, 4, NO_ROWS))], ("noisy", "clean"))
    + _rows([(246, 4, (8, 2, NO_ROWS)), (247, 4, (8, 4, NO_ROWS)), (331, 4, (8, 4, NO_ROWS))], ("noisy",))
    # the lookup path of every n_q but 41 (clamped indices into the 0xffff padding), at size.  (n_q 1: the one phred is 0, so its
    # noisy tables are the worst ones as well.  Rows of 31 words (n_q 60) do not fit the LDS at four slots and 160 positions, rows
    # of 5 words (n_q 7) still do at two slots and 331)
    + _rows([(160, 4, (8, 2, NO_ROWS))], ("noisy", "worst"), n_q=60)
    + _rows([(331, 2, (8, 4, ROWS))], ("noisy", "worst"), n_q=7)
    + _rows([(246, 1, (8, 2, ROWS))], ("noisy", "worst"), n_q=1)
    # gc_bias with a custom fragment length (2 RL + 60, 25): the polar loop's words and the gc draw on top of a full pair
    + _rows([(246, 1, (8, 2, ROWS)), (331, 1, (8, 4, NO_ROWS)), (160, 4, (8, 2, NO_ROWS))], ("noisy", "worst"), gc_frag=True)
    # --store_mutations rows, every field
    + [_case(193, 4, "noisy", (8, 2, NO_ROWS), mutations=True), _case(331, 1, "worst", (8, 4, NO_ROWS), mutations=True)]
    # the one thing zero indel tables leave out: the indel-candidate check, which moves from a spare wavefront into the position
    # lanes at 193.  Rates of INDELS keep the model eligible (about 0.03 candidates a pair); every candidate goes to the walker
    + _rows([(192, 4, (8, 2, NO_ROWS)), (193, 4, (8, 2, NO_ROWS))], ("noisy",), mutations=True, indels=True)
)
INDELS = (2e-5, 4e-5)
# the worker set (k_mt_resolve_w, k_mt_emit_w): one case for every instantiation the sweep reaches
WORKER_CASES = tuple(c.id for c in CASES if c.id in ("RL246-NB1-noisy", "RL159-NB4-noisy", "RL308-NB1-noisy", "RL246-NB4-noisy",
                                                     "RL331-NB1-noisy"))
REACHED = ((8, 2, ROWS), (4, 2, ROWS), (8, 4, ROWS), (8, 2, NO_ROWS), (8, 4, NO_ROWS))  # ISS_MT_RESOLVERS, in its order
assert len({c.id for c in CASES}) == len(CASES) and len(WORKER_CASES) == len(REACHED)


def case(cid):
    return next(c for c in CASES if c.id == cid)


def fragment(c):
    """(fragment_length, fragment_sd) of a gc_frag case, else (None, None)."""
    return (2.0 * c.RL + 60.0, 25.0) if c.gc_frag else (None, None)


def model(c):
    """The case's dense model: random tables without indels (but for the two cases that are about them) at its bin layout, the
    quality CDFs by flavour."""
    d = synthetic_model(c.RL, c.n_q, N_ISIZE, seed=7000 + c.RL, indel=INDELS if c.indels else (0.0, 0.0), nonempty=SLOTS[c.NB])
    assert c.indels or not (d.ins.any() or d.dele.any())
    if c.flavour == "clean":
        d.qcdf[..., :30] = 0.0
    elif c.flavour == "worst":
        d.qcdf[...] = 1.0  # (iss_model_upload takes a CDF whose first entry is 1.0: a threshold of 2^53)
    else:
        assert c.flavour == "noisy"
    return d


@functools.lru_cache(maxsize=None)
def genome(RL):
    g = np.frombuffer(random_genome(RL, 40 * RL).encode(), dtype=np.uint8).copy()
    g[N_SPACING - 1::N_SPACING] = ord("N")
    return g.tobytes().decode()


def oracle_sample(c, n=PAIRS + PAIRS_SECOND, seed=MT_SEED):
    """The oracle's MT sample of the case: n pairs from seed, with coordinates and mutation rows, and the oracle's Rng behind it
    (its next words are what the device's streams must show)."""
    from oracle import oracle as O

    rng = O.Rng().seed_mt(seed)
    mu, sd = fragment(c)
    res = O.Oracle(model(c)).simulate(rng, genome(c.RL), n, fragment_length=mu, fragment_sd=sd, gc_bias=c.gc_frag,
                                      store_mutations=True, want_coords=True)
    return res, rng


def templates(c, coords):
    """The two templates of every pair as letters [n, RL]: the forward strand at fs, the reverse complement ending at re."""
    g = np.frombuffer(genome(c.RL).encode(), dtype=np.uint8)
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGTN")] = list(b"TGCAN")
    p = np.arange(c.RL)
    fwd = g[coords[:, 0:1] + p]
    rev = comp[g[coords[:, 2:3] - 1 - p]]
    return fwd, rev


def touches_n(c, coords):
    """Per pair: a letter outside ACGT in either template."""
    fwd, rev = templates(c, coords)
    return (fwd == ord("N")).any(axis=1) | (rev == ord("N")).any(axis=1)


def indel_pairs(rows):
    """Pairs with an insertion or deletion row among the mutation rows of a sample."""
    return np.unique(rows["pair"][rows["type"] != 0])
