"""Shared helpers for the parity tests."""
import collections
import json
import os
import re

import numpy as np

from insilicoseq_amd.model import DenseModel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PROFILES = os.path.join(os.path.dirname(GOLDEN), "..", "insilicoseq_amd", "profiles")


def dense_model(name, indel=None):
    path = os.path.join(PROFILES, name + ".dense.npz")
    if not os.path.exists(path):  # models minted for the tests only (tests/golden/models: the reference's `iss model` on data/ecoli.bam)
        path = os.path.join(GOLDEN, "models", name + ".dense.npz")
    d = DenseModel.basic() if name == "basic" else DenseModel.load(path)
    if indel is not None:
        d.ins[:] = indel[0]
        d.dele[:] = indel[1]
    return d


def load_pairs_case(case):
    z = np.load(os.path.join(GOLDEN, "pairs", case + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    return z, meta


def pairs_cases():
    return sorted(f[:-4] for f in os.listdir(os.path.join(GOLDEN, "pairs")) if f.endswith(".npz"))


def random_genome(seed, n, alphabet="ACGT"):
    rng = np.random.RandomState(seed)
    idx = rng.randint(0, len(alphabet), size=n)
    return np.frombuffer(alphabet.encode(), dtype=np.uint8)[idx].tobytes().decode()


def mixed_genome(seed, n):
    rng = np.random.RandomState(seed)
    x = rng.random_sample(n)
    plain = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, n)]
    lower = np.frombuffer(b"acgt", dtype=np.uint8)[rng.randint(0, 4, n)]
    amb = np.frombuffer(b"NRYWSMKHBVD", dtype=np.uint8)[rng.randint(0, 11, n)]
    ambl = np.frombuffer(b"nrywsmkhbvd", dtype=np.uint8)[rng.randint(0, 11, n)]
    out = np.where(x < 0.8, plain, np.where(x < 0.92, lower, np.where(x < 0.97, amb, ambl)))
    return out.astype(np.uint8).tobytes().decode()


def synthetic_model(read_length, n_q, n_isize, seed, indel=(1e-3, 2e-3), nonempty=((1, 1, 1, 1), (1, 0, 1, 1))):
    """A random but valid dense model at arbitrary sizes (limits of the engine: read_length 1024, 60 phred entries,
    8000 insert sizes).  phred_thr follows util.phred_to_prob like the real profiles."""
    rng = np.random.RandomState(seed)
    RL = read_length

    def cdf(shape):
        w = rng.gamma(0.3, size=shape) + 1e-12
        c = np.cumsum(w, axis=-1)
        c /= c[..., -1:]
        c[..., -1] = 1.0
        return c

    isize = cdf((n_isize,))
    bin_w = rng.random_sample((2, 4)) * np.asarray(nonempty, dtype=np.float64) + 1e-9 * np.asarray(nonempty)
    bin_cdf = np.cumsum(bin_w, axis=1)
    bin_cdf /= bin_cdf[:, -1:]
    qcdf = cdf((2, 4, RL, n_q))
    subst_cdf = cdf((2, RL, 4, 3))
    alts = {0: b"TCG", 1: b"ACG", 2: b"ATG", 3: b"ATC"}  # base order A, T, C, G
    subst_alt = np.zeros((2, RL, 4, 3), dtype=np.uint8)
    for b in range(4):
        subst_alt[:, :, b, :] = np.frombuffer(alts[b], dtype=np.uint8)
    ins = np.full((2, RL, 4), indel[0]) * rng.random_sample((2, RL, 4))
    dele = np.full((2, RL, 4), indel[1]) * rng.random_sample((2, RL, 4))
    ins_letter = np.zeros((2, RL, 4), dtype=np.uint8)
    ins_letter[:] = np.frombuffer(b"ATCG", dtype=np.uint8)
    phred_thr = 1.0 - 10.0 ** (-np.arange(n_q + 1) / 10.0)
    return DenseModel(RL, isize, bin_cdf, np.asarray(nonempty, dtype=np.uint8), qcdf, subst_cdf, subst_alt, ins, ins_letter,
                      dele, phred_thr)


# ------------------------------------------------------------------ the plain formatters (no library code: the expected text)
def fastq_text(record_id, first_i, cpu_number, mate, bases, quals):
    """FASTQ text of one mate's reads (uint8 [n, read_length] letters and phreds), pair k named record_id_(first_i + k)_cpu/mate
    (SeqIO.write(..., 'fastq-sanger'), iss/generator.py:64-65).  record_id: str, or bytes as the C ABI takes them."""
    out = []
    rid = record_id if isinstance(record_id, bytes) else record_id.encode()
    for k in range(len(bases)):
        out.append(b"@%s_%d_%d/%d\n" % (rid, first_i + k, cpu_number, mate) + bases[k].tobytes() + b"\n+\n"
                   + (quals[k].astype(np.uint8) + 33).tobytes() + b"\n")
    return b"".join(out)


def vcf_lines(record_id, first_i, cpu_number, mutations):
    """The --store_mutations lines of the oracle's mutation rows (iss/generator.py:598-620): an insertion's alt is ref + the
    inserted letter, only a substitution carries its phred."""
    lines = []
    for m in mutations:
        ref, alt = chr(m["ref"]), chr(m["alt"])
        alt = ref + alt if m["type"] == 1 else alt
        qual = str(int(m["quality"])) if m["type"] == 0 else "."
        lines.append("\t".join(["%s_%d_%d/%d" % (record_id, first_i + int(m["pair"]), cpu_number, 1 + int(m["mate"])),
                                str(int(m["position"]) + 1), ".", ref, alt, qual, "", ""]) + "\n")
    return lines


# ------------------------------------------------------------------ the read-length sweep of the row readers
# 2, 5, 7: one partial piece; 8, 16: pitch == RL; 32, 64, 128, 256, 1024: no padding in the last line; 9, 31, 33, 100, 250,
# 997: a partial last piece; 997, 1024: the engine's limit (128 pieces a mate)
ROW_SWEEP = (2, 5, 7, 8, 9, 16, 31, 32, 33, 64, 100, 128, 250, 256, 997, 1024)
ROW_SWEEP_PAIRS = 205  # rows of a case: 200 pairs from first pair 5
ROW_SWEEP_SEED, ROW_SWEEP_FIRST_ORDINAL, ROW_SWEEP_MT_SEED = 31, 3, 4321
ROW_SWEEP_WORK = (70, 0, 130)  # pairs of the --store_mutations work list's three records
ROW_SWEEP_WORKER_SEED, ROW_SWEEP_CPU = 11, 2


def row_sweep_model(RL):
    """The sweep's model at read length RL (random tables with indels, two empty mean-quality bins).  Few phreds: a
    substitution at every third position or so (from 100 positions on a few more phreds, to keep the VCF of a case below a
    megabyte or two).  Below 100 positions the default indel rates would leave the 200 pairs of a case with a handful of
    insertions and deletions at best, so they are raised there."""
    n_q = 1 if RL == 2 else 3 if RL < 8 else 9 if RL < 100 else 30
    return synthetic_model(RL, n_q, 7, seed=4000 + RL, indel=(0.02, 0.04) if RL < 100 else (1e-3, 2e-3))


def row_sweep_genome(RL, k=0):
    return mixed_genome(50 * RL + k, max(8 * RL + 7, 64) + 100 * k)


def row_sweep_oracle_rows(dense, rng, genome, n, first_ordinal=0, oracle_kw=None):
    """The oracle's reads as (bases [n, 2, RL], phreds [n, 2, RL], coordinates [n, 4])."""
    from oracle import oracle as O

    res = O.Oracle(dense, **(oracle_kw or {})).simulate(rng, genome, n, first_ordinal=first_ordinal, want_coords=True)
    assert res["status"] == 0 and res["n_done"] == n
    return {"bases": np.stack([res["r1_base"], res["r2_base"]], axis=1), "qual": np.stack([res["r1_qual"], res["r2_qual"]], axis=1),
            "coords": res["coords"]}


def row_sweep_worker_files(dense, RL):
    """The sweep's --store_mutations work list (three records, the second with no pairs) and what worker_iterator has to write
    for it in Philox mode: (record ids, sequences, pair counts), R1 text, R2 text, VCF text, the rows' types."""
    from oracle import oracle as O

    ids = ["w%d.%d" % (RL, k) for k in range(3)]
    seqs = [row_sweep_genome(RL, 1 + k) for k in range(3)]
    orc, rng = O.Oracle(dense), O.Rng().seed_philox(ROW_SWEEP_WORKER_SEED + ROW_SWEEP_CPU)
    r1, r2, lines, types, ordinal = [], [], [], [], 0
    for rid, seq, n in zip(ids, seqs, ROW_SWEEP_WORK):
        res = orc.simulate(rng, seq, n, first_ordinal=ordinal, store_mutations=True)
        assert res["status"] == 0 and res["n_done"] == n
        ordinal += n
        r1.append(fastq_text(rid, 0, ROW_SWEEP_CPU, 1, res["r1_base"], res["r1_qual"]))
        r2.append(fastq_text(rid, 0, ROW_SWEEP_CPU, 2, res["r2_base"], res["r2_qual"]))
        lines += vcf_lines(rid, 0, ROW_SWEEP_CPU, res["mutations"])
        types += res["mutations"]["type"].tolist()
    return (ids, seqs, ROW_SWEEP_WORK), b"".join(r1), b"".join(r2), "".join(lines), types


def export_tile_pairs(RL, max_tile=64, lds_budget=48 * 1024):
    """Pairs of a k_rows_export workgroup, by the rule of iss_export.hip.h: at most 64, both dense images of the tile (each
    tile * 2 RL bytes rounded up to 16, + 16 for the offset of its first byte) within 48 KB of LDS."""
    def region(t):
        return ((t * 2 * RL + 15) // 16 + 1) * 16

    t = min(max_tile, (lds_budget - 64) // (4 * RL))
    while t > 0 and 2 * region(t) > lds_budget:
        t -= 1
    return t


def export_tile_alignments(RL, n_pairs, shift):
    """Addresses mod 16 at which the tiles of one export of n_pairs pairs start in an output array that begins at ``shift``."""
    tile = export_tile_pairs(RL)
    return [(shift + t0 * 2 * RL) % 16 for t0 in range(0, n_pairs, tile)]


# ------------------------------------------------------------------ the position-tile geometries of k_main / k_main_g
# What the two kernels execute is fixed at model upload by the position tiling (iss_api_model.hip.h, fits()): TS superitems (of 8
# positions) per tile, n_tiles, ni = ceil(TS / 4) iterations per pass, how short the last tile is -- and from ni the width of the
# iteration field of a deferred entry's tag (it_bits), the script rows per tile and read (sc_gpt = ceil(ni / 8)) and the
# k_main_g<NI, NP> instantiation.  The shipped profiles reach ni 1, 2, 4 and 5 only; these rows reach the rest.  Guide bits are
# pinned to 6 (TILE_GEOMETRY_ENV), so the width of a table row -- and with it the tiling -- follows from n_q alone.
# test_tile_geometry_host.py derives (n_tiles, TS, last, ni) of every row from its (RL, n_q, slots, ISS_TILES); the GPU sweep
# asserts what the library reports (model_geometry) against the row before it compares a single read.
TileGeometry = collections.namedtuple("TileGeometry", "id RL n_q nonempty tiles n_tiles TS last ni what")
SLOTS_DEFAULT = ((1, 1, 1, 1), (1, 0, 1, 1))  # synthetic_model's own: 4 / 3 mean-quality bins with histograms
SLOTS_TWO = ((1, 0, 1, 0), (0, 1, 0, 1))
SLOTS_ONE = ((1, 0, 0, 0), (0, 0, 1, 0))
TILE_GEOMETRIES = (
    TileGeometry("A", 65, 9, SLOTS_DEFAULT, 0, 1, 9, 9, 3, "k_main_g<3, 1>; third iteration: one lane of work, one valid position in the last superitem"),
    TileGeometry("B", 96, 9, SLOTS_DEFAULT, 0, 1, 12, 12, 3, "ni == 3 exact, row without padding"),
    TileGeometry("C", 151, 9, SLOTS_DEFAULT, 2, 2, 12, 7, 3, "NI == 3 with a last tile of two iterations"),
    TileGeometry("D", 185, 9, SLOTS_DEFAULT, 2, 2, 12, 12, 3, "two full tiles, RL % 8 == 1"),
    TileGeometry("E", 33, 9, SLOTS_DEFAULT, 2, 2, 4, 1, 1, "last tile: one superitem with one position; k_main_g<1, 2>"),
    TileGeometry("F", 301, 4, SLOTS_TWO, 0, 1, 38, 38, 10, "sc_gpt == 2, it_bits == 4"),
    TileGeometry("G", 260, 4, SLOTS_TWO, 0, 1, 33, 33, 9, "ninth iteration: lane 0 only; group 1 of the script rows holds one iteration"),
    TileGeometry("H", 384, 3, SLOTS_ONE, 0, 1, 48, 48, 12, "pitch == AP_MAX_PITCH, the last scripted length"),
    TileGeometry("I", 392, 3, SLOTS_ONE, 0, 1, 49, 49, 13, "first pitch above it: all listed reads to k_indel_fixup, idle scripts of two groups"),
    TileGeometry("J", 520, 2, SLOTS_ONE, 0, 1, 65, 65, 17, "it_bits == 5, sc_gpt == 3"),
    TileGeometry("K", 640, 3, SLOTS_ONE, 0, 1, 80, 80, 20, "largest one-tile model: about 153 KB of the 158 KB LDS budget"),
)
TILE_GEOMETRY_ENV = {"ISS_GUIDE_BITS": "6", "ISS_DEBUG_MODEL": "1"}
# the grouped route of the sweep: geometry -> (ISS_MAIN_GROUP, the kernel that must have run).  F has no instantiation (ni == 10):
# the host keeps k_main.  test_tile_geometry_host.py holds ISS_MAIN_G_LIST to these and test_gpu_grouped.FORCED.
TILE_GROUPED = {"A": (1, "k_main_g<3, 1>"), "B": (1, "k_main_g<3, 1>"), "C": (1, "k_main_g<3, 1>"), "D": (1, "k_main_g<3, 1>"),
                "E": (2, "k_main_g<1, 2>"), "F": (1, "k_main<false, true, false>")}
TILE_INDEL = (1e-3, 2e-3)
ModelGeometry = collections.namedtuple("ModelGeometry", "RL NB GB TG TS n_tiles ni")


def tile_geometry(gid):
    return next(g for g in TILE_GEOMETRIES if g.id == gid)


def tile_geometry_model(geo, indel=False):
    """The dense model of a row of TILE_GEOMETRIES: random tables, without indels or with TILE_INDEL's rates."""
    return synthetic_model(geo.RL, geo.n_q, 7, seed=7000 + geo.RL, indel=TILE_INDEL if indel else (0.0, 0.0), nonempty=geo.nonempty)


def tile_geometry_genome_length(geo):
    return max(8 * geo.RL + 7, 64) + 1000


def model_geometry(stderr_text):
    """The layout iss_model_upload reports under ISS_DEBUG_MODEL=1 -- its line
    `[model] RL .. G .. NB .. GB .. stride_w .. GS .. TG .. n_tiles ..` (the last one of the text) -- as (RL, NB, GB, TG,
    TS = TG / 2, n_tiles, ni = ceil(TS / 4))."""
    found = re.findall(r"\[model\] RL (\d+) G \d+ NB (\d+) GB (\d+) stride_w \d+ GS \d+ TG (\d+) n_tiles (\d+)", stderr_text)
    assert found, "no [model] layout line in: %r" % stderr_text[-400:]
    RL, NB, GB, TG, n_tiles = (int(x) for x in found[-1])
    assert TG % 2 == 0
    return ModelGeometry(RL, NB, GB, TG, TG // 2, n_tiles, (TG // 2 + 3) // 4)


def tag_iteration_bits(ni):
    """Bits of the iteration field of a deferred entry's tag (k_main: it_bits), of the 13 that hold (pass, iteration)."""
    return (ni - 1).bit_length()


GUARD = 64


class Guarded(object):
    """A device buffer of ``nbytes`` with GUARD bytes of 0xA5 on either side (``shift``: the payload's address mod 16)."""

    def __init__(self, nbytes, dtype, shape, shift=0, fill=0xA5):
        import torch

        self.torch, self.dtype, self.shape, self.nbytes = torch, dtype, shape, nbytes
        self.buf = torch.full((GUARD + shift + nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda:0")
        self.at = GUARD + shift
        assert (self.buf.data_ptr() + self.at) % 16 == shift % 16
        self.ptr = self.buf.data_ptr() + self.at

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return bool((b[:self.at] == 0xA5).all() and (b[self.at + self.nbytes:] == 0xA5).all())

    def untouched(self):
        return bool((self.buf.cpu().numpy() == 0xA5).all())

    def value(self):
        return self.buf.cpu().numpy()[self.at:self.at + self.nbytes].view(self.dtype).reshape(self.shape)
