"""`generate --variants` without a GPU (insilicoseq_amd/variants.py, iss_variants_core.h through the library's host entries): the
VCF parser, the splice and the lift against the naive definitions, the chain file, the exports."""
import gzip
import io
import os
import re

import numpy as np
import pytest

import variant_cases as VC
from insilicoseq_amd import variants as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("iss_genome_upload_variants", "iss_genome_download", "iss_variants_lift", "iss_variants_apply_tile",
               "iss_variants_host_apply", "iss_variants_host_lift")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge

    ge.build()
    from insilicoseq_amd import _native

    return _native


# ---------------------------------------------------------------------- 1. the parser
HEADER = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\n"
RECORDS = {"chr1": 40, "chr2": 12}


def _vcf(tmp_path, lines, name="v.vcf"):
    path = str(tmp_path / name)
    text = HEADER + "".join("\t".join(str(x) for x in line) + "\n" for line in lines)
    if name.endswith(".gz"):
        with gzip.open(path, "wt") as fh:
            fh.write(text)
    else:
        with open(path, "w") as fh:
            fh.write(text)
    return path


def _line(chrom, pos, ref, alt, gt="0|1"):
    return (chrom, pos, ".", ref, alt, ".", "PASS", ".", "GT:DP", gt + ":9", "1|1:3")


def _rows(table):
    return [(int(p), bytes(table.ref[ro:ro + r]).decode(), bytes(table.alt[ao:ao + a]).decode())
            for p, r, a, ro, ao in zip(table.pos0, table.ref_len, table.alt_len, table.ref_off, table.alt_off)]


def test_trimming_keeps_only_what_changes(tmp_path):
    path = _vcf(tmp_path, [
        _line("chr1", 3, "gAT", "gC"),       # anchor g (lower case) kept: AT -> C at pos0 3
        _line("chr1", 10, "A", "ATT"),       # insertion behind the anchor: pos0 10
        _line("chr1", 15, "ACGT", "AT"),     # prefix A, suffix T: CG -> "" at pos0 15
        _line("chr1", 20, "c", "C"),         # nothing changes when case is ignored: dropped
        _line("chr1", 25, "TCA", "tGa"),     # prefix and suffix in another case: C -> G at pos0 25
        _line("chr2", 1, "G", "T"),
    ])
    tables, skipped = V.read_vcf(path, RECORDS)
    assert _rows(tables["chr1"]) == [(3, "AT", "C"), (10, "", "TT"), (15, "CG", ""), (25, "C", "G")]
    assert _rows(tables["chr2"]) == [(0, "G", "T")]
    assert skipped["no_change"] == 1 and sum(skipped.values()) == 1
    t = tables["chr1"]
    assert t.out_pos.tolist() == [3, 9, 16, 24, 40 - 1 + 2 - 2] and t.haplotype_length(40) == 39
    assert t.out_pos.dtype == np.int64 and t.pos0.dtype == np.int64 and t.alt_off.dtype == np.int64 and t.ref_off.dtype == np.int64
    assert t.ref_len.dtype == np.int32 and t.alt_len.dtype == np.int32 and t.alt.dtype == np.uint8 and t.ref.dtype == np.uint8
    assert t.counts() == {"snv": 1, "mnv": 0, "insertion": 1, "deletion": 2, "bases_inserted": 2, "bases_deleted": 3}


def test_gzip_input_and_multi_allelic_lines(tmp_path):
    lines = [_line("chr1", 5, "A", "C,G", "2|1"), _line("chr1", 9, "AT", "A,ATT,<DEL>", "3|2")]
    for name in ("v.vcf", "v.vcf.gz"):
        path = _vcf(tmp_path, lines, name)
        tables, skipped = V.read_vcf(path, RECORDS)  # the first ALT of every line, the GT ignored
        assert _rows(tables["chr1"]) == [(4, "A", "C"), (9, "T", "")]
        tables, skipped = V.read_vcf(path, RECORDS, haplotype=1)
        assert _rows(tables["chr1"]) == [(4, "A", "G")] and skipped["symbolic"] == 1
        tables, skipped = V.read_vcf(path, RECORDS, haplotype=2)
        assert _rows(tables["chr1"]) == [(4, "A", "C"), (10, "", "T")]


def test_haplotype_choice(tmp_path):
    lines = [_line("chr1", 2, "A", "C", "0|1"), _line("chr1", 4, "A", "C", "1|0"), _line("chr1", 6, "A", "C", "1/1"),
             _line("chr1", 8, "A", "C", "./."), _line("chr1", 10, "A", "C", "0/0")]
    path = _vcf(tmp_path, lines)
    t1, s1 = V.read_vcf(path, RECORDS, haplotype=1)
    t2, s2 = V.read_vcf(path, RECORDS, haplotype=2)
    assert [r[0] for r in _rows(t1["chr1"])] == [3, 5] and s1["haplotype_ref"] == 3
    assert [r[0] for r in _rows(t2["chr1"])] == [1, 5] and s2["haplotype_ref"] == 3
    t0, s0 = V.read_vcf(path, RECORDS)
    assert [r[0] for r in _rows(t0["chr1"])] == [1, 3, 5, 7, 9] and sum(s0.values()) == 0


def test_unphased_heterozygous_is_one_line(tmp_path):
    path = _vcf(tmp_path, [_line("chr1", 2, "A", "C", "1|0"), _line("chr1", 7, "A", "C", "0/1")])
    V.read_vcf(path, RECORDS)  # (without a haplotype the GT is not read)
    with pytest.raises(V.VcfError) as e:
        V.read_vcf(path, RECORDS, haplotype=2)
    msg = str(e.value)
    assert "\n" not in msg and path in msg and "line 4" in msg and "0/1" in msg


def test_every_skipped_class_is_counted(tmp_path):
    path = _vcf(tmp_path, [
        _line("chr1", 2, "A", "<DUP>"), _line("chr1", 3, "A", "<INS:ME>"), _line("chr1", 4, "A", "*"),
        _line("chr1", 5, "A", "A[chr2:3["), _line("chr1", 6, "A", "]chr2:3]A"), _line("chr1", 7, "A", "."),
        _line("chrUn", 8, "A", "C"), _line("chrUn", 9, "A", "C"), _line("chrUn", 10, "A", "C"), _line("chr1", 11, "A", "a"),
        _line("chr1", 12, "A", "C"),
    ])
    tables, skipped = V.read_vcf(path, RECORDS)
    assert skipped == {"symbolic": 2, "star": 1, "breakend": 2, "missing_alt": 1, "unknown_chrom": 3, "haplotype_ref": 0, "no_change": 1}
    assert list(tables) == ["chr1"] and _rows(tables["chr1"]) == [(11, "A", "C")]


@pytest.mark.parametrize("lines, words", [
    ([_line("chr1", 5, "ACG", "A"), _line("chr1", 7, "G", "T")], ("chr1", "POS 5", "POS 7")),           # overlap
    ([_line("chr1", 9, "A", "AC"), _line("chr1", 9, "A", "AGG")], ("chr1", "POS 9")),                      # two insertions at one place
    ([_line("chr2", 12, "AC", "A")], ("chr2", "POS 12", "end")),                                           # past the end
    ([_line("chr2", 14, "A", "C")], ("chr2", "POS 14", "end")),
])
def test_table_errors_are_single_lines(tmp_path, lines, words):
    with pytest.raises(V.VcfError) as e:
        V.read_vcf(_vcf(tmp_path, lines), RECORDS)
    msg = str(e.value)
    assert "\n" not in msg
    for w in words:
        assert w in msg, (w, msg)


def test_an_insertion_behind_the_last_letter_is_allowed(tmp_path):
    tables, _ = V.read_vcf(_vcf(tmp_path, [_line("chr2", 12, "A", "ACC")]), RECORDS)
    assert _rows(tables["chr2"]) == [(12, "", "CC")]


# ---------------------------------------------------------------------- 2. the splice
def _check_splice(seq, variants):
    t = VC.table_of(seq, variants)
    want = VC.naive_splice(seq, variants)
    assert t.apply_host(seq).tobytes().decode() == want
    assert t.apply_native(seq).tobytes().decode() == want
    assert t.haplotype_length(len(seq)) == len(want) == int(t.out_pos[-1])
    assert t.ref_mismatches(seq) == []
    return t


@pytest.mark.parametrize("case", VC.hand_cases(), ids=lambda c: c[0])
def test_splice_hand_cases(native, case):
    _name, seq, variants = case
    _check_splice(seq, variants)


def test_splice_random_cases(native):
    rng = np.random.RandomState(20240)
    kinds = set()
    for _ in range(300):
        seq, variants = VC.random_case(rng)
        t = _check_splice(seq, variants)
        kinds.update(k for k, v in t.counts().items() if v)
    assert kinds == {"snv", "mnv", "insertion", "deletion", "bases_inserted", "bases_deleted"}


def test_host_apply_refuses_bad_tables(native):
    seq = "ACGTACGTAC"
    t = VC.table_of(seq, [(2, "G", "T"), (5, "CG", "")])
    t.pos0[1] = 9  # the deletion now reaches past the end
    with pytest.raises(native.EngineError):
        t.apply_native(seq)
    t = VC.table_of(seq, [(2, "G", "T"), (5, "CG", "")])
    t.out_pos[1] += 1
    with pytest.raises(native.EngineError):
        t.apply_native(seq)
    t = VC.table_of(seq, [(2, "G", "TT")])
    t.alt_off[0] = 1
    with pytest.raises(native.EngineError):
        t.apply_native(seq)


# ---------------------------------------------------------------------- 3. the lift
def _leading_deleted(t):
    """Letters deleted in front of the first kept one: lift(0) is the first letter the haplotype kept (0 unless the record's
    first letters are deleted outright -- `last variant with out_pos <= 0, behind its ALT run` then says pos0 + ref_len)."""
    at = 0
    for p, r, a in zip(t.pos0.tolist(), t.ref_len.tolist(), t.alt_len.tolist()):
        if p != at or a:
            break
        at = p + r
    return at


def _check_lift(t, L, rng):
    h = np.arange(int(t.out_pos[-1]) + 1, dtype=np.int64)
    got = t.lift_host(h)
    assert np.array_equal(t.lift_native(h), got)
    assert np.all(np.diff(got) >= 0)
    assert got[0] == _leading_deleted(t) and got[-1] == L
    for i in range(len(t)):  # every letter of an ALT run beyond the replaced ones maps to the end of what it replaced
        op, a, r, p = int(t.out_pos[i]), int(t.alt_len[i]), int(t.ref_len[i]), int(t.pos0[i])
        assert got[op:op + a].tolist() == [p + min(k, r) for k in range(a)]
    probe = VC.lift_probe(t, rng, 50)
    assert np.array_equal(t.lift_native(probe), t.lift_host(probe))


def test_lift_hand_and_random_cases(native):
    rng = np.random.RandomState(5)
    for _name, seq, variants in VC.hand_cases():
        _check_lift(VC.table_of(seq, variants), len(seq), rng)
    for _ in range(100):
        seq, variants = VC.random_case(rng)
        _check_lift(VC.table_of(seq, variants), len(seq), rng)


def test_lift_of_zero_is_zero_unless_the_start_is_deleted(native):
    s = "ACGTACGT"
    for variants in ([], [(0, "A", "T")], [(0, "", "GG")], [(0, "", "GG"), (0, "AC", "T")], [(3, "T", "")]):
        t = VC.table_of(s, variants)
        assert t.lift_host([0])[0] == 0 and t.lift_native([0])[0] == 0
    t = VC.table_of(s, [(0, "AC", "")])
    assert t.lift_host([0])[0] == 2 and t.lift_native([0])[0] == 2


def test_an_insertion_maps_to_its_point(native):
    t = VC.table_of("ACGTACGT", [(4, "", "TTTT")])
    assert t.lift_host(np.arange(13)).tolist() == [0, 1, 2, 3, 4, 4, 4, 4, 4, 5, 6, 7, 8]
    assert t.lift_native(np.arange(13)).tolist() == [0, 1, 2, 3, 4, 4, 4, 4, 4, 5, 6, 7, 8]


def test_lift_past_32_bits(native):
    """Tables alone (the lift reads no letters): pos0 and out_pos beyond 2^32, differences that need 64 bits."""
    base = (1 << 32) + 12345
    n = 1000
    rng = np.random.RandomState(9)
    gaps = rng.randint(1, 1 << 23, n).astype(np.int64)
    ref_len = rng.randint(0, 50, n).astype(np.int32)
    alt_len = np.where(ref_len == 0, rng.randint(1, 50, n), rng.randint(0, 50, n)).astype(np.int32)
    pos0 = base + np.cumsum(gaps + np.concatenate(([0], ref_len[:-1])))
    L = int(pos0[-1] + ref_len[-1] + 777)
    t = V.VariantTable(pos0, ref_len, alt_len, [b"A" * int(a) for a in alt_len], [b"C" * int(r) for r in ref_len], L)
    assert t.out_pos[0] > 1 << 32 and t.pos0.max() < 1 << 34
    probe = VC.lift_probe(t, rng, 5000)
    want = t.lift_host(probe)
    assert np.array_equal(t.lift_native(probe), want)
    order = np.argsort(probe, kind="stable")
    assert np.all(np.diff(want[order]) >= 0)
    assert t.lift_native([0, int(t.out_pos[-1]), base])[:].tolist() == [0, L, base]
    # the formula, spelled out for one variant in the middle
    i = n // 2
    h = int(t.out_pos[i]) + int(alt_len[i]) + 5
    assert int(t.lift_native([h])[0]) == int(pos0[i]) + int(ref_len[i]) + 5


# ---------------------------------------------------------------------- 4. the chain
def test_chain_blocks_and_positions(native):
    rng = np.random.RandomState(11)
    cases = [(s, v) for _n, s, v in VC.hand_cases()] + [VC.random_case(rng) for _ in range(40)]
    for k, (seq, variants) in enumerate(cases):
        t = VC.table_of(seq, variants)
        L, Lh = len(seq), int(t.out_pos[-1])
        buf = io.StringIO()
        V.write_chain(buf, "rec%d" % k, L, t)
        text = buf.getvalue()
        head = text.split("\n")[0].split()
        assert head[0] == "chain" and head[2] == head[7] == "rec%d" % k
        assert [int(head[i]) for i in (3, 5, 6, 8, 10, 11)] == [Lh, 0, Lh, L, 0, L] and head[4] == head[9] == "+"
        chains = V.read_chain(io.StringIO(text))
        t_size, q_size, blocks = chains["rec%d" % k]
        assert (t_size, q_size) == (Lh, L) and len(blocks) == len(t) + 1
        assert sum(b[0] for b in blocks) + sum(b[1] for b in blocks[:-1]) == Lh
        assert sum(b[0] for b in blocks) + sum(b[2] for b in blocks[:-1]) == L
        h = np.arange(Lh + 1, dtype=np.int64)
        assert np.array_equal(V.lift_chain(chains["rec%d" % k], h), t.lift_host(h))


# ---------------------------------------------------------------------- 5. the exports
def test_new_entries_are_declared_and_exported(native):
    header = open(os.path.join(ROOT, "include", "iss_mi355x.h")).read()
    declared = set(re.findall(r"\b(iss_[a-z0-9_]+)\s*\(", header))
    lib = native.lib()
    for name in NEW_ENTRIES:
        assert name in native.EXPORTS and name in declared and hasattr(lib, name), name
    assert lib.iss_abi_version() == 8
    assert re.search(r"#define ISS_ABI_VERSION 8\b", header)
    tile = lib.iss_variants_apply_tile()
    assert tile > 0 and tile % 16 == 0
