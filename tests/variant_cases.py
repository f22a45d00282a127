"""Cases of `generate --variants` shared by tests/test_variants_host.py and tests/test_gpu_variants.py: hand-written splices,
seeded random ones, and the naive list splice every implementation is compared with."""
import numpy as np

from insilicoseq_amd.variants import VariantTable

LETTERS = "ACGT" * 6 + "acgt" * 2 + "NRYWSMKHBVD" + "nrykm"


def naive_splice(seq, variants):
    """The definition: the variants (pos0, ref letters, alt letters) put into a Python list from the right to the left."""
    out = list(seq)
    for pos0, ref, alt in sorted(variants, key=lambda v: (v[0], len(v[1])), reverse=True):
        assert "".join(out[pos0:pos0 + len(ref)]).upper() == ref.upper(), (pos0, ref)
        out[pos0:pos0 + len(ref)] = list(alt)
    return "".join(out)


def table_of(seq, variants):
    return VariantTable.from_variants([(p, r.encode(), a.encode()) for p, r, a in variants], len(seq))


def hand_cases():
    """(name, record, [(pos0, ref, alt)])"""
    s = "ACGTTGCAAGGCTTAC"
    every_other = [(i, s[i], "ACGT"[("ACGT".index(s[i]) + 1) % 4]) for i in range(0, len(s), 2)]
    return [
        ("variant_at_pos_1", s, [(0, "A", "T")]),
        ("deletion_of_the_last_base", s, [(len(s) - 1, "C", "")]),
        ("insertion_after_the_last_base", s, [(len(s), "", "GGA")]),
        ("deletion_then_insertion", s, [(2, "GT", ""), (4, "", "CCC")]),
        ("insertion_at_the_start_of_a_substitution", s, [(5, "", "AA"), (5, "GC", "TT")]),
        ("every_other_base", s, every_other),
        ("empty_table", s, []),
        ("length_1_snv", "g", [(0, "G", "t")]),
        ("length_1_insertions", "A", [(0, "", "CC"), (1, "", "T")]),
        ("length_1_empty", "N", []),
        ("deletion_at_the_start", s, [(0, "ACG", "")]),
        ("adjacent_deletions", s, [(3, "T", ""), (4, "T", ""), (5, "GC", "")]),
        ("lower_case_record", s.lower(), [(1, "C", "G"), (6, "CAA", "c")]),
    ]


def random_case(rng, max_len=300, min_len=1, letters=LETTERS, rate=0.15):
    """(record, [(pos0, ref, alt)]) with L' >= 1: substitutions, insertions and deletions of 1 .. 6 letters, some adjacent."""
    L = int(rng.randint(min_len, max_len + 1))
    seq = "".join(letters[i] for i in rng.randint(0, len(letters), L))
    variants, p, last_ins = [], 0, -1
    rate = rate * rng.random_sample()
    while p <= L:
        if rng.random_sample() >= rate:
            p += 1
            continue
        kind = rng.randint(0, 4)
        alt = "".join("ACGTacgtNn"[i] for i in rng.randint(0, 10, int(rng.randint(1, 7))))
        n = int(min(rng.randint(1, 7), L - p))
        if kind == 0 and last_ins != p:  # insertion (also behind the last letter)
            variants.append((p, "", alt))
            last_ins = p
            p += int(rng.randint(0, 2))
        elif kind == 1 and n:  # deletion
            variants.append((p, seq[p:p + n].upper(), ""))
            p += n
        elif kind == 2 and n:  # substitution of n letters by as many
            variants.append((p, seq[p:p + n], alt[:n].ljust(n, "A")))
            p += n
        elif n:  # n letters replaced by another number
            variants.append((p, seq[p:p + n].swapcase(), alt))
            p += n
        else:
            p += 1
    if L + sum(len(a) - len(r) for _p, r, a in variants) < 1:  # (everything deleted: keep the record as it is)
        variants = []
    return seq, variants


def lift_probe(table, rng=None, n_random=0):
    """Coordinates worth lifting: every out_pos[i] - 1, out_pos[i], out_pos[i] + alt_len[i], 0 and L', and random ones."""
    Lh = int(table.out_pos[-1])
    op = table.out_pos[:-1]
    pts = np.concatenate((op - 1, op, op + table.alt_len, [0, Lh]))
    if n_random:
        pts = np.concatenate((pts, rng.randint(0, Lh + 1, n_random)))
    return np.clip(pts, 0, Lh).astype(np.int64)
