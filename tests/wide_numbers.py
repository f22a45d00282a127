"""Pair ids and coordinates that need more than 32 bits: the plain references and the cases of test_wide_numbers_host.py and
test_gpu_wide_numbers.py.

The references format Python integers with "%d" and call nothing of the library.  uBAM records come from tests/ubam_twin.py and
BEDPE lines from insilicoseq_amd.origins.lines_host, which both run on Python integers already."""
import numpy as np

U64 = 1 << 64


def chars_before(x):
    """Characters of the decimal numbers 0 .. x - 1 written one after the other, exact (what iss::digits_before counts mod 2^64)."""
    if x <= 0:
        return 0
    d = len(str(x))
    return 1 + sum(k * 9 * 10 ** (k - 1) for k in range(1, d)) + d * (x - 10 ** (d - 1))  # ("0" is the 1)


def first_id_past_2_64_chars():
    """x*: the smallest x whose chars_before(x) reaches 2^64 -- there the count itself wraps in 64-bit arithmetic."""
    base = 10 ** 18  # every number from here to 10^19 - 1 has 19 digits
    x = base + -((chars_before(base) - U64) // 19)
    assert chars_before(x) >= U64 > chars_before(x - 1)
    return x


X_STAR = first_id_past_2_64_chars()
assert 1.02e18 < X_STAR < 1.04e18, X_STAR

# (first pair id, pairs): a boundary lies inside every item
WIDE_ITEMS = [
    (999_999_990, 25),            # 9 | 10 digits, still 32-bit
    (2 ** 31 - 5, 12),            # the sign bit of a 32-bit id
    (2 ** 32 - 7, 20),            # 32 | 33 bits with ten digits on both sides
    (10 ** 10 - 9, 20),           # 10 | 11 digits: the first width only a 64-bit writer can give
    (10 ** 15 - 3, 8),            # 15 | 16 digits
    (10 ** 18 - 6, 15),           # 18 | 19 digits
    (X_STAR - 8, 16),             # the character count of all smaller ids passes 2^64
    (2 ** 63 - 1 - 40, 40),       # first_i + n == 2^63 - 1: the largest id an int64 entry takes
]
WIDE_ROWS = sum(n for _, n in WIDE_ITEMS)
WIDE_CPUS = (0, 7, 2147483647)    # one digit, and the ten characters an item's cpu[12] has to hold
WIDE_IDS = ("g", "NZ_" + "k" * 194 + ".12")
assert [len(r) for r in WIDE_IDS] == [1, 200]
assert all(a <= X_STAR - 1 < a + n for a, n in WIDE_ITEMS[6:7]) and all(a + n <= 2 ** 63 - 1 for a, n in WIDE_ITEMS)


def wide_items(rid_of=lambda k: WIDE_IDS[k % 2], row0=0):
    """WIDE_ITEMS as the tuples of ReadEngine.fastq_emit_batch -- (record id, first pair id, first output row, pairs) -- on
    consecutive rows from ``row0``, the record ids alternating between one and 200 characters."""
    out, row = [], row0
    for k, (first_i, n) in enumerate(WIDE_ITEMS):
        out.append((rid_of(k), first_i, row, n))
        row += n
    return out


def _b(s):
    return s if isinstance(s, bytes) else str(s).encode()


def fastq_text(rid, first_i, cpu, bases, quals, mate):
    """FASTQ text of one mate (1 or 2): row k of ``bases`` / ``quals`` (uint8 [n, RL] letters and phreds) is pair first_i + k."""
    rid = _b(rid)
    return b"".join(b"@%s_%d_%d/%d\n%s\n+\n%s\n" % (rid, first_i + k, cpu, mate, bases[k].tobytes(), (quals[k].astype(np.uint8) + 33).tobytes())
                    for k in range(len(bases)))


def fastq_items_text(items, cpu, bases, quals, mate):
    """The text of emit-batch items over the rows of one mate, item after item."""
    return b"".join(fastq_text(rid, first_i, cpu, bases[row:row + n], quals[row:row + n], mate) for rid, first_i, row, n in items)


def vcf_lines(rid, first_i, cpu, mutations, pair0=0, n_pairs=None):
    """The --store_mutations lines of mutation rows (pair, mate, type, position, ref, alt, quality) whose pair lies in
    [pair0, pair0 + n_pairs): pair p is named first_i + (p - pair0); an insertion's alt is ref + the inserted letter, only a
    substitution carries its phred."""
    rid = _b(rid).decode()
    lines = []
    for m in mutations:
        p = int(m["pair"]) - pair0
        if p < 0 or (n_pairs is not None and p >= n_pairs):
            continue
        ref, alt = chr(m["ref"]), chr(m["alt"])
        alt = ref + alt if m["type"] == 1 else alt
        qual = "%d" % int(m["quality"]) if m["type"] == 0 else "."
        lines.append("%s_%d_%d/%d\t%d\t.\t%s\t%s\t%s\t\t\n" % (rid, first_i + p, cpu, 1 + int(m["mate"]), int(m["position"]) + 1, ref, alt, qual))
    return lines


def vcf_items_text(items, cpu, mutations, row0=0):
    """The text of emit items (record id, first pair id, first output row, pairs) over the rows of a call whose pair 0 is output
    row ``row0``: the rows stand in pair order, so the items' lines follow each other."""
    return "".join("".join(vcf_lines(rid, first_i, cpu, mutations, row - row0, n)) for rid, first_i, row, n in items).encode()


def ubam_records(items, cpu, r1_base, r1_qual, r2_base, r2_qual):
    import ubam_twin

    return ubam_twin.records(items, cpu, r1_base, r1_qual, r2_base, r2_qual)


def bedpe_text(items, record_lengths, cpu, coords, read_length):
    from insilicoseq_amd.origins import lines_host

    return lines_host(items, record_lengths, cpu, coords, read_length)


def synthetic_rows(n, RL, seed):
    """n rows of letters (upper and lower case, IUPAC) and phreds: [r1_base, r1_qual, r2_base, r2_qual], uint8 [n, RL]."""
    rng = np.random.RandomState(seed)
    alphabet = np.frombuffer(b"ACGTACGTACGTacgtNRYKMnry", dtype=np.uint8)
    return [alphabet[rng.randint(0, len(alphabet), size=(n, RL))] if k % 2 == 0 else rng.randint(0, 42, size=(n, RL)).astype(np.uint8)
            for k in range(4)]


def prime_period_record(length, period=67_108_859, seed=5):
    """The `mixed` record of test_records_of_2_31_bases_and_more: a prime-period tile of helpers.mixed_genome (IUPAC and lower-case
    stretches), so that a coordinate off by a power of two reads other letters.  uint8 [length]."""
    from helpers import mixed_genome

    block = np.frombuffer(mixed_genome(seed, period).encode(), dtype=np.uint8)
    return np.ascontiguousarray(np.tile(block, length // period + 1)[:length])
