"""The texts the device's gzip members are held to the twin on (tests/deflate_twin.py): the table of cases shared by
tests/test_deflate_twin_host.py, which asserts every case's shape without a GPU, and tests/test_gpu_deflate_streams.py, and the
few lines that make a case's text from the oracle's arrays."""
import functools

import numpy as np

from deflate_twin import BLOCK, as_bytes

# ------------------------------------------------------------------ the cases
CPU = 2  # (helpers.ROW_SWEEP_CPU)
ROWS = {2: 64, 5: 200, 8: 200, 151: 700}  # rows generated per read length


def digits_before(x):
    """Decimal digits of 0, 1, ... x - 1 written out (the closed form of iss::digits_before)."""
    n, p = x, 10
    while p < x:
        n += x - p
        p *= 10
    return n


def text_bytes(items, RL, cpu=CPU):
    return sum(n * (len(as_bytes(rid)) + len(str(cpu)) + 2 * RL + 10) + digits_before(first_i + n) - digits_before(first_i)
               for rid, first_i, _, n in items)


@functools.lru_cache(maxsize=None)
def sized_item(RL, target, max_pairs, letter):
    """One item (id of one letter repeated, first pair number, row 0, pairs) whose text has exactly `target` bytes: the first
    (pairs, id length) counted down from max_pairs / up from 1 for which a first pair number fits, found by bisection
    (the digits of n consecutive numbers grow with the first one)."""
    for n in range(max_pairs, max_pairs // 2, -1):
        for idlen in range(1, 301):
            need = target - n * (idlen + len(str(CPU)) + 2 * RL + 10)
            if need < n:
                break
            if need > 5 * n:
                continue
            lo, hi = 0, 100000
            while lo < hi:
                mid = (lo + hi) // 2
                if digits_before(mid + n) - digits_before(mid) < need:
                    lo = mid + 1
                else:
                    hi = mid
            if digits_before(lo + n) - digits_before(lo) == need:
                return (letter * idlen, lo, 0, n)
    raise AssertionError("no item of %d bytes at read length %d" % (target, RL))


DEEP_COUNTS = (1, 1, 2, 3, 5, 6, 13, 21, 42, 55, 62, 144, 233, 377, 610, 25)
DEEP_LETTERS = b"EFIJLOPQUXZefijl"  # (none of them a base, an IUPAC letter, a phred or a digit of the text)


def deep_id():
    """An id of 16 distinct byte values whose counts grow like the Fibonacci numbers up to 610 (1600 bytes), laid out so that no
    byte repeats its predecessor (the frequent half on the even places): literals of the member's first record only -- every
    later record finds them `dist` earlier, so against the bases, phreds and digits of the whole member they are rare.  Where the
    counts leave the Fibonacci numbers they were searched on the CPU, with the text of the case, for what
    test_deflate_twin_host.py::test_deep_code asserts: the tree of the text's counts AND the tree of the builder's counts are
    deeper than 15, and a step of the Kraft repair chooses among tied symbols of which the lowest is not on the lowest lane."""
    pool = b"".join(bytes([c]) * k for k, c in sorted(zip(DEEP_COUNTS, DEEP_LETTERS), reverse=True))
    out, half = bytearray(len(pool)), (len(pool) + 1) // 2
    out[0::2], out[1::2] = pool[:half], pool[half:]
    return bytes(out)


def random_ids(n, seed):
    """n ids of 200 .. 4096 bytes (both ends among them) drawn from every byte value 1 .. 255 but the line feed."""
    rng = np.random.RandomState(seed)
    alphabet = np.array([b for b in range(1, 256) if b != 10], dtype=np.uint8)
    sizes = [200, 4096] + rng.randint(200, 4097, size=n - 2).tolist()
    return [alphabet[rng.randint(0, len(alphabet), size=k)].tobytes() for k in sizes]


def cases():
    """name -> (read length, emit calls: a list of items (record id, first pair number, first row, pairs) each, modes)."""
    k = 2
    many = random_ids(32, 77)
    return {
        "one_record": (2, [[("g", 0, 3, 1)]], ("matches",)),
        "short_records_5": (5, [[("g", 4, 0, 200)]], ("matches", "runs only")),
        "short_records_8": (8, [[("g", 4, 0, 200)]], ("matches", "runs only")),
        "block_multiple": (151, [[sized_item(151, k * BLOCK, 200, "m")]], ("matches",)),
        "block_plus_sliver": (151, [[sized_item(151, k * BLOCK + 5, 210, "p")]], ("matches",)),
        "block_minus_sliver": (151, [[sized_item(151, k * BLOCK - 7, 190, "s")]], ("matches",)),
        "shipped_shape": (151, [[("NZ_CP012345.1_Esche_K", 600, 0, 700)]], ("matches",)),
        "deep_code": (151, [[(deep_id(), 1000, 0, 150)]], ("matches",)),
        "run_at_block_edge": (151, [[("e" * 16, 0, 0, 300)]], ("matches",)),
        "many_symbols": (2, [[(rid, 7 * j, j, 1) for j, rid in enumerate(many)]], ("matches",)),
        "most_pairs_not_first": (8, [[("g", 0, 0, 20), ("NZ_kkkkkkkk.1", 95, 20, 150), ("abcdefg", 0, 170, 30)]], ("matches",)),
        "slot_reuse": (151, [[("first", 0, 0, 300)], [("second_of_four", 998, 300, 3)], [("third", 50, 303, 150)],
                             [("4", 0, 453, 40)]], ("matches",)),
    }


def oracle_rows(RL):
    """The oracle's arrays for the case rows at read length RL (helpers.row_sweep_model over a lower-case / IUPAC record)."""
    import helpers as H
    from oracle import oracle as O

    rng = O.Rng().seed_philox(H.ROW_SWEEP_SEED)
    return H.row_sweep_oracle_rows(H.row_sweep_model(RL), rng, H.row_sweep_genome(RL), ROWS[RL], H.ROW_SWEEP_FIRST_ORDINAL)


def call_text(items, exp, mate):
    """The FASTQ text of one emit call (mate 1 or 2) from the oracle's arrays."""
    import helpers as H

    return b"".join(H.fastq_text(rid, first_i, CPU, mate, exp["bases"][row:row + n, mate - 1], exp["qual"][row:row + n, mate - 1])
                    for rid, first_i, row, n in items)
