"""FASTQ text for the tests of `report` (insilicoseq_amd.fastq_report): seeded records with every letter and quality the tallies tell
apart, and the six records whose tally test_fastq_report_host.py works out by hand."""
import numpy as np

LETTERS = np.frombuffer(b"ACGTacgtNnRYKMSWBDHVrykmswbdhv", dtype=np.uint8)
LENGTHS = (0, 1, 63, 64, 65, 151, 301, 1024)


def records(lengths, seed, names=None):
    """One (name, bases, quals) per length: bases over both cases, N and IUPAC letters; qualities over '!' .. '~', every third
    quality line starting with '@', every third with '+', '!' and '~' in every read that has room."""
    rng = np.random.RandomState(seed)
    out = []
    for k, n in enumerate(lengths):
        bases = LETTERS[rng.randint(0, LETTERS.size, n)].copy()
        quals = rng.randint(33, 127, n).astype(np.uint8)
        if n > 0 and k % 3 != 2:
            quals[0] = ord("@") if k % 3 == 0 else ord("+")
        if n > 2:
            quals[1], quals[-1] = 33, 126
        name = names[k] if names else b"read_%d_%d/1" % (seed, k)
        out.append((name, bases.tobytes(), quals.tobytes()))
    return out


def text(recs, eol=b"\n"):
    return b"".join(b"@" + name + eol + bases + eol + b"+" + eol + quals + eol for name, bases, quals in recs)


def mixed(n_records, seed, lengths=LENGTHS, eol=b"\n"):
    """n_records records, the lengths drawn from `lengths` (each at least once when there is room)."""
    rng = np.random.RandomState(seed + 1000)
    ls = list(lengths)[:n_records] + [int(x) for x in rng.choice(lengths, max(0, n_records - len(lengths)))]
    rng.shuffle(ls)
    return text(records(ls, seed), eol)


def sized(n_bytes, seed, read_length=100):
    """Exactly n_bytes of whole records: the last record's name is padded to fit."""
    recs = records([read_length] * (n_bytes // (2 * read_length + 8) + 2), seed)
    body, k = b"", 0
    while len(body) + len(text(recs[k:k + 1])) + len(text([(b"x",) + recs[k + 1][1:]])) <= n_bytes:
        body += text(recs[k:k + 1])
        k += 1
    name, bases, quals = recs[k]
    out = body + text([(b"x" * (n_bytes - len(body) - len(text([(b"", bases, quals)]))), bases, quals)])
    assert len(out) == n_bytes
    return out


# Six records, worked out by hand in test_fastq_report_host.py: CRLF on record 1, a quality line starting with '@' (record 0) and
# one starting with '+' (record 2), an empty read (record 3), a bad record (4: lengths differ), lower case and N (record 5).
SIX = (b"@r0\nACGT\n+\n@III\n"
       b"@r1\r\nGGCC\r\n+r1\r\n!!!~\r\n"
       b"@r2\nAC\n+\n+5\n"
       b"@r3\n\n+\n\n"
       b"@r4\nACGT\n+\nIII\n"
       b"@r5\nacgNn\n+\n5555~\n")
