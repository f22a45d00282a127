"""Record sets of the `report --bam` tests (test_bam_report_host.py, test_gpu_bam_report.py): plain records for bam_synth.encode_record,
the byte patches it has no argument for, and chunks made from them without the library."""
import random
import struct

import numpy as np

import bam_synth
from insilicoseq_amd.bam import Chunk

R1F, R1R, R2F, R2R = 0x41, 0x51, 0x81, 0x91  # paired: first / second read, forward / reverse
LETTERS = bam_synth.SEQ_CODES


def rec(seq, qual=None, flag=R1F, tlen=0, name="r", n_cigar=None, tags=(), **more):
    """A record for encode_record: qual defaults to position-dependent phreds, the CIGAR to one M (none for an empty read)."""
    if qual is None:
        qual = [(11 * i + 5) % 94 for i in range(len(seq))]
    cigar = [(0, len(seq))] if seq else []
    if n_cigar is not None:  # the count matters, not the meaning: SEQ moves by four bytes an operation
        cigar = [(0, 1)] * n_cigar
    return dict(name=name, flag=flag, tlen=tlen, cigar=cigar, seq=seq, qual=None if qual == "none" else list(qual), tags=list(tags), **more)


def encode(r):
    """encode_record and the patches: ``ref`` / ``next_ref`` (refID, next_refID), ``l_read_name``, ``l_seq`` as stored."""
    b = bytearray(bam_synth.encode_record(r))
    for key, at, fmt in (("ref", 4, "<i"), ("next_ref", 24, "<i"), ("l_read_name", 12, "<B"), ("l_seq", 20, "<i")):
        if key in r:
            struct.pack_into(fmt, b, at, r[key])
    return bytes(b)


def chunk_of(records):
    """One Chunk holding the records, offsets by the block_size chain."""
    blobs = [encode(r) for r in records]
    offs = np.cumsum([0] + [len(b) for b in blobs[:-1]], dtype=np.int64) if blobs else np.zeros(0, dtype=np.int64)
    return Chunk(np.frombuffer(b"".join(blobs), dtype=np.uint8), offs)


def split(chunk, per):
    """The chunk's records `per` to a chunk, each with bytes of its own."""
    o = list(chunk.offsets) + [chunk.data.size]
    out = []
    for k in range(0, len(o) - 1, per):
        hi = min(k + per, len(o) - 1)
        out.append(Chunk(chunk.data[o[k]:o[hi]].copy(), np.asarray(o[k:hi], dtype=np.int64) - o[k]))
    return out


def random_seq(rnd, n, letters="ACGT"):
    return "".join(rnd.choice(letters) for _ in range(n))


def mixed(lengths, n, seed, max_q=93):
    """n records over the lengths in turn, every length on both strands and both mates in turn, all sixteen letters."""
    rnd = random.Random(seed)
    out = []
    for k in range(n):
        l = lengths[k % len(lengths)]
        flag = (R1F, R2R, R1R, R2F)[(k // len(lengths)) % 4]
        seq = random_seq(rnd, l, "ACGT" * 6 + LETTERS)
        qual = [rnd.randint(0, max_q) for _ in range(l)]
        out.append(rec(seq, qual, flag, tlen=rnd.choice((0, 300, -450, 2 * l + 17, 5000)), name="m%d" % k))
    return out


def insert_cases(l=10):
    """(record, expected bin or None) for every insert rule, reads of l bases."""
    seq = "ACGTACGTAC"[:l]
    big = 2 * l
    cases = [(rec(seq, tlen=t), b) for t, b in (
        (0, None), (1, 0), (-1, 0), (big, 0), (-big, 0), (big + 1, 1), (big + 2046, 2046), (-(big + 2046), 2046), (big + 2047, 2047),
        (-(big + 2047), 2047), (big + 5000, 2047), (-(big + 5000), 2047), (-2 ** 31, 2047), (2 ** 31 - 1, 2047), (300, 300 - big))]
    cases += [
        (rec(seq, tlen=300, flag=R2F), None),                 # mate 1 does not count: once a pair
        (rec(seq, tlen=300, flag=0x40), None),                # not paired
        (rec(seq, tlen=300, flag=0), None),
        (rec(seq, tlen=300, flag=R1F | 4), None),             # unmapped
        (rec(seq, tlen=300, flag=R1F | 8), None),             # mate unmapped
        (rec(seq, tlen=-300, flag=R1R), 300 - big),           # the strand does not matter
        (rec(seq, tlen=300, flag=R1F | 2), 300 - big),        # nor proper-pair
        (rec(seq, tlen=300, next_ref=1), None),               # different references
        (rec(seq, tlen=300, ref=3, next_ref=3), 300 - big),
        (rec(seq, tlen=300, next_ref=-1), None),
        (rec(seq, tlen=300, ref=-1, next_ref=-1), None),      # equal but unplaced
        (rec(seq, tlen=300, flag=R1F | 0x100), None),         # skipped records count nowhere
        (rec(seq, tlen=300, flag=0xC1), None),
        (rec("", tlen=7, qual=[]), 7),                        # a read of length 0 has a template all the same
    ]
    return cases
