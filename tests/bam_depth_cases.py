"""Record sets of the `report --bam --depth` tests (test_bam_depth_host.py, test_gpu_bam_depth.py): a header and a record builder
for several references (bam_synth.header_bytes knows one), the hand-made case table, and what the records must give worked out
base by base from the dicts -- not from the bytes, and with nothing of insilicoseq_amd.bam_depth."""
import struct

import numpy as np

import bam_synth
from insilicoseq_amd.bam import Chunk

M, I, D, N, S, H, P, EQ, X = range(9)
REFS = [("ref50", 50), ("ref1", 1), ("ref300", 300), ("skipped", 40)]  # row 3 is the skipped row of the tests that have one
SKIPPED_ROW = 3
R1F, R2R = 0x41, 0x91


def header_bytes(refs):
    text = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (name.encode(), ln) for name, ln in refs)
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, ln in refs:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    return out


def rec(name, ref, pos, cigar, flag=R1F, mapq=60):
    """A record dict: ``cigar`` [(op, len)]; SEQ and QUAL take the length the query-consuming ops add up to (at most 1 024)."""
    return dict(name=name, ref=ref, pos=pos, cigar=list(cigar), flag=flag, mapq=mapq)


def encode(r):
    l_seq = sum(ln for op, ln in r["cigar"] if op in (M, I, S, EQ, X))
    assert l_seq <= 1024, r["name"]
    name = r["name"].encode() + b"\0"
    cig = b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in r["cigar"])
    seq = bytes(0x12 if k % 2 else 0x48 for k in range((l_seq + 1) // 2))
    qual = bytes((7 * k + 3) % 41 for k in range(l_seq))
    body = struct.pack("<iiBBHHHiiii", r["ref"], r["pos"], len(name), r["mapq"], 4680, len(r["cigar"]), r["flag"], l_seq, -1, -1, 0)
    body += name + cig + seq + qual
    return struct.pack("<i", len(body)) + body


def chunk_of(records):
    blobs = [encode(r) for r in records]
    offs = np.cumsum([0] + [len(b) for b in blobs[:-1]], dtype=np.int64) if blobs else np.zeros(0, dtype=np.int64)
    return Chunk(np.frombuffer(b"".join(blobs), dtype=np.uint8), offs)


def split(chunk, per):
    o = list(chunk.offsets) + [chunk.data.size]
    out = []
    for k in range(0, len(o) - 1, per):
        hi = min(k + per, len(o) - 1)
        out.append(Chunk(chunk.data[o[k]:o[hi]].copy(), np.asarray(o[k:hi], dtype=np.int64) - o[k]))
    return out


def write_bam(path, refs, records):
    with open(path, "wb") as fh:
        fh.write(bam_synth.bgzf(header_bytes(refs) + b"".join(encode(r) for r in records)))


def alternating(n_ops, other):
    """1M 1<other> 1M ... over n_ops operations."""
    return [(M, 1) if k % 2 == 0 else (other, 1) for k in range(n_ops)]


def valid_cases():
    """The case table: every record is valid on REFS and marks something, or is filtered."""
    t = []
    add = lambda *a, **kw: t.append(rec(*a, **kw))
    add("one_M_at_0", 0, 0, [(M, 10)])
    add("M_to_the_end", 0, 30, [(M, 20)])                       # its -1 lands in the sink
    add("whole_ref50", 0, 0, [(M, 50)], flag=R2R)
    add("ref1_covered", 1, 0, [(M, 1)])
    add("clips_and_pads", 0, 5, [(H, 3), (S, 2), (M, 4), (I, 2), (P, 1), (M, 4), (S, 1), (H, 2)])  # covers [5, 13) in one piece
    add("D_splits", 2, 10, [(M, 5), (D, 3), (M, 5)])            # [10, 15) and [18, 23); with COUNT_DEL [10, 23)
    add("N_splits", 2, 40, [(M, 5), (N, 20), (M, 5)], flag=R2R)  # always two pieces
    add("eq_and_X", 2, 100, [(EQ, 6), (X, 1), (EQ, 3)])
    add("M_then_eq", 2, 120, [(M, 4), (EQ, 4)])
    add("twice_a", 2, 200, [(M, 30)])
    add("twice_b", 2, 210, [(M, 30)], flag=R2R)                 # [210, 230) has depth 2
    add("D_first_and_last", 2, 250, [(D, 2), (M, 3), (D, 2)])
    add("only_N_and_D", 2, 260, [(N, 3), (D, 2)])               # marks nothing without COUNT_DEL, is still `marked`
    add("M_zero_length", 2, 270, [(M, 0), (M, 2), (D, 0)])
    add("ops64_MD", 2, 0, alternating(64, D))
    add("ops65_MN", 2, 100, alternating(65, N), flag=R2R)
    add("ops129_MI", 2, 150, alternating(129, I))                # 65 M in a row on the reference
    add("ops129_MD", 2, 160, alternating(129, D))
    add("ops300_MD", 2, 0, alternating(300, D))                  # spans the whole of ref300
    add("ops300_MX", 0, 0, [(M, 1) if k % 6 == 0 else (X, 0) if k % 2 else (N, 0) for k in range(300)])  # 50 M of 1: ref50 whole
    # filters
    add("f_unmapped", 0, 0, [(M, 10)], flag=R1F | 0x4)
    add("f_secondary", 0, 0, [(M, 10)], flag=R1F | 0x100)
    add("f_supplementary", 0, 0, [(M, 10)], flag=R1F | 0x800)
    add("f_qcfail", 0, 0, [(M, 10)], flag=R1F | 0x200)
    add("f_duplicate", 0, 0, [(M, 10)], flag=R2R | 0x400)
    add("f_both_mates", 0, 0, [(M, 10)], flag=0x1 | 0x40 | 0x80)
    add("f_no_cigar", 0, 0, [])
    add("f_no_ref", -1, 0, [(M, 10)])
    add("f_no_ref_no_pos", -1, -1, [(M, 10)])
    add("f_unmapped_and_dup", 0, 0, [(M, 10)], flag=R1F | 0x4 | 0x400)   # not aligned comes first
    add("f_dup_low_mapq", 0, 0, [(M, 10)], flag=R1F | 0x400, mapq=0)      # filtered comes before mapq
    add("mapq_19", 0, 20, [(M, 10)], mapq=19)
    add("mapq_20", 0, 20, [(M, 10)], mapq=20)
    add("mapq_0", 0, 20, [(M, 10)], mapq=0)
    add("mapq_255", 0, 20, [(M, 10)], mapq=255)
    add("on_row_3", SKIPPED_ROW, 0, [(M, 10)])
    add("on_row_3_past_its_end", SKIPPED_ROW, 35, [(M, 10)])     # valid only where row 3 is skipped: its length is not looked at
    return t


def bad_cases():
    """(record, code): what validation must refuse, with nothing marked."""
    big = (1 << 28) - 1
    return [
        (rec("bad_op9", 0, 0, [(M, 5), (9, 1), (M, 5)]), 1),
        (rec("bad_op15_last", 2, 0, alternating(64, D) + [(15, 1)]), 1),
        (rec("bad_op_and_ref", 4, 0, [(M, 5), (12, 1)]), 1),       # the first code that applies
        (rec("bad_ref_is_n_table", 4, 0, [(M, 5)]), 2),
        (rec("bad_ref_huge", 2 ** 31 - 1, 0, [(M, 5)]), 2),
        (rec("bad_ref_and_pos", 4, -1, [(M, 5)]), 2),
        (rec("bad_pos_minus_1", 0, -1, [(M, 5)]), 3),
        (rec("bad_one_past_the_end", 0, 41, [(M, 10)]), 3),
        (rec("bad_one_past_ref1", 1, 0, [(M, 2)]), 3),
        (rec("bad_pos_is_length", 1, 1, [(M, 1)]), 3),
        (rec("bad_D_past_the_end", 0, 45, [(M, 5), (D, 1)]), 3),
        (rec("bad_N_past_the_end", 0, 45, [(M, 5), (N, 1)]), 3),
        (rec("bad_sum_past_2_32", 2, 0, [(M, 10)] + [(N, big)] * 17 + [(M, 10)]), 3),     # 17 * (2^28 - 1) > 2^32
        (rec("bad_sum_is_2_32_and_5", 2, 0, [(D, big)] * 16 + [(N, 16), (M, 5)]), 3),     # low 32 bits of the sum: 5
        (rec("bad_300_ops_one_past", 2, 1, alternating(300, D)), 3),
    ]


def between_good(bad, k):
    """The bad record at place k of three, good ones around it."""
    good = [rec("good%d_%s" % (j, bad["name"]), 2, 5 + 7 * j, [(M, 8), (D, 1), (M, 8)], (R1F, R2R)[j]) for j in range(2)]
    return good[:k] + [bad] + good[k:]


# ---------------------------------------------------------------------------------------------------- base by base
def taken(flag):
    """The read tally's rule (bam_report.py): neither secondary nor supplementary, and mate flags that name a mate."""
    return not (flag & 0x900 or (flag & 1 and (flag & 0xC0) in (0, 0xC0)))


def expected(records, table, count_del=False, min_mapq=0):
    """(depth per word of the accumulator -- int64, the sinks 0 --, counts [6], first bad (index, code) or (-1, 0)), base by base."""
    table = np.asarray(table, dtype=np.int64).reshape(-1, 2)
    n_words = int(max(off + ln + 1 for off, ln in table.tolist() if off >= 0))
    depth = np.zeros(n_words, dtype=np.int64)
    counts, bad = [0] * 6, (-1, 0)
    for k, r in enumerate(records):
        if not taken(r["flag"]):
            continue
        if r["flag"] & 4 or not r["cigar"] or r["ref"] < 0:
            counts[1] += 1
            continue
        if r["flag"] & 0x600:
            counts[2] += 1
            continue
        if r["mapq"] < min_mapq:
            counts[3] += 1
            continue
        code, bases = 0, []
        if any(op > 8 for op, _ln in r["cigar"]):
            code = 1
        elif r["ref"] >= table.shape[0]:
            code = 2
        else:
            off, length = table[r["ref"]].tolist()
            if off < 0:
                counts[4] += 1
                continue
            at = r["pos"]
            for op, ln in r["cigar"]:
                if op in (M, EQ, X) or (op == D and count_del):
                    if ln > (1 << 20):
                        at = length + 1  # (far past any reference of the tests)
                        break
                    bases.extend(range(at, at + ln))
                if op in (M, D, N, EQ, X):
                    at += ln
            if r["pos"] < 0 or at > length:
                code = 3
        if code:
            if bad[0] < 0:
                bad = (k, code)
            continue
        counts[0] += 1
        counts[5] += len(bases)
        for b in bases:
            depth[off + b] += 1
    return depth, counts, bad
