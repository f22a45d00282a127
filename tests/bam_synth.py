"""Deterministic synthetic BAM files for the `model` tests (SAM/BAM specification v1, sections 4.1-4.2).

``write_bam(path, seed, ...)`` writes real BGZF (gzip members with the BC extra field, at most 65280 payload bytes per
block, the 28-byte EOF block) holding paired records with CIGAR, MD, flags, template lengths and qualities drawn from
``random.Random(seed)``: the same seed gives the same bytes.  The records exercise what the reference's `iss model`
(iss/bam.py:118-170, iss/modeller.py) does with them: soft and hard clips, insertions and deletions (long early deletions
move dispatch_indels' position below zero), N bases and N reference letters, unmapped / secondary / supplementary
records, records flagged neither read1 nor read2, unpaired records, reversed reads and mean qualities in every bin
(and at 40 and above, which lands in no bin).  ``records(...)`` returns the same records as dicts without writing them.
"""
import hashlib
import random
import struct
import zlib

SEQ_CODES = "=ACMGRSVTWYHKDBN"
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_block(payload, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = co.compress(payload) + co.flush()
    bsize = 18 + len(body) + 8
    head = struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, bsize - 1)
    return head + body + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload))


def bgzf(data, level=6, block=65280):
    return b"".join(bgzf_block(data[i:i + block], level) for i in range(0, len(data), block)) + BGZF_EOF


def header_bytes(ref_name="chr1", ref_len=1000000):
    text = b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:%s\tLN:%d\n" % (ref_name.encode(), ref_len)
    name = ref_name.encode() + b"\0"
    return b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<ii", 1, len(name)) + name + struct.pack("<i", ref_len)


def encode_record(r):
    """One alignment record (block_size included) from a dict with name, flag, pos, tlen, cigar [(op, len)], seq (str),
    qual (list of int or None for 0xFF), tags [(tag, type, value)]."""
    name = r["name"].encode() + b"\0"
    seq, qual = r["seq"], r["qual"]
    l_seq = len(seq)
    codes = [SEQ_CODES.index(c) for c in seq]
    packed = bytes(((codes[i] << 4) | (codes[i + 1] if i + 1 < l_seq else 0)) for i in range(0, l_seq, 2))
    qb = bytes([0xFF] * l_seq) if qual is None else bytes(qual)
    cig = b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in r["cigar"])
    aux = b""
    for tag, typ, val in r.get("tags", ()):
        if typ == "Z":
            aux += tag.encode() + b"Z" + val.encode() + b"\0"
        elif typ == "i":
            aux += tag.encode() + b"i" + struct.pack("<i", val)
        elif typ == "C":
            aux += tag.encode() + b"C" + struct.pack("<B", val)
        elif typ == "B":
            aux += tag.encode() + b"BC" + struct.pack("<i", len(val)) + bytes(val)
    ref_id = -1 if r.get("unplaced") else 0
    body = struct.pack("<iiBBHHHiiii", ref_id, r.get("pos", 0), len(name), 60, 4680, len(r["cigar"]), r["flag"], l_seq,
                       ref_id, r.get("mpos", 0), r.get("tlen", 0))
    body += name + cig + packed + qb + aux
    return struct.pack("<i", len(body)) + body


def _md(ref_cols, cigar):
    """MD string from the reference letters of the aligned columns (None = match) and the deleted letters of each D."""
    out, run, col = [], 0, 0
    for op, ln, dl in cigar:
        if op == 0:
            for _ in range(ln):
                if ref_cols[col] is None:
                    run += 1
                else:
                    out.append(str(run))
                    out.append(ref_cols[col])
                    run = 0
                col += 1
        elif op == 2:
            out.append(str(run))
            out.append("^" + dl)
            run = 0
    out.append(str(run))
    return "".join(out)


def _indel_positions_ok(cigar, l_seq):
    """True when dispatch_indels (iss/modeller.py:262-315) stays inside query_sequence / query_alignment_sequence."""
    lo = cigar[0][1] if cigar and cigar[0][0] == 4 else 0
    if cigar and cigar[0][0] == 5 and len(cigar) > 1 and cigar[1][0] == 4:
        lo = cigar[1][1]
    hi = cigar[-1][1] if len(cigar) > 1 and cigar[-1][0] == 4 else 0
    if len(cigar) > 1 and cigar[-1][0] == 5 and cigar[-2][0] == 4:
        hi = cigar[-2][1]
    la = l_seq - lo - hi
    pos = 0
    for op, ln in cigar:
        if op == 0:
            pos += ln
        elif op == 1:
            if not -l_seq <= pos < l_seq:
                return False
            pos += ln
        elif op == 2:
            if not -la <= pos < la:
                return False
            pos -= ln
    return True


def _random_read(rnd, length, p_indel, p_sub, p_n, long_del):
    """CIGAR (with deleted letters), query sequence and MD for one read of `length` query bases."""
    while True:
        ops = []
        left = length
        if rnd.random() < 0.15:
            s = rnd.randint(1, min(12, length // 4))
            ops.append([4, s, ""])
            left -= s
        right = 0
        if rnd.random() < 0.15:
            right = rnd.randint(1, min(12, length // 4))
            left -= right
        if long_del:  # a long deletion early in the read: the next event's position goes negative
            m = rnd.randint(2, 6)
            ops.append([0, m, ""])
            dl = rnd.randint(m + 1, m + 20)
            ops.append([2, dl, "".join(rnd.choice("ACGTN") for _ in range(dl))])
            i = rnd.randint(1, 3)
            ops.append([1, i, ""])
            left -= m + i
        while left > 0:
            r = rnd.random()
            if r < p_indel and ops and ops[-1][0] == 0:
                if rnd.random() < 0.5 and left > 1:
                    i = rnd.randint(1, min(4, left - 1))
                    ops.append([1, i, ""])
                    left -= i
                else:
                    dl = rnd.randint(1, 4)
                    ops.append([2, dl, "".join(rnd.choice("ACGT") for _ in range(dl))])
                continue
            m = min(left, rnd.randint(5, 60))
            if ops and ops[-1][0] == 0:
                ops[-1][1] += m
            else:
                ops.append([0, m, ""])
            left -= m
        if ops[-1][0] != 0:
            ops.append([0, 1, ""])
            if ops[-2][0] == 1 and ops[-2][1] > 1:
                ops[-2][1] -= 1
            else:
                continue
        if right:
            ops.append([4, right, ""])
        if rnd.random() < 0.05 and ops[0][0] != 4:
            ops.insert(0, [5, rnd.randint(1, 30), ""])
        if rnd.random() < 0.05 and ops[-1][0] != 4:
            ops.append([5, rnd.randint(1, 30), ""])
        cig = [(op, ln) for op, ln, _ in ops]
        if sum(ln for op, ln in cig if op in (0, 1, 4)) != length or not _indel_positions_ok(cig, length):
            continue
        break
    seq = [rnd.choice("ACGT") if rnd.random() > p_n else "N" for _ in range(length)]
    ref_cols = []
    for op, ln, _ in ops:
        if op == 0:
            for _ in range(ln):
                if rnd.random() < p_sub:
                    ref_cols.append(rnd.choice("ACGTN"))  # may equal the query letter: "aA" is no dispatch key either
                else:
                    ref_cols.append(None)
    return cig, "".join(seq), _md(ref_cols, ops)


def records(seed, n_pairs=2000, read_length=151, var_lengths=None, p_indel=0.01, p_sub=0.01, p_n=0.002, quirks=True,
            qual_mode="spread", long_del_rate=0.01):
    """The records write_bam writes, in file order.  var_lengths: (lo, hi) inclusive for per-read lengths."""
    rnd = random.Random(seed)
    out = []
    for k in range(n_pairs):
        tlen = rnd.randint(-50, 2100) if rnd.random() < 0.02 else rnd.randint(250, 700)
        kind = "pair"
        if quirks:
            r = rnd.random()
            kind = ("unmapped" if r < 0.01 else "secondary" if r < 0.02 else "supplementary" if r < 0.03 else
                    "neither" if r < 0.04 else "unpaired" if r < 0.05 else "pair")
        for mate in (0, 1):
            length = read_length if var_lengths is None else rnd.randint(*var_lengths)
            long_del = rnd.random() < long_del_rate
            cigar, seq, md = _random_read(rnd, length, p_indel, p_sub, p_n, long_del)
            if qual_mode == "spread":
                level = rnd.choice((2, 8, 14, 22, 27, 33, 36, 38, 41)) if rnd.random() < 0.3 else rnd.randint(28, 38)
                qual = [max(0, min(93, level + rnd.randint(-6, 6))) for _ in range(length)]
            elif qual_mode == "binned":  # NovaSeq-like binned qualities
                qual = [rnd.choice((2, 12, 23, 37, 37, 37, 37)) for _ in range(length)]
            elif qual_mode == "high":  # mean quality 40 and above: the read lands in no bin
                qual = [rnd.randint(40, 45) for _ in range(length)]
            elif qual_mode == "const_head":  # the first positions hold one value in every read: np.std == 0 there
                qual = [35 if i < 5 else rnd.randint(28, 38) for i in range(length)]
            else:
                qual = [rnd.randint(0, 41) for _ in range(length)]
            reverse = (mate == 1) ^ (rnd.random() < 0.1)
            flag = 1 | 2 | (64 if mate == 0 else 128) | (16 if reverse else 0) | (32 if not reverse else 0)
            if kind == "unmapped" and mate == 1:
                flag |= 4
            elif kind == "secondary":
                flag |= 256
            elif kind == "supplementary" and mate == 0:
                flag |= 2048
            elif kind == "neither":
                flag &= ~(64 | 128)
            elif kind == "unpaired":
                flag &= ~(1 | 2 | 32 | 64 | 128)
            tags = [("MD", "Z", md), ("NM", "i", 0)]
            if rnd.random() < 0.3:
                tags.insert(0, ("RG", "Z", "grp%d" % rnd.randint(0, 3)))
            if rnd.random() < 0.1:
                tags.append(("XB", "B", [1, 2, 3]))
            out.append(dict(name="r%d" % k, flag=flag, pos=rnd.randint(0, 900000), tlen=tlen if mate == 0 else -tlen,
                            cigar=cigar, seq=seq, qual=qual, tags=tags))
    return out


def case_records(parts):
    """The records of a golden case (tests/golden/bam/cases.json), in file order: parts of records(**kw) with two edits --
    neither: read1 / read2 flags cleared; read1_level: read1's qualities at that level past position 4, read2 unmapped."""
    out = []
    for part in parts:
        kw = dict(part)
        neither = kw.pop("neither", False)
        level = kw.pop("read1_level", None)
        if kw.get("var_lengths"):
            kw["var_lengths"] = tuple(kw["var_lengths"])
        recs = records(**kw)
        for r in recs:
            if neither:
                r["flag"] &= ~(64 | 128)
            if level is not None and r["flag"] & 64:
                r["qual"] = [level if i >= 5 else 35 for i in range(len(r["qual"]))]
            if level is not None and r["flag"] & 128:
                r["flag"] |= 4  # its mate unmapped: read2's bins are left as they are
        out.extend(recs)
    return out


def write_records(path, recs, level=6):
    data = header_bytes() + b"".join(encode_record(r) for r in recs)
    blob = bgzf(data, level)
    with open(path, "wb") as fh:
        fh.write(blob)
    return hashlib.sha256(blob).hexdigest()


def write_bam(path, seed, **kw):
    """Write the records of records(seed, **kw) as a BAM file; returns the file's sha256."""
    return write_records(path, records(seed, **kw))
