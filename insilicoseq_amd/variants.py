"""`generate --variants`: a VCF's alleles spliced into the records the reads are cut from.

The host's share: ``read_vcf`` (the file -> one ``VariantTable`` per record), the table itself with the plain numpy twin of the
device's splice and lift (``apply_host``, ``lift_host``: the specification the kernels of iss_variants.hip.h are held to),
``write_chain`` / ``read_chain`` / ``lift_chain`` (a UCSC chain from the haplotype back to the record) and ``HaplotypeSeq``, what a
record's ``seq`` becomes so that every ``len(record.seq)`` of the work loops is the haplotype's length while the letters are only
ever spliced on the device (ReadEngine.add_genome_variants)."""
import gzip

import numpy as np

from . import _native

SKIP_REASONS = ("symbolic", "star", "breakend", "missing_alt", "unknown_chrom", "haplotype_ref", "no_change")


def apply_tile():
    """APPLY_TILE: output letters per workgroup of the device's splice kernel (tests put variants across its boundaries)."""
    return int(_native.lib().iss_variants_apply_tile())


class VcfError(ValueError):
    """One line: what is wrong with the file, and where."""


def _u8(seq):
    if isinstance(seq, str):
        seq = seq.encode("ascii")
    if isinstance(seq, (bytes, bytearray)):
        return np.frombuffer(seq, dtype=np.uint8)
    return np.ascontiguousarray(seq, dtype=np.uint8)


class VariantTable(object):
    """One record's variants, normalised, sorted and disjoint: ``pos0`` (int64, the first replaced letter), ``ref_len`` / ``alt_len``
    (int32), ``alt_off`` / ``ref_off`` (int64, into the uint8 blobs ``alt`` / ``ref``) and ``out_pos`` (int64, n + 1 entries):
    out_pos[i] = pos0[i] + the sum of alt_len[j] - ref_len[j] over j < i, where variant i's ALT letters start in the haplotype;
    out_pos[n] = L', its length.  ``record_length`` is L."""

    def __init__(self, pos0, ref_len, alt_len, alts, refs, record_length):
        self.pos0 = np.ascontiguousarray(pos0, dtype=np.int64)
        self.ref_len = np.ascontiguousarray(ref_len, dtype=np.int32)
        self.alt_len = np.ascontiguousarray(alt_len, dtype=np.int32)
        n = self.pos0.size
        assert self.ref_len.size == n and self.alt_len.size == n
        # (the letters: one bytes object per variant, or the whole blob as a uint8 array)
        self.alt = _u8(alts if isinstance(alts, np.ndarray) else b"".join(bytes(a) for a in alts))
        self.ref = _u8(refs if isinstance(refs, np.ndarray) else b"".join(bytes(r) for r in refs))
        self.alt_off = np.zeros(n, dtype=np.int64)
        self.ref_off = np.zeros(n, dtype=np.int64)
        if n:
            self.alt_off[1:] = np.cumsum(self.alt_len[:-1], dtype=np.int64)
            self.ref_off[1:] = np.cumsum(self.ref_len[:-1], dtype=np.int64)
        self.record_length = int(record_length)
        # (a cumulative sum on the host: L' has to be known before anything is allocated on the device)
        delta = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(self.alt_len.astype(np.int64) - self.ref_len.astype(np.int64), out=delta[1:])
        self.out_pos = np.concatenate((self.pos0, [self.record_length])).astype(np.int64) + delta

    @classmethod
    def from_variants(cls, variants, record_length, record_id="record"):
        """``variants``: (pos0, ref letters, alt letters) already normalised; sorted and checked here (VcfError)."""
        items = sorted(((int(v[0]), bytes(_u8(v[1])), bytes(_u8(v[2])), int(v[3]) if len(v) > 3 else int(v[0]) + 1) for v in variants),
                       key=lambda v: (v[0], len(v[1])))  # (the fourth: the line's POS, for the messages)
        for (p, r, a, pos), nxt in zip(items, items[1:] + [None]):
            if p + len(r) > record_length or p > record_length:
                raise VcfError("record %s: the variant at POS %d reaches past the record's end (%d letters)" % (record_id, pos, record_length))
            if nxt is not None and (nxt[0] < p + len(r) or (nxt[0] == p and not r and not nxt[1])):
                raise VcfError("record %s: the variants at POS %d and POS %d overlap" % (record_id, pos, nxt[3]))
        return cls([v[0] for v in items], [len(v[1]) for v in items], [len(v[2]) for v in items], [v[2] for v in items],
                   [v[1] for v in items], record_length)

    def __len__(self):
        return int(self.pos0.size)

    def haplotype_length(self, L=None):
        L = self.record_length if L is None else int(L)
        return L + int(self.out_pos[-1]) - self.record_length

    def counts(self):
        r, a = self.ref_len.astype(np.int64), self.alt_len.astype(np.int64)
        return {"snv": int(((r == 1) & (a == 1)).sum()), "mnv": int(((r == a) & (r > 1)).sum()),
                "insertion": int((a > r).sum()), "deletion": int((a < r).sum()),
                "bases_inserted": int(np.maximum(a - r, 0).sum()), "bases_deleted": int(np.maximum(r - a, 0).sum())}

    # ------------------------------------------------------------------ the twin of the device's kernels
    def apply_host(self, seq):
        """The haplotype of ``seq`` as a uint8 array: the record's letters between the variants, their ALT letters in place of
        the letters they replace."""
        src = _u8(seq)
        assert src.size == self.record_length, (src.size, self.record_length)
        out = np.empty(int(self.out_pos[-1]), dtype=np.uint8)
        src_at = 0
        out_at = 0
        for i in range(len(self)):
            p, r, a = int(self.pos0[i]), int(self.ref_len[i]), int(self.alt_len[i])
            out[out_at:out_at + p - src_at] = src[src_at:p]
            out_at += p - src_at
            assert out_at == int(self.out_pos[i])
            out[out_at:out_at + a] = self.alt[int(self.alt_off[i]):int(self.alt_off[i]) + a]
            out_at += a
            src_at = p + r
        out[out_at:] = src[src_at:]
        return out

    def ref_mismatches(self, seq):
        """Indices of the variants whose REF letters differ from ``seq`` (case ignored)."""
        src = _u8(seq)
        up = lambda x: bytes(x).upper()  # noqa: E731
        return [i for i in range(len(self)) if up(src[int(self.pos0[i]):int(self.pos0[i]) + int(self.ref_len[i])]) !=
                up(self.ref[int(self.ref_off[i]):int(self.ref_off[i]) + int(self.ref_len[i])])]

    def lift_host(self, h):
        """Haplotype coordinates (0 .. L', any shape) -> record coordinates."""
        h = np.asarray(h, dtype=np.int64)
        if not len(self):
            return h.copy()
        i = np.searchsorted(self.out_pos[:-1], h, side="right") - 1  # the last variant with out_pos <= h
        j = np.maximum(i, 0)
        k = h - self.out_pos[j]
        a, r = self.alt_len[j].astype(np.int64), self.ref_len[j].astype(np.int64)
        inside = self.pos0[j] + np.minimum(k, r)
        behind = self.pos0[j] + r + (k - a)
        return np.where(i < 0, h, np.where(k < a, inside, behind))

    # ------------------------------------------------------------------ the library's host entries (the same source as the kernels)
    def _ptrs(self):
        return [x.ctypes.data for x in (self.pos0, self.ref_len, self.alt_len)]

    def apply_native(self, seq):
        src = _u8(seq)
        out = np.empty(max(int(self.out_pos[-1]), 1), dtype=np.uint8)
        lib = _native.lib()
        _native.check(None, lib.iss_variants_host_apply(src.ctypes.data, src.size, len(self), *self._ptrs(), self.alt_off.ctypes.data,
                                                       self.alt.ctypes.data, self.alt.size, self.out_pos.ctypes.data, out.ctypes.data, out.size))
        return out[:int(self.out_pos[-1])]

    def lift_native(self, h):
        h = np.ascontiguousarray(h, dtype=np.int64)
        out = np.empty_like(h)
        lib = _native.lib()
        _native.check(None, lib.iss_variants_host_lift(len(self), *self._ptrs(), self.out_pos.ctypes.data, h.ctypes.data, h.size, out.ctypes.data))
        return out


def normalise(pos0, ref, alt):
    """Trim the longest common prefix, then the longest common suffix of REF and ALT (case ignored): only letters that change are
    replaced, an anchor base keeps the record's own letter and case.  (pos0, ref, alt) or None when nothing is left."""
    ref, alt = bytes(_u8(ref)), bytes(_u8(alt))
    ru, au = ref.upper(), alt.upper()
    k = 0
    while k < len(ru) and k < len(au) and ru[k] == au[k]:
        k += 1
    ref, alt, ru, au, pos0 = ref[k:], alt[k:], ru[k:], au[k:], pos0 + k
    k = 0
    while k < len(ru) and k < len(au) and ru[-1 - k] == au[-1 - k]:
        k += 1
    if k:
        ref, alt = ref[:-k], alt[:-k]
    return (pos0, ref, alt) if ref or alt else None


def _open_text(path):
    path = str(path)
    return gzip.open(path, "rt") if path.endswith(".gz") else open(path, "r")


def read_vcf(path, record_ids, haplotype=None, record_lengths=None):
    """``{record id: VariantTable}`` for the records of ``record_ids`` that have variants, and the counts of what was skipped
    (SKIP_REASONS).  ``record_ids``: the ids, or ``{id: length}``; ``record_lengths`` may give the lengths apart.  Without
    ``haplotype`` the first ALT allele of every line is applied; with ``haplotype`` = 1 or 2 the allele the first sample's GT names
    for that haplotype.  Errors are VcfError, one line each."""
    if haplotype not in (None, 1, 2):
        raise VcfError("%s: the haplotype is 1 or 2, not %r" % (path, haplotype))
    lengths = dict(record_ids) if isinstance(record_ids, dict) else dict(zip(record_ids, record_lengths or [None] * len(record_ids)))
    skipped = dict.fromkeys(SKIP_REASONS, 0)
    per_record = {}
    with _open_text(path) as fh:
        for lineno, line in enumerate(fh, 1):
            if line.startswith("#") or not line.strip():
                continue
            f = line.rstrip("\r\n").split("\t")
            if len(f) < 5:
                raise VcfError("%s: line %d: fewer than five columns" % (path, lineno))
            chrom, pos, ref, alts = f[0], f[1], f[3], f[4].split(",")
            try:
                pos0 = int(pos) - 1
            except ValueError:
                raise VcfError("%s: line %d: POS %r is not a number" % (path, lineno, pos))
            if pos0 < 0:
                raise VcfError("%s: line %d: POS %s is not positive" % (path, lineno, pos))
            if chrom not in lengths:
                skipped["unknown_chrom"] += 1
                continue
            allele = 1
            if haplotype is not None:
                if len(f) < 10 or "GT" not in f[8].split(":"):
                    raise VcfError("%s: line %d: no GT field for the haplotype" % (path, lineno))
                gt = f[9].split(":")[f[8].split(":").index("GT")]
                parts = gt.replace("/", "|").split("|")
                if "/" in gt and len(set(parts)) > 1:
                    raise VcfError("%s: line %d: the unphased heterozygous GT %s names no haplotype" % (path, lineno, gt))
                which = parts[haplotype - 1] if len(parts) >= haplotype else parts[-1]
                if which in (".", "0"):
                    skipped["haplotype_ref"] += 1
                    continue
                try:
                    allele = int(which)
                except ValueError:
                    raise VcfError("%s: line %d: the GT %s is not understood" % (path, lineno, gt))
                if allele < 1 or allele > len(alts):
                    raise VcfError("%s: line %d: the GT %s names an allele the line does not have" % (path, lineno, gt))
            alt = alts[allele - 1]
            if alt.startswith("<"):
                skipped["symbolic"] += 1
            elif alt == "*":
                skipped["star"] += 1
            elif "[" in alt or "]" in alt:
                skipped["breakend"] += 1
            elif alt in (".", ""):
                skipped["missing_alt"] += 1
            else:
                v = normalise(pos0, ref, alt)
                if v is None:
                    skipped["no_change"] += 1
                else:
                    per_record.setdefault(chrom, []).append(v + (int(pos),))
    tables = {}
    for rid, items in per_record.items():
        L = lengths[rid]
        if L is None:
            raise VcfError("%s: the length of record %s is not known" % (path, rid))
        tables[rid] = VariantTable.from_variants(items, L, rid)
    return tables, skipped


# ---------------------------------------------------------------------- the chain file
def chain_blocks(L, table):
    """[(size, dt, dq)] of the chain haplotype -> record: one ungapped block per gap between variants (n + 1 of them; a block may
    be empty), behind each but the last the variant's letters on either side: dt = alt_len in the haplotype, dq = ref_len in the
    record."""
    n = len(table)
    starts = np.concatenate(([0], table.pos0 + table.ref_len)).astype(np.int64)
    ends = np.concatenate((table.pos0, [L])).astype(np.int64)
    sizes = ends - starts
    return [(int(sizes[i]), int(table.alt_len[i]) if i < n else None, int(table.ref_len[i]) if i < n else None) for i in range(n + 1)]


def write_chain(handle, record_id, L, table):
    """One UCSC chain: the target is the haplotype (``record_id``, L' letters), the query the record (``record_id``, L letters)."""
    blocks = chain_blocks(L, table)
    Lh = table.haplotype_length(L)
    handle.write("chain %d %s %d + 0 %d %s %d + 0 %d %d\n" % (sum(b[0] for b in blocks), record_id, Lh, Lh, record_id, L, L, 1))
    for size, dt, dq in blocks:
        handle.write("%d\n" % size if dt is None else "%d\t%d\t%d\n" % (size, dt, dq))
    handle.write("\n")


def read_chain(handle):
    """``{target name: (tSize, qSize, [(size, dt, dq)])}`` of a file write_chain wrote (one chain per name, both strands +)."""
    chains, cur = {}, None
    for line in handle:
        f = line.split()
        if not f:
            cur = None
        elif f[0] == "chain":
            cur = chains[f[2]] = (int(f[3]), int(f[8]), [])
        elif cur is not None:
            cur[2].append((int(f[0]), int(f[1]) if len(f) > 1 else None, int(f[2]) if len(f) > 2 else None))
    return chains


def lift_chain(chain, h):
    """Haplotype coordinates -> record coordinates through the blocks of one chain: a coordinate in a block moves with it, one in
    the gap behind a block (the haplotype's dt letters) to the gap's start in the record plus min(offset, dq)."""
    _t_size, _q_size, blocks = chain
    h = np.asarray(h, dtype=np.int64)
    out = np.empty_like(h)
    for idx, x in np.ndenumerate(h):
        t = q = 0
        for size, dt, dq in blocks:
            if x < t + size or dt is None:
                out[idx] = q + (x - t)
                break
            t, q = t + size, q + size
            if x < t + dt:
                out[idx] = q + min(int(x) - t, dq)
                break
            t, q = t + dt, q + dq
    return out


# ---------------------------------------------------------------------- records whose letters are a haplotype
class HaplotypeSeq(object):
    """A record's ``seq`` under --variants: ``len()`` is the haplotype's length, so the work divider, the short-record rule, the
    depth tables and the headers count the letters the reads are cut from; ``ref`` and ``table`` are what the device splices them
    from (GenomeStore -> ReadEngine.add_genome_variants).  ``str()`` is the host twin's haplotype, for a caller that insists."""

    def __init__(self, ref, table):
        self.ref, self.table = ref, table

    def __len__(self):
        return self.table.haplotype_length(len(self.ref))

    def __str__(self):
        return self.table.apply_host(self.ref).tobytes().decode("ascii")


def with_haplotypes(records, tables):
    """The records with the ``seq`` of those that have a table replaced by a HaplotypeSeq (new Record objects; the rest as they are)."""
    from .generator import Record

    def letters(seq):  # (--device_fasta: a record with variants materialises its letters on the host, fasta.FastaSeq.__str__)
        return str(seq) if hasattr(seq, "body_off") else seq

    return [Record(HaplotypeSeq(letters(r.seq), tables[r.id]), id=r.id, description=getattr(r, "description", "")) if r.id in tables else r
            for r in records]


def load(path, records, haplotype=None):
    """read_vcf for ``records`` -> (the records with haplotypes, tables, skipped counts)."""
    tables, skipped = read_vcf(path, {r.id: len(r.seq) for r in records}, haplotype)
    return with_haplotypes(records, tables), tables, skipped
