"""Genome inputs of `generate` besides --genomes: draft assemblies (--draft) and a random subset of records (--n_genomes / -u).

Mirrors iss/generator.py:424-494 (load_genomes), iss/generator.py:519-587 (the draft branches of
load_readcount_or_abundance), iss/abundance.py:254-317 (draft, expand_draft_abundance) and iss/util.py:179-210
(reservoir), quirks included:

* a draft file is one genome: the distribution is drawn over ``complete + draft paths``, where ``complete`` is
  ``list(set(record ids) - set(draft contig ids))`` -- the order of that set is the order the numpy draws follow;
  ``_abundance.txt`` names the draft files by the paths given on the command line;
* a draft's abundance is spread over its contigs by length, a coverage is given to every contig as it is;
* a contig id repeated across drafts keeps the value of the later one (a dict), and every record of that id gets it;
* ``--n_genomes`` draws ``sorted(sample(range(0, total - 1), n))`` from a freshly OS-seeded RNG (the reference calls
  ``random.seed()``: not reproducible with --seed; the last record is never chosen), and only without --draft.
"""
import logging
import random
import shutil
import sys

from .generator import parse_fasta, read_genome_bytes


def concatenate(file_list, output, device_inflate=None):
    """util.concatenate (iss/util.py:213-234): the files' bytes one after the other.  A file that starts with the gzip magic
    (.fa.gz, bgzip-ped or not) is inflated on the way (generator.read_genome_bytes: BGZF on the device when ``device_inflate`` or
    ISS_DEVICE_INFLATE=1, gzip on the host otherwise)."""
    with open(output, "wb") as out:
        for name in file_list:
            if name is not None:
                with open(name, "rb") as fh:
                    if fh.read(2) == b"\x1f\x8b":
                        out.write(read_genome_bytes(name, device_inflate))
                        continue
                    fh.seek(0)
                    shutil.copyfileobj(fh, out)


def reservoir_indices(total, n, rng):
    """The records util.reservoir keeps (iss/util.py:179-210): ordinals in file order.  ``rng``: a random.Random."""
    if not n < total:
        logging.getLogger(__name__).error("-u should be strictly smaller than total number of records.")
        sys.exit(1)
    return sorted(rng.sample(range(0, total - 1), n))


def write_fasta(records, path):
    """SeqIO.write(records, path, "fasta") for records parsed from FASTA: the header line as it was, 60 letters per line."""
    with open(path, "w") as fh:
        for r in records:
            fh.write(">%s\n" % r.description)
            seq = r.seq if isinstance(r.seq, str) else str(r.seq)
            for i in range(0, len(seq), 60):
                fh.write(seq[i:i + 60] + "\n")


def load_genomes(genomes, draft, output, n_genomes, rng=None, device_fasta=False):
    """load_genomes (iss/generator.py:424-494) without --ncbi: concatenates --genomes, then --draft into
    ``<output>.iss.tmp.genomes.fasta``; with --n_genomes (and no --draft) keeps a random subset and rewrites the file.
    Returns (path, records).  ``device_fasta``: the file is indexed on device 0 and the records' letters stay in it (fasta.read)."""
    logger = logging.getLogger(__name__)
    if not (genomes or draft):
        logger.error("One of --genomes/-g, --draft, --ncbi/-k is required")
        sys.exit(1)
    genome_file = output + ".iss.tmp.genomes.fasta"
    concatenate(list(genomes or []) + list(draft or []), genome_file, True if device_fasta else None)

    def read():
        if device_fasta:
            from . import fasta

            return fasta.read(genome_file, device=0)
        return list(parse_fasta(genome_file))

    records = read()
    if n_genomes and not draft:
        keep = reservoir_indices(len(records), n_genomes, rng if rng is not None else random.Random())
        # (the letters as str before the file they stand in is written anew)
        records = [type(r)(str(r.seq), id=r.id, description=r.description) if device_fasta else r for r in (records[i] for i in keep)]
        write_fasta(records, genome_file)
        records = read()
    return genome_file, records


def draft_contigs(path):
    """(id, length) of the records of one draft file (SeqIO.parse(path, "fasta"))."""
    return [(r.id, len(r.seq)) for r in parse_fasta(path)]


def expand_draft_abundance(abundance_dic, draft, mode="abundance", contigs=None):
    """iss/abundance.py:282-317: a draft's value for each of its contigs -- by length (abundance) or as it is (coverage).
    ``contigs``: {path: draft_contigs(path)} when the caller has read them already."""
    draft_dic = {}
    for key, value in abundance_dic.items():
        if key in draft:
            recs = contigs[key] if contigs is not None and key in contigs else draft_contigs(key)
            total_length = sum(n for _rid, n in recs)
            for rid, n in recs:
                if mode == "abundance":
                    draft_dic[rid] = value * (n / total_length)
                elif mode == "coverage":
                    draft_dic[rid] = value
    return draft_dic


def complete_genomes(genome_ids, draft, contigs=None):
    """``list(set(genomes) - set(draft_records))`` of abundance.draft (iss/abundance.py:268-271)."""
    draft_records = []
    for d in draft:
        draft_records.extend([rid for rid, _n in (contigs[d] if contigs is not None else draft_contigs(d))])
    return list(set(genome_ids) - set(draft_records))


def draft_abundance(genome_ids, draft, distribution, write, mode="abundance"):
    """abundance.draft (iss/abundance.py:254-279): ``distribution`` drawn over the complete genomes and the draft files,
    ``write(dic)`` writes ``_abundance.txt`` (file paths as keys), then the drafts are expanded to their contigs.  (Each
    draft file is read once here; the reference reads it twice.)"""
    contigs = {d: draft_contigs(d) for d in draft}
    abundance_dic = distribution(complete_genomes(genome_ids, draft, contigs) + list(draft))
    complete = {k: v for k, v in abundance_dic.items() if k not in draft}
    write(abundance_dic)
    return {**complete, **expand_draft_abundance(abundance_dic, draft, mode, contigs)}


def expand_file_dic(dic, draft, mode):
    """--abundance_file / --coverage_file with --draft (iss/generator.py:529-545): keys naming a draft file are expanded,
    the others kept."""
    complete = {k: v for k, v in dic.items() if k not in draft}
    return {**complete, **expand_draft_abundance(dic, draft, mode)}
