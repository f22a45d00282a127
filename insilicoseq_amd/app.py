"""`generate` and `model`.  `generate`: the reference's ``iss generate`` flow (iss/app.py:23-144) on GPUs.

Same steps, same file names, same flag names for the options this engine supports: load the error
model, concatenate the genome FASTA files, draw / read abundances (written to ``<out>_abundance.txt``),
cut the work into ``ceil(n_pairs / workers)``-sized chunks (iss/app.py:81-83), run one worker per GPU
(``worker_iterator``; a process pool like the reference's, each process owning one device), concatenate
``<out>.iss.tmp.<k>_R{1,2}.fastq`` in worker order and clean up (iss/app.py:119-143).

Differences a user must know: uniforms come from Philox keyed by ``seed + worker``
(not the reference's Mersenne Twisters), and the reference's dropped surplus chunk / missing-temp-file
failure modes are reproduced deliberately so outputs stay comparable.
"""
import argparse
import gzip
import random
import logging
import multiprocessing as mp
import os
import sys
import time

import numpy as np

from . import drafts
from .distributed import VCF_HEADER, concatenate_rank_files, temp_prefix
from .generator import WorkerSetNotSetUp, generate_work_divider, parse_fasta, worker_iterator, worker_set_iterator
from .model import BasicErrorModel, KDErrorModel, PerfectErrorModel
from .origins import SUFFIX as ORIGINS_SUFFIX

PROFILES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
# names of iss/generator.py:377-387 -> dense files converted from the reference's profiles
PRECOMPUTED = {"hiseq": "hiseq", "novaseq": "novaseq", "miseq": "miseq", "miseq-20": "miseq-20", "miseq-24": "miseq-24",
               "miseq-28": "miseq-28", "miseq-32": "miseq-32", "miseq-36": "miseq-36", "nextseq": "nextseq"}


def convert_n_reads(unit):
    """iss/util.py:137-161: 'k', 'm', 'g' suffixes."""
    suffixes = {"k": 3, "m": 6, "g": 9}
    unit = str(unit)
    if unit[-1].lower() in suffixes:
        return int(float(unit[:-1]) * 10 ** suffixes[unit[-1].lower()])
    return int(unit)


def load_error_model(mode, seed, model, fragment_length, fragment_length_sd, store_mutations, rng="philox"):
    """iss/generator.py:359-421: kde, basic and perfect."""
    logger = logging.getLogger(__name__)
    if fragment_length is not None and fragment_length_sd is not None:
        logger.info("Using custom fragment length %s and default fragment length sd %s" % (fragment_length,
                                                                                           fragment_length_sd))
    elif bool(fragment_length) ^ bool(fragment_length_sd):  # generator.py:393-395
        logger.error("fragment_length and fragment_length_sd must be specified together")
        sys.exit(1)
    if seed:  # generator.py:397-400 (seed 0 leaves the parent unseeded)
        random.seed(seed)
        np.random.seed(seed)
    if mode == "basic":  # generator.py:412-416
        if model is not None:
            logger.warning("--model %s will be ignored in --mode %s" % (model, mode))
        return BasicErrorModel(fragment_length, fragment_length_sd, store_mutations)
    if mode == "perfect":  # generator.py:417-421 (the reference's model with store_mutations = False supplied: SURVEY.md A-8)
        if model is not None:
            logger.warning("--model %s will be ignored in --mode %s" % (model, mode))
        return PerfectErrorModel(fragment_length, fragment_length_sd, store_mutations)
    if model is None:
        logger.error("--model is required in --mode kde")
        sys.exit(1)
    if model.lower() in PRECOMPUTED:
        npz = os.path.join(PROFILES, PRECOMPUTED[model.lower()] + ".dense.npz")
    else:
        npz = model
    return KDErrorModel(npz, fragment_length, fragment_length_sd, store_mutations)


def parse_abundance_file(path):
    """iss/abundance.py:13-44: tab separated `record<TAB>abundance`."""
    logger = logging.getLogger(__name__)
    out = {}
    try:
        with open(path) as fh:
            for line in fh:
                if not line.strip():
                    continue
                rid, val = line.split()[0], float(line.split()[1])
                out[rid] = val
    except (IOError, IndexError, ValueError) as e:
        logger.error("Failed to read abundance file: %s" % e)
        sys.exit(1)
    return out


def parse_readcount_file(path):
    return {k: int(v) for k, v in parse_abundance_file(path).items()}


def lognormal(record_list):
    """iss/abundance.py:137-154 (global numpy stream, seeded by load_error_model like the reference)."""
    dist = np.random.lognormal(size=len(record_list))
    scaled = dist / sum(dist)
    return {r: a for r, a in zip(record_list, scaled)}


def uniform(record_list):
    return {r: 1 / len(record_list) for r in record_list}


def exponential(record_list):
    dist = np.random.exponential(size=len(record_list))
    scaled = dist / sum(dist)
    return {r: a for r, a in zip(record_list, scaled)}


def halfnormal(record_list):
    """iss/abundance.py:97-114: scipy's half-normal variates (drawn from numpy's global stream, like the reference's)."""
    from scipy import stats

    dist = stats.halfnorm.rvs(loc=0.00, scale=1.00, size=len(record_list))
    scaled = dist / sum(dist)
    return {r: a for r, a in zip(record_list, scaled)}


def zero_inflated_lognormal(record_list):
    """iss/abundance.py:157-175: a fifth of the records (Bernoulli 0.2) get no reads at all."""
    from scipy import stats

    zero_inflated = stats.bernoulli.rvs(p=0.2, size=len(record_list))
    dist = (1 - zero_inflated) * np.random.lognormal(size=len(record_list))
    scaled = dist / sum(dist)
    return {r: a for r, a in zip(record_list, scaled)}


ABUNDANCE = {"lognormal": lognormal, "uniform": uniform, "exponential": exponential, "halfnormal": halfnormal,
             "zero_inflated_lognormal": zero_inflated_lognormal}


def coverage_scaling(total_n_reads, coverage_dic, records, read_length):
    """iss/abundance.py:196-228: scale a coverage distribution so that it adds up to the requested number of reads."""
    logger = logging.getLogger(__name__)
    total_reads = 0
    for record in records:
        if record.id not in coverage_dic:
            logger.error("Fasta record not found in abundance file: %r" % record.id)
            sys.exit(1)
        total_reads += coverage_dic[record.id] * len(record.seq) / read_length / 2
    scale_factor = total_n_reads / total_reads
    for key in coverage_dic:
        coverage_dic[key] *= scale_factor
    return coverage_dic


def _write_distribution(dic, output, mode):
    """abundance.to_file (iss/abundance.py:231-251): <out>_abundance.txt or <out>_coverage.txt"""
    with open(output + ("_abundance.txt" if mode == "abundance" else "_coverage.txt"), "w") as fh:
        for rid, a in dic.items():
            fh.write("%s\t%s\n" % (rid, a))


def compress_file(path, block_bytes=32 << 20, threads=None):
    """gzip `path` to `path + ".gz"` and remove it, like iss/util.py:255-268, but block-parallel: every block of the
    file becomes one gzip member compressed on its own thread (zlib releases the GIL); concatenated members are
    one valid gzip stream with the same content as the reference's single-member file."""
    import zlib
    from concurrent.futures import ThreadPoolExecutor

    threads = threads or min(32, os.cpu_count() or 1)

    def member(block):
        c = zlib.compressobj(6, zlib.DEFLATED, 31)  # wbits 31: gzip container
        return c.compress(block) + c.flush()

    with open(path, "rb") as fi, open(path + ".gz", "wb") as fo, ThreadPoolExecutor(threads) as pool:
        pending = []
        while True:
            block = fi.read(block_bytes)
            if block:
                pending.append(pool.submit(member, block))
            while pending and (not block or len(pending) >= 2 * threads):
                fo.write(pending.pop(0).result())
            if not block:
                break
        if os.path.getsize(path) == 0:
            fo.write(member(b""))
    os.remove(path)
    return path + ".gz"


def _worker(rank, device, genome_file, work_spec, npz, seed, prefix, sequence_type, gc_bias, rng, store_mutations,
            fragment, compress=False, mode=None, report=False, depth=False, records=None, ubam=False, origins=False, bgzip=False,
            error_report=False, variants=None, device_fasta=False):
    """One pool process == one GPU.  Records are re-read from the concatenated FASTA (the reference
    pickles them; same content) unless the caller runs in this process and hands its own over.  ``report``: the worker tallies
    its reads on the device into ``<prefix>.tally.npy``; ``depth``: it marks their template intervals into ``<prefix>.depth.npz``
    (worker_iterator); ``ubam``: it writes ``<prefix>.bam``, BGZF record blocks, instead of the two FASTQ files; ``origins``: it also
    writes ``<prefix>_origins.bedpe``, every pair's source intervals; ``bgzip``: its ``.vcf`` and ``_origins.bedpe`` hold BGZF members
    compressed on the device instead of text; ``error_report``: it tallies its mutation rows on the device into
    ``<prefix>.errtally.npy``; ``variants``: (VCF path, haplotype or None) -- records re-read here get their variants again
    (variants.load), records handed over carry them already."""
    logging.basicConfig(level=logging.WARNING)
    if report or depth or error_report:
        from .tensors import _torch

        _torch()  # (the tally words / the depth accumulator are torch tensors: torch's HIP runtime has to be the process's first)
    # (records are identified by their ordinal in the concatenated FASTA, not by id: draft assemblies repeat ids)
    reread = records is None
    if reread and device_fasta:  # (--device_fasta: indexed on this worker's device, the bodies stay in the file)
        from . import fasta

        records = fasta.read(genome_file, device=device)
    records = list(records if records is not None else parse_fasta(genome_file))
    if variants is not None and reread:
        from . import variants as V

        records = V.load(variants[0], records, variants[1])[0]
    if mode is None:  # (callers that name no mode: a model file is kde, none is basic)
        mode = "kde" if npz is not None else "basic"
    if mode == "basic":
        model = BasicErrorModel(fragment[0], fragment[1], store_mutations)
    elif mode == "perfect":
        model = PerfectErrorModel(fragment[0], fragment[1], store_mutations)
    else:
        model = KDErrorModel(npz, fragment[0], fragment[1], store_mutations)
    work = [(records[idx], n, "default") for idx, n in work_spec]
    more = {"depth": True, "ordinals": [idx for idx, _n in work_spec]} if depth else {}  # (without the flag: the call as it was)
    if ubam:
        more["ubam"] = True
    if origins:
        more["origins"] = True
    if bgzip:
        more["bgzip"] = True
    if error_report:
        more["error_report"] = True
    worker_iterator(work, model, rank, prefix, seed, sequence_type, gc_bias, device=device, rng=rng, compress=compress, report=report, **more)


def _run_worker_set(jobs, records, error_model, args, device_gzip, workers):
    """The reference's N workers as N chains side by side on ONE GPU (worker_set_iterator; up to 1024 of them).  Returns whether
    the FINAL files were written (else the temp files were), or None when the set cannot be set up -- more workers than the engine takes, not enough memory for their stream buffers (three turns of
    stream words per worker and buffer: tens of GB from W = 512 on with long reads) -- BEFORE anything was written: the caller
    then takes the process pool, which has no such limit.  (ISS_HOST_FASTQ=1, the host formatter, is a Worker switch: the pool.)"""
    logger = logging.getLogger(__name__)
    works = [[(records[idx], n, "default") for idx, n in j[3]] for j in jobs]
    try:
        # text mode: the workers write at their places of the FINAL files -- the concatenation has nothing left to do (fewer
        # chunks than workers: the reference fails on the missing temp file, util.py:233 -- that path keeps the temp files)
        return worker_set_iterator(
            works, error_model, [j[0] for j in jobs], [j[6] for j in jobs], args.seed, args.sequence_type, args.gc_bias, device=0,
            compress=device_gzip, vcf_files=bool(getattr(args, "store_mutations", False)),
            final_prefix=args.output if len(jobs) == workers and os.environ.get("ISS_SET_TEMP_FILES", "") != "1" else None)
    except WorkerSetNotSetUp as e:  # (seeding, the row pool of --store_mutations, or the first call's stream buffers: nothing ran yet)
        logger.warning("%d workers side by side do not fit the device (%s): one process per worker instead" % (workers, e))
        return None


def _write_report(output, n_workers, read_length):
    """--report: the workers' tallies (``<temp prefix>.tally.npy``) summed into ``<output>_tally.npy`` -- the raw uint64 words,
    tally.tally_layout -- and ``<output>_report.json`` (tally.report_dict); the workers' files are removed."""
    import json

    from .tally import merge_tallies, report_dict

    paths = ["%s.tally.npy" % temp_prefix(output, rank) for rank in range(n_workers)]
    words = merge_tallies([np.load(path) for path in paths])
    np.save(output + "_tally.npy", words)
    with open(output + "_report.json", "w") as fh:
        json.dump(report_dict(words, read_length), fh)
        fh.write("\n")
    for path in paths:
        os.remove(path)


def _write_errors(output, n_workers, read_length, with_report):
    """--error_report: the workers' error tallies (``<temp prefix>.errtally.npy``) summed into ``<output>_errtally.npy`` -- the raw
    uint64 words, errtally.layout -- and ``<output>_errors.json`` (errtally.report_dict; with --report, whose ``<output>_tally.npy``
    is then read back, also its ``calibration``); the workers' files are removed.  Returns the sum's ``dropped``."""
    import json

    from .errtally import merge, report_dict, split

    paths = ["%s.errtally.npy" % temp_prefix(output, rank) for rank in range(n_workers)]
    words = merge([np.load(path) for path in paths])
    np.save(output + "_errtally.npy", words)
    tally = np.load(output + "_tally.npy") if with_report else None
    with open(output + "_errors.json", "w") as fh:
        json.dump(report_dict(words, read_length, tally), fh)
        fh.write("\n")
    for path in paths:
        os.remove(path)
    return int(split(words, read_length)["dropped"][0])


def _write_depth(output, n_workers, records, bin):
    """--depth: the workers' accumulators (``<temp prefix>.depth.npz``) merged into one difference array over all records in FASTA
    order (depth.merge_into: a record split across two workers' chunks is summed), finished ONCE on device 0 through a bare engine
    context (ReadEngine.depth_finish), then ``<output>_depth.txt`` and, with ``bin`` > 0, ``<output>_depth.bedgraph``; the
    workers' files are removed."""
    from . import depth as D
    from .engine import ReadEngine
    from .tensors import _torch

    torch = _torch()
    table, n_words = D.depth_table([len(r.seq) for r in records])
    diff = np.zeros(n_words, dtype=np.int32)
    paths = ["%s.depth.npz" % temp_prefix(output, rank) for rank in range(n_workers)]
    for path in paths:
        with np.load(path) as z:
            D.merge_into(diff, table, z["diff"], z["table"], z["ordinals"])
    n_bins = int(D.n_windows(table, bin).sum())
    with ReadEngine(0) as eng, torch.cuda.device(0):
        dev = torch.device("cuda", 0)
        d_diff, d_table = torch.from_numpy(diff).to(dev), torch.from_numpy(table).to(dev)
        d_stats = torch.empty((len(records), 4), dtype=torch.int64, device=dev)
        d_bins = torch.empty(max(n_bins, 1), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()  # (uploaded on torch's stream; the engine works on its own)
        eng.depth_finish(d_diff.data_ptr(), n_words, None, d_table.data_ptr(), len(records), bin, d_stats.data_ptr(),
                         d_bins.data_ptr() if n_bins else None)
        eng.synchronize()
        stats, bins = d_stats.cpu().numpy().view(np.uint64), d_bins.cpu().numpy().view(np.uint64)[:n_bins]
    ids = [r.id for r in records]
    D.write_depth_table(output + "_depth.txt", D.depth_rows(stats, table, ids))
    if bin > 0:
        D.write_bedgraph(output + "_depth.bedgraph", bins, table, ids, bin)
    for path in paths:
        os.remove(path)


def _load_variants(args, records):
    """--variants: the records with their haplotypes in place of their letters (variants.HaplotypeSeq: every length from here on
    is the haplotype's), after ``<output>_variants.json`` (per record L, the haplotype's length and the variants by class; what was
    skipped, by reason) and ``<output>_haplotype.chain`` (haplotype -> record, one chain per record) are written; with
    --write_haplotype also ``<output>_haplotype.fasta``, every record as the reads will see it, the spliced ones downloaded from
    the device that built them."""
    import json

    from . import variants as V
    from ._native import EngineError, NativeLibraryError

    logger = logging.getLogger(__name__)
    try:
        spliced, tables, skipped = V.load(args.variants, records, args.variants_haplotype)
        if getattr(args, "write_haplotype", False):
            from .engine import ReadEngine

            if any(getattr(args, flag, None) for flag in ("report", "depth", "depth_bin", "error_report")):
                from .tensors import _torch

                _torch()  # (those flags work on torch tensors later in this process: torch's HIP runtime has to be its first)
            with ReadEngine(0) as eng, open(args.output + "_haplotype.fasta", "wb") as fh:
                for old, new in zip(records, spliced):
                    if new is old:
                        seq = str(old.seq) if hasattr(old.seq, "body_off") else old.seq  # (--device_fasta: the letters on demand)
                        letters = seq.encode("ascii") if isinstance(seq, str) else bytes(seq)
                    else:
                        letters = eng.genome_letters(eng.add_genome_variants(new.seq.ref, new.seq.table, record_id=old.id)).tobytes()
                        eng.clear_genomes()
                    fh.write(b">" + (getattr(old, "description", "") or old.id).encode() + b"\n")
                    fh.write(b"\n".join(letters[at:at + 80] for at in range(0, len(letters), 80)) + b"\n")
    except (V.VcfError, EngineError, NativeLibraryError, OSError) as e:
        logger.error("--variants: %s" % (str(e).splitlines()[0] if str(e) else type(e).__name__))
        sys.exit(1)
    summary = {"vcf": args.variants, "haplotype": args.variants_haplotype, "skipped": skipped, "records": {}}
    with open(args.output + "_haplotype.chain", "w") as fh:
        for old, new in zip(records, spliced):
            table = tables.get(old.id) if new is not old else None
            entry = {"L": len(old.seq), "L_haplotype": len(new.seq)}
            entry.update(table.counts() if table is not None else V.VariantTable([], [], [], [], [], len(old.seq)).counts())
            summary["records"][old.id] = entry
            if table is not None:
                V.write_chain(fh, old.id, len(old.seq), table)
    with open(args.output + "_variants.json", "w") as fh:
        json.dump(summary, fh, indent=1)
        fh.write("\n")
    logger.info("--variants: %d records with variants, %d lines skipped" % (len(tables), sum(skipped.values())))
    return spliced


def load_readcount_or_abundance(args, records, error_model):
    """load_readcount_or_abundance (iss/generator.py:497-594), in the reference's order of precedence, with --draft:
    returns (readcount_dic, abundance_dic, n_reads) and writes _abundance.txt / _coverage.txt like the reference."""
    logger = logging.getLogger(__name__)
    draft = args.draft or []
    ids = [r.id for r in records]
    readcount_dic = abundance_dic = None
    if args.readcount_file:
        logger.warning("--readcount_file disables --n_reads, n_reads will be calculated from the readcount file")
        if draft:  # generator.py:519-520 (a RuntimeError there)
            logger.error("readcount_file is only supported using --genomes, not --draft")
            sys.exit(1)
        readcount_dic = parse_readcount_file(args.readcount_file)
        n_reads = sum(readcount_dic.values())
    else:
        n_reads = convert_n_reads(args.n_reads)
        if args.abundance_file:
            abundance_dic = parse_abundance_file(args.abundance_file)
            if draft:  # file paths as keys: spread over the contigs by length
                abundance_dic = drafts.expand_file_dic(abundance_dic, draft, "abundance")
        elif args.coverage_file:  # coverages instead of shares: the reads per record no longer depend on --n_reads
            logger.warning("--coverage_file disables --n_reads")
            abundance_dic = parse_abundance_file(args.coverage_file)
            if draft:
                abundance_dic = drafts.expand_file_dic(abundance_dic, draft, "coverage")
        elif args.coverage in ABUNDANCE:
            if draft:  # drawn from the --abundance distribution (generator.py:554-561), _abundance.txt written on the way
                abundance_dic = drafts.draft_abundance(ids, draft, ABUNDANCE[args.abundance],
                                                       lambda d: _write_distribution(d, args.output, "abundance"), "coverage")
            else:
                abundance_dic = ABUNDANCE[args.coverage](ids)
            if args.n_reads:
                abundance_dic = coverage_scaling(n_reads, abundance_dic, records, error_model.read_length)
            _write_distribution(abundance_dic, args.output, "coverage")
        elif args.abundance in ABUNDANCE:
            if draft:
                abundance_dic = drafts.draft_abundance(ids, draft, ABUNDANCE[args.abundance],
                                                       lambda d: _write_distribution(d, args.output, "abundance"))
            else:
                abundance_dic = ABUNDANCE[args.abundance](ids)
                _write_distribution(abundance_dic, args.output, "abundance")
        else:
            logger.error("Could not get abundance, or coverage or readcount information")
            sys.exit(1)
    return readcount_dic, abundance_dic, n_reads


def _worker_set_wanted(args, report, depth):
    """Do the workers of this command run side by side in one context (worker_set_iterator) rather than one process each?"""
    return args.gpus > 1 and args.rng == "mt" and args.devices == 1 and args.seed is not None and args.gpus <= 1024 \
        and os.environ.get("ISS_HOST_FASTQ", "") != "1" and not report and not depth \
        and not getattr(args, "origins", False) and not getattr(args, "error_report", False)
    # (--report, --depth, --origins, --error_report: the set has no tally, depth, origins or error-tally writer of its own -- the pool)


def _remove_ubam_files(output, workers):
    for path in [output + ".bam"] + ["%s.bam" % temp_prefix(output, rank) for rank in range(workers)]:
        if os.path.exists(path):
            os.remove(path)


def generate_reads(args):
    logger = logging.getLogger(__name__)
    if getattr(args, "error_report", False) and not args.store_mutations:
        logger.error("--error_report tallies the --store_mutations rows: add --store_mutations")
        sys.exit(1)
    ubam = bool(getattr(args, "ubam", False))
    if ubam and _worker_set_wanted(args, bool(getattr(args, "report", False)),
                                   bool(getattr(args, "depth", False)) or int(getattr(args, "depth_bin", None) or 0) > 0):
        logger.error("--ubam is not supported with --rng mt --cpus %d --devices 1 (workers side by side in one context): "
                     "use one device per worker, or --cpus 1" % args.gpus)
        sys.exit(1)
    if ubam and os.environ.get("ISS_HOST_FASTQ", "") == "1":
        logger.error("--ubam builds its records on the device: unset ISS_HOST_FASTQ")
        sys.exit(1)
    if getattr(args, "origins", False) and os.environ.get("ISS_HOST_FASTQ", "") == "1":
        logger.error("--origins builds its text on the device: unset ISS_HOST_FASTQ")
        sys.exit(1)
    if getattr(args, "bgzip", False):
        for switch in ("ISS_HOST_FASTQ", "ISS_HOST_VCF"):
            if os.environ.get(switch, "") == "1":
                logger.error("--bgzip compresses its text on the device: unset %s" % switch)
                sys.exit(1)
    try:
        _generate_reads(args, ubam)
    except BaseException:
        if ubam:  # (no half-written final file, and no blocks without their frame)
            _remove_ubam_files(args.output, args.gpus)
        raise


def _generate_reads(args, ubam):
    logger = logging.getLogger(__name__)
    error_model = load_error_model(args.mode, args.seed, args.model, args.fragment_length, args.fragment_length_sd,
                                   args.store_mutations, args.rng)
    # load_genomes (generator.py:424-494): --genomes then --draft into <out>.iss.tmp.genomes.fasta; --n_genomes (no --draft)
    # --device_fasta: the records are places in the file (fasta.FastaSeq), indexed on device 0 in a session of its own
    device_fasta = bool(getattr(args, "device_fasta", False)) or os.environ.get("ISS_DEVICE_FASTA", "") == "1"
    if device_fasta and any(getattr(args, flag, None) for flag in ("report", "depth", "depth_bin", "error_report")):
        from .tensors import _torch

        _torch()  # (those flags work on torch tensors later in this process: torch's HIP runtime has to be its first)
    genome_file, records = drafts.load_genomes(args.genomes, args.draft, args.output, args.n_genomes,
                                               **({"device_fasta": True} if device_fasta else {}))
    if not records:
        logger.error("Genome(s) file seems empty: %s" % genome_file)
        sys.exit(1)
    variants_spec = None
    if getattr(args, "variants", None):  # the genome the reads are cut from changes here: every length below is a haplotype's
        records = _load_variants(args, records)
        variants_spec = (args.variants, args.variants_haplotype)
    readcount_dic, abundance_dic, n_reads = load_readcount_or_abundance(args, records, error_model)
    workers = args.gpus
    report = bool(getattr(args, "report", False))
    origins = bool(getattr(args, "origins", False))
    error_report = bool(getattr(args, "error_report", False))
    # --bgzip: the .vcf and the origins text leave the GPU as BGZF members; the parent frames the workers' members (bgzf.py)
    bgzip = bool(getattr(args, "bgzip", False))
    if bgzip and not (args.store_mutations or origins):
        logger.warning("--bgzip has no effect without --store_mutations or --origins")
        bgzip = False
    depth_bin = int(getattr(args, "depth_bin", None) or 0)
    if depth_bin < 0:
        logger.error("--depth_bin must be positive")
        sys.exit(1)
    depth = bool(getattr(args, "depth", False)) or depth_bin > 0  # (--depth_bin implies --depth)
    # --compress: the workers' FASTQ files already hold gzip members built on the device (one per batch); concatenated
    # they are the .gz files util.compress would have made from the text (iss/util.py:255-268), which never exists
    # --ubam: the workers write BGZF record blocks (one .bam stream instead of the two FASTQ files); --compress then applies to the .vcf only
    device_gzip = bool(args.compress) and not ubam and os.environ.get("ISS_HOST_FASTQ", "") != "1"
    gz = {"_R1.fastq": "_R1.fastq.gz", "_R2.fastq": "_R2.fastq.gz"} if device_gzip else None
    chunk_size = -((n_reads // 2) // -workers)  # ceildiv, app.py:82
    chunks = list(generate_work_divider(records, readcount_dic, abundance_dic, n_reads, args.coverage, args.coverage_file,
                                        error_model, args.output, chunk_size))
    jobs = []
    ordinal_of = {id(r): i for i, r in enumerate(records)}
    for rank, chunk in enumerate(chunks[:workers]):  # zip(work_chunks, temp_file_list), app.py:104
        spec = [(ordinal_of[id(rec)], n) for rec, n, _ in chunk]
        jobs.append((rank, rank % max(args.devices, 1), genome_file, spec, error_model.npz_path, args.seed,
                     temp_prefix(args.output, rank), args.sequence_type, args.gc_bias, args.rng, args.store_mutations,
                     (args.fragment_length, args.fragment_length_sd), device_gzip, args.mode, report, depth))
    t_gen = time.perf_counter()
    in_place = None
    if workers == 1:
        for j in jobs:
            _worker(*j, records=records, ubam=ubam, origins=origins, bgzip=bgzip, **({"error_report": True} if error_report else {}))
    elif _worker_set_wanted(args, report, depth):
        in_place = _run_worker_set(jobs, records, error_model, args, device_gzip, workers)
        if in_place is not None:
            logger.info("%d workers side by side on one device (%s)" % (workers, "final files" if in_place else "temporary files"))
    if workers > 1 and in_place is None:  # one process per worker (and what the set could not take)
        with mp.get_context("spawn").Pool(workers) as pool:
            if device_fasta:  # (the workers index the file again, each on its device)
                pool.starmap(_worker, [j + (None, ubam, origins, bgzip, error_report, variants_spec, True) for j in jobs])
            elif variants_spec is not None:  # (the workers read the records again: the VCF too)
                pool.starmap(_worker, [j + (None, ubam, origins, bgzip, error_report, variants_spec) for j in jobs])
            elif error_report:
                pool.starmap(_worker, [j + (None, ubam, origins, bgzip, True) for j in jobs])
            else:
                pool.starmap(_worker, [j + (None, ubam, origins, bgzip) for j in jobs] if ubam or origins or bgzip else jobs)
    t_cat = time.perf_counter()
    # the side-by-side worker set keeps its text VCF route (one text job split over the workers' files): host BGZF further down
    bgzip_vcf_device = bgzip and bool(args.store_mutations) and in_place is None
    if bgzip_vcf_device:  # the header as a member of its own, the workers' members in worker order, the EOF block
        from . import bgzf

        bgzf.assemble(args.output + ".vcf.gz", ["%s.vcf" % temp_prefix(args.output, rank) for rank in range(workers)],
                      header=(VCF_HEADER + "\n").encode())
    cat_vcf = bool(args.store_mutations) and not bgzip_vcf_device
    if ubam:  # header, the workers' record blocks in worker order, the EOF block; a worker without a chunk is an error as below
        from .ubam import assemble

        assemble(args.output + ".bam", ["%s.bam" % temp_prefix(args.output, rank) for rank in range(workers)])
        if cat_vcf:
            concatenate_rank_files(args.output, workers, suffixes=(".vcf",), headers={".vcf": VCF_HEADER})
        else:
            concatenate_rank_files(args.output, workers, suffixes=())  # (removes the workers' empty .vcf files)
    elif in_place:
        if cat_vcf:  # the FASTQ files are final; a VCF's size is not arithmetic: the workers' .vcf behind the header
            concatenate_rank_files(args.output, workers, suffixes=(".vcf",), headers={".vcf": VCF_HEADER})
    elif cat_vcf:  # app.py:128-133
        concatenate_rank_files(args.output, workers, suffixes=("_R1.fastq", "_R2.fastq", ".vcf"),
                               headers={".vcf": VCF_HEADER}, out_suffixes=gz)
    else:
        concatenate_rank_files(args.output, workers, out_suffixes=gz)  # raises if a worker had no chunk (util.py:233)
    if origins and bgzip:  # the workers' members in worker order, the EOF block (no pairs at all: the EOF block alone)
        from . import bgzf

        bgzf.assemble(args.output + ORIGINS_SUFFIX + ".gz", [temp_prefix(args.output, rank) + ORIGINS_SUFFIX for rank in range(workers)])
    elif origins:  # the workers' lines in worker order, like their FASTQ files
        concatenate_rank_files(args.output, workers, suffixes=(ORIGINS_SUFFIX,))
    if bgzip and cat_vcf:  # (the worker set's text: the same container, compressed on host threads)
        from . import bgzf

        bgzf.compress_file(args.output + ".vcf")
    logger.info("Workers %.2f s, concatenation of their files %.2f s" % (t_cat - t_gen, time.perf_counter() - t_cat))
    if report:
        _write_report(args.output, len(jobs), error_model.read_length)
    if error_report:
        dropped = _write_errors(args.output, len(jobs), error_model.read_length, report)
        if dropped:  # (cannot happen: a call that overflows its row slots is repeated before it is tallied)
            logger.error("--error_report: %d generate calls overflowed their mutation row slots and were not tallied" % dropped)
            sys.exit(1)
    if depth:
        _write_depth(args.output, len(jobs), records, depth_bin)
    os.remove(genome_file)
    if args.compress:  # util.compress (iss/util.py:255-268): <file>.gz next to the file, original removed
        for suffix in (() if device_gzip or ubam else ("_R1.fastq", "_R2.fastq")) + ((".vcf",) if args.store_mutations and not bgzip else ()):
            compress_file(args.output + suffix)
        if origins and not bgzip:
            compress_file(args.output + ORIGINS_SUFFIX)
    logger.info("Read generation complete")


def model_from_bam(args):
    """`model` (iss/app.py:147-169): errors are one line on stderr and exit status 1."""
    from ._native import EngineError, NativeLibraryError
    from .bam import BamError
    from .modeller import to_model

    logging.basicConfig(level=logging.ERROR if args.quiet else logging.DEBUG if args.debug else logging.INFO)
    logger = logging.getLogger(__name__)
    try:
        timings = {}
        logger.info("Starting model: %s" % args.bam)
        path = to_model(args.bam, args.output, seed=args.seed, device=args.device, dense=args.dense, timings=timings,
                        device_inflate=True if args.device_inflate else None)
        logger.debug("seconds: %s" % ", ".join("%s %.3f" % kv for kv in sorted(timings.items())))
        logger.info("Model written to %s" % path)
    except (BamError, EngineError, NativeLibraryError, OSError) as e:
        sys.stderr.write("ERROR: %s: %s\n" % (args.bam, str(e).splitlines()[0] if str(e) else type(e).__name__))
        return 1
    return 0


def _report_fail(message):
    sys.stderr.write("ERROR: %s\n" % message)
    return 1


def _report_against(args):
    """--against of `report`: (the other tally's words or None, its read length, an error message or None); read before the GPU
    is opened."""
    import numpy as np

    from . import fastq_report

    if not args.against:
        return None, None, None
    try:
        other = np.load(args.against, allow_pickle=False)
    except (OSError, ValueError) as e:
        return None, None, "%s: %s" % (args.against, str(e).splitlines()[0] if str(e) else type(e).__name__)
    other_length = fastq_report.read_length_of_words(other.size) if other.ndim == 1 else None
    if other_length is None:
        return None, None, ("%s: %s words fit no read length (a tally of read length L has %s words)"
                            % (args.against, "x".join(str(n) for n in other.shape), "200 L + 2239"))
    return other, other_length, None


def _report_write(args, res, other, other_length, more=None):
    """The files of `report` from a result (fastq_report.finish's keys); ``more``: further keys of <prefix>_report.json."""
    import json

    import numpy as np

    from . import fastq_report, tally

    L = res["read_length"]
    np.save(args.output + "_tally.npy", res["tally"])
    np.save(args.output + "_lengths.npy", res["lengths"])
    report = tally.report_dict(res["tally"], L)
    report["read_length_histogram"] = [tally._trim(res["lengths"][m]) for m in range(2)]
    report.update(more or {})
    with open(args.output + "_report.json", "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    if other is not None:
        with open(args.output + "_compare.json", "w") as fh:
            json.dump(fastq_report.compare_tallies(res["tally"], L, other, other_length), fh, indent=1)
            fh.write("\n")


def report_from_fastq(args):
    """`report`: the --report tallies of existing FASTQ files, or with --bam of the reads of a BAM file, built on the GPU
    (fastq_report.py, bam_report.py); errors are one line on stderr and exit status 1."""
    import zlib

    from . import fastq_report
    from ._native import FQ_REC_ERRORS, EngineError, NativeLibraryError
    from .inflate import InflateError

    logging.basicConfig(level=logging.ERROR if args.quiet else logging.INFO)
    logger = logging.getLogger(__name__)
    fail = _report_fail
    bam = getattr(args, "bam", None)
    if bool(args.read1) == bool(bam):
        return fail("report takes exactly one of -1 R1.fastq and --bam reads.bam")
    if getattr(args, "errors", False) and not bam:
        return fail("report --errors reads the alignments of a BAM file: it goes with --bam")
    if getattr(args, "against_errors", None) and not getattr(args, "errors", False):
        return fail("report --against_errors compares the --errors tally: add --errors")
    if _report_depth_wanted(args) and not bam:
        return fail("report --depth reads the alignments of a BAM file: it goes with --bam")
    if bam:
        if args.read2:
            return fail("report --bam takes no -2: the mates of a BAM file are told apart by their flags")
        return _report_from_bam(args, logger)

    try:
        other, other_length, message = _report_against(args)  # (before the GPU is opened)
        if message:
            return fail(message)
        files = [args.read1] + ([args.read2] if args.read2 else [])
        t0 = time.perf_counter()
        with fastq_report.FastqTally(args.device, args.max_length) as dev:
            for mate, path in enumerate(files):
                logger.info("Tallying %s" % path)
                dev.feed_file(path, mate)
            res = dev.result()
        logger.info("%s records in %.2f s" % (" + ".join(str(n) for n in res["records"][:len(files)]), time.perf_counter() - t0))
        for mate, path in enumerate(files):
            if res["bad_record"][mate] >= 0:
                code = res["bad_code"][mate]
                return fail("%s: record %d: %s" % (path, res["bad_record"][mate], FQ_REC_ERRORS.get(code, "error %d" % code)))
        if args.read2 and res["records"][0] != res["records"][1]:
            return fail("%s holds %d records and %s holds %d: not the two files of one run"
                        % (args.read1, res["records"][0], args.read2, res["records"][1]))
        _report_write(args, res, other, other_length)
    except InflateError as e:  # (a BGZF member that does not inflate on the device: the message names the file)
        return fail(str(e).splitlines()[0])
    except (EngineError, NativeLibraryError, OSError, EOFError, ValueError, zlib.error) as e:  # (a broken .gz: the last two)
        return fail("%s: %s" % (args.read1, str(e).splitlines()[0] if str(e) else type(e).__name__))
    return 0


def _report_against_errors(args, other, other_length):
    """--against_errors of `report --bam --errors`: (the other error tally's words, its read length, its bases [2][L][94] or None,
    an error message or None); read before the GPU is opened.  The bases: the ``qual`` field of the --against tally when that is
    given (it has to be of the error tally's read length), else OTHER_errbases.npy beside the file when it exists, else None (``pairs`` then)."""
    import numpy as np

    from . import errtally, tally

    path = args.against_errors
    try:
        words = np.load(path, allow_pickle=False)
    except (OSError, ValueError) as e:
        return None, None, None, "%s: %s" % (path, str(e).splitlines()[0] if str(e) else type(e).__name__)
    L, rest = divmod(int(words.size) - 386, 258) if words.ndim == 1 else (0, 1)
    if rest or L < 1 or errtally.words(L) != words.size:
        return None, None, None, ("%s: %s words fit no read length (an error tally of read length L has 258 L + 386 words)"
                                  % (path, "x".join(str(n) for n in words.shape)))
    bases = None
    if other is not None:
        if other_length != L:
            return None, None, None, "%s is of read length %d and %s of read length %d: not one run's" % (args.against, other_length, path, L)
        bases = np.array(tally.split_tally(np.asarray(other, dtype=np.uint64), L)["qual"])
    else:
        beside = path[:-len("_errtally.npy")] + "_errbases.npy" if path.endswith("_errtally.npy") else None
        if beside and os.path.exists(beside):
            try:
                bases = np.load(beside, allow_pickle=False)
            except (OSError, ValueError) as e:
                return None, None, None, "%s: %s" % (beside, str(e).splitlines()[0] if str(e) else type(e).__name__)
            if bases.shape != (2, L, errtally.PHREDS):
                return None, None, None, "%s: shape %r does not go with read length %d" % (beside, tuple(bases.shape), L)
    return words, L, bases, None


def _report_write_errors(args, res, against):
    """The files of --errors from a result with errors (BamReadTally.result()); ``against``: _report_against_errors' first three."""
    import json

    import numpy as np

    from . import bam_errors

    L = res["read_length"]
    err, bases = bam_errors.errors_and_bases(res["errors"], L)
    np.save(args.output + "_errtally.npy", err)
    np.save(args.output + "_errbases.npy", bases)
    report = bam_errors.report_dict(res["errors"], L, res["error_counts"])
    report["bad_alignment"] = {"record": int(res["bad_alignment"]), "code": int(res["bad_alignment_code"])}
    with open(args.output + "_errors.json", "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    if against[0] is not None:
        with open(args.output + "_errors_compare.json", "w") as fh:
            json.dump(bam_errors.compare_errors(err, bases, L, against[0], against[2], against[1]), fh, indent=1)
            fh.write("\n")


def _report_depth_wanted(args):
    """--depth of `report`, or one of the flags that imply it (--depth_bin) or only make sense with it."""
    return bool(getattr(args, "depth", False)) or getattr(args, "depth_bin", None) is not None \
        or bool(getattr(args, "depth_deletions", False)) or getattr(args, "min_mapq", None) is not None \
        or bool(getattr(args, "against_depth", None))


def _report_write_depth(args, dres, bin, other):
    """The files of --depth from BamReadTally.depth_result(): <prefix>_depth.txt and, with a bin, <prefix>_depth.bedgraph -- byte
    compatible with `generate --depth`'s --, <prefix>_coverage.txt for `generate --coverage_file` and, with ``other`` (a
    bam_depth.read_depth_table dict), <prefix>_depth_compare.json."""
    import json

    from . import bam_depth
    from . import depth as D

    rows = D.depth_rows(dres["stats"], dres["table"], dres["ids"])
    D.write_depth_table(args.output + "_depth.txt", rows)
    if bin > 0:
        D.write_bedgraph(args.output + "_depth.bedgraph", dres["bins"], dres["table"], dres["ids"], bin)
    bam_depth.write_coverage_file(args.output + "_coverage.txt", bam_depth.coverage_rows(dres["stats"], dres["table"], dres["ids"]))
    if other is not None:
        mine = {row[0]: tuple(row[1:]) for row in rows}
        with open(args.output + "_depth_compare.json", "w") as fh:
            json.dump(bam_depth.compare_depth_tables(mine, other), fh, indent=1)
            fh.write("\n")


def _report_from_bam(args, logger):
    """`report --bam`: the reads of a BAM file, insert sizes included (bam_report.py).  The BGZF blocks are inflated in the host
    pool unless --device_inflate or ISS_DEVICE_INFLATE=1 asks for the device; ISS_HOST_INFLATE=1 wins over both.  With --errors
    also the alignments' errors (bam_errors.py), with --depth the coverage depth of the references (bam_depth.py)."""
    from . import bam_depth, bam_report
    from ._native import BR_ALN_ERRORS, BR_DEPTH_ERRORS, BR_REC_ERRORS, EngineError, NativeLibraryError
    from .bam import BamError
    from .inflate import InflateError
    from .modeller import device_inflater

    fail = _report_fail
    try:
        other, other_length, message = _report_against(args)  # (before the GPU is opened)
        if message:
            return fail(message)
        errors = bool(getattr(args, "errors", False))
        against = (None, None, None)
        if errors and args.against_errors:
            *against, message = _report_against_errors(args, other, other_length)
            if message:
                return fail(message)
        more = {"errors": True} if errors else {}  # (without the flags: the call as it was)
        depth, depth_bin, other_depth = _report_depth_wanted(args), int(getattr(args, "depth_bin", None) or 0), None
        if depth:
            min_mapq = int(getattr(args, "min_mapq", None) or 0)
            if getattr(args, "depth_bin", None) is not None and depth_bin < 1:
                return fail("--depth_bin must be positive")
            if not 0 <= min_mapq <= 255:
                return fail("--min_mapq outside 0 .. 255")
            if getattr(args, "against_depth", None):
                try:
                    other_depth = bam_depth.read_depth_table(args.against_depth)  # (before the GPU is opened)
                except (OSError, ValueError) as e:
                    return fail("%s: %s" % (args.against_depth, str(e).splitlines()[0] if str(e) else type(e).__name__))
            more.update(depth=True, depth_flags=bam_depth.COUNT_DEL if getattr(args, "depth_deletions", False) else 0, min_mapq=min_mapq)
        t0 = time.perf_counter()
        with bam_report.BamReadTally(args.device, args.max_length, **more) as dev, \
                device_inflater(args.device, True if args.device_inflate else None) as inflater:
            logger.info("Tallying %s" % args.bam)
            dev.feed_file(args.bam, inflater)
            res = dev.result()
            dres = dev.depth_result(depth_bin) if depth else None
        logger.info("%d + %d records in %.2f s" % (res["records"][0], res["records"][1], time.perf_counter() - t0))
        if res["bad_record"] >= 0:
            code = res["bad_code"]
            return fail("%s: record %d: %s" % (args.bam, res["bad_record"], BR_REC_ERRORS.get(code, "error %d" % code)))
        if res["records"][1] and res["records"][0] != res["records"][1]:  # (a filtered BAM: normal)
            logger.warning("%s holds %d first and %d second reads" % (args.bam, res["records"][0], res["records"][1]))
        keys = {"records_skipped": {"secondary_or_supplementary": int(res["skipped"][0]), "mate_flags": int(res["skipped"][1])}}
        if depth:
            keys["depth"] = bam_depth.counts_dict(dres["depth_counts"])
            keys["depth"]["bad_record"] = {"record": int(dres["bad_depth_record"]), "code": int(dres["bad_depth_code"])}
        _report_write(args, res, other, other_length, keys)
        if depth:
            if dres["bad_depth_record"] >= 0:  # (one odd record must not cost the user the report)
                code = dres["bad_depth_code"]
                logger.warning("%s: record %d: %s (%d records are in neither the depth nor its counts)"
                               % (args.bam, dres["bad_depth_record"], BR_DEPTH_ERRORS.get(code, "error %d" % code),
                                  res["records"][0] + res["records"][1] - sum(dres["depth_counts"][:5])))
            _report_write_depth(args, dres, depth_bin, other_depth)
        if errors:
            if res["bad_alignment"] >= 0:  # (one odd record must not cost the user the report: the counts are in the json)
                code = res["bad_alignment_code"]
                logger.warning("%s: record %d: %s (%d such records are not in the error tally)"
                               % (args.bam, res["bad_alignment"], BR_ALN_ERRORS.get(code, "error %d" % code),
                                  int(res["errors"][0])))
            if not sum(res["error_counts"][:2]) and res["error_counts"][3]:
                return fail("%s: its aligned records have no MD tags; add them with `samtools calmd -b reads.bam ref.fasta`" % args.bam)
            _report_write_errors(args, res, against)
    except InflateError as e:  # (the message names the file)
        return fail(str(e).splitlines()[0])
    except (BamError, EngineError, NativeLibraryError, OSError) as e:
        return fail("%s: %s" % (args.bam, str(e).splitlines()[0] if str(e) else type(e).__name__))
    return 0


def build_parser():
    p = argparse.ArgumentParser(prog="insilicoseq_amd", description="iss generate on MI355X")
    sub = p.add_subparsers(dest="cmd")
    g = sub.add_parser("generate")
    g.add_argument("--genomes", "-g", nargs="+")
    g.add_argument("--draft", nargs="+", metavar="<draft.fasta>", help="draft genome(s): the contigs of a file are one genome")
    g.add_argument("--n_genomes", "-u", type=int, metavar="<int>",
                   help="take this many random records from the --genomes input (ignored with --draft)")
    g.add_argument("--model", "-m")
    g.add_argument("--mode", "-e", default="kde", choices=["kde", "basic", "perfect"])
    g.add_argument("--n_reads", "-n", default="1000000")
    g.add_argument("--seed", type=int, default=None)
    g.add_argument("--gpus", "--cpus", "-p", type=int, default=1, dest="gpus", help="workers (one per GPU)")
    g.add_argument("--devices", type=int, default=0, help="visible GPUs (default: one per worker)")
    g.add_argument("--abundance", "-a", default="lognormal", choices=sorted(ABUNDANCE))
    g.add_argument("--abundance_file", "-b")
    g.add_argument("--coverage", "-C", default=None, choices=sorted(ABUNDANCE))
    g.add_argument("--coverage_file", "-D")
    g.add_argument("--readcount_file", "-R")
    g.add_argument("--gc_bias", "-c", action="store_true")
    g.add_argument("--sequence_type", "-t", default="metagenomics", choices=["metagenomics", "amplicon"])
    g.add_argument("--fragment-length", "-l", type=int, default=None, dest="fragment_length")
    g.add_argument("--fragment-length-sd", "-s", type=int, default=None, dest="fragment_length_sd")
    g.add_argument("--store_mutations", "-M", action="store_true")
    g.add_argument("--compress", "-z", action="store_true")
    g.add_argument("--rng", default="philox", choices=["philox", "mt"],
                   help="philox: parallel counter-based streams (default); mt: the reference's Mersenne-Twister "
                        "streams consumed sequentially on the GPU -- output identical to `iss generate` for the same --seed")
    g.add_argument("--report", action="store_true",
                   help="tally the reads on the GPU as they are generated and write <output>_report.json (per-position quality "
                        "profile, base composition, GC, mean-quality and insert-size histograms) and <output>_tally.npy (the raw "
                        "counters) next to the FASTQ files; with --rng mt --devices 1 the workers then run as one process each "
                        "instead of side by side in one context (same files, byte for byte)")
    g.add_argument("--error_report", action="store_true",
                   help="with --store_mutations: tally the mutation rows on the GPU as they are made and write <output>_errors.json "
                        "(substitution, insertion and deletion rates per position, the substitution matrix, substitutions by phred, "
                        "events per read; with --report also the phred calibration) and <output>_errtally.npy (the raw counters); "
                        "like --report it makes --rng mt --devices 1 run one process per worker (same files, byte for byte)")
    g.add_argument("--depth", action="store_true",
                   help="mark where the reads fall on the GPU as they are generated and write <output>_depth.txt: per record, in "
                        "FASTA order, id, length, mean_depth, depth_variance, covered_fraction, max_depth of the nominal per-base "
                        "depth (the template intervals the reads were cut from); like --report it makes --rng mt --devices 1 run "
                        "one process per worker (same files, byte for byte)")
    g.add_argument("--depth_bin", type=int, default=None, metavar="N",
                   help="with --depth (implied): also <output>_depth.bedgraph, the mean depth of every N-base window of every record")
    g.add_argument("--ubam", action="store_true",
                   help="write <output>.bam instead of the two FASTQ files: unaligned BAM (flags 77 / 141, R1 then R2 of every pair, "
                        "names without /1 and /2, lower-case bases as their capitals), records and BGZF blocks built on the GPU; "
                        "--compress then applies to the .vcf only; not with the side-by-side workers of --rng mt --cpus W --devices 1")
    g.add_argument("--origins", action="store_true",
                   help="also write <output>_origins.bedpe: one BEDPE line per pair, in FASTQ order, with the record and the two nominal "
                        "template intervals its reads were cut from (read 1 '+', read 2 '-', the name without /1 and /2, the insert "
                        "size as the eleventh column), text built on the GPU; --compress gzips it; like --report it makes --rng mt "
                        "--devices 1 run one process per worker (same FASTQ and VCF files, byte for byte)")
    g.add_argument("--bgzip", action="store_true",
                   help="write the --store_mutations VCF as <output>.vcf.gz and the --origins text as <output>_origins.bedpe.gz: BGZF "
                        "(blocked gzip: gzip.open, zcat and htslib read it), compressed on the GPU with copies from the line above, so "
                        "the text never reaches the host; the FASTQ files are not affected (--compress and --ubam work beside it, and "
                        "with both --compress and --bgzip these two files take this route); with the side-by-side workers of --rng mt "
                        "--cpus W --devices 1 the .vcf is compressed into the same container on host threads")
    g.add_argument("--variants", default=None, metavar="v.vcf[.gz]",
                   help="splice the alleles of a VCF into the records on the GPU before any read is cut: SNVs, substitutions, insertions "
                        "and deletions (symbolic alleles, '*', breakends and lines of other records are skipped and counted); the run "
                        "writes exactly what it would write for the haplotype given as FASTA, every coordinate in haplotype "
                        "coordinates, plus <output>_variants.json (lengths and counts per record) and <output>_haplotype.chain "
                        "(haplotype -> record); the first ALT of every line unless --variants_haplotype is given")
    g.add_argument("--variants_haplotype", type=int, default=None, choices=[1, 2],
                   help="with --variants: apply the allele the first sample's GT names for this haplotype (0 and '.': the line is "
                        "skipped; an unphased heterozygous GT is an error)")
    g.add_argument("--write_haplotype", action="store_true",
                   help="with --variants: also write <output>_haplotype.fasta, the records as the reads see them, downloaded from the GPU")
    g.add_argument("--device_fasta", action="store_true",
                   help="index the genome FASTA on the GPU and upload the records as they stand in the file, their line ends removed "
                        "there, instead of parsing it on the host (also: ISS_DEVICE_FASTA=1); the output is the same.  Gzip-compressed "
                        "--genomes / --draft files are taken either way; with this flag or ISS_DEVICE_INFLATE=1 a BGZF file is inflated "
                        "on the GPU (ISS_HOST_INFLATE=1 keeps gzip on the host)")
    g.add_argument("--output", "-o", required=True)
    g.add_argument("--quiet", "-q", action="store_true")
    m = sub.add_parser("model", help="build a KDE error model from a BAM file (iss model)")
    m.add_argument("--bam", "-b", required=True,
                   help="aligned reads (BAM with MD tags); no index needed")
    m.add_argument("--device_inflate", action="store_true",
                   help="inflate the BAM's BGZF blocks on the GPU instead of in the pool of host threads (also: ISS_DEVICE_INFLATE=1; "
                        "the host pool is the default because it is the faster route end to end, DESIGN.md section 27)")
    m.add_argument("--output", "-o", required=True, help="output prefix: writes <prefix>.npz")
    m.add_argument("--quiet", "-q", action="store_true")
    m.add_argument("--debug", "-d", action="store_true")
    m.add_argument("--seed", type=int, default=0, help="Philox key of the subsample (more than 1 000 000 mapped records)")
    m.add_argument("--device", type=int, default=0, help="GPU ordinal")
    m.add_argument("--dense", action="store_true", help="also write <prefix>.dense.npz (this project's pickle-free form)")
    r = sub.add_parser("report", help="the --report tallies of existing FASTQ files, or of the reads of a BAM file, built on the GPU; "
                                      "--against compares them with another tally")
    r.add_argument("--read1", "-1", default=None, metavar="R1.fastq[.gz]",
                   help="the first reads; a .gz written by bgzip (BGZF) is inflated on the GPU, any other gzip on the host "
                        "(exactly one of -1 and --bam)")
    r.add_argument("--bam", default=None, metavar="reads.bam",
                   help="the reads of a BAM file instead of FASTQ files, aligned or not (generate --ubam): each read as sequenced "
                        "(reverse-strand records turned back), mates by their flags, secondary and supplementary records skipped, "
                        "and the insert-size histogram from the template lengths of the aligned pairs; no index needed")
    r.add_argument("--device_inflate", action="store_true",
                   help="with --bam: inflate the BGZF blocks on the GPU instead of in the pool of host threads (also: "
                        "ISS_DEVICE_INFLATE=1; ISS_HOST_INFLATE=1 keeps the host pool)")
    r.add_argument("--read2", "-2", default=None, metavar="R2.fastq[.gz]", help="the second reads (without it mate 2's fields are zero)")
    r.add_argument("--output", "-o", required=True,
                   help="output prefix: writes <prefix>_tally.npy (the counters, in the layout of generate --report at the longest "
                        "read seen), <prefix>_report.json and <prefix>_lengths.npy (reads per mate and length)")
    r.add_argument("--against", default=None, metavar="OTHER_tally.npy",
                   help="also write <prefix>_compare.json: these reads against another tally (of generate --report, or of report)")
    r.add_argument("--errors", action="store_true",
                   help="with --bam: also tally the alignments' errors as CIGAR and MD tell them, on the GPU -- <prefix>_errtally.npy "
                        "(the counters, in the layout of generate --error_report), <prefix>_errbases.npy (aligned bases per mate, "
                        "position and phred: the denominators) and <prefix>_errors.json (rates per aligned base, substitution matrix, "
                        "indels, errors per read, phred calibration); the BAM needs MD tags (samtools calmd)")
    r.add_argument("--against_errors", default=None, metavar="OTHER_errtally.npy",
                   help="with --errors: also write <prefix>_errors_compare.json, these errors against another error tally (of generate "
                        "--error_report, or of report --bam --errors); the other side's denominators come from --against "
                        "OTHER_tally.npy when given, else from OTHER_errbases.npy beside the file, else its pairs")
    r.add_argument("--depth", action="store_true",
                   help="with --bam: also mark where the alignments fall on the references, on the GPU, as their CIGARs tell it -- "
                        "<prefix>_depth.txt (per reference of the header: id, length, mean_depth, depth_variance, covered_fraction, "
                        "max_depth; the file generate --depth writes), <prefix>_coverage.txt (id and mean depth: what generate "
                        "--coverage_file reads) and the counts under `depth` in <prefix>_report.json.  Counted: the records the "
                        "tally takes that are aligned, with 0x200 and 0x400 clear (samtools depth's default filter; supplementary "
                        "records are skipped anyway); M, = and X cover, N never does")
    r.add_argument("--depth_bin", type=int, default=None, metavar="N",
                   help="with --depth (implied): also <prefix>_depth.bedgraph, the mean depth of every N-base window of every reference")
    r.add_argument("--depth_deletions", action="store_true", help="with --depth (implied): the bases of a D count as covered too")
    r.add_argument("--min_mapq", type=int, default=None, metavar="Q",
                   help="with --depth (implied): leave out the records whose mapping quality is below Q (0 .. 255, default 0)")
    r.add_argument("--against_depth", default=None, metavar="OTHER_depth.txt",
                   help="with --depth (implied): also write <prefix>_depth_compare.json, this depth table against another (of generate "
                        "--depth, or of report --bam --depth): per id the differences of mean depth and covered fraction, their "
                        "maxima, the total-variation distance of the normalised mean depths, the ids only one side has")
    r.add_argument("--max_length", type=int, default=1024, metavar="N", help="longest read taken (1 .. 1024, default 1024)")
    r.add_argument("--device", type=int, default=0, help="GPU ordinal")
    r.add_argument("--quiet", "-q", action="store_true")
    return p


def main(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if args.cmd == "model":
        return model_from_bam(args)
    if args.cmd == "report":
        return report_from_fastq(args)
    if args.cmd != "generate":
        p.print_help()
        return 1
    if not args.devices:
        args.devices = args.gpus
    logging.basicConfig(level=logging.ERROR if args.quiet else logging.INFO)
    generate_reads(args)
    return 0
