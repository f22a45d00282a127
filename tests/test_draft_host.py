"""`generate --draft` / `--n_genomes` on the host: the abundance / coverage expansion of draft assemblies and the files it
writes (iss/abundance.py:254-317, iss/generator.py:497-594) against the reference's own runs, the work divider on the expanded
values, the complete-genome set, `--n_genomes`'s draw (iss/util.py:179-210) and the CLI's errors."""
import collections
import logging
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from helpers import GOLDEN
from insilicoseq_amd import app, drafts
from insilicoseq_amd.generator import generate_work_divider, parse_fasta

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(GOLDEN, "generate")
CASES = ["cpus1", "cpus2", "cpus3", "complete", "abundance_file", "coverage_file", "coverage_lognormal", "basic"]


def write_inputs(d):
    """The golden cases' input files (two drafts, one complete genome, the abundance / coverage files) into directory d."""
    z = np.load(os.path.join(GEN, "draft_inputs.npz"))
    for name in ("d1.fasta", "d2.fasta", "complete.fasta"):
        with open(os.path.join(d, name), "wb") as fh:
            fh.write(z[name.replace(".", "_")].tobytes())
    for name in ("abundance_file", "coverage_file"):
        with open(os.path.join(d, name + ".txt"), "wb") as fh:
            fh.write(z[name].tobytes())


def golden(case):
    z = np.load(os.path.join(GEN, "draft_%s.npz" % case))
    return {k: z[k] for k in z.files}


def parse_args(flags):
    """The generate command line of a golden case (its @files renamed as the tooling writes them)."""
    argv = ["generate", "-o", "out"] + [f[1:] + ".txt" if f.startswith("@") else f for f in flags]
    seen = {}
    orig = app.generate_reads
    try:
        app.generate_reads = lambda args: seen.setdefault("args", args)
        app.main(argv)
    finally:
        app.generate_reads = orig
    return seen["args"]


def host_run(case, tmp_path, monkeypatch):
    """The host half of `generate` for a golden case in tmp_path: error model (seeding numpy like the reference),
    genomes, abundances (files written).  Returns (args, error model, records, readcount dic, abundance dic, n_reads)."""
    write_inputs(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    args = parse_args(str(golden(case)["flags"]).split())
    em = app.load_error_model(args.mode, args.seed, args.model, args.fragment_length, args.fragment_length_sd,
                              args.store_mutations, args.rng)
    genome_file, records = drafts.load_genomes(args.genomes, args.draft, args.output, args.n_genomes)
    rc, ab, n_reads = app.load_readcount_or_abundance(args, records, em)
    os.remove(genome_file)
    return args, em, records, rc, ab, n_reads


@pytest.mark.parametrize("case", CASES)
def test_distribution_files_match_the_reference(case, tmp_path, monkeypatch):
    host_run(case, tmp_path, monkeypatch)
    g = golden(case)
    for key, suffix in (("abundance", "_abundance.txt"), ("coverage", "_coverage.txt")):
        path = tmp_path / ("out" + suffix)
        assert path.exists() == bool(g["has_" + key]), suffix
        if path.exists():
            assert path.read_bytes() == g[key].tobytes(), suffix


def fastq_pairs(r1):
    """(record id, worker) -> read pairs in a golden R1 file (read ids {record.id}_{i}_{cpu}/1)."""
    out = collections.Counter()
    lines = r1.tobytes().decode().split("\n")
    for head in lines[0::4]:
        if head:
            rid, _i, cpu = head[1:].rsplit("_", 2)
            out[(rid, int(cpu.split("/")[0]))] += 1
    return out


@pytest.mark.parametrize("case", CASES)
def test_work_divider_on_expanded_values(case, tmp_path, monkeypatch):
    args, em, records, rc, ab, n_reads = host_run(case, tmp_path, monkeypatch)
    chunk_size = -((n_reads // 2) // -args.gpus)
    chunks = list(generate_work_divider(records, rc, ab, n_reads, args.coverage, args.coverage_file, em, "out", chunk_size))
    got = collections.Counter()
    for k, chunk in enumerate(chunks[:args.gpus]):
        for rec, n, _mode in chunk:
            if em.read_length < len(rec.seq):  # (shorter records are skipped by the workers)
                got[(rec.id, k)] += n
    assert got == fastq_pairs(golden(case)["r1"])


def test_draft_expansion_by_length_and_repeated_ids(tmp_path, monkeypatch):
    write_inputs(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    d1, d2 = list(parse_fasta("d1.fasta")), list(parse_fasta("d2.fasta"))
    dic = drafts.expand_file_dic({"complete_1": 0.2, "d1.fasta": 0.5, "d2.fasta": 0.3}, ["d1.fasta", "d2.fasta"], "abundance")
    assert dic["complete_1"] == 0.2 and "d1.fasta" not in dic
    t1, t2 = sum(len(r.seq) for r in d1), sum(len(r.seq) for r in d2)
    for r in d1:
        if r.id not in {x.id for x in d2}:
            assert dic[r.id] == 0.5 * (len(r.seq) / t1)
    for r in d2:  # a repeated id keeps the later file's value
        assert dic[r.id] == 0.3 * (len(r.seq) / t2)
    assert {"NODE_1", "NODE_11"} <= {r.id for r in d1} & {r.id for r in d2}
    cov = drafts.expand_file_dic({"d1.fasta": 1.5, "d2.fasta": 2.25, "other": 3.0}, ["d1.fasta", "d2.fasta"], "coverage")
    assert cov["other"] == 3.0 and cov["NODE_1"] == 2.25 and cov["NODE_8_mixed"] == 1.5


def test_complete_genome_set_is_the_references_expression(tmp_path, monkeypatch):
    write_inputs(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    with open("more.fasta", "w") as fh:
        for k in range(7):
            fh.write(">genome_%d\n%s\n" % (k, "ACGT" * 50))
    draft = ["d1.fasta", "d2.fasta"]
    genomes = [r.id for r in parse_fasta("more.fasta")] + [r.id for d in draft for r in parse_fasta(d)]
    # abundance.draft (iss/abundance.py:266-271), evaluated here: the same set built from the same sequence
    draft_records = []
    for d in draft:
        draft_records.extend([record.id for record in parse_fasta(d)])
    expected = list(set(genomes) - set(draft_records))
    assert drafts.complete_genomes(genomes, draft) == expected
    assert sorted(expected) == ["genome_%d" % k for k in range(7)]
    seen = []
    drafts.draft_abundance(genomes, draft, lambda ids: seen.append(list(ids)) or {i: 1.0 for i in ids}, lambda d: None)
    assert seen == [expected + draft]


def test_reservoir_indices_with_an_injected_rng():
    for seed in range(50):
        total, n = 20, 1 + seed % 19
        got = drafts.reservoir_indices(total, n, random.Random(seed))
        assert len(got) == n and got == sorted(got) and len(set(got)) == n
        assert all(0 <= i < total - 1 for i in got)  # the last record is never chosen
        assert got == sorted(random.Random(seed).sample(range(0, total - 1), n))
    assert drafts.reservoir_indices(5, 4, random.Random(1)) == [0, 1, 2, 3]


def test_reservoir_n_not_below_total_exits(caplog):
    with caplog.at_level(logging.ERROR), pytest.raises(SystemExit) as e:
        drafts.reservoir_indices(4, 4, random.Random(0))
    assert e.value.code == 1
    assert "-u should be strictly smaller than total number of records." in caplog.text


def test_load_genomes_n_genomes(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with open("g.fasta", "w") as fh:
        for k in range(12):
            fh.write(">rec_%d desc %d\n%s\n" % (k, k, "ACGTTGCA" * (10 + k)))
    path, records = drafts.load_genomes(["g.fasta"], None, "out", 5, rng=random.Random(3))
    keep = sorted(random.Random(3).sample(range(0, 11), 5))
    assert [r.id for r in records] == ["rec_%d" % i for i in keep]
    assert [r.description for r in records] == ["rec_%d desc %d" % (i, i) for i in keep]
    assert [r.seq for r in records] == ["ACGTTGCA" * (10 + i) for i in keep]
    assert [r.id for r in parse_fasta(path)] == [r.id for r in records]  # the temp file holds only them (the workers re-read it)
    write_inputs(str(tmp_path))
    _path, all_recs = drafts.load_genomes(["g.fasta"], ["d1.fasta"], "out", 5, rng=random.Random(3))
    assert len(all_recs) == 12 + len(list(parse_fasta("d1.fasta")))  # ignored with --draft


def cli(tmp_path, *argv):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run([sys.executable, "-m", "insilicoseq_amd", "generate"] + list(argv), cwd=str(tmp_path), env=env,
                          capture_output=True, text=True, timeout=300)


def test_cli_readcount_file_with_draft_is_an_error(tmp_path):
    write_inputs(str(tmp_path))
    (tmp_path / "rc.txt").write_text("NODE_1\t10\n")
    p = cli(tmp_path, "--draft", "d1.fasta", "--readcount_file", "rc.txt", "--model", "hiseq", "-o", "out")
    assert p.returncode == 1, p.stderr
    assert "readcount_file is only supported using --genomes, not --draft" in p.stderr


def test_cli_n_genomes_too_large_is_an_error(tmp_path):
    write_inputs(str(tmp_path))
    n = len(list(parse_fasta(str(tmp_path / "d1.fasta"))))
    p = cli(tmp_path, "--genomes", "d1.fasta", "-u", str(n), "--model", "hiseq", "-o", "out")
    assert p.returncode == 1, p.stderr
    assert "-u should be strictly smaller than total number of records." in p.stderr


def test_cli_without_genome_input_names_every_source(tmp_path):
    p = cli(tmp_path, "--model", "hiseq", "-o", "out")
    assert p.returncode == 1, p.stderr
    assert "One of --genomes/-g, --draft, --ncbi/-k is required" in p.stderr
