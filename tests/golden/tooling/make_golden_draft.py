#!/usr/bin/env python3
"""Golden outputs of `iss generate --draft` (iss/generator.py:424-594, iss/abundance.py:254-317), captured by running the
reference like make_golden_cli.py does (same stand-in Bio package, a private copy of the reference).

Inputs: two seeded synthetic draft assemblies (40 contigs, about 60 kbp together) with contigs shorter than HiSeq's read
length of 125, one contig of lower-case and IUPAC letters, and contig ids that appear in both files; one complete genome.
Every run has the work directory as its cwd and names the drafts by relative paths, so `_abundance.txt` (which names the
draft files as given) is reproducible.

Outputs: tests/golden/generate/draft_inputs.npz (the FASTA files and the abundance / coverage files given) and
tests/golden/generate/draft_<case>.npz (R1, R2, _abundance.txt, _coverage.txt of each run, its flags).

Usage:  python tests/golden/tooling/make_golden_draft.py   (from the repo root, build container only)
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
SHIM = os.path.join(HERE, "bio_shim")
REF = "/root/reference"


def synth_inputs(seed=2024):
    """{file name: FASTA bytes} of the two drafts and the complete genome."""
    rng = np.random.RandomState(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)

    def seq(n):
        return letters[rng.randint(0, 4, size=n)].tobytes().decode()

    def fasta(recs):
        return "".join(">%s\n%s\n" % (rid, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))) for rid, s in recs).encode()

    d1 = []
    for k in range(22):
        n = int(np.exp(rng.uniform(np.log(300), np.log(4500))))
        d1.append(("NODE_%d_length_%d" % (k + 1, n) if k % 5 else "NODE_%d" % (k + 1), seq(n)))
    d1[4] = ("NODE_5_short", seq(90))   # shorter than the read length: skipped with warnings
    d1[11] = ("NODE_12_short", seq(124))
    mixed = list(seq(1800))
    for i in range(200, 420):
        mixed[i] = mixed[i].lower()
    for i, c in zip(range(900, 1500, 37), "NRYKMSWBDHVnry"):
        mixed[i] = c
    d1[7] = ("NODE_8_mixed", "".join(mixed))
    d2 = []
    for k in range(18):
        n = int(np.exp(rng.uniform(np.log(300), np.log(4500))))
        d2.append(("contig_%d" % (k + 1), seq(n)))
    d2[3] = ("contig_4_short", seq(60))
    d2[9] = ("NODE_1", seq(2100))   # ids of d1 again: the later file's value wins for every record of that id
    d2[14] = ("NODE_11", seq(1300))
    complete = [("complete_1 a complete genome", seq(6000))]
    return {"d1.fasta": fasta(d1), "d2.fasta": fasta(d2), "complete.fasta": fasta(complete)}


GIVEN = {
    "abundance_file": "complete_1\t0.2\nd1.fasta\t0.5\nd2.fasta\t0.3\n",
    "coverage_file": "d1.fasta\t1.5\nd2.fasta\t2.25\n",
}
BASE = ["--model", "hiseq", "--seed", "42"]
CASES = {
    "cpus1": ["--draft", "d1.fasta", "d2.fasta", "-n", "1000", "--cpus", "1"],
    "cpus2": ["--draft", "d1.fasta", "d2.fasta", "-n", "1000", "--cpus", "2"],
    "cpus3": ["--draft", "d1.fasta", "d2.fasta", "-n", "1000", "--cpus", "3"],
    "complete": ["--genomes", "complete.fasta", "--draft", "d1.fasta", "d2.fasta", "-n", "1000", "--cpus", "2"],
    "abundance_file": ["--genomes", "complete.fasta", "--draft", "d1.fasta", "d2.fasta", "--abundance_file", "@abundance_file",
                       "-n", "1000", "--cpus", "2"],
    "coverage_file": ["--draft", "d1.fasta", "d2.fasta", "--coverage_file", "@coverage_file", "--cpus", "1"],
    "coverage_lognormal": ["--draft", "d1.fasta", "d2.fasta", "--coverage", "lognormal", "-n", "1000", "--cpus", "2"],
    "basic": ["--draft", "d1.fasta", "d2.fasta", "--mode", "basic", "-n", "1000", "--cpus", "2"],
}


def case_argv(flags):
    """The command line of a case: @name -> name.txt (written next to the drafts)."""
    return [f[1:] + ".txt" if f.startswith("@") else f for f in flags]


if __name__ == "__main__":
    work = tempfile.mkdtemp(prefix="iss_ref_")
    REFCOPY = os.path.join(work, "refcopy")
    shutil.copytree(REF, REFCOPY)
    subprocess.check_call(["chmod", "-R", "u+w", REFCOPY])
    env = dict(os.environ, PYTHONPATH=SHIM + ":" + REFCOPY)
    inputs = synth_inputs()
    os.makedirs(os.path.join(GOLDEN, "generate"), exist_ok=True)
    np.savez_compressed(os.path.join(GOLDEN, "generate", "draft_inputs.npz"),
                        **{k.replace(".", "_"): np.frombuffer(v, dtype=np.uint8) for k, v in inputs.items()},
                        **{k: np.frombuffer(v.encode(), dtype=np.uint8) for k, v in GIVEN.items()})
    for case, flags in CASES.items():
        cwd = os.path.join(work, case)
        os.makedirs(cwd)
        for name, blob in inputs.items():
            with open(os.path.join(cwd, name), "wb") as fh:
                fh.write(blob)
        for name, text in GIVEN.items():
            with open(os.path.join(cwd, name + ".txt"), "w") as fh:
                fh.write(text)
        subprocess.check_call([sys.executable, "-m", "iss", "generate"] + BASE + ["-o", "out", "--quiet"] + case_argv(flags),
                              env=env, cwd=cwd)
        blobs = {}
        for suffix in ("_R1.fastq", "_R2.fastq", "_abundance.txt", "_coverage.txt"):
            path = os.path.join(cwd, "out" + suffix)
            blobs[suffix] = np.frombuffer(open(path, "rb").read(), dtype=np.uint8) if os.path.exists(path) else None
        np.savez_compressed(os.path.join(GOLDEN, "generate", "draft_%s.npz" % case), r1=blobs["_R1.fastq"], r2=blobs["_R2.fastq"],
                            abundance=blobs["_abundance.txt"] if blobs["_abundance.txt"] is not None else np.zeros(0, np.uint8),
                            coverage=blobs["_coverage.txt"] if blobs["_coverage.txt"] is not None else np.zeros(0, np.uint8),
                            has_abundance=np.array(blobs["_abundance.txt"] is not None),
                            has_coverage=np.array(blobs["_coverage.txt"] is not None),
                            flags=np.array(" ".join(BASE + flags)))
        print(case, len(blobs["_R1.fastq"]), "abundance" if blobs["_abundance.txt"] is not None else "",
              "coverage" if blobs["_coverage.txt"] is not None else "")
    shutil.rmtree(work, ignore_errors=True)
