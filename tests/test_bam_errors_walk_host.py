"""The tag walk and the MD walk of k_be_records (insilicoseq_amd/csrc/iss_bam_record.h) compiled for the host and driven by
tools/bam_errors_walk.cpp over every valid and damaged case: the verdicts and the row counts of the constructions, under
AddressSanitizer and UBSan where the compiler has them (a stand-alone program; nothing is loaded into Python)."""
import os
import shutil
import subprocess

import bam_error_cases as EC
import bam_synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError("no C++ compiler found")


def _build(tmp_path):
    out = str(tmp_path / "bam_errors_walk")
    cmd = [_compiler(), "-std=c++17", "-g", "-O1", "-I", os.path.join(ROOT, "insilicoseq_amd", "csrc"), "-o", out,
           os.path.join(ROOT, "tools", "bam_errors_walk.cpp")]
    sanitized = subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    if sanitized.returncode:  # (a compiler without the sanitizers' runtimes: the verdicts are still checked)
        subprocess.run(cmd, check=True)
    return out


def _expected_line(r):
    c = r["_case"]
    what = c["expect"]
    if what == "tallied":
        return "T %d %d" % (len(c["mism"]), sum(len(d) for d in c["dels"]))
    return {"unaligned": "U", "no_md": "N"}.get(what, str(what))


def test_walks_on_every_case(tmp_path):
    records = [r for r in EC.valid_cases() + EC.damaged_cases() if r["_case"]["expect"] != "skipped"]  # (skipped: the flags, not the walks)
    path = str(tmp_path / "records.bin")
    with open(path, "wb") as fh:
        for r in records:
            fh.write(EC.BC.encode(r))
    run = subprocess.run([_build(tmp_path), path], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(records)
    assert [(r["name"], got) for r, got in zip(records, lines) if got != _expected_line(r)] == []


def test_walks_on_synthetic_records(tmp_path):
    records = bam_synth.records(5, n_pairs=300, var_lengths=(1, 301)) + bam_synth.edge_table()
    records = [r for r in records if r["qual"] is not None]
    path = str(tmp_path / "records.bin")
    with open(path, "wb") as fh:
        for r in records:
            fh.write(bam_synth.encode_record(r))
    run = subprocess.run([_build(tmp_path), path], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(records) and set(line[0] for line in lines) <= {"T", "U"} and sum(line[0] == "T" for line in lines) > 600
