"""The BGZF member decoder (insilicoseq_amd/csrc/iss_inflate_core.h: plain C++17, the text k_bgzf_inflate runs on 64 lanes) in a
stand-alone program, inflate_core_main.cpp, built with the system compiler under the address and undefined-behaviour sanitizers and
run on the case table: every case's payload and output buffers are allocated at their exact sizes, so a read behind the payload or
a write outside [0, ISIZE) ends the program with the sanitizer's report.  Status, CRC and bytes are compared with the table."""
import os
import shutil
import struct
import subprocess
import sys
import zlib

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "insilicoseq_amd", "csrc")
sys.path.insert(0, HERE)

import inflate_cases as IC  # noqa: E402


def _has_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        if _has_gpu():
            pytest.skip("no g++ on the GPU machine")
        pytest.fail("g++ not found: the decoder's host test needs the system compiler")
    exe = str(tmp_path_factory.mktemp("inflate_core") / "inflate_core")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, "-o", exe,
                            os.path.join(HERE, "inflate_core_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def run_cases(exe, cases, tmp_path):
    """[(status, crc)] per case and the bytes of the cases that ended OK or TRAILING."""
    path, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for c in cases:
            pay, crc, isize = IC.split_member(c["member"])
            fh.write(struct.pack("<III", len(pay), isize, crc) + pay)
    run = subprocess.run([exe, path, out], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    rows = [line.split() for line in run.stdout.splitlines()]
    assert [int(r[0]) for r in rows] == list(range(len(cases)))
    with open(out, "rb") as fh:
        return [(int(r[1]), int(r[2], 16)) for r in rows], fh.read()


def test_good_cases_inflate_to_their_bytes(program, tmp_path):
    cases = IC.good_cases()
    rows, data = run_cases(program, cases, tmp_path)
    at = 0
    for c, (status, crc) in zip(cases, rows):
        assert status == IC.OK, (c["name"], IC.STATUS_NAMES[status])
        assert crc == zlib.crc32(c["data"]) & 0xFFFFFFFF, c["name"]
        assert data[at:at + len(c["data"])] == c["data"], c["name"]
        at += len(c["data"])
    assert at == len(data)


def test_bad_cases_end_with_their_status(program, tmp_path):
    cases = IC.bad_cases()
    rows, _ = run_cases(program, cases, tmp_path)
    for c, (status, _crc) in zip(cases, rows):
        assert status == c["status"], (c["name"], IC.STATUS_NAMES[status])


def test_interleaved_cases_do_not_depend_on_their_neighbours(program, tmp_path):
    cases = IC.all_cases()
    rows, data = run_cases(program, cases, tmp_path)
    assert [r[0] for r in rows] == [c["status"] for c in cases]
    text = IC.fastq_text(4000, 3)  # what the TRAILING case holds
    assert data == b"".join(c["data"] if c["status"] == IC.OK else text for c in cases if c["status"] in (IC.OK, IC.TRAILING))


def test_every_truncation_ends_with_a_status(program, tmp_path):
    """Streams cut short, byte by byte: the reader must stop at the payload's end (the sanitizer watches) and say IN_OVERRUN."""
    by_name = {c["name"]: c for c in IC.good_cases()}
    cases = []
    for name in ("lit_code_15_bits_cl_7_bits", "hlit_286_hdist_30", "repeat_16_across_the_boundary", "match_len_258", "stored_blocks"):
        pay, crc, isize = IC.split_member(by_name[name]["member"])
        step = max(1, len(pay) // 300)
        for cut in list(range(0, min(len(pay), 120))) + list(range(120, len(pay), step)):
            cases.append({"member": IC.member(pay[:cut], crc=crc, isize=isize), "name": "%s[:%d]" % (name, cut)})
    rows, _ = run_cases(program, cases, tmp_path)
    for c, (status, _crc) in zip(cases, rows):
        assert status == IC.IN_OVERRUN, (c["name"], IC.STATUS_NAMES[status])
