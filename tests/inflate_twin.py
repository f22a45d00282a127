"""The host twin of the BGZF member decoder, shared by tests/test_inflate_core_host.py, tests/test_inflate_gen_host.py and
tests/golden/tooling/make_inflate_gen_twin.py: inflate_core_main.cpp built with the system compiler under the address and
undefined-behaviour sanitizers (one recipe), and the case file it reads."""
import os
import shutil
import struct
import subprocess
import sys

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


def build_program(directory):
    """The sanitizer-built twin in `directory`: its path, or None where there is no g++."""
    gxx = shutil.which("g++")
    if gxx is None:
        return None
    exe = os.path.join(str(directory), "inflate_core")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, "-o", exe,
                            os.path.join(HERE, "inflate_core_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = build_program(tmp_path_factory.mktemp("inflate_core"))
    if exe is None:
        if _has_gpu():
            pytest.skip("no g++ on the GPU machine")
        pytest.fail("g++ not found: the decoder's host test needs the system compiler")
    return exe


def run_cases(exe, cases, tmp_path):
    """[(status, crc)] per case and the bytes of the cases that ended OK or TRAILING."""
    path, out = os.path.join(str(tmp_path), "cases.bin"), os.path.join(str(tmp_path), "out.bin")
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
