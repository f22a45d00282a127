"""The owning handle of the library's host side (insilicoseq_amd/csrc/iss_own.h: plain C++17, no HIP) in a stand-alone program,
own_host_main.cpp, with a counting release: built with the system compiler under the address and undefined-behaviour sanitizers
and run.  The program checks empty construction, moves (self-assignment included), reset, vectors and arrays of handles, and the
conversion to a pointer; a double release, a leak or a use after release ends it with the sanitizer's report."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "insilicoseq_amd", "csrc")


def _has_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


def test_handle_releases_once(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        if _has_gpu():
            pytest.skip("no g++ on the GPU machine")
        pytest.fail("g++ not found: the handle's host test needs the system compiler")
    exe = str(tmp_path / "own_host")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, "-o", exe, os.path.join(HERE, "own_host_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "own ok: 209 releases"
