#!/usr/bin/env python3
"""The host twin's status of every damaged stream of tests/inflate_gen.py, as the fixture the GPU leg compares with where there is
no system compiler: tests/golden/inflate_gen/twin_status.npz (`status`: one byte per stream of inflate_gen.damage(), in order;
`digest`: inflate_gen.digest(), the SHA-256 of the corpus the streams were made from).

The twin is tests/inflate_core_main.cpp built by tests/inflate_twin.py's recipe (system compiler, address and undefined-behaviour
sanitizers, buffers of exact size).  tests/test_inflate_gen_host.py builds the twin from the tree again and asserts that the fixture
is what it says, so a change of the decoder or of the generator that moves a status fails there until this script has run.

Usage:  python tests/golden/tooling/make_inflate_gen_twin.py   (from the repo root; needs g++)
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, TESTS)

import inflate_gen as G  # noqa: E402
import inflate_twin as T  # noqa: E402

OUT = os.path.join(TESTS, "golden", "inflate_gen", "twin_status.npz")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = T.build_program(tmp)
        if exe is None:
            sys.exit("g++ not found")
        rows, _ = T.run_cases(exe, G.damage(), tmp)
    status = np.array([r[0] for r in rows], dtype=np.uint8)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, status=status, digest=np.frombuffer(G.digest().encode(), dtype=np.uint8))
    print("%s: %d statuses, %d bytes" % (OUT, status.size, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
