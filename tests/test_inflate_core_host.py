"""The BGZF member decoder (insilicoseq_amd/csrc/iss_inflate_core.h: plain C++17, the text k_bgzf_inflate runs on 64 lanes) in a
stand-alone program, inflate_core_main.cpp, built with the system compiler under the address and undefined-behaviour sanitizers and
run on the case table: every case's payload and output buffers are allocated at their exact sizes, so a read behind the payload or
a write outside [0, ISIZE) ends the program with the sanitizer's report.  Status, CRC and bytes are compared with the table."""
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import inflate_cases as IC  # noqa: E402
from inflate_twin import program, run_cases  # noqa: E402,F401  (the recipe, shared with test_inflate_gen_host.py)


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
