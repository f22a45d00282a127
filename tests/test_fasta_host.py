"""`generate --device_fasta` without a GPU (insilicoseq_amd/fasta.py, iss_fasta_core.h through the library's host entry): the numpy
twin, the library's host index and `fasta.read` against `parse_fasta(path)` on the hand cases and on seeded random files; the exports;
gzip and BGZF genome inputs through the host inflate."""
import gzip
import os

import numpy as np
import pytest

import fasta_cases as FC
from insilicoseq_amd import fasta as F
from insilicoseq_amd.generator import parse_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("iss_fa_create", "iss_fa_destroy", "iss_fa_last_error", "iss_fa_index", "iss_fasta_host_index", "iss_fasta_tile",
               "iss_fasta_scan_span", "iss_genome_upload_fasta")
RANDOM_SEEDS = range(300)


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge

    ge.build()
    from insilicoseq_amd import _native

    return _native


def naive_index(data):
    """The grammar of DESIGN.md section 31 byte by byte, as plainly as it can be said."""
    rows, n = [], len(data)
    heads = [i for i in range(n) if data[i] == 62 and (i == 0 or data[i - 1] == 10)]
    for r, h in enumerate(heads):
        end = heads[r + 1] if r + 1 < len(heads) else n
        eol = data.find(b"\n", h, end)
        eol = end if eol < 0 else eol
        body_off = eol + 1 if eol < end else end
        body = data[body_off:end]
        rows.append((h, eol - h - 1, body_off, end - body_off, sum(1 for c in body if c not in b"\r\n"),
                     int(any(c not in b"\r\n" and not 0x21 <= c <= 0x7E for c in body))))
    return rows


def rows_of(index):
    return [tuple(int(x) for x in row) for row in zip(*index)]


def same_records(got, want):
    assert [(r.id, r.description, len(r.seq), str(r.seq)) for r in got] == [(r.id, r.description, len(r.seq), str(r.seq)) for r in want]


def check_text(native, data, path):
    want = naive_index(data)
    assert rows_of(F.index_host(data)) == want
    assert rows_of(F.index_native_host(data)) == want
    with open(path, "wb") as fh:
        fh.write(data)
    got = F.read(path)
    same_records(got, list(parse_fasta(path)))
    for rec, row in zip(got, want):  # a flagged record took the host parser, every other one stays in the file
        assert isinstance(rec.seq, str) == bool(row[5] & F.ODD)
        if not row[5]:
            assert bytes(rec.seq.raw()) == data[row[2]:row[2] + row[3]] and len(rec.seq) == row[4]


@pytest.mark.parametrize("name", sorted(FC.HAND))
def test_hand_cases(native, name, tmp_path):
    check_text(native, FC.HAND[name], str(tmp_path / "x.fasta"))


def test_hand_cases_are_what_they_say():
    flagged = {name for name, data in FC.HAND.items() if any(row[5] for row in naive_index(data))}
    assert flagged == {n for n in FC.HAND if n.startswith("body_with_")}
    assert naive_index(FC.HAND["empty_file"]) == [] and naive_index(FC.HAND["no_header_at_all"]) == []
    assert [row[4] for row in naive_index(FC.HAND["four_tiny_records_in_16_bytes"])] == [2, 2, 2, 2]
    assert [row[2] for row in naive_index(FC.HAND["four_tiny_records_in_one_lane"])] == [16, 21, 26, 31]
    assert [row[4] for row in naive_index(FC.HAND["empty_record_between_headers"])] == [0, 4, 0]
    assert naive_index(FC.HAND["header_as_last_line"])[1][1:5] == (12, 21, 0, 0)


def test_random_files(native, tmp_path):
    odd = 0
    for seed in RANDOM_SEEDS:
        data = FC.random_file(seed)
        odd += any(row[5] for row in naive_index(data))
        check_text(native, data, str(tmp_path / "r.fasta"))
    assert 10 <= odd <= 30  # a tenth of the files carry an odd byte


def test_count_alone_and_small_capacity(native):
    data = FC.HAND["four_tiny_records_in_16_bytes"]
    a = np.frombuffer(data, np.uint8)
    n = native.C.c_int64(-1)
    lib = native.lib()
    assert lib.iss_fasta_host_index(a.ctypes.data, a.size, 0, None, None, None, None, None, None, native.C.byref(n)) == 0 and n.value == 4
    rows = [np.full(2, -7, np.int64) for _ in range(5)] + [np.full(2, -7, np.int32)]
    n.value = -1
    assert lib.iss_fasta_host_index(a.ctypes.data, a.size, 2, *([r.ctypes.data for r in rows] + [native.C.byref(n)])) == 0
    assert n.value == 4 and all((r == -7).all() for r in rows)  # (no room: the count alone)
    assert lib.iss_fasta_host_index(None, 5, 0, None, None, None, None, None, None, native.C.byref(n)) == native.E_INVALID


def test_upload_runs_cut_at_files_gaps_and_order():
    src, other = object(), object()
    seqs = [F.FastaSeq(src, 10, 5, 5), F.FastaSeq(src, 20, 5, 5), F.FastaSeq(src, 25 + (1 << 20) + 1, 5, 5), F.FastaSeq(other, 0, 3, 3),
            F.FastaSeq(src, 100, 5, 5), F.FastaSeq(src, 50, 5, 5)]
    assert F.upload_runs(seqs) == [(0, 2), (2, 3), (3, 4), (4, 5), (5, 6)]
    assert F.upload_runs(seqs[:2], gap=4) == [(0, 1), (1, 2)] and F.upload_runs([]) == []


def test_the_switch_is_off_unless_asked_for():
    import inspect

    from insilicoseq_amd import app, drafts

    common = ["generate", "--genomes", "g.fa", "-o", "out"]
    assert app.build_parser().parse_args(common).device_fasta is False
    assert app.build_parser().parse_args(common + ["--device_fasta"]).device_fasta is True
    assert inspect.signature(app._worker).parameters["device_fasta"].default is False
    assert inspect.signature(drafts.load_genomes).parameters["device_fasta"].default is False


def test_exports(native):
    import re

    header = open(os.path.join(ROOT, "include", "iss_mi355x.h")).read()
    declared = set(re.findall(r"\b(iss_[a-z0-9_]+)\s*\(", header))
    lib = native.lib()
    for name in NEW_ENTRIES:
        assert name in native.EXPORTS and name in declared and hasattr(lib, name), name
    assert lib.iss_fasta_tile() == 4096 and lib.iss_fasta_scan_span() >= 256


@pytest.mark.parametrize("container", ["gzip", "bgzf"])
def test_gz_genome_inputs_on_the_host_inflate(native, container, tmp_path, monkeypatch):
    from insilicoseq_amd import drafts, inflate

    monkeypatch.setenv("ISS_HOST_INFLATE", "1")
    data = FC.HAND["junk_in_front"] + FC.HAND["crlf"]
    plain, packed = str(tmp_path / "g.fa"), str(tmp_path / "g.fa.gz")
    with open(plain, "wb") as fh:
        fh.write(data)
    with open(packed, "wb") as fh:
        fh.write(gzip.compress(data) if container == "gzip" else FC.bgzf(data))
    assert inflate.is_bgzf(packed) == (container == "bgzf")
    want = list(parse_fasta(plain))
    assert len(want) == 4
    same_records(list(parse_fasta(packed)), want)
    same_records(F.read(packed), want)
    assert drafts.draft_contigs(packed) == drafts.draft_contigs(plain)
    drafts.concatenate([plain, packed], str(tmp_path / "cat.fa"), device_inflate=True)  # (ISS_HOST_INFLATE=1 wins)
    assert (tmp_path / "cat.fa").read_bytes() == data + data
    genome_file, records = drafts.load_genomes([packed], None, str(tmp_path / "out"), None)
    same_records(records, want)
    assert open(genome_file, "rb").read() == data
