"""The generated corpus of tests/inflate_gen.py without a GPU: zlib inflates every member to the generator's bytes, the corpus is the
pinned one and holds what its ledger says, the rule that judges damaged streams is checked by hand on one stream per outcome, and
the sanitizer-built host twin (tests/inflate_twin.py: exact-size buffers) runs the corpus and every damaged stream -- bytes and CRC
exact for the good members, a status the rule allows for the damaged ones, and the fixture the GPU leg compares with
(tests/golden/inflate_gen/twin_status.npz) equal to what the twin built from this tree says."""
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import inflate_cases as IC  # noqa: E402
import inflate_gen as G  # noqa: E402
from inflate_twin import program, run_cases  # noqa: E402,F401

DIGEST = "9029975e736808efc0adff852fa390cce811c583fc39831e8f2fba1f6bf334f6"
N_MEMBERS, N_DAMAGED = 1756, 34507
FIXTURE = os.path.join(HERE, "golden", "inflate_gen", "twin_status.npz")


def test_corpus_is_the_pinned_one():
    assert len(G.corpus()) == N_MEMBERS and len(G.damage()) == N_DAMAGED
    assert G.digest() == DIGEST
    names = [m["name"] for m in G.corpus()]
    assert len(set(names)) == len(names)


def test_zlib_inflates_every_member_to_the_generators_bytes():
    for m in G.corpus():
        pay, crc, isize = IC.split_member(m["member"])
        d = zlib.decompressobj(-15)
        data = d.decompress(pay)
        assert d.eof and d.unused_data == b"" and data == m["data"], m["name"]
        assert isize == len(data) <= 65536 and crc == zlib.crc32(data) & 0xFFFFFFFF, m["name"]
        assert len(m["member"]) <= 65536


def test_size_plans():
    by = {}
    for m in G.corpus():
        by.setdefault(m["plan"], []).append(len(m["data"]))
    assert set(by) == {"tiny", "small", "boundary"}
    assert sorted(set(by["tiny"])) == list(range(10)) and max(by["small"]) <= 2048 and max(by["small"]) > 1500
    assert min(by["boundary"]) > 16384 and max(by["boundary"]) == 65536
    assert len(by["tiny"]) + len(by["small"]) >= 1500


@pytest.mark.parametrize("k", range(22))  # (by number, so that collecting the suite does not build the corpus)
def test_ledger(k):
    conditions = G.ledger_conditions()
    assert len(conditions) == 22
    what, missing = conditions[k]
    assert not missing, (what, missing[:20])


def test_base_members_of_the_damage():
    bases = G.base_members()
    assert all(len(IC.split_member(m["member"])[0]) <= G.MAX_BASE_PAYLOAD for m in bases)
    have = set().union(*(m["features"] for m in bases))
    assert {("type", t) for t in ("stored", "fixed", "dyn")} <= have
    assert {("op", o) for o in ("len", "rep16", "z17", "z18")} <= have
    assert {("incomplete", "lit"), ("incomplete", "dist"), ("no_distance_code",)} <= have
    assert {("empty", t, f) for t in ("stored", "fixed", "dyn") for f in (False, True)} <= have
    assert {("lit_longest", 15), ("dist_longest", 15), ("cl_longest", 7), ("cl_longest", 1)} <= have
    names = [c["name"] for c in G.damage()]
    for mark in ("^", "[:", "+byte@", "-byte@", " crc", " isize+1", " isize-1", " isize+258", " isize-258", " isize=0", " isize=65536", "hclen_4"):
        assert any(mark in n for n in names), mark


# ---------------------------------------------------------------------------------------------------- the rule, by hand
def _fixed(tokens, tail=b"\0\0\0\0"):
    w = IC.BitWriter()
    IC.fixed_block(w, tokens)
    return w.done() + tail


def test_verdict_by_hand():
    w = IC.BitWriter()
    IC.stored_block(w, b"abc")
    good, crc = w.done(), zlib.crc32(b"abc") & 0xFFFFFFFF
    assert G.verdict(good, crc, 3) == ("finished", (IC.OK,), b"abc")
    assert G.verdict(good + b"\0", crc, 3) == ("finished", (IC.TRAILING,), b"abc")
    assert G.verdict(good, crc ^ 1, 3) == ("finished", (IC.CRC,), b"abc")
    assert G.verdict(good, crc, 4) == ("finished", (IC.SHORT,), None)
    assert G.verdict(good, crc, 2) == ("finished", (IC.OUT_OVERRUN,), None)
    assert G.verdict(good + b"\0", crc ^ 1, 2) == ("finished", (IC.OUT_OVERRUN,), None)  # the order: size, CRC, tail
    assert G.verdict(good + b"\0", crc ^ 1, 3) == ("finished", (IC.CRC,), b"abc")
    assert G.verdict(good[:6], crc, 3) == ("input ran out", (IC.IN_OVERRUN, IC.OUT_OVERRUN), None)
    assert G.verdict(b"", 0, 0) == ("input ran out", (IC.IN_OVERRUN, IC.OUT_OVERRUN), None)
    # zlib's errors, with room in the output (ISIZE 10) and four bytes behind the error: the class alone
    w = IC.BitWriter()
    IC.stored_block(w, b"abc", nlen=0x1234)
    for payload, allowed in ((b"\x07\0\0\0\0", (IC.BAD_BTYPE,)), (w.done(), (IC.STORED_LEN,)),
                             (_fixed(IC.lits(b"abc") + [("match", 3, 4), ("end",)]), (IC.BAD_DISTANCE,)),
                             (_fixed(IC.lits(b"ab") + [("lsym", 286), ("end",)]), (IC.BAD_SYMBOL, IC.BAD_CODE)),
                             (_fixed(IC.lits(b"ab") + [("lsym", 257), ("dsym", 30), ("end",)]), (IC.BAD_SYMBOL, IC.BAD_CODE))):
        assert G.verdict(payload, 0, 10) == ("error", allowed, None), payload
    # the error stands behind byte ISIZE: the output overran first
    six = _fixed(IC.lits(b"abcdef") + [("lsym", 286)])
    assert G.verdict(six, 0, 2) == ("error", (IC.OUT_OVERRUN,), None)
    assert G.verdict(six, 0, 4) == ("error", (IC.OUT_OVERRUN,), None)
    assert G.verdict(six, 0, 7) == ("error", (IC.BAD_SYMBOL, IC.BAD_CODE), None)
    for isize in (5, 6):  # the error stands 6 bytes in: with room for 6 zlib may or may not show which came first
        got = G.verdict(six, 0, isize)
        assert got[0] == "error" and IC.OUT_OVERRUN in got[1] or isize == 6
        assert set((IC.BAD_SYMBOL, IC.BAD_CODE)) <= set(got[1]) <= set((IC.BAD_SYMBOL, IC.BAD_CODE, IC.OUT_OVERRUN))
    # ISIZE 0: a byte before the error, and none
    w = IC.BitWriter()
    IC.stored_block(w, b"a", final=False)
    assert G.verdict(w.done() + b"\x07\0\0\0\0", 0, 0) == ("error", (IC.OUT_OVERRUN,), None)
    got = G.verdict(b"\x07\0\0\0\0", 0, 0)
    assert got[0] == "error" and set(got[1]) == set((IC.BAD_BTYPE, IC.OUT_OVERRUN))
    # the error in the payload's last two bytes: the decoder may have wanted more bits than there are
    got = G.verdict(_fixed(IC.lits(b"ab") + [("lsym", 286)], tail=b""), 0, 10)
    assert got[0] == "error" and set(got[1]) == set((IC.BAD_SYMBOL, IC.BAD_CODE, IC.IN_OVERRUN))


@pytest.mark.parametrize("case", IC.bad_cases(), ids=lambda c: c["name"])
def test_verdict_allows_the_tables_status(case):
    """The hand-built bad members of inflate_cases.py: the rule allows the status the table states, and where zlib names one cause or
    finishes, nothing else."""
    outcome, allowed, _ = G.verdict(*IC.split_member(case["member"]))
    assert case["status"] in allowed, (outcome, allowed)
    assert set(allowed) - {case["status"]} <= {IC.IN_OVERRUN, IC.OUT_OVERRUN, IC.BAD_SYMBOL, IC.BAD_CODE}
    if outcome == "finished":
        assert allowed == (case["status"],)


def test_every_message_of_the_map_is_met():
    met = set()
    for c in G.damage() + IC.bad_cases():
        try:
            zlib.decompressobj(-15).decompress(IC.split_member(c["member"])[0])
        except zlib.error as e:
            met.update(text for text, _ in G.MESSAGES if text in str(e))
    assert met == set(text for text, _ in G.MESSAGES)


# ---------------------------------------------------------------------------------------------------- the host twin
def test_twin_inflates_the_corpus(program, tmp_path):
    cases = G.corpus()
    rows, data = run_cases(program, cases, tmp_path)
    at = 0
    for c, (status, crc) in zip(cases, rows):
        assert status == IC.OK, (c["name"], IC.STATUS_NAMES[status])
        assert crc == zlib.crc32(c["data"]) & 0xFFFFFFFF, c["name"]
        assert data[at:at + len(c["data"])] == c["data"], c["name"]
        at += len(c["data"])
    assert at == len(data)


def test_twin_on_the_damaged_streams(program, tmp_path):
    cases, verdicts = G.damage(), G.verdicts()
    rows, data = run_cases(program, cases, tmp_path)
    at = 0
    for c, (outcome, allowed, want), (status, crc) in zip(cases, verdicts, rows):
        assert status in allowed, (c["name"], outcome, [IC.STATUS_NAMES[s] for s in allowed], IC.STATUS_NAMES[status])
        if status in (IC.OK, IC.TRAILING):
            assert data[at:at + len(want)] == want and crc == zlib.crc32(want) & 0xFFFFFFFF, c["name"]
            at += len(want)
        elif status == IC.CRC:
            assert crc == zlib.crc32(want) & 0xFFFFFFFF, c["name"]
    assert at == len(data)
    fixture = np.load(FIXTURE)
    assert fixture["digest"].tobytes().decode() == G.digest() == DIGEST
    assert fixture["status"].dtype == np.uint8 and fixture["status"].tolist() == [r[0] for r in rows], \
        "tests/golden/tooling/make_inflate_gen_twin.py has to run again"


def test_fixture_without_the_twin():
    """Where there is no system compiler the fixture still has to fit the corpus and the rule."""
    fixture = np.load(FIXTURE)
    assert fixture["digest"].tobytes().decode() == G.digest()
    status = fixture["status"]
    assert status.size == len(G.damage())
    for c, v, s in zip(G.damage(), G.verdicts(), status.tolist()):
        assert s in v[1], c["name"]
