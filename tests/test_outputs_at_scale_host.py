"""tests/scale_cases.py held to its own contract (no GPU; DESIGN section 4, "What holds the readers of a call at scale").

The cases are what the ledger says -- a change of a model, a record, a seed or a size cannot pass unseen; the batch's short item
has the pairs it was made for and its seams fall where they should; and every expectation builder, run on the oracle's arrays,
agrees with an independent statement of it where the project has one."""
import io

import numpy as np
import pytest

import scale_cases as S


@pytest.fixture(scope="module", params=list(S.CASES))
def call(request):
    return S.expected(request.param)


# ---------------------------------------------------------------------------------------------------- the cases
def test_the_cases_run_the_readers_they_should():
    assert {k: (c.kind, c.model, c.n_pairs, c.first_ordinal) for k, c in S.CASES.items()} == {
        "fixup": ("generate", "patterned", 1 << 14, 11), "scripted": ("generate", "patterned-plain", 1 << 14, 0),
        "batch": ("batch", "patterned", 1 << 14, S.BATCH_FIRST_ORDINAL), "mt": ("mt", "flat", 1 << 13, 0)}
    assert S.CASES["fixup"].readers == S.CASES["scripted"].readers == tuple(range(1, 11))
    assert S.CASES["batch"].readers == (1, 2, 3, 6, 7, 8, 9) and S.CASES["mt"].readers == (1, 2, 4, 5, 8)
    assert S.SEED == 2024 and all(0 < c < S.N_PAIRS and c % 64 for c in S.WINDOW_CUTS)


def test_the_ledger(call):
    got = S.ledger(call)
    assert got == S.LEDGER[call.name], got
    assert got["rows"] == sum(got["by type"]) and all(got["by type"])
    assert len(call.bases) == len(call.qual) == len(call.coords) == len(call.item) == call.n
    if call.name != "mt":  # a noisy call: most reads carry an indel row, the text runs over more than a hundred blocks
        assert got["reads with an indel row"] > 0.8 * 2 * call.n and got["vcf members"] >= 128


def test_fixup_is_the_noisy_call_it_was_sized_as():
    led = S.LEDGER["fixup"]
    assert led["most rows of a pair"] <= 26 and led["most rows of a read"] <= 23
    assert round(led["reads with an indel row"] / (2.0 * S.N_PAIRS), 3) == 0.825
    assert led["vcf members"] == 129 and led["fastq bytes of mate 1"] == 10196122


def test_fixup_from_ordinal_0_has_the_figures_the_case_was_sized_by():
    from helpers import vcf_lines
    from oracle import oracle as O

    c = S.expected("fixup")
    res = O.Oracle(c.dense).simulate(O.Rng().seed_philox(S.SEED), c.records[0][1], c.n, store_mutations=True)
    rows = res["mutations"]
    assert res["status"] == 0 and res["n_done"] == c.n
    text = "".join(vcf_lines("rec.1", 0, S.CPU, rows))
    assert (len(rows), tuple(int((rows["type"] == t).sum()) for t in range(3)), len(text)) == S.FIXUP_FROM_ORDINAL_0
    assert -(-len(text) // S.BGZF_BLOCK) == 129


def test_the_batch_has_what_it_was_made_for():
    c = S.expected("batch")
    assert [it[3] for it in c.items] == list(S.BATCH_PAIRS) and sum(S.BATCH_PAIRS) == S.N_PAIRS
    assert all(n % 16 and n % 64 for n in S.BATCH_PAIRS)
    for _rid, _i, row, _n in c.items[1:]:  # a seam inside a group of 16 pairs and inside an export tile
        assert row % 16 and row % 64
    assert np.array_equal(np.flatnonzero(np.diff(c.item)) + 1, [it[2] for it in c.items[1:]])
    assert [len(seq) for _rid, seq in c.records] == [S.BATCH_LONG, S.BATCH_SHORT, S.BATCH_LONG]
    assert set(c.records[0][1]) == set("ACGT") == set(c.records[1][1]) and set(c.records[2][1]) - set("ACGT")
    short = S.short_item(c)
    assert short["fell back"] > 0.05 and short["cut by the end"] > 0.05 and short["windows that leave"] > 0, short
    for k in range(3):  # every item is noisy by itself
        rows = c.rows_of_item(k)
        assert ((rows["type"] != 0).sum()) > c.items[k][3]
    # the mixed item's reads with an indel row -- the fix-up's for their record's letters -- are more than its grid has wavefronts
    ind = rows[rows["type"] != 0]
    assert np.unique(ind["pair"].astype(np.int64) * 2 + ind["mate"]).size > 8 * 4 * 256
    # the oracle ran item after item on running ordinals: the second item is not the call from ordinal 0
    from oracle import oracle as O

    res = O.Oracle(c.dense).simulate(O.Rng().seed_philox(S.SEED), c.records[1][1], 64, first_ordinal=0, want_coords=True)
    assert not np.array_equal(res["coords"], c.coords[c.items[1][2]:c.items[1][2] + 64])
    res = O.Oracle(c.dense).simulate(O.Rng().seed_philox(S.SEED), c.records[1][1], 64, first_ordinal=S.BATCH_FIRST_ORDINAL + S.BATCH_PAIRS[0],
                                     want_coords=True)
    assert np.array_equal(res["coords"], c.coords[c.items[1][2]:c.items[1][2] + 64])


# ---------------------------------------------------------------------------------------------------- the builders
def test_vcf_text_agrees_with_the_other_statements(call):
    """helpers.vcf_lines against test_gpu_vcf._oracle_text (row by row) and generator.write_mutations (columns), item by item."""
    from insilicoseq_amd.generator import write_mutations
    from test_gpu_vcf import _oracle_text

    text = S.vcf_text(call)
    buf = io.StringIO()
    other = []
    for k, (rid, first_i, _row, _n) in enumerate(call.items):
        rows = call.rows_of_item(k)
        other.append(_oracle_text(rows, rid, first_i, S.CPU))
        write_mutations(rows, buf, rid, first_i, S.CPU)
    assert text == b"".join(other)
    assert text == buf.getvalue().encode()
    assert text.count(b"\n") == len(call.rows)


def test_bgzf_members_counts_and_rejects():
    from insilicoseq_amd import bgzf

    assert bgzf.BLOCK == S.BGZF_BLOCK
    call = S.expected("mt")
    text = S.vcf_text(call)
    out = io.BytesIO()
    bgzf.write_member(out, text)
    raw = out.getvalue()
    assert S.bgzf_members(raw, text) == S.LEDGER["mt"]["vcf members"]
    with pytest.raises(AssertionError):
        S.bgzf_members(raw, text[:-1] + b"x")
    last = len(raw) - 8  # the last member's CRC-32
    for damaged in (raw[:-1], raw[:12] + b"XX" + raw[14:], raw[:last] + bytes([raw[last] ^ 1]) + raw[last + 1:]):
        with pytest.raises(bgzf.BgzfError):
            S.bgzf_members(damaged, text)


def test_truth_and_events_of_the_rows(call):
    """Truth differs from the bases exactly at the substitution rows and holds their ref letters; the events are the rows."""
    from insilicoseq_amd.tensors import recode

    truth, events = S.truth_and_events(call, 0, call.n, "ascii")
    sub = call.rows[call.rows["type"] == 0]
    differs = np.zeros(call.bases.shape, dtype=bool)
    differs[sub["pair"], sub["mate"], sub["position"]] = True
    assert np.array_equal(truth != call.bases, differs) and differs.sum() == len(sub)
    assert np.array_equal(truth[differs], sub["ref"]) and np.array_equal(call.bases[differs], sub["alt"])
    assert len(events) == len(call.rows) and np.array_equal(events[:, 0], call.rows["pair"]) and np.array_equal(events[:, 3], call.rows["position"])
    codes, _ = S.truth_and_events(call, 0, call.n, "codes")
    assert np.array_equal(codes, recode(truth))
    first, n = S.windows(call)[1]
    t, e = S.truth_and_events(call, first, n, "ascii")
    inside = events[(events[:, 0] >= first) & (events[:, 0] < first + n)]
    assert np.array_equal(t, truth[first:first + n]) and 0 < len(inside) < len(events)
    assert np.array_equal(e[:, 1:], inside[:, 1:]) and np.array_equal(e[:, 0], inside[:, 0] - first)


def test_error_tally_of_the_rows(call):
    from insilicoseq_amd import errtally as E

    L = call.RL
    whole = S.error_tally(call, 0, call.n)
    t = E.split(whole, L)
    by_type = S.LEDGER[call.name]["by type"]
    assert (int(t["sub_q"].sum()), int(t["ins"].sum()), int(t["del"].sum())) == by_type and t["sub_mat"].sum() == by_type[0]
    assert t["pairs"][0] == call.n and t["dropped"][0] == 0 and (t["per_read"].sum(axis=2) == call.n).all()
    wins = S.windows(call)
    parts = [S.error_tally(call, first, n) for first, n in wins]
    assert len(wins) == 3 and sum(n for _, n in wins) == call.n and np.array_equal(E.merge(parts), whole) and all(E.split(p, L)["sub_q"].sum() > 0 for p in parts)


def test_read_tally_and_fastq_text_say_the_same(call):
    """The tally's per-position base and phred counts against counts taken from the FASTQ text's own lines."""
    from insilicoseq_amd.tally import split_tally

    t = split_tally(S.read_tally(call), call.RL)
    assert t["pairs"][0] == call.n and t["insert"].sum() == call.n
    texts = S.fastq_texts(call)
    assert len(texts[0]) == S.LEDGER[call.name]["fastq bytes of mate 1"]
    for mate in (0, 1):
        lines = texts[mate].split(b"\n")
        assert len(lines) == 4 * call.n + 1 and lines[-1] == b""
        rid, first_i, _row, n = call.items[-1]
        assert lines[-5] == b"@%s_%d_%d/%d" % (rid.encode(), first_i + n - 1, S.CPU, mate + 1)
        seq = np.frombuffer(b"".join(lines[1::4]), dtype=np.uint8).reshape(call.n, call.RL)
        phred = np.frombuffer(b"".join(lines[3::4]), dtype=np.uint8).reshape(call.n, call.RL) - 33
        assert np.array_equal(seq, call.bases[:, mate]) and np.array_equal(phred, call.qual[:, mate])
        assert np.array_equal(t["qual"][mate, :, :].argmax(axis=1), [np.bincount(phred[:, p]).argmax() for p in range(call.RL)])
        assert (t["qual"][mate].sum(axis=1) == call.n).all() and (t["base"][mate].sum(axis=1) == call.n).all()
        assert t["base"][mate, :, 2].sum() == np.isin(seq, np.frombuffer(b"Gg", dtype=np.uint8)).sum()


def test_depth_and_origins_say_the_same(call, tmp_path):
    """The depth marked from the coordinates against the depth of the intervals parsed back out of the origins text."""
    from insilicoseq_amd import depth as D
    from insilicoseq_amd import origins as G

    table, n_words, diff, depth, stats, bins = S.depth(call)
    path = tmp_path / "o.bedpe"
    path.write_bytes(S.origins_text(call))
    parsed = G.parse(str(path))
    assert len(parsed["isz"]) == call.n and np.array_equal(parsed["isz"], call.coords[:, 3])
    rid, first_i, _row, n = call.items[-1]
    assert parsed["name"][-1] == "%s_%d_%d" % (rid, first_i + n - 1, S.CPU)
    coords, item, ids = G.intervals_for_depth(parsed)
    assert ids == [it[0] for it in call.items]
    again = D.mark_host(np.zeros(n_words, dtype=np.int32), coords, item, table, 0)
    assert np.array_equal(again, diff)
    assert int(depth.sum()) == int(stats[:, 0].sum()) == int(bins.sum()) == int((parsed["e1"] - parsed["s1"] + parsed["e2"] - parsed["s2"]).sum())
    assert (stats[:, 3] >= 2).all()


def test_ubam_records_parse_back_to_the_arrays():
    import ubam_twin as U

    call = S.expected("mt")  # (the smallest case: the parser is a loop over records)
    parsed = U.parse_records(S.ubam_records(call))
    assert len(parsed) == 2 * call.n
    assert [p[1] for p in parsed[:4]] == [77, 141, 77, 141] and parsed[-1][0] == b"rec.1_%d_%d" % (call.n - 1, S.CPU)
    assert np.array_equal(np.stack([p[3] for p in parsed]).reshape(call.n, 2, call.RL), call.qual)
    assert b"".join(p[2] for p in parsed) == call.bases.tobytes().upper()
