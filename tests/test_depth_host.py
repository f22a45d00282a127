"""insilicoseq_amd.depth without a GPU: the accumulator's layout, the numpy twins of the device's depth kernels against a plain
per-base loop, the merge of the workers' accumulators, the tables `generate --depth` writes and the command line."""
import numpy as np
import pytest

from insilicoseq_amd import depth as D

RL = 151


def _loop_depth(coords, item, table, read_length):
    """Per-base depth by the definition, one base at a time: {table row: [depth of every base]}."""
    out = {k: [0] * int(ln) for k, (off, ln) in enumerate(table.tolist()) if off >= 0}
    total = {k: 0 for k in out}
    for (fs, rs, re, _isz), k in zip(coords.tolist(), item):
        if k not in out:
            continue
        ln = int(table[k, 1])
        for s, e in ((fs, fs + read_length), (rs, re)):
            s, e = min(max(s, 0), ln), min(max(e, 0), ln)
            for x in range(s, e):
                out[k][x] += 1
            total[k] += max(e - s, 0)
    return out, total


def test_depth_table():
    for lengths in ([1], [RL], [RL + 1], [1, RL, RL + 1, 7, 4096, 2]):
        table, n_words = D.depth_table(lengths)
        assert table.dtype == np.int64 and table.shape == (len(lengths), 2)
        assert table[:, 1].tolist() == lengths and table[0, 0] == 0
        assert n_words == sum(lengths) + len(lengths)
        ends = table[:, 0] + table[:, 1] + 1  # one past the sink
        assert ends[:-1].tolist() == table[1:, 0].tolist() and ends[-1] == n_words
    table, n_words = D.depth_table([])
    assert table.shape == (0, 2) and n_words == 0
    with pytest.raises(ValueError):
        D.depth_table([3, -1])


def _hand_made():
    """Three records in use and one skipped row; coordinates (fs, rs, re, isz) with rs = re - RL as the engine gives them."""
    table, n_words = D.depth_table([400, RL + 1, 1000])
    table = np.concatenate([table, [[-1, 500]]]).astype(np.int64)
    rows = [
        (0, 400 - RL, 400, 400, 0),            # touching 0 and len
        (100, 150, 150 + RL, 201, 0),          # forward and reverse overlapping
        (0, -31, RL - 31, 120, 0),             # rs < 0: clamped, not wrapped
        (300, 300, 300 + RL, 151, 0),          # re > len
        (380, 380 - RL + 10, 390, 10, 0),      # forward cut by the record's end
        (10, 500, 500 + RL, 641, 0),           # wholly outside: rs >= len
        (50, -200, -200 + RL, -99, 0),         # re <= 0 with rs < 0: empty
        (0, 1, RL + 1, RL + 1, 1),             # the record of RL + 1 bases: the reverse interval ends in the sink
        (1, 0, RL, RL, 1),
        (0, 1000 - RL, 1000, 1000, 2),         # amplicon geometry: the whole record is the template
        (0, 1000 - RL, 1000, 1000, 2),
        (17, 600, 600 + RL, 734, 3),           # an item with offset -1
    ]
    coords = np.array([r[:4] for r in rows], dtype=np.int64)
    item = [r[4] for r in rows]
    return table, n_words, coords, item


def test_mark_and_finish_against_the_loop():
    table, n_words, coords, item = _hand_made()
    diff = np.zeros(n_words, dtype=np.int32)
    assert D.mark_host(diff, coords, item, table, RL) is diff
    for off, ln in table.tolist():
        if off >= 0:
            assert diff[off:off + ln + 1].sum() == 0  # every record's words sum to zero
    assert diff[table[1, 0] + table[1, 1]] == -2      # the sink of the RL + 1 record took both reverse ends
    exp, total = _loop_depth(coords, item, table, RL)
    for bin in (0, 1, 7, 64, 1000, 5000):
        depth, stats, bins = D.finish_host(diff, table, bin)
        assert depth.dtype == np.uint32 and stats.dtype == np.uint64 and stats.shape == (4, 4)
        first = 0
        for k, (off, ln) in enumerate(table.tolist()):
            w = int(D.n_windows(table, bin)[k])
            if off < 0:
                assert stats[k].tolist() == [0, 0, 0, 0]
                assert bin == 0 or not bins[first:first + w].any()
                first += w
                continue
            d = exp[k]
            assert depth[off:off + ln].tolist() == d and depth[off + ln] == 0
            assert stats[k].tolist() == [sum(d), sum(x * x for x in d), sum(1 for x in d if x), max(d)]
            assert int(stats[k, 0]) == total[k]  # = the sum of the clamped interval lengths
            if bin:
                assert w == -(-ln // bin)
                assert bins[first:first + w].tolist() == [sum(d[i:i + bin]) for i in range(0, ln, bin)]  # (the last one short)
                assert int(bins[first:first + w].sum()) == int(stats[k, 0])
            first += w
        if bin:
            assert bins.dtype == np.uint64 and bins.shape == (first,)
        else:
            assert bins is None
    # depth >= 2 where forward and reverse overlap; a scalar item serves all pairs
    assert max(exp[0]) >= 2
    one = np.zeros(n_words, dtype=np.int32)
    D.mark_host(one, coords[:7], 0, table, RL)
    two = np.zeros(n_words, dtype=np.int32)
    D.mark_host(two, coords[:7], item[:7], table, RL)
    assert np.array_equal(one, two)


def test_finish_refuses_a_prefix_out_of_range():
    with pytest.raises(ValueError):
        D.finish_host(np.array([-1, 1], dtype=np.int32), np.array([[0, 1]]), 0)


def test_merge_of_two_workers_sharing_a_record():
    table, n_words, coords, item = _hand_made()
    table = table[:3]
    whole = np.zeros(n_words, dtype=np.int32)
    D.mark_host(whole, coords[:11], item[:11], table, RL)
    # worker A: records 2 and 0 (in that order) with pairs 0..4, 9, 10; worker B: records 0 and 1 with pairs 5..8 -- record 0 is shared
    ta, na = D.depth_table([1000, 400])
    tb, nb = D.depth_table([400, RL + 1])
    a, b = np.zeros(na, dtype=np.int32), np.zeros(nb, dtype=np.int32)
    D.mark_host(a, coords[[0, 1, 2, 3, 4, 9]], [1, 1, 1, 1, 1, 0], ta, RL)
    D.mark_host(b, coords[[5, 6, 7, 8]], [0, 0, 1, 1], tb, RL)
    D.mark_host(a, coords[[10]], [0], ta, RL)
    merged = np.zeros(n_words, dtype=np.int32)
    D.merge_into(merged, table, a, ta, [2, 0])
    D.merge_into(merged, table, b, tb, [0, 1])
    assert np.array_equal(merged, whole)
    with pytest.raises(ValueError):
        D.merge_into(merged, table, b, tb, [1, 0])  # lengths differ
    with pytest.raises(ValueError):
        D.merge_into(merged, table, b, tb, [0])


def test_rows_and_writers(tmp_path):
    table, n_words = D.depth_table([4, 3, 0])
    diff = np.zeros(n_words, dtype=np.int32)
    # record 0: depths 1 3 3 0; record 1: 2 2 2
    for s, e in ((0, 3), (1, 3), (1, 3)):
        diff[s] += 1
        diff[e] -= 1
    diff[table[1, 0]] += 2
    diff[table[1, 0] + 3] -= 2
    depth, stats, bins = D.finish_host(diff, table, 2)
    assert depth.tolist() == [1, 3, 3, 0, 0, 2, 2, 2, 0, 0]
    rows = D.depth_rows(stats, table, ["a", "b", "c"])
    assert rows[0] == ("a", 4, 1.75, 19 / 4 - 1.75 ** 2, 0.75, 3)
    assert rows[1] == ("b", 3, 2.0, 0.0, 1.0, 2)
    assert rows[2] == ("c", 0, 0.0, 0.0, 0.0, 0)
    path = str(tmp_path / "d.txt")
    D.write_depth_table(path, rows)
    lines = open(path).read().split("\n")
    assert lines[0] == "id\tlength\tmean_depth\tdepth_variance\tcovered_fraction\tmax_depth"
    assert lines[1] == "a\t4\t1.75\t1.6875\t0.75\t3" and lines[2] == "b\t3\t2.0\t0.0\t1.0\t2" and lines[3] == "c\t0\t0.0\t0.0\t0.0\t0"
    assert lines[4:] == [""]
    assert bins.tolist() == [4, 3, 4, 2]
    assert D.bin_means(bins, table, 2) == [(0, 0, 2, 2.0), (0, 2, 4, 1.5), (1, 0, 2, 2.0), (1, 2, 3, 2.0)]
    bed = str(tmp_path / "d.bedgraph")
    D.write_bedgraph(bed, bins, table, ["a", "b", "c"], 2)
    assert open(bed).read() == "a\t0\t2\t2.0\na\t2\t4\t1.5\nb\t0\t2\t2.0\nb\t2\t3\t2.0\n"


def test_marked_pairs_are_bounded():
    from insilicoseq_amd._native import E_INVALID, EngineError

    assert D.count_marked(0, 5) == 5 and D.count_marked((1 << 30) - 1, 1) == 1 << 30
    with pytest.raises(EngineError) as e:
        D.count_marked(1 << 30, 1)
    assert e.value.code == E_INVALID


def test_command_line_takes_the_flags(monkeypatch):
    from insilicoseq_amd import app

    seen = []
    monkeypatch.setattr(app, "generate_reads", seen.append)
    app.main(["generate", "-o", "out", "--genomes", "g.fasta", "--depth"])
    app.main(["generate", "-o", "out", "--genomes", "g.fasta", "--depth_bin", "100"])
    app.main(["generate", "-o", "out", "--genomes", "g.fasta"])
    assert [(a.depth, a.depth_bin) for a in seen] == [(True, None), (False, 100), (False, None)]
