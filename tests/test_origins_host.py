"""`generate --origins` without a GPU: the twin (insilicoseq_amd.origins.lines_host) against the definition spelled out pair by pair,
the host formatter iss_origins_host_text against the twin, the parser, the depth the intervals stand for, and the command line."""
import gzip
import os

import numpy as np
import pytest

from insilicoseq_amd import depth as D
from insilicoseq_amd import origins as G

RL = 100
LEN = 100000 + RL  # a record on which the starts 99 999 / 100 000 are still inside

# (fs, rs, re, isz): hand-made rows, what each is there for
HAND = [
    (9, 300, 400, 191),               # a start of one digit ...
    (10, 300, 400, 190),              # ... and of two
    (99, 1000, 1100, 801),            # two / three
    (100, 1000, 1100, 800),
    (99999, 50000, 50100, -50099),    # five / six; a negative isz
    (100000, 50000, 50100, -50100),   # e1 == len
    (0, LEN - RL, LEN, LEN - 2 * RL),  # fs == 0, e2 == len
    (5, -30, 70, -135),               # rs < 0: the clamped start
    (5, -200, -100, -305),            # the whole reverse interval in front of the record: empty at 0
    (LEN - 10, LEN - 50, LEN + 50, 0),  # e1 and re beyond the record's end
    (LEN + 5, LEN + 7, LEN + 107, 2),   # both intervals behind the record: empty at len
    (40, 500, 500, 360),              # re == rs
    (40, 500, 450, -1),               # re < rs: written "500 500"
]


def by_definition(items, lengths, cpu, coords, read_length):
    """The file's definition, one pair at a time with "%d"."""
    out, at = [], 0
    for (rid, first_i, _row, n), ln in zip(items, lengths):
        rid = rid.decode() if isinstance(rid, bytes) else rid
        for j in range(n):
            fs, rs, re, isz = (int(x) for x in coords[at])
            at += 1
            s1 = min(max(fs, 0), ln)
            e1 = max(min(max(fs + read_length, 0), ln), s1)
            s2 = min(max(rs, 0), ln)
            e2 = max(min(max(re, 0), ln), s2)
            out.append("%s\t%d\t%d\t%s\t%d\t%d\t%s_%d_%d\t.\t+\t-\t%d\n" % (rid, s1, e1, rid, s2, e2, rid, first_i + j, cpu, isz))
    return "".join(out).encode()


def random_coords(n, ln, read_length, seed):
    """Rows like the engine's, with some that reach over either end of the record."""
    rng = np.random.RandomState(seed)
    fs = rng.randint(-read_length, ln + 5, size=n)
    re = rng.randint(-5, ln + read_length, size=n)
    rs = re - read_length
    return np.stack([fs, rs, re, rs - fs - read_length], axis=1).astype(np.int64)


def test_twin_is_the_definition():
    coords = np.asarray(HAND, dtype=np.int64)
    items = [("NZ_CP012345.1", 0, 0, len(HAND))]
    text = G.lines_host(items, [LEN], 2, coords, RL)
    assert text == by_definition(items, [LEN], 2, coords, RL)
    lines = text.decode().split("\n")
    assert lines[0] == "NZ_CP012345.1\t9\t109\tNZ_CP012345.1\t300\t400\tNZ_CP012345.1_0_2\t.\t+\t-\t191"
    assert lines[5].split("\t")[1:3] == ["100000", str(LEN)] and lines[5].split("\t")[10] == "-50100"
    assert lines[6].split("\t")[1:3] == ["0", "100"] and lines[6].split("\t")[5] == str(LEN)
    assert lines[7].split("\t")[4:6] == ["0", "70"]
    assert lines[8].split("\t")[4:6] == ["0", "0"]
    assert lines[9].split("\t")[1:3] == [str(LEN - 10), str(LEN)] and lines[9].split("\t")[4:6] == [str(LEN - 50), str(LEN)]
    assert lines[10].split("\t")[1:6] == [str(LEN), str(LEN), "NZ_CP012345.1", str(LEN), str(LEN)]
    assert lines[11].split("\t")[4:6] == ["500", "500"] and lines[12].split("\t")[4:6] == ["500", "500"]
    assert lines[12].split("\t")[10] == "-1" and lines[-1] == "" and len(lines) == len(HAND) + 1
    # several items, a zero-pair item between two others, bytes ids
    items = [("a", 7, 0, 5), (b"zero", 3, 5, 0), ("c" * 17, 95, 5, 8)]
    assert G.lines_host(items, [LEN, 50, 400], 123, coords, RL) == by_definition(items, [LEN, 50, 400], 123, coords, RL)
    assert G.lines_host([], [], 0, np.zeros((0, 4)), RL) == b""
    with pytest.raises(ValueError):
        G.lines_host(items, [LEN, 50, 400], 123, coords[:-1], RL)


@pytest.mark.parametrize("cpu", [0, 123])
@pytest.mark.parametrize("first_i,n", [(7, 5), (95, 10)])
@pytest.mark.parametrize("rid", ["g", "NZ_CP0123456789.1", "x" * 200])
def test_host_formatter_equals_the_twin(tmp_path, rid, first_i, n, cpu):
    from insilicoseq_amd import _native

    assert len(rid) in (1, 17, 200)
    for k, (coords, ln, rl) in enumerate(((np.asarray(HAND[:n], dtype=np.int64), LEN, RL), (random_coords(n, 700, 151, 3 * n + cpu), 700, 151))):
        path = tmp_path / ("text%d.bedpe" % k)
        with open(path, "wb") as fh:
            fh.write(b"in front\n")
            fh.flush()
            assert _native.lib().iss_origins_host_text(fh.fileno(), rid.encode(), first_i, cpu, n, rl, ln, coords.ctypes.data) == 0
        want = G.lines_host([(rid, first_i, 0, n)], [ln], cpu, coords, rl)
        assert open(path, "rb").read() == b"in front\n" + want and want.count(b"\n") == n


def test_host_formatter_beyond_32_bits(tmp_path):
    """Coordinates, a record length and pair ids that need more than 32 bits (the engine takes records of up to 2^34 - 4096 bases)."""
    from insilicoseq_amd import _native

    ln, rl = (1 << 34) - 4096, 151
    coords = np.asarray([[(1 << 32) - 100, (1 << 32) + 7, (1 << 32) + 7 + rl, 107 - rl], [(1 << 33) + 5, ln - 10, ln + 141, 0],
                         [9999999999, 10000000000, 10000000151, -150], [4294967295, 4294967296, 4294967447, 1 - rl],
                         [5, -(1 << 33), -(1 << 33) + rl, -(1 << 33) - 5 - rl]], dtype=np.int64)
    first_i = (1 << 32) - 3
    path = tmp_path / "wide.bedpe"
    with open(path, "wb") as fh:
        assert _native.lib().iss_origins_host_text(fh.fileno(), b"chr1", first_i, 7, len(coords), rl, ln, coords.ctypes.data) == 0
    want = G.lines_host([("chr1", first_i, 0, len(coords))], [ln], 7, coords, rl)
    assert open(path, "rb").read() == want == by_definition([("chr1", first_i, 0, len(coords))], [ln], 7, coords, rl)
    assert b"chr1_4294967295_7" in want and b"chr1_4294967296_7" in want and b"\t-8589934748\n" in want


def test_host_formatter_refuses(tmp_path):
    from insilicoseq_amd import _native

    L, c = _native.lib(), np.zeros((2, 4), dtype=np.int64)
    with open(tmp_path / "t", "wb") as fh:
        assert L.iss_origins_host_text(fh.fileno(), b"r", 0, 0, 2, 100, 0, c.ctypes.data) == _native.E_INVALID  # record_len < 1
        assert L.iss_origins_host_text(fh.fileno(), b"r", 0, 0, 2, 0, 10, c.ctypes.data) == _native.E_INVALID
        assert L.iss_origins_host_text(fh.fileno(), b"r", 0, 0, 2, 100, 10, None) == _native.E_INVALID
        assert L.iss_origins_host_text(fh.fileno(), b"r", 0, 0, 0, 100, 10, None) == 0
    assert os.path.getsize(tmp_path / "t") == 0


def test_parse_and_depth(tmp_path):
    """The parser gives the numbers back; the depth of the parsed intervals is the depth of the coordinates (the --depth rule)."""
    ids, lengths, counts, rl = ["rec0", "rec.1", "r2"], [700, 152, 5000], [200, 40, 300], 151
    coords = np.concatenate([random_coords(n, ln, rl, 50 + k) for k, (n, ln) in enumerate(zip(counts, lengths))])
    items, row = [], 0
    for rid, n in zip(ids, counts):
        items.append((rid, 10 * row, row, n))
        row += n
    text = G.lines_host(items, lengths, 4, coords, rl)
    for name, opener in (("o_origins.bedpe", open), ("o_origins.bedpe.gz", gzip.open)):
        with opener(tmp_path / name, "wb") as fh:
            fh.write(text)
        p = G.parse(str(tmp_path / name))
        item = np.repeat(np.arange(3), counts)
        ln = np.asarray(lengths)[item]
        s1, e1 = G.clamp(coords[:, 0], coords[:, 0] + rl, ln)
        s2, e2 = G.clamp(coords[:, 1], coords[:, 2], ln)
        for key, want in (("s1", s1), ("e1", e1), ("s2", s2), ("e2", e2), ("isz", coords[:, 3])):
            assert p[key].dtype == np.int64 and np.array_equal(p[key], want), key
        assert p["id"].tolist() == np.asarray(ids, dtype=object)[item].tolist()
        assert p["name"][0] == "rec0_0_4" and p["name"][-1] == "r2_%d_4" % (2400 + 299)
        # the text written from the parsed arrays is the file
        again = "".join("%s\t%d\t%d\t%s\t%d\t%d\t%s\t.\t+\t-\t%d\n" % (i, a, b, i, c, d, nm, z) for i, a, b, c, d, nm, z in zip(
            p["id"], p["s1"], p["e1"], p["s2"], p["e2"], p["name"], p["isz"]))
        assert again.encode() == text
    table, n_words = D.depth_table(lengths)
    want = D.mark_host(np.zeros(n_words, dtype=np.int32), coords, item, table, rl)
    c2, item2, ids2 = G.intervals_for_depth(p)
    assert ids2 == ids and c2.shape == (2 * len(coords), 4)
    got = D.mark_host(np.zeros(n_words, dtype=np.int32), c2, item2, table, 0)
    assert np.array_equal(got, want) and want.any()
    depth, stats, _bins = D.finish_host(got, table)
    total = int((p["e1"] - p["s1"]).sum() + (p["e2"] - p["s2"]).sum())
    assert total == int(stats[:, 0].sum()) and total > 0
    # records named in another order than the file meets them
    c3, item3, ids3 = G.intervals_for_depth(p, ids=ids[::-1])
    t3, _ = D.depth_table(lengths[::-1])
    got3 = D.mark_host(np.zeros(n_words, dtype=np.int32), c3, item3, t3, 0)
    assert D.finish_host(got3, t3)[1][::-1].tolist() == stats.tolist()
    with open(tmp_path / "bad.bedpe", "w") as fh:
        fh.write("a\t1\t2\tb\t3\t4\ta_0_0\t.\t+\t-\t5\n")
    with pytest.raises(ValueError):
        G.parse(str(tmp_path / "bad.bedpe"))


def test_cli_parses_origins():
    from insilicoseq_amd import app

    p = app.build_parser()
    assert p.parse_args(["generate", "-g", "x.fa", "-o", "out"]).origins is False
    args = p.parse_args(["generate", "-g", "x.fa", "-o", "out", "--origins", "--ubam", "--depth", "--report", "--store_mutations"])
    assert args.origins is True and args.ubam is True


def test_cli_refuses_the_host_formatter(tmp_path, caplog, monkeypatch):
    """ISS_HOST_FASTQ=1 with --origins: one error line and exit status 1, before anything is read or written."""
    from insilicoseq_amd import app

    monkeypatch.setenv("ISS_HOST_FASTQ", "1")
    with pytest.raises(SystemExit) as e:
        app.main(["generate", "-g", str(tmp_path / "none.fa"), "-o", str(tmp_path / "out"), "--origins", "--seed", "3", "--mode", "basic"])
    assert e.value.code == 1
    lines = [r.getMessage() for r in caplog.records if r.levelname == "ERROR"]
    assert len(lines) == 1 and "--origins" in lines[0] and "ISS_HOST_FASTQ" in lines[0] and "\n" not in lines[0]
    assert os.listdir(tmp_path) == []


def test_worker_iterator_refuses_the_host_formatter(tmp_path, monkeypatch):
    from insilicoseq_amd.generator import worker_iterator

    monkeypatch.setenv("ISS_HOST_FASTQ", "1")
    with pytest.raises(ValueError):
        worker_iterator([], None, 0, str(tmp_path / "w"), 1, "metagenomics", False, origins=True)
    assert os.listdir(tmp_path) == []


def test_origins_takes_the_pool_not_the_worker_set(monkeypatch):
    """Like --report: --rng mt --cpus W --devices 1 runs one process per worker with the flag (the set has no origins writer)."""
    from insilicoseq_amd import app

    monkeypatch.delenv("ISS_HOST_FASTQ", raising=False)
    p = app.build_parser()
    base = ["generate", "-g", "x.fa", "-o", "out", "--rng", "mt", "--cpus", "4", "--devices", "1", "--seed", "3"]
    assert app._worker_set_wanted(p.parse_args(base), False, False) is True
    assert app._worker_set_wanted(p.parse_args(base + ["--origins"]), False, False) is False


def test_assembly_and_gz_suffix(tmp_path):
    """The parent's part without a GPU: the workers' files in worker order under the final name, then --compress's .gz."""
    from insilicoseq_amd import app
    from insilicoseq_amd.distributed import concatenate_rank_files, temp_prefix

    assert app.ORIGINS_SUFFIX == G.SUFFIX == "_origins.bedpe"
    out = str(tmp_path / "run")
    parts = [G.lines_host([("r%d" % k, 0, 0, 3)], [500], k, random_coords(3, 500, 100, k), 100) for k in range(2)]
    for k, text in enumerate(parts):
        with open(temp_prefix(out, k) + G.SUFFIX, "wb") as fh:
            fh.write(text)
        open(temp_prefix(out, k) + ".vcf", "w").close()
    concatenate_rank_files(out, 2, suffixes=(G.SUFFIX,))
    assert sorted(os.listdir(tmp_path)) == ["run_origins.bedpe"]
    assert open(out + G.SUFFIX, "rb").read() == parts[0] + parts[1]
    assert app.compress_file(out + G.SUFFIX) == out + "_origins.bedpe.gz"
    assert sorted(os.listdir(tmp_path)) == ["run_origins.bedpe.gz"]
    assert gzip.open(out + "_origins.bedpe.gz", "rb").read() == parts[0] + parts[1]
    assert G.parse(out + "_origins.bedpe.gz")["name"].tolist() == ["r0_0_0", "r0_1_0", "r0_2_0", "r1_0_1", "r1_1_1", "r1_2_1"]
