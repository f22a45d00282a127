"""The member twin (tests/deflate_twin.py) pinned before it judges the device, and the precondition of every case of
tests/test_gpu_deflate_streams.py, all on the CPU: gzip.decompress(member) is the text (zlib verifies CRC-32 and ISIZE on the
way), a one-block member is the pinned one-block packer's bytes, and every case has the shape its row of the table says."""
import gzip
import zlib

import numpy as np
import pytest

import deflate_cases as K
import deflate_twin as T

CASES = K.cases()


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge

    ge.build()
    from insilicoseq_amd import _native

    return _native


@pytest.fixture(scope="module")
def rows():
    got = {}

    def get(RL):
        if RL not in got:
            got[RL] = K.oracle_rows(RL)
        return got[RL]

    return get


def record_lengths(text):
    lines = text.split(b"\n")[:-1]
    return [sum(len(x) + 1 for x in lines[k:k + 4]) for k in range(0, len(lines), 4)]


def built(native, rows, name, monkeypatch, mode="matches"):
    """Per emit call of the case: (items, distance, [text of mate 1, mate 2], [twin layout of mate 1, mate 2])."""
    RL, calls, modes = CASES[name]
    assert mode in modes
    monkeypatch.delenv("ISS_DEFLATE_RUNS_ONLY", raising=False)
    if mode == "runs only":
        monkeypatch.setenv("ISS_DEFLATE_RUNS_ONLY", "1")
    out = []
    for items in calls:
        dist = T.record_distance(items, RL, K.CPU)
        texts = [K.call_text(items, rows(RL), m) for m in (1, 2)]
        assert len(texts[0]) == len(texts[1]) == K.text_bytes(items, RL) <= 300 * 1024
        assert all(first + n <= K.ROWS[RL] for _, _, first, n in items)
        lay = [T.layout(native, t, dist) for t in texts]
        for t, m in zip(texts, lay):
            assert m["bytes"][:10] == T.HEAD and m["bytes"][:4] == b"\x1f\x8b\x08\x00"
            assert gzip.decompress(m["bytes"]) == t, name
        out.append((items, dist, texts, lay))
    return RL, out


def test_one_block_member_is_the_pinned_block(native):
    """member() packs with numpy; on one block it must give the bytes of _deflate_block, which zlib pins in test_host_cpu.py."""
    rng = np.random.RandomState(2)
    rec = b"@g_%d_2/1\n" + b"ACGTTTTTNNacgtACGTAAAACCCC\n+\n" + b"FFFFFFFFFFFFF:FFF,FFFFFFF#\n"
    fastq = b"".join(rec % (100 + k) for k in range(400))
    for data, dist in ((fastq, len(rec % 100)), (fastq, 0), (fastq[:17], 17), (b"A", 0), (bytes(rng.randint(0, 256, 9000).astype(np.uint8)), 1000),
                       (b"ab" + b"c" * 9 + b"dd" + b"e" * 3, 4), (b"F" * 32768, 8)):
        block, _ = T._deflate_block(native, data, dist=dist)
        want = T.HEAD + block + (zlib.crc32(data) & 0xffffffff).to_bytes(4, "little") + len(data).to_bytes(4, "little")
        assert T.member(native, data, dist) == want, (len(data), dist)
        assert gzip.decompress(want) == data


def test_block_boundaries_carry_predecessor_and_source(native):
    """Two members' worth of blocks: the tokens of a later block are those of _tokens over the whole text (a run and a record
    match that begin at a block's first byte), not those of the block tokenized alone."""
    text = (b"x" * 29 + b"ACG") * 3072  # 3 blocks of a 32-byte period: every chunk but the first is one match
    lay = T.layout(native, text, 64)
    assert len(lay["blocks"]) == 3 and gzip.decompress(lay["bytes"]) == text
    first_of_block_1 = lay["tokens"][lay["tokens"][:, 4] == T.BLOCK][0]
    assert first_of_block_1[1] == 2 and first_of_block_1[0] == 272  # a 32-byte record match across the block boundary
    alone = T.token_table(text[T.BLOCK:], 64)
    assert alone[0][1] == 0
    assert lay["hist"][256] == 3 and lay["hist"].sum() == len(lay["tokens"]) + 3


def test_record_distance_rule(monkeypatch):
    monkeypatch.delenv("ISS_DEFLATE_RUNS_ONLY", raising=False)
    assert T.record_distance([("g", 0, 0, 1)], 2, 2) == 17
    assert T.record_distance([("g", 0, 0, 1)], 2, 12) == 18
    assert T.record_distance([("ab", 0, 0, 5), ("g", 95, 0, 6), ("abc", 0, 0, 6)], 2, 2) == 19  # the first of the largest; 100: 3 digits
    assert T.record_distance([("ab", 0, 0, 0)], 2, 2) == 0 and T.record_distance([], 2, 2) == 0
    assert T.record_distance([(b"\xff" * 4096, 0, 0, 1)], 1024, 2) == 4096 + 1 + 2048 + 10 + 1
    assert T.record_distance([("k" * 4096, 0, 0, 1)], 14400, 2) == 0  # longer than the window
    monkeypatch.setenv("ISS_DEFLATE_RUNS_ONLY", "1")
    assert T.record_distance([("g", 0, 0, 1)], 2, 2) == 0
    assert [K.digits_before(x) for x in (0, 1, 10, 11, 100, 1001)] == [0, 1, 10, 12, 190, 2894]


def test_one_record(native, rows, monkeypatch):
    RL, ((items, dist, texts, lay),) = built(native, rows, "one_record", monkeypatch)
    assert len(texts[0]) == 17 and dist == 17  # one partial chunk, and no byte has a source: at < dist everywhere
    assert all((m["tokens"][:, 1] != 2).all() and len(m["blocks"]) == 1 for m in lay)


@pytest.mark.parametrize("RL", [5, 8])
def test_short_records(native, rows, monkeypatch, RL):
    name = "short_records_%d" % RL
    _, ((items, dist, texts, lay),) = built(native, rows, name, monkeypatch)
    _, ((_, dist0, texts0, lay0),) = built(native, rows, name, monkeypatch, "runs only")
    lengths = set(record_lengths(texts[0]) + record_lengths(texts[1]))
    assert len(lengths) == 3 and all(17 <= x <= 31 for x in lengths), sorted(lengths)  # the match source overlaps its own chunk
    assert dist == max(lengths) and dist0 == 0 and texts == texts0
    for a, b in zip(lay, lay0):
        assert a["bytes"] != b["bytes"] and (a["tokens"][:, 1] == 2).any() and not (b["tokens"][:, 1] == 2).any()


@pytest.mark.parametrize("name,rest", [("block_multiple", (0, 0)), ("block_plus_sliver", (1, 31)), ("block_minus_sliver", (T.BLOCK - 31, T.BLOCK - 1))])
def test_block_edges(native, rows, monkeypatch, name, rest):
    RL, ((items, dist, texts, lay),) = built(native, rows, name, monkeypatch)
    n = len(texts[0])
    assert n >= 2 * T.BLOCK - 31 and rest[0] <= n % T.BLOCK <= rest[1], (n, items[0][1:])
    assert len(lay[0]["blocks"]) == (n + T.BLOCK - 1) // T.BLOCK >= 2
    assert (n % T.CHUNK != 0) == (name != "block_multiple")  # a partial last chunk, alone in its block behind k full ones or not
    assert len(set(record_lengths(texts[0]))) >= 2  # (the pair numbers change their width inside the member)


def test_shipped_shape(native, rows, monkeypatch, capsys):
    RL, ((items, dist, texts, lay),) = built(native, rows, "shipped_shape", monkeypatch)
    assert set(record_lengths(texts[0])) == {dist - 1, dist}  # 999 -> 1000 inside the member
    for m in lay:
        assert len(m["blocks"]) >= 6 and set(m["tokens"][:, 1].tolist()) == {0, 1, 2}
    with capsys.disabled():
        for k, (t, m) in enumerate(zip(texts, lay)):
            z1, z6 = len(zlib.compress(t, 1)), len(zlib.compress(t, 6))
            print("\nshipped_shape mate %d: text %d bytes, twin member %d (%.3f of the text), zlib level 1 %d (%.3f), level 6 %d (%.3f)" % (
                k + 1, len(t), len(m["bytes"]), len(m["bytes"]) / len(t), z1, z1 / len(t), z6, z6 / len(t)))


def test_run_at_block_edge(native, rows, monkeypatch):
    """A run of >= 3 bytes that wins (r1 >= rd) begins at the first byte of a FULL block b > 0 and continues the previous block's
    last byte: the one place where the predecessor k_deflate_len's staged path takes from outside its LDS stage decides a token."""
    RL, ((items, dist, texts, lay),) = built(native, rows, "run_at_block_edge", monkeypatch)
    at = T.BLOCK
    for t, m in zip(texts, lay):
        assert len(t) >= 2 * T.BLOCK and t[at - 1] == t[at] == t[at + 1] == t[at + 2]
        tok = m["tokens"]
        chunk = tok[(tok[:, 4] >= at) & (tok[:, 4] < at + T.CHUNK)]
        assert chunk[0][4] == at and chunk[0][1] == 1, chunk[0]
        # the same chunk without its predecessor (another byte in front of the block; the source `dist` earlier stays): other tokens
        assert dist > T.CHUNK
        other = T.token_table(t[:at - 1] + bytes([t[at - 1] ^ 0x20]) + t[at:at + T.CHUNK], dist)
        other = other[other[:, 4] >= at]
        assert other[0][1] != 1 and other[:, :4].tolist() != chunk[:, :4].tolist()


def test_deep_code(native, rows, monkeypatch):
    RL, ((items, dist, texts, lay),) = built(native, rows, "deep_code", monkeypatch)
    rid = items[0][0]
    assert len(items) == 1 and len(rid) <= 4096 and len(set(rid)) == 16 and all(a != b for a, b in zip(rid, rid[1:]))
    for m in lay:
        # the unlimited tree of the twin's histogram, and of the counts deflate_build_code makes of it (every symbol keeps a code):
        # both deeper than 15, so the lengths clamped to 15 overfill the code space and the step-by-step repair has to run
        assert max(T.huffman_depths(m["hist"]).values()) > 15
        depth = T.huffman_depths(T.smoothed(m["hist"]))
        assert len(depth) == T.SYMS and max(depth.values()) > 15, max(depth.values())
        assert sum(2.0 ** -min(d, 15) for d in depth.values()) > 1.0
        assert sum(int(m["hist"][c]) for c in set(rid)) < 0.05 * int(m["hist"].sum())  # rare against the bases, phreds and digits
        # the repair in plain Python is the builder's on one lane ...
        entry = T.code_tables(native, m["hist"], dist)[0]
        length, steps = T.limited_lengths(T.smoothed(m["hist"]))
        assert length == (entry >> 16).tolist() and max(length) == 15 and sum(2.0 ** -x for x in length) == 1.0
        # ... and it stops inside a tie: 64 lanes whose proposals were merged in lane order would build ANOTHER code
        other, other_steps = T.limited_lengths(T.smoothed(m["hist"]), lanes=64)
        assert other != length and sum(2.0 ** -x for x in other) == 1.0
        assert any(a[0] != b[0] and a[1] >= 2 for a, b in zip(steps, other_steps))


def test_many_symbols(native, rows, monkeypatch):
    RL, ((items, dist, texts, lay),) = built(native, rows, "many_symbols", monkeypatch)
    sizes = [len(it[0]) for it in items]
    assert min(sizes) == 200 and max(sizes) == 4096 and all(it[3] == 1 for it in items)
    assert not any(b"\n" in it[0] or b"\0" in it[0] for it in items)
    for m in lay:
        literal = m["tokens"][m["tokens"][:, 1] == 0]
        assert len(set(literal[:, 0].tolist())) >= 200 and len(literal) >= 0.95 * len(m["tokens"]) and len(m["blocks"]) >= 3
        # (the host's capacity rule for the compressed bytes, at the text that comes closest to it)
        assert len(m["bytes"]) <= len(texts[0]) + len(texts[0]) // 8 + len(m["blocks"]) * 320 + 64


def test_most_pairs_not_first(native, rows, monkeypatch):
    RL, ((items, dist, texts, lay),) = built(native, rows, "most_pairs_not_first", monkeypatch)
    assert len(items) == 3 and len(set(len(it[0]) for it in items)) == 3 and items[1][3] > max(items[0][3], items[2][3])
    assert dist != T.record_distance(items[:1], RL, K.CPU) and dist == T.record_distance(items[1:2], RL, K.CPU)
    assert T.layout(native, texts[0], T.record_distance(items[:1], RL, K.CPU))["bytes"] != lay[0]["bytes"]


def test_slot_reuse(native, rows, monkeypatch):
    RL, calls = built(native, rows, "slot_reuse", monkeypatch)
    assert len(calls) == 4
    for mate in (0, 1):
        hists = [c[3][mate]["hist"] for c in calls]
        assert all(not np.array_equal(hists[a], hists[b]) for a in range(4) for b in range(a))
        whole = b"".join(c[3][mate]["bytes"] for c in calls)
        assert gzip.decompress(whole) == b"".join(c[2][mate] for c in calls)
    # the first call is the largest: the later ones reuse its buffers, and a slot's second member is shorter than its first
    assert len(calls[0][2][0]) > len(calls[2][2][0]) and len(calls[1][2][0]) < len(calls[3][2][0]) < len(calls[0][2][0])


def test_describe_difference_names_the_part(native):
    text = (b"@r_%d_2/1\nACGTNNNN\n+\nFFFFFFF#\n" * 3000) % tuple(range(3000))
    lay = T.layout(native, text, 30)
    good = lay["bytes"]
    assert len(lay["blocks"]) == 3

    def broken(at):
        return good[:at] + bytes([good[at] ^ 0x10]) + good[at + 1:]

    second = lay["blocks"][1]
    assert "member 1 of 2, block 1 of 3" in T.describe_difference(good + broken(second + 2), [lay, lay])
    assert "header bits (the code)" in T.describe_difference(broken(second + 2), [lay])
    assert "block 1 of 3" in T.describe_difference(broken(second + lay["hdr_bits"] // 8 + 9), [lay])
    assert "the tokens behind" in T.describe_difference(broken(second + lay["hdr_bits"] // 8 + 9), [lay])
    assert "block 0 of 3" in T.describe_difference(broken(second - 1), [lay])
    assert "CRC-32" in T.describe_difference(broken(len(good) - 3), [lay])
    assert "first difference at byte %d" % (len(good) - 2) in T.describe_difference(good[:-2], [lay])
