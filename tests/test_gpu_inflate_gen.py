"""k_bgzf_inflate on the MI355X against the generated corpus and the damaged streams of tests/inflate_gen.py: what exists only at 64
lanes.  The host leg (tests/test_inflate_gen_host.py) holds the same bytes -- tied by the corpus digest -- against zlib and runs them
through the sanitizer-built host twin; here the device has to give the corpus' bytes, for every damaged stream a status that zlib's
verdict allows and that equals the twin's (tests/golden/inflate_gen/twin_status.npz), the same result for a member whatever stood
before it in its wave (a wave's Work -- ring, tables, code lengths -- survives from one member to the next, a bad one included), at
every alignment of a member's output and payload, and in several feeds as in one.  No tolerance anywhere."""
import os
import struct
import time
import zlib

import numpy as np
import pytest
import torch  # noqa: F401  (when the module is collected: torch's HIP runtime has to be the process's first, see test_gpu_tensors.py)

import inflate_cases as IC
import inflate_gen as G

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inflate_gen", "twin_status.npz")
WHOLE = (IC.OK, IC.TRAILING, IC.CRC)  # the statuses behind which all of a member's bytes were produced


@pytest.fixture(scope="module")
def Z():
    import __graft_entry__ as ge

    ge.build()
    from insilicoseq_amd import inflate

    return inflate


@pytest.fixture(scope="module")
def inf(Z):
    with Z.BgzfInflater(0) as d:
        yield d


@pytest.fixture()
def fresh(inf):
    inf.reset()
    return inf


@pytest.fixture(scope="module")
def corpus():
    return G.corpus()


@pytest.fixture(scope="module")
def damaged():
    """(cases, zlib's verdicts, the host twin's statuses)."""
    fixture = np.load(FIXTURE)
    assert fixture["digest"].tobytes().decode() == G.digest(), "the fixture is of another corpus"
    cases = G.damage()
    assert fixture["status"].size == len(cases)
    return cases, G.verdicts(), fixture["status"]


def feed(Z, inf, cases):
    blob = b"".join(c["member"] for c in cases)
    members, used = Z.scan(blob)
    assert used == len(blob) and members.offset.size == len(cases)
    inf.feed(blob, members)
    return members


def pieces(data, members):
    """The bytes of every member of a collected group."""
    ends = np.cumsum(members.isize.astype(np.int64))
    assert data.size == (int(ends[-1]) if ends.size else 0)
    return [data[int(e) - int(n):int(e)] for e, n in zip(ends, members.isize)]


def test_whole_corpus_in_one_feed(Z, fresh, corpus):
    t0 = time.time()
    members = feed(Z, fresh, corpus)
    data, status = fresh.collect()
    wall = time.time() - t0
    print("\ncorpus feed: %d members, %d -> %d bytes, wall %.1f ms, kernel %.2f ms" %
          (len(corpus), sum(len(c["member"]) for c in corpus), data.size, 1e3 * wall, fresh.kernel_ms()))
    bad = [(c["name"], IC.STATUS_NAMES[s]) for c, s in zip(corpus, status) if s]
    assert not bad, bad[:10]
    for c, got in zip(corpus, pieces(data, members)):
        assert got.tobytes() == c["data"], c["name"]
    assert fresh.first_bad() == (-1, 0)


def test_damaged_streams_in_one_feed(Z, fresh, damaged):
    cases, verdicts, twin = damaged
    t0 = time.time()
    members = feed(Z, fresh, cases)
    data, status = fresh.collect()
    print("\ndamaged feed: %d members, wall %.1f ms, kernel %.2f ms" % (len(cases), 1e3 * (time.time() - t0), fresh.kernel_ms()))
    for c, (outcome, allowed, want), s, t, got in zip(cases, verdicts, status.tolist(), twin.tolist(), pieces(data, members)):
        assert s in allowed, (c["name"], outcome, [IC.STATUS_NAMES[a] for a in allowed], IC.STATUS_NAMES[s])
        assert s == t, (c["name"], IC.STATUS_NAMES[s], "the host twin:", IC.STATUS_NAMES[t])
        if s in WHOLE:
            assert got.tobytes() == want, c["name"]
    first = int(np.flatnonzero(status)[0])
    assert fresh.first_bad() == (first, int(status[first]))
    assert int(np.flatnonzero(twin)[0]) == first


def test_first_bad_is_the_first_nonzero_status_whatever_it_is(Z, fresh, corpus, damaged):
    cases, _, twin = damaged
    for want in range(1, 11):
        k = int(np.flatnonzero(twin == want)[0])
        group = corpus[:37] + [cases[k]] + corpus[37:50] + [c for c, t in zip(cases[:400], twin[:400]) if t and t != want][:5]
        fresh.reset()
        feed(Z, fresh, group)
        _, status = fresh.collect()
        assert status[:38].tolist() == [0] * 37 + [want] and fresh.first_bad() == (37, want), IC.STATUS_NAMES[want]


def order_subset(corpus, damaged):
    """At most 256 small members and four boundary members with a damaged stream at every third place: [(case, status, bytes or None)]."""
    cases, verdicts, twin = damaged
    small = [c for c in corpus if c["plan"] != "boundary"]
    small = small[::len(small) // 170][:170]
    boundary = [c for c in corpus if c["plan"] == "boundary"]
    good = small[:40] + boundary[5:6] + small[40:90] + boundary[70:71] + small[90:130] + boundary[140:141] + small[130:] + boundary[-1:]
    bad = [k for k in range(0, len(cases), 97) if IC.split_member(cases[k]["member"])[2] <= 4096]
    out = []
    for i, c in enumerate(good):
        out.append((c, IC.OK, c["data"]))
        if i % 2 and bad:
            k = bad.pop(0)
            out.append((cases[k], int(twin[k]), verdicts[k][2] if twin[k] in WHOLE else None))
    return out


@pytest.fixture(scope="module")
def order_runs():
    return {}


@pytest.mark.parametrize("wgs", [1, 3])
@pytest.mark.parametrize("order", ["generated", "reversed", "shuffled"])
def test_order_and_neighbours(Z, fresh, corpus, damaged, order_runs, order, wgs, monkeypatch):
    """The same members as generated, reversed and shuffled, in launches of one workgroup and of three: every member's status and
    bytes are what they are alone, so the same in all six runs (for a member that ended early the bytes are unspecified)."""
    subset = order_subset(corpus, damaged)
    n_small = sum(1 for c, _, _ in subset if c.get("plan") in ("tiny", "small"))
    assert n_small <= 256 and sum(1 for c, _, _ in subset if c.get("plan") == "boundary") == 4
    assert sum(1 for c, s, _ in subset if "plan" not in c) >= len(subset) // 3 - 1 and len(set(s for _, s, _ in subset)) >= 8
    assert sum(IC.split_member(c["member"])[2] for c, _, _ in subset) <= 1 << 20
    index = list(range(len(subset)))
    if order == "reversed":
        index.reverse()
    elif order == "shuffled":
        np.random.default_rng(5).shuffle(index)
    monkeypatch.setenv("ISS_INFLATE_WGS", str(wgs))
    members = feed(Z, fresh, [subset[i][0] for i in index])
    data, status = fresh.collect()
    result = [None] * len(subset)
    for i, s, got in zip(index, status.tolist(), pieces(data, members)):
        result[i] = (s, got.tobytes() if s in WHOLE else None)
    for (c, want_status, want), (s, got) in zip(subset, result):
        assert s == want_status, (c["name"], order, wgs, IC.STATUS_NAMES[s], IC.STATUS_NAMES[want_status])
        assert got == want, (c["name"], order, wgs)
    order_runs[(order, wgs)] = result
    first = next(iter(order_runs.values()))
    assert result == first


def _stored(data):
    w = IC.BitWriter()
    IC.stored_block(w, data)
    return IC.member(w.done(), data)


def test_output_alignment(Z, fresh):
    """Every member's output at every offset mod 4, set by a stored member of 0 .. 3 bytes in front; sizes around nothing, a piece
    and a whole member.  One feed; the bytes are compared as a whole, so a byte written before or behind a member's output shows in
    its neighbour, and the last member is a guard."""
    text, noise = IC.fastq_text(65536, 5), IC.noise(65536, 6)
    sizes = list(range(10)) + list(range(16383, 16388)) + list(range(65533, 65537))
    cases, at, seen = [], 0, set()
    for off in range(4):
        for n in sizes:
            for kind in range(3):
                filler = bytes(bytearray(0xF0 + i for i in range((off - at) % 4)))
                cases.append({"member": _stored(filler), "data": filler})
                at += len(filler)
                assert at % 4 == off
                seen.add((off, n, kind))
                if kind == 0:
                    data = noise[:n] if n < 60000 else (noise[:1000] * 66)[:n]
                    m = _stored(data) if n < 60000 else IC.member(IC.deflate(data, 6), data)
                elif kind == 1:
                    data = text[:n]
                    m = IC.member(IC.deflate(data, 6), data)
                else:
                    data = text[100:100 + n // 2] + noise[:n - n // 2]
                    m = IC.member(IC.deflate(data, 9, zlib.Z_FIXED if n < 100 else zlib.Z_DEFAULT_STRATEGY), data)
                cases.append({"member": m, "data": data})
                at += n
    assert len(seen) == 4 * len(sizes) * 3
    guard = b"\xa5guard\x5a" * 3
    cases.append({"member": _stored(guard), "data": guard})
    members = feed(Z, fresh, cases)
    data, status = fresh.collect()
    assert not status.any()
    assert set((int(o) % 4, int(n)) for o, n in zip(np.cumsum(members.isize.astype(np.int64)) - members.isize, members.isize)) >= \
        set((off, n) for off in range(4) for n in sizes)
    for k, (c, got) in enumerate(zip(cases, pieces(data, members))):
        assert got.tobytes() == c["data"], (k, len(c["data"]))
    assert fresh.first_bad() == (-1, 0)


def test_payload_alignment(Z, fresh):
    """Every payload offset mod 4 (a foreign subfield in front of BC moves it) with every payload length mod 4, for a stored payload
    (the copy reads the payload strided) and a coded one (the 4-byte preload and the single bytes at the payload's end)."""
    text = IC.fastq_text(3000, 9)
    cases, at = [], 0
    for po in range(4):
        for pl in range(4):
            for kind in ("stored", "coded"):
                n = 200
                while True:
                    data = text[:n]
                    if kind == "stored":
                        w = IC.BitWriter()
                        IC.stored_block(w, data)
                        pay = w.done()
                    else:
                        pay = IC.deflate(data, 6)
                    if len(pay) % 4 == pl:
                        break
                    n += 1
                pad = (po - (at + 12 + 4 + 6)) % 4
                m = IC.member(pay, data, before=b"XY" + struct.pack("<H", pad) + b"\x77" * pad)
                cases.append({"member": m, "data": data, "want": (po, pl, kind)})
                at += len(m)
    members = feed(Z, fresh, cases)
    assert [(int(o) % 4, int(n) % 4) for o, n in zip(members.pay_off, members.pay_len)] == [c["want"][:2] for c in cases]
    data, status = fresh.collect()
    assert not status.any()
    for c, got in zip(cases, pieces(data, members)):
        assert got.tobytes() == c["data"], c["want"]


@pytest.mark.parametrize("depth", [2, 3, 5])
def test_corpus_in_several_feeds(Z, fresh, corpus, depth):
    """The corpus cut inside its run of boundary members, all feeds in flight before the first collect: the bytes of the one feed."""
    first = next(k for k, c in enumerate(corpus) if c["plan"] == "boundary")
    assert all(c["plan"] == "boundary" for c in corpus[first:])
    n = len(corpus) - first
    cuts = [0] + [first + n * j // depth + 1 for j in range(1, depth)] + [len(corpus)]
    groups = [corpus[a:b] for a, b in zip(cuts, cuts[1:])]
    assert all(g[0]["plan"] == "boundary" and corpus[a - 1]["plan"] == "boundary" for g, a in zip(groups[1:], cuts[1:]))
    members = [feed(Z, fresh, g) for g in groups]
    assert fresh.in_flight == depth
    for g, m in zip(groups, members):
        data, status = fresh.collect(copy=False)
        assert not status.any()
        for c, got in zip(g, pieces(data, m)):
            assert got.tobytes() == c["data"], c["name"]
    assert fresh.first_bad() == (-1, 0)
