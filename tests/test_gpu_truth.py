"""The mutation rows as device arrays (ReadEngine.export_mutations, k_truth_scatter / k_truth_events):
truth and events against the numpy twins applied to the oracle's rows, the windows, the guard bytes, a capacity below the row
count, the overflow of the row slots, and ReadTensorStream(truth=True)'s contract."""
import numpy as np
import pytest
import torch  # noqa: F401  (here, when the module is collected: torch's HIP runtime has to be the process's first)

from helpers import Guarded, dense_model, mixed_genome, random_genome

pytestmark = pytest.mark.gpu

SLOTS = 4_000_000  # row slots of the engines below: far above what any case needs (the kernels take 256 per wavefront)
FIRST_ORDINAL = 11

# model -> (read length, seed): with this seed the oracle's rows of pairs [0, 333) hold a substitution at position 0, one at
# position L - 1, one in mate 1 and a pair with substitutions in both mates (found on the CPU; asserted again below)
MODELS = {"novaseq": (151, 1), "basic": (125, 1), "miseq": (301, 1)}

_engines, _oracle = {}, {}


def _genome(name):
    return random_genome(500 + MODELS[name][0], 50000)


def _engine(name):
    """One engine per model with rows reserved (made once)."""
    if name not in _engines:
        from insilicoseq_amd.engine import ReadEngine

        eng = ReadEngine(0)
        eng.load_model(dense_model(name))
        gid = eng.add_genome(_genome(name))
        eng.mutations_reserve(SLOTS)
        _engines[name] = (eng, gid)
    return _engines[name]


def teardown_module(module):
    for eng, _ in _engines.values():
        eng.close()
    _engines.clear()
    _oracle.clear()


def _oracle_call(name, n):
    """The oracle's bases and rows of a call of n pairs (made once per size, left unchanged)."""
    if (name, n) not in _oracle:
        from oracle import oracle as O

        res = O.Oracle(dense_model(name)).simulate(O.Rng().seed_philox(MODELS[name][1]), _genome(name), n, first_ordinal=FIRST_ORDINAL,
                                                   store_mutations=True)
        assert res["status"] == 0 and res["n_done"] == n
        _oracle[(name, n)] = (np.stack([res["r1_base"], res["r2_base"]], axis=1), res["mutations"])
    return _oracle[(name, n)]


def _simulate(dense, genome, n, seed, first_ordinal=0, **kw):
    from oracle import oracle as O

    res = O.Oracle(dense).simulate(O.Rng().seed_philox(seed), genome, n, first_ordinal=first_ordinal, store_mutations=True, **kw)
    assert res["status"] == 0 and res["n_done"] == n
    return np.stack([res["r1_base"], res["r2_base"]], axis=1), res["mutations"]


def _outputs(n, RL, capacity, shift=0):
    return {"truth": Guarded(n * 2 * RL, np.uint8, (n, 2, RL), shift), "events": Guarded(capacity * 24, np.int32, (capacity, 6)),
            "n_events": Guarded(8, np.int64, ())}


def _export(eng, first, n, outs, encoding="ascii", want=("truth", "events"), capacity=None):
    torch.cuda.synchronize()  # (the buffers were filled on torch's stream, the engine works on its own)
    ev = "events" in want
    eng.export_mutations(first, n, truth_ptr=outs["truth"].ptr if "truth" in want else None, events_ptr=outs["events"].ptr if ev else None,
                         capacity=(outs["events"].shape[0] if capacity is None else capacity) if ev else 0,
                         n_events_ptr=outs["n_events"].ptr if ev else None, encoding=encoding)
    eng.synchronize()


def _expected(bases, rows, first, n, encoding):
    """truth and events of the window [first, first + n) of a call whose bases / rows these are (pair 0 = output row 0)."""
    from insilicoseq_amd.tensors import events_host, recode, truth_host

    w = rows[(rows["pair"] >= first) & (rows["pair"] < first + n)].copy()
    w["pair"] -= first
    b = bases[first:first + n]
    return truth_host(recode(b) if encoding == "codes" else b, w, encoding), events_host(rows, first, n)


def _presences(rows, L, n):
    s = rows[(rows["type"] == 0) & (rows["pair"] < n)]
    both = set(s["pair"][s["mate"] == 0].tolist()) & set(s["pair"][s["mate"] == 1].tolist())
    return {"position 0": bool((s["position"] == 0).any()), "position L - 1": bool((s["position"] == L - 1).any()),
            "mate 1": bool((s["mate"] == 1).any()), "both mates of a pair": bool(both)}


# ---------------------------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("encoding", ["ascii", "codes"])
@pytest.mark.parametrize("window", ["whole", "inside"])
@pytest.mark.parametrize("n_pairs", [1, 63, 64, 65, 333])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_truth_and_events_equal_the_oracle(name, n_pairs, window, encoding):
    """whole: a call of n_pairs pairs, all of it exported; inside: a call of n_pairs + 71 pairs, of which the 64 pairs from
    pair 7 are exported."""
    eng, gid = _engine(name)
    RL = eng.read_length
    assert RL == MODELS[name][0]
    call, first, n = (n_pairs, 0, n_pairs) if window == "whole" else (n_pairs + 71, 7, 64)
    bases, rows = _oracle_call(name, call)
    if n_pairs == 333:  # (not vacuous: the rows hold what the scatter can get wrong)
        have = _presences(rows, RL, 333)
        assert all(have.values()), have
    eng.generate(gid, call, first_ordinal=FIRST_ORDINAL, seed=MODELS[name][1])
    truth, events = _expected(bases, rows, first, n, encoding)
    outs = _outputs(n, RL, len(events) + 3, shift=(n_pairs + first) % 16)
    _export(eng, first, n, outs, encoding)
    assert int(outs["n_events"].value()) == len(events)
    assert np.array_equal(outs["truth"].value(), truth)
    assert np.array_equal(outs["events"].value()[:len(events)], events)
    assert (outs["events"].value()[len(events):].view(np.uint8) == 0xA5).all()  # (rows behind the last one are not written)
    assert all(o.guards_intact() for o in outs.values())
    if n >= 63:
        assert (events[:, 2] == 0).any()  # (the window holds substitution rows)


# ---------------------------------------------------------------------------------------------------- 2. rebuilt reads
@pytest.mark.parametrize("case", ["fragment", "indel_heavy", "light_stale"])
def test_reads_the_fix_up_rebuilt(case, monkeypatch):
    """fragment: a short custom fragment length on a genome barely longer than a read (templates are cut: irregular pairs,
    rebuilt by the fix-up); indel_heavy: reads with events; light_stale: a light model with indels (ISS_LIGHT_INDELS=1), whose
    reads with an event are rebuilt after k_main wrote their rows -- stale rows exist and must be dropped (that case against
    the host route's rows, which other tests pin to the oracle).  The call stands at output row 5 and the window reaches over
    both of its ends: rows of the older call carry nothing."""
    from insilicoseq_amd.engine import ReadEngine
    from insilicoseq_amd.tensors import events_host, truth_host

    if case == "light_stale":
        monkeypatch.setenv("ISS_LIGHT_INDELS", "1")
    dense = dense_model("novaseq", {"fragment": None, "indel_heavy": (0.01, 0.03), "light_stale": (0.001, 0.003)}[case])
    RL = dense.read_length
    genome = random_genome(520, 30000 if case == "indel_heavy" else RL + 40)
    frag = {} if case == "indel_heavy" else {"fragment_length": 200, "fragment_sd": 60}
    n, row0, seed = 1500, 5, 21
    total = row0 + n + 3
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        gid = eng.add_genome(genome)
        eng.generate(gid, total, seed=4)  # (every row holds something)
        eng.mutations_reserve(SLOTS)
        if frag:
            eng.set_fragment(200, 60)
        eng.generate(gid, n, first_ordinal=3, seed=seed, out_first_pair=row0)
        eng.synchronize()
        d = eng.download(0, total)
        got_bases = np.stack([d["r1_base"], d["r2_base"]], axis=1)
        if case == "light_stale":
            rows = eng.mutations()
        else:
            bases, rows = _simulate(dense, genome, n, seed, first_ordinal=3, **frag)
            assert np.array_equal(got_bases[row0:row0 + n], bases)
        stats = eng.stats_read()
        assert stats["fixup_reads"] > 0, "no read was rebuilt: the case does not test what it claims"
        if case != "fragment":
            assert (rows["type"] == 1).any() and (rows["type"] == 2).any()
        shifted = rows.copy()
        shifted["pair"] += row0
        for encoding in ("ascii", "codes"):
            from insilicoseq_amd.tensors import recode

            exp_truth = truth_host(recode(got_bases) if encoding == "codes" else got_bases, shifted, encoding)
            exp_events = events_host(shifted, 0, total)
            assert len(exp_events) == len(rows) > 100
            outs = _outputs(total, RL, len(rows) + 1, shift=3)
            _export(eng, 0, total, outs, encoding)
            assert int(outs["n_events"].value()) == len(rows)
            assert np.array_equal(outs["truth"].value(), exp_truth)
            assert np.array_equal(outs["events"].value()[:len(rows)], exp_events)
            assert all(o.guards_intact() for o in outs.values())


# ---------------------------------------------------------------------------------------------------- 3. other letters
@pytest.mark.parametrize("encoding", ["ascii", "codes"])
def test_letters_outside_acgt(encoding):
    from insilicoseq_amd.engine import ReadEngine

    dense = dense_model("novaseq")
    genome = mixed_genome(530, 40000)
    n, seed = 700, 8
    bases, rows = _simulate(dense, genome, n, seed)
    sub = rows[rows["type"] == 0]
    assert set(sub["ref"].tolist()) & set(b"acgt"), "no lower-case ref"
    iupac = np.isin(bases, np.frombuffer(b"NRYWSMKHBVDnrywsmkhbvd", dtype=np.uint8))
    assert iupac.sum() > 1000 and not np.isin(sub["ref"], np.frombuffer(b"NRYWSMKHBVDnrywsmkhbvd", dtype=np.uint8)).any()
    truth, events = _expected(bases, rows, 0, n, encoding)
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        gid = eng.add_genome(genome)
        eng.mutations_reserve(SLOTS)
        eng.generate(gid, n, seed=seed)
        outs = _outputs(n, eng.read_length, len(events), shift=9)
        _export(eng, 0, n, outs, encoding)
    got = outs["truth"].value()
    assert np.array_equal(got, truth) and np.array_equal(outs["events"].value(), events)
    assert int(outs["n_events"].value()) == len(events)
    if encoding == "ascii":
        assert np.array_equal(got[iupac], bases[iupac])  # (IUPAC positions take no substitution)
        lower = np.isin(got, np.frombuffer(b"acgt", dtype=np.uint8)) & (got != bases)
        assert lower.any()  # a lower-case ref put back
    else:
        assert (got[iupac] == 4).all() and got.max() == 4
    assert all(o.guards_intact() for o in outs.values())


# ---------------------------------------------------------------------------------------------------- 4. guards, NULL outputs
@pytest.mark.parametrize("shift", [0, 1, 8, 15])
@pytest.mark.parametrize("want", [("truth",), ("events",), ("truth", "events"), ()])
def test_guard_bytes_and_null_outputs(want, shift):
    name = "novaseq"
    eng, gid = _engine(name)
    call, first, n = 140, 2, 130  # (three export tiles, the last one short)
    bases, rows = _oracle_call(name, call)
    eng.generate(gid, call, first_ordinal=FIRST_ORDINAL, seed=MODELS[name][1])
    truth, events = _expected(bases, rows, first, n, "ascii")
    assert len(events) > 10
    outs = _outputs(n, eng.read_length, len(events), shift)
    _export(eng, first, n, outs, "ascii", want=want)
    for k, o in outs.items():
        assert o.guards_intact(), k
    assert outs["truth"].untouched() if "truth" not in want else np.array_equal(outs["truth"].value(), truth)
    if "events" in want:
        assert np.array_equal(outs["events"].value(), events) and int(outs["n_events"].value()) == len(events)
    else:
        assert outs["events"].untouched() and outs["n_events"].untouched()


# ---------------------------------------------------------------------------------------------------- 5. capacity
@pytest.mark.parametrize("short", ["rows - 1", "0"])
def test_capacity_below_the_row_count(short):
    name = "miseq"
    eng, gid = _engine(name)
    call = 90
    bases, rows = _oracle_call(name, call)
    eng.generate(gid, call, first_ordinal=FIRST_ORDINAL, seed=MODELS[name][1])
    truth, events = _expected(bases, rows, 0, call, "ascii")
    assert len(events) > 300  # (more rows than one workgroup of k_truth_events has lanes)
    capacity = len(events) - 1 if short == "rows - 1" else 0
    outs = _outputs(call, eng.read_length, capacity)
    _export(eng, 0, call, outs)
    assert int(outs["n_events"].value()) == len(events)  # the full count
    assert np.array_equal(outs["events"].value(), events[:capacity])
    assert all(o.guards_intact() for o in outs.values())  # (the guard behind row `capacity`)
    assert np.array_equal(outs["truth"].value(), truth)


# ---------------------------------------------------------------------------------------------------- 6. overflow
def test_slot_buffer_overflow():
    from insilicoseq_amd._native import E_NOMEM, EngineError
    from insilicoseq_amd.engine import ReadEngine
    from insilicoseq_amd.tensors import ReadTensorStream

    dense = dense_model("novaseq")
    genome = random_genome(560, 60000)
    n = 3000
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        gid = eng.add_genome(genome)
        eng.generate(gid, n, seed=5)
        eng.synchronize()
        d = eng.download(0, n)
        plain = np.stack([d["r1_base"], d["r2_base"]], axis=1).copy(), np.stack([d["r1_qual"], d["r2_qual"]], axis=1).copy()
        eng.generate(gid, n, seed=6)  # (other rows in between)
        eng.mutations_reserve(256)
        eng.generate(gid, n, seed=5)
        outs = _outputs(n, eng.read_length, 64)
        bases = Guarded(n * 2 * eng.read_length, np.uint8, (n, 2, eng.read_length))
        torch.cuda.synchronize()
        eng.export(0, n, bases_ptr=bases.ptr)
        _export(eng, 0, n, outs)
        assert int(outs["n_events"].value()) == -1
        assert outs["events"].untouched()
        assert np.array_equal(outs["truth"].value(), bases.value())  # truth holds the plain bases
        d = eng.download(0, n)
        assert np.array_equal(np.stack([d["r1_base"], d["r2_base"]], axis=1), plain[0])  # the reads are those of a run without rows
        assert np.array_equal(np.stack([d["r1_qual"], d["r2_qual"]], axis=1), plain[1])
        assert np.array_equal(bases.value(), plain[0])
        with pytest.raises(EngineError) as e:  # (the host route says the same, behind its wait)
            eng.mutations()
        assert e.value.code == E_NOMEM
        assert all(o.guards_intact() for o in outs.values())
    with ReadTensorStream([genome], dense, [(0, n)], 1000, seed=5, truth=True, mutation_slots=256) as stream:
        assert stream.mutation_slots == 256
        with pytest.raises(EngineError) as e:
            for _ in stream:
                pass
        assert e.value.code == E_NOMEM and "mutation_slots=256" in str(e.value) and "batch 0" in str(e.value)


# ---------------------------------------------------------------------------------------------------- 7, 8. the stream
RECORDS = None
WORK = [(0, 700), (1, 50), (2, 0), (0, 57), (2, 1343)]  # record 1 is shorter than a read: skipped, 2 100 pairs remain


def _records():
    global RECORDS
    if RECORDS is None:
        RECORDS = [mixed_genome(571, 6000), random_genome(572, 120), random_genome(573, 9000)]
    return RECORDS


def test_stream_does_not_depend_on_batch_pairs():
    from insilicoseq_amd.tensors import ReadTensorStream, events_host, truth_host
    from oracle import oracle as O

    dense = dense_model("novaseq")
    recs = _records()
    seed, total = 77, 2100
    # the oracle per item of the whole list, the ordinals running on
    orc, rng = O.Oracle(dense), O.Rng().seed_philox(seed)
    bases, rows, ordinal = [], [], 0
    for k, n in WORK:
        if k == 1 or n == 0:
            continue
        res = orc.simulate(rng, recs[k], n, first_ordinal=ordinal, store_mutations=True)
        assert res["status"] == 0 and res["n_done"] == n
        bases.append(np.stack([res["r1_base"], res["r2_base"]], axis=1))
        m = res["mutations"].copy()
        m["pair"] += ordinal
        rows.append(m)
        ordinal += n
    bases, rows = np.concatenate(bases), np.concatenate(rows)
    assert ordinal == total and len(rows) > 500
    exp_truth, exp_events = truth_host(bases, rows, "ascii"), events_host(rows, 0, total)
    with ReadTensorStream(recs, dense, WORK, 4096, seed=seed, encoding="ascii") as plain:
        (ref,) = list(plain)
        assert ref.truth is None and ref.events is None and ref.n_events is None
        assert plain.engine.mutations_capacity == 0 and plain.mutation_slots == 0  # truth=False: no reservation was ever made
    ref = [getattr(ref, f).cpu().numpy() for f in ("bases", "qual", "coords", "record")]
    assert np.array_equal(ref[0], bases)
    for batch_pairs in (1, 64, 333, 4096):
        capacity = 64 if batch_pairs == 1 else len(rows)
        with ReadTensorStream(recs, dense, WORK, batch_pairs, seed=seed, encoding="ascii", truth=True, events_capacity=capacity) as stream:
            assert stream.engine.mutations_capacity == stream.mutation_slots > 0
            batches = list(stream)
        assert len(batches) == -(-total // batch_pairs)
        b0 = batches[0]
        assert b0.truth.dtype == torch.uint8 and b0.truth.shape == b0.bases.shape and b0.truth.device == b0.bases.device
        assert b0.events.dtype == torch.int32 and tuple(b0.events.shape) == (capacity, 6)
        assert b0.n_events.dtype == torch.int64 and b0.n_events.dim() == 0 and b0.n_events.is_cuda
        for f, want in zip(("bases", "qual", "coords", "record"), ref):
            assert np.array_equal(torch.cat([getattr(b, f) for b in batches]).cpu().numpy(), want), (f, batch_pairs)
        assert np.array_equal(torch.cat([b.truth for b in batches]).cpu().numpy(), exp_truth), batch_pairs
        got, first = [], 0
        for b in batches:
            k = int(b.n_events.item())
            assert 0 <= k <= capacity
            ev = b.events[:k].cpu().numpy().copy()
            ev[:, 0] += first  # (the batch's first ordinal back)
            got.append(ev)
            first += b.bases.shape[0]
        assert np.array_equal(np.concatenate(got), exp_events), batch_pairs


def test_truth_off_is_unchanged_and_truth_alone_carries_no_events():
    from insilicoseq_amd.tensors import ReadTensorStream

    dense = dense_model("novaseq")
    recs = _records()
    with ReadTensorStream(recs, dense, WORK, 500, seed=3) as off:
        batches = list(off)
        assert all(b.truth is None and b.events is None and b.n_events is None for b in batches)
        assert off.engine.mutations_capacity == 0 and not hasattr(off.engine, "_pmut_cap")  # mutations_reserve was never called
        assert off.engine.main_kernel().startswith("k_main_g") or off.engine.main_kernel().startswith("k_main<false")
    with ReadTensorStream(recs, dense, WORK, 500, seed=3, truth=True) as on:
        with_truth = list(on)
        assert on.engine.main_kernel().startswith("k_main<true")
    assert all(b.truth is not None and b.events is None and b.n_events is None for b in with_truth)
    for a, b in zip(batches, with_truth):
        assert torch.equal(a.bases, b.bases) and torch.equal(a.qual, b.qual) and torch.equal(a.coords, b.coords) and torch.equal(a.record, b.record)
    diff = sum(int((a.bases != b.truth).sum().item()) for a, b in zip(batches, with_truth))
    assert diff > 100


# ---------------------------------------------------------------------------------------------------- 9. errors
def test_errors_launch_nothing():
    from insilicoseq_amd._native import E_INVALID, EngineError
    from insilicoseq_amd.engine import ReadEngine

    with ReadEngine(0) as eng:
        eng.load_model(dense_model("basic"))
        gid = eng.add_genome(random_genome(590, 5000))
        outs = _outputs(4, eng.read_length, 8)

        def refused(first=0, n=4, **kw):
            with pytest.raises(EngineError) as e:
                _export(eng, first, n, outs, **kw)
            assert e.value.code == E_INVALID
            assert all(o.untouched() for o in outs.values())

        eng.generate(gid, 16, seed=1)
        refused()                      # no reservation
        eng.mutations_reserve(100000)
        refused()                      # no generate call under the reservation
        eng.generate(gid, 16, seed=1)
        torch.cuda.synchronize()
        for ev, cnt in ((outs["events"].ptr, None), (None, outs["n_events"].ptr)):  # events without n_events, and the other way round
            with pytest.raises(EngineError) as e:
                eng.export_mutations(0, 4, truth_ptr=outs["truth"].ptr, events_ptr=ev, capacity=8, n_events_ptr=cnt)
            assert e.value.code == E_INVALID
        refused(first=15, n=2)         # a window outside the reserved rows
        refused(first=-1, n=2)
        refused(encoding="2bit")
        eng.synchronize()
        assert all(o.untouched() for o in outs.values())
        _export(eng, 0, 4, outs)       # (and the same call, complete, works)
        assert int(outs["n_events"].value()) >= 0 and not outs["truth"].untouched()
        eng.mutations_reserve(0)
        outs = _outputs(4, eng.read_length, 8)  # (fresh ones: the call above wrote the others)
        refused()                      # the reservation given up


# ---------------------------------------------------------------------------------------------------- 10. stream order
def test_stream_order_without_synchronisation():
    from insilicoseq_amd.engine import ReadEngine
    from insilicoseq_amd.tensors import default_mutation_slots, events_host, export_tensors, truth_host

    dense = dense_model("novaseq")
    n = 1 << 16
    with ReadEngine(0) as eng:
        eng.load_model(dense)
        gid = eng.add_genome(random_genome(111, 200000))
        eng.mutations_reserve(default_mutation_slots(dense, n, torch.cuda.get_device_properties(0).multi_processor_count))
        # the synchronous route: what the first generation's truth and events are
        eng.generate(gid, n, seed=1)
        eng.synchronize()
        d = eng.download(0, n)
        bases = np.stack([d["r1_base"], d["r2_base"]], axis=1)
        rows = eng.mutations()
        exp_truth, exp_events = truth_host(bases, rows, "ascii"), events_host(rows, 0, n)
        assert len(rows) > 1000
        for stream in (torch.cuda.Stream(device=0), torch.cuda.current_stream(0)):  # a stream of the caller's, torch's default stream
            eng.generate(gid, n, seed=9)  # (other rows in between)
            eng.generate(gid, n, seed=1)
            with torch.cuda.stream(stream):
                batch = export_tensors(eng, 0, n, encoding="ascii", truth=True, events_capacity=len(rows) + 5)
                changed = (batch.truth != batch.bases).sum()  # queued behind the export, no wait
            eng.generate(gid, n, seed=2)  # the rows and the row slots are written anew right behind the export
            torch.cuda.synchronize()
            assert int(changed.item()) == int((exp_truth != bases).sum())
            assert np.array_equal(batch.truth.cpu().numpy(), exp_truth) and np.array_equal(batch.bases.cpu().numpy(), bases)
            assert int(batch.n_events.item()) == len(rows)
            assert np.array_equal(batch.events[:len(rows)].cpu().numpy(), exp_events)
            assert eng.stream_ptr == 0  # (the engine is back on its own stream)
