"""`model` on the MI355X at its edges: hand-built records (bam_synth.edge_table) tallied one by one and together against the Python
twin, the same tallies whatever wave or feed a record lands in, the first bad record in file order for every error code, and
k_kde_cdf on chosen histograms against the definition at 60 digits (kde_ref) with scipy's own rounding error as the yardstick."""
import random

import numpy as np
import pytest

import bam_synth
import bam_twin
import kde_ref

pytestmark = pytest.mark.gpu

TABLE = bam_synth.edge_table()
BAD = bam_synth.edge_bad_records()
TALLY_WAVES = 4  # waves per workgroup of k_bam_tally (iss_bam.hip.h: TALLY_THREADS / 64)


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge

    ge.build()
    from insilicoseq_amd.engine import BamTally

    with BamTally(0) as d:
        yield d


# iss_api_bam.hip.h:157-160: grid = min(ceil(n / 4), 2 * CUs) workgroups of 4 waves, n_iter = ceil(n / (4 * grid)).  Two iterations of
# the full grid hold 16 * CUs records, so 16 * CUs + 1 is the smallest count with three iterations per wave, and it has 2 * CUs
# workgroups: 4097 records on the 256 CUs of an MI355X.
CUS = 256
N_PLACED = 16 * CUS + 1


@pytest.fixture(scope="module")
def n_placed():
    return N_PLACED


def blob(r):
    if "_blob" not in r:
        r["_blob"] = bam_synth.encode_record(r)
    return r["_blob"]


def feed(dev, recs, select=None):
    blobs = [blob(r) for r in recs]
    data = np.frombuffer(b"".join(blobs), np.uint8)
    offs = np.cumsum([0] + [len(b) for b in blobs[:-1]], dtype=np.int64)
    if select is None:
        select = [0 if r["flag"] & 4 else 1 for r in recs]
    dev.feed(data, offs, np.array(select, np.uint8))


def device_tallies(dev, feeds):
    from insilicoseq_amd.modeller import unpack_tallies

    dev.reset()
    for recs in feeds:
        feed(dev, recs)
    words, bad, code = dev.tallies()
    assert (bad, code) == (-1, 0)
    return unpack_tallies(words)


def twin(recs):
    return bam_twin.tallies(bam_twin.from_dicts(recs))


def times(t, k):
    return dict({key: t[key] * np.uint64(k) for key in ("subst", "indel", "qhist", "tlen", "nread")}, minlen=t["minlen"], taken=t["taken"] * k)


def mismatch(got, exp):
    return [k for k in ("subst", "indel", "qhist", "tlen", "nread", "minlen") if not np.array_equal(got[k], exp[k])] + \
        (["taken"] if got["taken"] != exp["taken"] else [])


@pytest.fixture(scope="module")
def twin_all():
    return twin(TABLE)


# ---- 1. tallies, record by record

def test_each_record_alone(dev):
    failed = []
    for r in TABLE:
        miss = mismatch(device_tallies(dev, [[r]]), twin([r]))
        if miss:
            failed.append((r["name"], miss))
    assert not failed, failed


def test_whole_table_in_one_feed(dev, twin_all):
    assert not mismatch(device_tallies(dev, [TABLE]), twin_all)


# ---- 2. placement and order

def test_permutation(dev, twin_all, n_placed):
    reps = -(-n_placed // len(TABLE))
    recs = TABLE * reps
    plain = device_tallies(dev, [recs])
    assert not mismatch(plain, times(twin_all, reps))
    shuffled = list(recs)
    random.Random(20).shuffle(shuffled)
    assert not mismatch(device_tallies(dev, [shuffled]), plain)


def test_split_feeds(dev, twin_all):
    unmapped = [r for r in TABLE if r["flag"] & 4]
    for size in (1, 3, len(TABLE)):
        dev.reset()
        for i in range(0, len(TABLE), size):
            feed(dev, TABLE[i:i + size])
            if i == 3 * size:
                dev.feed(np.zeros(0, np.uint8), np.zeros(0, np.int64), np.zeros(0, np.uint8))  # no records
                feed(dev, TABLE[:7], select=[0] * 7)                                           # none selected
                feed(dev, unmapped)
        words, bad, code = dev.tallies()
        from insilicoseq_amd.modeller import unpack_tallies

        assert (bad, code) == (-1, 0)
        assert not mismatch(unpack_tallies(words), twin_all), size


# ---- 2b. the optional fields: `model` and `report --bam --errors` read them with one walk (iss_bam_record.h: be_tag_walk)

def _tag_cases():
    import bam_error_cases as EC

    cases = [r for r in EC.damaged_cases() if "raw_aux" in r] + [r for r in EC.op_cases() if r["name"] == "two_bytes_left"]
    assert sorted(str(r["_case"]["expect"]) for r in cases) == ["2"] * 10 + ["no_md"] * 3 + ["tallied"]
    return EC, cases


def _tag_verdict(r, index):
    """(bad record, code) of `model` from the case's own expectation: ALN_TAGS -> E_REC_MALFORMED, "no_md" -> E_REC_NO_MD."""
    what = r["_case"]["expect"]
    return (-1, 0) if what == "tallied" else (index, 5 if what == "no_md" else 1)


def _tag_tallies(dev, recs, good, case_recs):
    """Feeds recs; -> (bad record, code), and the fields that differ from the twin.  A record dropped for its optional fields has
    added its header phase by then (taken, the quality slice: k_bam_tally's phase A, as before), so those fields are the twin's
    of the record with a plain MD:Z in place of its bytes; subst, indel and tlen are those of the good records alone."""
    dev.reset()
    feed(dev, recs)
    words, bad, code = dev.tallies()
    from insilicoseq_amd.modeller import unpack_tallies

    got = unpack_tallies(words)
    plain = [dict(r, tags=r["tags"] or [("MD", "Z", "20")], raw_aux=b"") for r in case_recs]
    rows, head = twin(good + [p for p in plain if p["_case"]["expect"] == "tallied"]), twin(good + plain)
    exp = dict(head, subst=rows["subst"], indel=rows["indel"], tlen=rows["tlen"])
    return (bad, code), mismatch(got, exp)


def test_optional_fields_get_the_error_stage_verdict(dev):
    """The records of bam_error_cases whose optional fields are raw bytes (ten damaged: code 1; three without MD:Z: code 5; one that
    ends two bytes behind its MD:Z: tallied), each alone, each between two good records, and all of them in one feed (which can
    show the first bad record only).  Of the tallies, subst, indel and tlen equal the twin of the good neighbours alone.  taken,
    nread, minlen and qhist do not and never did: k_bam_tally counts a record's header phase before it looks at the optional
    fields, so these are held to the twin of the neighbours plus each dropped record with a plain MD:Z:20 (_tag_tallies)."""
    EC, cases = _tag_cases()
    failed = []
    for r in cases:
        for recs, index in (([r], 0), (EC.between_good(r, 1), 1)):
            good = [g for g in recs if g is not r]
            verdict, miss = _tag_tallies(dev, recs, good, [r])
            if verdict != _tag_verdict(r, index) or miss:
                failed.append((r["name"], len(recs), verdict, miss))
    assert not failed, failed
    recs = [x for r in cases for x in EC.between_good(r, 1)]
    good = [x for x in recs if not any(x is r for r in cases)]
    verdict, miss = _tag_tallies(dev, recs, good, cases)
    assert (verdict, miss) == (_tag_verdict(cases[0], 1), [])


def _good(n):
    return (TABLE * (-(-n // len(TABLE))))[:n]


def test_every_bad_record_alone_reports_its_code(dev):
    got = []
    for code, r in BAD:
        dev.reset()
        feed(dev, [TABLE[0], r, TABLE[1]])
        got.append((r["name"],) + dev.tallies()[1:])
    assert got == [(r["name"], 1, code) for code, r in BAD]
    assert {code for code, _ in BAD} == set(range(1, 10))


def test_first_error_in_file_order_wins_within_a_feed(dev, twin_all, n_placed):
    """Record r runs in iteration r // stride of wave r % stride (stride = 4 * grid): the later bad records sit in earlier waves of the
    grid than the first one, or the first one runs in the first iteration of the first workgroup, long before the later ones."""
    stride = (n_placed - 1) // 2
    assert stride % TALLY_WAVES == 0 and stride // TALLY_WAVES >= 2 and -(-n_placed // stride) == 3
    got, want = [], []
    for k, (code, r) in enumerate(BAD):
        later = [b for c, b in BAD[k + 1:] + BAD[:k] if c != code]
        for first, second, third in ((stride - 3, stride, 2 * stride), (1, stride - 1, 2 * stride)):
            recs = _good(n_placed)
            recs[first], recs[second], recs[third] = r, later[0], later[len(later) // 2]
            dev.reset()
            feed(dev, recs)
            got.append((r["name"],) + dev.tallies()[1:])
            want.append((r["name"], first, code))
    assert got == want
    reps = -(-n_placed // len(TABLE))
    assert not mismatch(device_tallies(dev, [TABLE * reps]), times(twin_all, reps))  # the same handle after reset()


def test_first_error_in_file_order_wins_across_feeds(dev, twin_all):
    n = len(TABLE)
    got, want = [], []
    for k, (code, r) in enumerate(BAD):
        other = next(b for c, b in BAD[k + 1:] + BAD[:k] if c != code)
        one, two = list(TABLE), list(TABLE)
        one[40], two[3] = r, other  # feed position 3 of the second feed is file position n + 3
        dev.reset()
        feed(dev, one)
        feed(dev, two)
        got.append((r["name"],) + dev.tallies()[1:])
        want.append((r["name"], 40, code))
        dev.reset()
        feed(dev, TABLE)
        feed(dev, two)
        got.append(dev.tallies()[1:])
        want.append((n + 3, next(c for c, b in BAD if b is other)))
    assert got == want
    assert not mismatch(device_tallies(dev, [TABLE]), twin_all)


def test_invalid_arguments_launch_nothing(dev, twin_all):
    """Argument validation of iss_bam_create: no handle, the thread's error; the context beside it is untouched."""
    import ctypes as C

    from insilicoseq_amd import _native

    lib = _native.lib()
    h = C.c_void_p()
    assert lib.iss_bam_create(1 << 20, C.byref(h)) == _native.E_INVALID and not h
    assert b"device ordinal out of range" in lib.iss_bam_last_error(None)
    assert lib.iss_bam_create(-1, C.byref(h)) == _native.E_INVALID and not h
    assert lib.iss_bam_create(0, None) == _native.E_INVALID
    assert lib.iss_bam_reset(None) == _native.E_INVALID
    lib.iss_bam_destroy(None)
    assert not mismatch(device_tallies(dev, [TABLE]), twin_all)


# ---- 3. k_kde_cdf against the definition

def tolerance(e_ref):
    return max(1e-12, 4 * e_ref)


@pytest.fixture(scope="module")
def qkde(dev):
    """Every quality case in one handle: (qcdf, tallies, {case: (mate, bin, position)}, {(mate, bin): qualities of its reads})."""
    from insilicoseq_amd.modeller import unpack_tallies

    dev.reset()
    where, quals = {}, {}
    for (mate, b), cols in kde_ref.Q_SLICES.items():
        recs, pos = kde_ref.slice_reads(mate, b, cols, "s%d%d" % (mate, b))
        feed(dev, recs)
        where.update({case: (mate, b, p) for case, p in pos.items()})
        quals[(mate, b)] = [r["qual"] for r in recs]
    recs, shape = kde_ref.shape_reads()
    feed(dev, recs)
    quals.update(shape)
    data, offs = kde_ref.big_block(1 << 17)
    for _ in range(16):
        dev.feed(data, offs, np.ones(offs.size, np.uint8))
    feed(dev, kde_ref.big_tail())
    words, bad, code = dev.tallies()
    assert (bad, code) == (-1, 0)
    qcdf, _ = dev.kde(4, with_isize=False)
    return qcdf, unpack_tallies(words), where, quals


def check_row(label, row, data, grid, worst):
    ref = kde_ref.cdf_scipy(data, grid)
    if np.isnan(ref).all():  # every term underflowed: 0 / 0 in the reference, and here
        print("%-28s reference all NaN" % label)
        assert np.isnan(row).all(), label
        return
    hp = kde_ref.cdf_decimal(kde_ref.moved(data), grid)
    assert not np.isnan(ref).any() and not np.isnan(row).any(), label
    e_ref, e_dev = float(np.max(np.abs(ref - hp))), float(np.max(np.abs(row - hp)))
    print("%-28s e_ref %.3g device %.3g" % (label, e_ref, e_dev))
    worst[0], worst[1] = max(worst[0], e_ref), max(worst[1], e_dev)
    assert e_dev <= tolerance(e_ref), (label, e_dev, e_ref)
    assert np.all(np.diff(row) >= 0) and row[-1] == 1.0, label


def test_quality_histograms_are_the_chosen_ones(qkde):
    _, t, where, _ = qkde
    for case, col in kde_ref.q_case_data().items():
        mate, b, p = where[case]
        assert np.array_equal(t["qhist"][mate, b, p], np.bincount(col, minlength=94).astype(np.uint64)), case
    m, b = kde_ref.BIG_SLICE
    assert t["qhist"][m, b, 0, 20] == kde_ref.BIG and t["nread"][m, b] == len(kde_ref.BIG_DATA) and t["minlen"][m, b] == 1


def test_quality_cdf_against_definition(qkde):
    qcdf, _, where, _ = qkde
    worst = [0.0, 0.0]
    for case, col in kde_ref.q_case_data().items():
        check_row(case, qcdf[where[case]], col, kde_ref.Q_GRID, worst)
    for case in kde_ref.NAN_CASES:
        assert np.isnan(qcdf[where[case]]).all(), case
    print("quality rows: largest e_ref %.3g, largest device deviation %.3g" % tuple(worst))


def test_quality_cdf_count_above_two_to_the_21(qkde):
    qcdf = qkde[0]
    worst = [0.0, 0.0]
    check_row("count_%d" % kde_ref.BIG, qcdf[kde_ref.BIG_SLICE + (0,)], kde_ref.BIG_DATA, kde_ref.Q_GRID, worst)
    assert np.isnan(qcdf[kde_ref.BIG_SLICE][1:]).all()


def test_quality_cdf_nan_pattern_and_shapes(qkde):
    """A row is a number exactly where the reference has one: slices of two reads or more (iss/modeller.py:85), positions below the
    slice's shortest read (zip(*) at :88).  Position minlen - 1 of the slice of 6, 6 and 4 bases goes through the definition."""
    qcdf, t, _, quals = qkde
    worst = [0.0, 0.0]
    for mate in range(2):
        for b in range(4):
            reads = quals.get((mate, b), [[20]] * 2 if (mate, b) == kde_ref.BIG_SLICE else [])
            n_rows = min(map(len, reads)) if len(reads) > 1 else 0
            rows = qcdf[mate, b]
            assert np.isnan(rows[n_rows:]).all(), (mate, b)
            for p in range(n_rows if (mate, b) != kde_ref.BIG_SLICE else 0):
                # the bandwidth is 0.2, so a datum v adds exp(-12.5 (v - 40)^2) at the last grid point: 0 in float64 from v = 48 on
                far = min(kde_ref.moved([q[p] for q in reads])) >= 48
                assert np.isnan(rows[p]).all() if far else not np.isnan(rows[p]).any(), (mate, b, p)
    assert len(quals[(1, 3)]) == 1 and len(quals[(1, 1)]) == 2
    assert not np.isnan(qcdf[1, 1, :3]).any() and np.isnan(qcdf[1, 3]).all()
    three = quals[(1, 0)]
    assert [len(q) for q in three] == [6, 6, 4]
    check_row("varlen_minlen_minus_1", qcdf[1, 0, 3], [q[3] for q in three], kde_ref.Q_GRID, worst)
    assert np.isnan(qcdf[1, 0, 4]).all()
    for p, col in enumerate(zip(*quals[(1, 1)])):
        check_row("two_reads_beside_one_p%d" % p, qcdf[1, 1, p], list(col), kde_ref.Q_GRID, worst)


@pytest.mark.parametrize("case", sorted(kde_ref.ISIZE_CASES))
def test_insert_size_cdf_against_definition(dev, case):
    tlens = kde_ref.ISIZE_CASES[case]
    recs = [bam_synth.edge_read("t%d" % i, [(0, 3)], flag=1 | 2, tlen=tl if i % 2 else -tl) for i, tl in enumerate(tlens)]
    dev.reset()
    feed(dev, recs[:len(recs) // 2])
    feed(dev, recs[len(recs) // 2:])
    worst = [0.0, 0.0]
    for read_length in (1, 301):
        _, cdf = dev.kde(read_length)
        isd, grid = kde_ref.isize_grid(tlens, read_length)
        assert min(isd) < 0 or read_length == 1
        check_row("%s rl=%d" % (case, read_length), cdf, isd, grid, worst)
