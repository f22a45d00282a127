"""insilicoseq_amd._native.TABLE, the one list of the C ABI's prototypes, held to include/iss_mi355x.h type for type; the structs and the
constants the binding mirrors; lib() and need() on a stand-in for ctypes.CDLL, with every group of entries missing in turn; and the
marshalling of the emit entries' work lists.  No GPU and no HIP library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from insilicoseq_amd import _native, engine

HEADER = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "iss_mi355x.h")).read()
GROUPS = ("vcf", "set_rows", "export", "mutations_export", "tally", "depth", "ubam", "origins", "bgzip", "errtally", "fq", "br",
          "br_errors", "br_depth", "inflate", "mt_resolver", "variants", "fasta")

# ---------------------------------------------------------------------------------------------------- the header, parsed
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "double": C.c_double, "char": C.c_char, "int8_t": C.c_int8, "uint8_t": C.c_uint8, "int16_t": C.c_int16}
RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "void": None, "const char *": C.c_char_p}
DECL = re.compile(r"\b((?:const\s+)?\w+\s*\*?)\s*\b(iss_\w+)\s*\(([^()]*)\)\s*;")


def strip_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)


def parse_declarator(text):
    """'const int64_t *d_table' -> ('int64_t', 1, None); 'double ms[4]' -> ('double', 0, 4); 'const char *const *ids' -> ('char', 2, None):
    (base type, pointer depth, array length)."""
    text, length = " ".join(text.split()), None
    if text.endswith("]"):
        text, length = text[:text.index("[")], int(text[text.index("[") + 1:-1])
    kind = re.match(r"^(.*?)\w+$", text).group(1)  # (the last word is the name)
    return " ".join(w for w in kind.replace("*", " ").split() if w != "const"), kind.count("*"), length


def declarations(text):
    """[(name, return type, [parameter])] of every function declaration of the header ``text``."""
    out = []
    for m in DECL.finditer(strip_comments(text)):
        params = m.group(3).strip()
        out.append((m.group(2), " ".join(m.group(1).replace("*", " * ").split()),
                    [] if params in ("", "void") else [parse_declarator(p) for p in params.split(",")]))
    return out


def struct_fields(name):
    """[(field, base type, pointer depth)] of ``typedef struct {...} name;``."""
    body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*%s\s*;" % name, strip_comments(HEADER)).group(1)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            first, *more = decl.split(",")  # ("uint8_t ref, alt")
            base, depth, _ = parse_declarator(first)
            out.append((first.split()[-1].lstrip("*"), base, depth))
            out.extend((m.strip(), base, 0) for m in more)
    return out


def defines():
    """{name: value} of the header's #defines whose value is one integer."""
    found = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(ISS_\w+)[ \t]+\(?(-?\d+)u?\)?[ \t]*$", strip_comments(HEADER), flags=re.M)
    return {name: int(value) for name, value in found}


def is_int32(t):
    return t in (C.c_int, C.c_int32) and C.sizeof(t) == 4


def param_problem(param, t):
    """None, or what is wrong with the ctypes type ``t`` for the header's parameter ``param``."""
    base, depth, length = param
    if depth or length is not None:
        if t in (C.c_void_p, C.c_char_p):
            return None
        if not (isinstance(t, type) and issubclass(t, C._Pointer)):
            return "%r for a pointer" % (t,)
        to, levels = t._type_, depth + (length is not None)
        if length is not None and issubclass(to, C.Array):  # an array parameter as a pointer to the array type
            return None if depth == 0 and (to._type_, to._length_) == (SCALARS.get(base), length) else "%r for %s[%d]" % (t, base, length)
        if isinstance(getattr(to, "_type_", None), str):  # POINTER(simple T): T is what the header points at
            want = C.c_void_p if levels > 1 else SCALARS.get(base)
            return None if to is want else "%r for %s%s" % (t, base, "*" * levels)
        return None
    if base in ("int", "int32_t"):
        return None if is_int32(t) else "%r for %s" % (t, base)
    if base in ("uint32_t", "int64_t", "uint64_t", "double"):
        return None if t is SCALARS[base] else "%r for %s" % (t, base)
    return "a %s parameter, which this test does not know" % base


def problems(text, table=None):
    """{entry: [what disagrees]} between the declarations of the header ``text`` and the rows of the table."""
    rows = {row[0]: row for row in (_native.TABLE if table is None else table)}
    out = {}
    for name, ret, params in declarations(text):
        bad = []
        if name not in rows:
            out[name] = ["no row"]
            continue
        _, restype, argtypes, _ = rows[name]
        if ret not in RETURNS:
            bad.append("return type %s, which this test does not know" % ret)
        elif not (is_int32(restype) if ret == "int" else restype is RETURNS[ret]):
            bad.append("returns %r for %s" % (restype, ret))
        if len(argtypes) != len(params):
            bad.append("%d argtypes for %d parameters" % (len(argtypes), len(params)))
        else:
            bad.extend("parameter %d: %s" % (k, p) for k, p in enumerate(map(param_problem, params, argtypes)) if p)
        if bad:
            out[name] = bad
    return out


# ---------------------------------------------------------------------------------------------------- header against table
def test_every_declaration_has_its_row_type_for_type():
    decls = declarations(HEADER)
    names = [d[0] for d in decls]
    declared = set(re.findall(r"\b(iss_\w+)\s*\(", strip_comments(HEADER))) - {"iss_ctx"}
    assert len(decls) == len(declared) == 125 and len(set(names)) == len(names)  # the parser leaves nothing out
    assert set(names) == set(_native.EXPORTS) and len(_native.EXPORTS) == len(names)
    assert list(_native.EXPORTS) == names  # the header's order
    assert problems(HEADER) == {}


@pytest.mark.parametrize("entry,old,new,what", [
    ("iss_generate", "int iss_generate(iss_ctx *ctx, int32_t genome_id,", "int iss_generate(iss_ctx *ctx, int64_t genome_id,", "parameter 1"),
    ("iss_output_reserve", "int iss_output_reserve(iss_ctx *ctx, int64_t capacity_pairs);", "int iss_output_reserve(iss_ctx *ctx);",
     "2 argtypes for 1 parameters"),
    ("iss_synchronize", "int iss_synchronize(", "int64_t iss_synchronize(", "returns"),
])
def test_a_doctored_header_is_reported_for_its_entry_alone(entry, old, new, what):
    assert HEADER.count(old) == 1
    found = problems(HEADER.replace(old, new))
    assert list(found) == [entry] and len(found[entry]) == 1 and what in found[entry][0]


def test_a_doctored_table_is_reported_too():
    """The other way round: a row with a pointer narrowed, a width changed, a pointee changed."""
    def doctored(name, k, t):
        return [(r[0], r[1], r[2][:k] + (t,) + r[2][k + 1:], r[3]) if r[0] == name else r for r in _native.TABLE]

    for name, k, t in (("iss_generate", 2, C.c_int32), ("iss_generate", 3, C.c_int64), ("iss_genome_upload", 3, C.POINTER(C.c_int64)),
                       ("iss_timing_read", 1, C.POINTER(C.c_double * 3)), ("iss_ctx_create", 1, C.c_int64), ("iss_fastq_emit", 1, C.c_int64)):
        assert list(problems(HEADER, doctored(name, k, t))) == [name], (name, k, t)


# ---------------------------------------------------------------------------------------------------- structs
def test_model_tables_is_the_headers_struct():
    fields = struct_fields("iss_model_tables")
    assert [f[0] for f in fields] == [f[0] for f in _native.ModelTables._fields_] and len(fields) == 18
    for (name, base, depth), (_, t) in zip(fields, _native.ModelTables._fields_):
        assert param_problem((base, depth, None), t) is None, name


def test_mut_dtype_is_the_headers_iss_mutation():
    fields = struct_fields("iss_mutation")
    assert tuple(f[0] for f in fields) == engine.MUT_DTYPE.names
    offset, widest = 0, 1
    for name, base, depth in fields:  # the C layout: every member aligned to its own size, the struct to its widest member
        size = C.sizeof(SCALARS[base])
        assert depth == 0 and engine.MUT_DTYPE[name].itemsize == size, name
        assert engine.MUT_DTYPE[name].kind == ("u" if base.startswith("u") else "i"), name
        offset = -(-offset // size) * size
        assert engine.MUT_DTYPE.fields[name][1] == offset, name
        offset, widest = offset + size, max(widest, size)
    assert engine.MUT_DTYPE.itemsize == -(-offset // widest) * widest == 12


# ---------------------------------------------------------------------------------------------------- constants
def test_constants_are_the_headers():
    d = defines()

    def under(prefix, but=()):
        return {k[len(prefix):]: v for k, v in d.items() if k.startswith(prefix) and k not in but}

    errors = under("ISS_E_")
    assert len(errors) == 5 and {"E_" + k: v for k, v in errors.items()} == {k: v for k, v in vars(_native).items() if k.startswith("E_")}
    assert _native.SEQ_TYPES == {k.lower(): v for k, v in under("ISS_SEQ_").items()} and len(_native.SEQ_TYPES) == 2
    assert _native.EXPORT_ENCODINGS == {k.lower(): v for k, v in under("ISS_EXPORT_").items()} and len(_native.EXPORT_ENCODINGS) == 2
    for name in ("BAM_MAX_LEN", "BAM_NQ", "BAM_NTLEN", "BAM_OFF_INDEL", "BAM_OFF_QHIST", "BAM_OFF_TLEN", "BAM_OFF_NREAD", "BAM_OFF_MINLEN",
                 "BAM_OFF_TAKEN", "BAM_TALLY_WORDS", "FQ_MAX_LEN", "BR_MAX_LEN", "BR_DEPTH_COUNT_DEL"):
        assert getattr(_native, name) == d["ISS_" + name], name
    assert {k for k in vars(_native) if k.startswith("BAM_OFF_")} == {"BAM_OFF_" + k for k in under("ISS_BAM_OFF_")}
    for table, prefix, n in ((_native.BAM_REC_ERRORS, "ISS_BAM_REC_", 9), (_native.FQ_REC_ERRORS, "ISS_FQ_REC_", 6),
                             (_native.BR_REC_ERRORS, "ISS_BR_REC_", 4), (_native.BR_ALN_ERRORS, "ISS_BR_ALN_", 3),
                             (_native.BR_DEPTH_ERRORS, "ISS_BR_DEPTH_", 3)):
        codes = under(prefix, but=("ISS_BR_DEPTH_COUNT_DEL",))
        assert set(table) == set(codes.values()) and len(codes) == len(table) == n, prefix
    status = under("ISS_BGZF_")
    assert {k: _native.BGZF_STATUS.index(k) for k in _native.BGZF_STATUS} == status
    assert (_native.BGZF_OK, _native.BGZF_TRAILING) == (status["OK"], status["TRAILING"])


# ---------------------------------------------------------------------------------------------------- loading
UNSET = object()


class Entry(object):
    def __init__(self):
        self.argtypes = self.restype = UNSET


def stand_in(missing=()):
    """A class to put in ctypes.CDLL's place: its iss_* attributes come into being when asked for and remember what is assigned;
    those of ``missing`` do not exist."""
    class Library(object):
        def __init__(self, path):
            self.path = path

        def __getattr__(self, name):
            if not name.startswith("iss_") or name in missing:
                raise AttributeError(name)
            setattr(self, name, Entry())
            return getattr(self, name)

    return Library


@pytest.fixture
def load(monkeypatch):
    def load(missing=()):
        monkeypatch.setattr(_native, "LIB_PATH", os.path.abspath(__file__))  # (a file that exists)
        monkeypatch.setattr(_native, "_lib", None)
        monkeypatch.setattr(_native.C, "CDLL", stand_in(missing))
        return _native.lib()

    return load


def applied(L, rows):
    return all(getattr(L, name).restype is restype and getattr(L, name).argtypes == list(argtypes) for name, restype, argtypes, _ in rows)


def test_groups_are_the_issues_labels():
    assert tuple(_native.GROUPS) != () and set(_native.GROUPS) == set(GROUPS) == {row[3] for row in _native.TABLE} - {None}
    assert sorted(n for names in _native.GROUPS.values() for n in names) == sorted(row[0] for row in _native.TABLE if row[3])


def test_a_whole_library_gets_every_row(load):
    L = load()
    assert L.path == _native.LIB_PATH and _native.lib() is L
    assert applied(L, _native.TABLE) and {k for k in vars(L) if k.startswith("iss_")} == set(_native.EXPORTS)
    for label in GROUPS:
        _native.need(L, label)


@pytest.mark.parametrize("label", GROUPS)
def test_a_library_without_one_group_loads_and_the_group_is_named(load, label):
    lacking = _native.GROUPS[label]
    L = load(missing=lacking)
    assert applied(L, [row for row in _native.TABLE if row[3] != label])
    assert not any(hasattr(L, name) for name in lacking)
    with pytest.raises(_native.NativeLibraryError) as e:
        _native.need(L, label)
    assert _native.LIB_PATH in str(e.value) and "does not export" in str(e.value) and "rebuild it" in str(e.value)
    assert all(name in str(e.value) for name in lacking)
    assert ("ISS_HOST_VCF=1" in str(e.value)) == (label == "vcf")
    for other in GROUPS:
        if other != label:
            _native.need(L, other)


def test_a_group_lacking_one_entry_names_that_one(load):
    L = load(missing=("iss_depth_finish",))
    with pytest.raises(_native.NativeLibraryError) as e:
        _native.need(L, "depth")
    assert "iss_depth_finish" in str(e.value) and "iss_depth_mark" not in str(e.value)


@pytest.mark.parametrize("name", ["iss_generate", "iss_bam_create", "iss_abi_version"])
def test_a_library_lacking_an_entry_every_build_has_does_not_load(load, name):
    with pytest.raises(_native.NativeLibraryError) as e:
        load(missing=(name,))
    assert name in str(e.value) and _native.LIB_PATH in str(e.value)
    assert _native._lib is None


def test_the_built_library_loads_with_every_row():
    if os.path.exists(_native.LIB_PATH):  # (the library is built: no GPU needed to look)
        L = _native.lib()
        for name, restype, argtypes, _ in _native.TABLE:
            assert getattr(L, name).restype is restype and tuple(getattr(L, name).argtypes) == tuple(argtypes), name


# ---------------------------------------------------------------------------------------------------- the work lists
def test_item_arrays():
    items = [("rec1", 5, 0, 3, 9, 100), (b"rec2", 1 << 40, 3, 2, 8, 200), (7, 0, 5, 1, 7, 300)]
    ids, a, b = engine._item_arrays(items, (3, 1))
    assert isinstance(ids, C.c_char_p * 3) and list(ids) == [b"rec1", b"b'rec2'", b"7"]  # (str() of whatever the id is)
    assert a.dtype == b.dtype == np.int64 and a.tolist() == [3, 2, 1] and b.tolist() == [5, 1 << 40, 0]  # the order asked for
    ids, = engine._item_arrays(items, (), bytes_ids=True)
    assert list(ids) == [b"rec1", b"rec2", b"7"]
    ids, off = engine._item_arrays(items, (5,), id_col=4)
    assert list(ids) == [b"9", b"8", b"7"] and off.tolist() == [100, 200, 300]
    ids, a = engine._item_arrays([], (1,))
    assert len(ids) == 0 and a.dtype == np.int64 and a.size == 0


class RecordingLib(object):
    """Every iss_* entry exists, returns 0 and notes its arguments, arrays read back through the addresses it was handed."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("iss_"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or 0


def int64s(address, n):
    return np.ctypeslib.as_array((C.c_int64 * n).from_address(address)).tolist() if n else []


def test_the_four_simple_emitters_hand_over_what_they_did():
    eng = engine.ReadEngine.__new__(engine.ReadEngine)
    eng._lib, eng._ctx = RecordingLib(), None
    items = [("contig_1", 0, 0, 4), ("NC_000913.3", 1 << 33, 4, 1), (b"raw", 17, 5, 1 << 32)]
    n = len(items)
    plain = [b"contig_1", b"NC_000913.3", b"b'raw'"]  # the ids through str(), as fastq_emit_batch and vcf_emit take them
    as_bytes = [b"contig_1", b"NC_000913.3", b"raw"]  # bytes as they are, as ubam_emit_batch and origins_emit_batch take them
    cols = [[it[k] for it in items] for k in (1, 2, 3)]
    seen = []

    def entry(name, *args):
        seen.append((name,) + args)

    lib = eng._lib
    lib.iss_fastq_emit_batch = lambda ctx, f1, f2, n_, ids, a, b, c, cpu: entry("fastq", ctx, f1, f2, n_, list(ids), int64s(a, n_), int64s(b, n_),
                                                                                  int64s(c, n_), cpu) or 0
    lib.iss_vcf_emit = lambda ctx, fd, src, n_, ids, a, b, c, cpu, need: entry("vcf", ctx, fd, src, n_, list(ids), int64s(a, n_), int64s(b, n_),
                                                                                 int64s(c, n_), cpu, need._obj.value) or 0
    lib.iss_ubam_emit_batch = lambda ctx, fd, n_, ids, a, b, c, cpu: entry("ubam", ctx, fd, n_, list(ids), int64s(a, n_), int64s(b, n_), int64s(c, n_),
                                                                            cpu) or 0
    lib.iss_origins_emit_batch = lambda ctx, fd, n_, ids, a, b, c, d, cpu: entry("origins", ctx, fd, n_, list(ids), int64s(a, n_), int64s(b, n_),
                                                                                 int64s(c, n_), int64s(d, n_), cpu) or 0
    eng.fastq_emit_batch(3, 4, items, 2)
    eng.vcf_emit(5, items, 1, source="mt")
    eng.ubam_emit_batch(6, items, 0)
    eng.origins_emit_batch(7, items, [100, 1 << 34, 300], 3)
    assert seen == [("fastq", None, 3, 4, n, plain) + tuple(cols) + (2,),
                    ("vcf", None, 5, 1, n, plain) + tuple(cols) + (1, 0),
                    ("ubam", None, 6, n, as_bytes) + tuple(cols) + (0,),
                    ("origins", None, 7, n, as_bytes) + tuple(cols) + ([100, 1 << 34, 300], 3)]
    assert eng.mutation_slots_needed == 0
    del seen[:]
    eng.fastq_emit_batch(3, 4, [], 2)
    eng.ubam_emit_batch(6, [], 0)
    assert seen == [("fastq", None, 3, 4, 0, [], [], [], [], 2), ("ubam", None, 6, 0, [], [], [], [], 0)]


def test_the_two_emitters_with_int32_columns():
    eng = engine.ReadEngine.__new__(engine.ReadEngine)
    eng._lib, eng._ctx = RecordingLib(), None
    seen = []

    def int32s(address, n):
        return np.ctypeslib.as_array((C.c_int32 * n).from_address(address)).tolist()

    eng._lib.iss_fastq_emit_scatter = lambda ctx, f1, f2, n, ids, a, b, c, cpus, off, thr: seen.append(
        (f1, f2, n, list(ids), int64s(a, n), int64s(b, n), int64s(c, n), int32s(cpus, n), int64s(off, n), thr)) or 0
    eng._lib.iss_vcf_emit_workers = lambda ctx, n, fds, ids, a, b, c, cpus: seen.append(
        (n, int32s(fds, n), list(ids), int64s(a, n), int64s(b, n), int64s(c, n), int32s(cpus, n))) or 0
    eng.fastq_emit_scatter(3, 4, [("a", 1, 2, 3, 4, 1 << 35), ("b", 5, 6, 7, 8, 9)], n_threads=2)
    eng.fastq_emit_scatter(3, 4, [])  # (nothing to do: no call)
    eng.vcf_emit_workers([(11, "a", 1, 2, 3, 4), (12, "b", 5, 6, 0, 7)])
    assert seen == [(3, 4, 2, [b"a", b"b"], [1, 5], [2, 6], [3, 7], [4, 8], [1 << 35, 9], 2),
                    (2, [11, 12], [b"a", b"b"], [1, 5], [2, 6], [3, 0], [4, 7])]
