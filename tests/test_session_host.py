"""insilicoseq_amd._native.Session, the base of the stand-alone device contexts' Python classes, against a fake library in plain
Python: what a failed create leaves behind, close, _check, reset and kernel_ms, and a library without the prefix's entries.  No GPU
and no HIP library."""
import ctypes as C

import pytest

from insilicoseq_amd import _native


class FakeLib(object):
    """iss_x_* over handles 1, 2, ...: `calls` lists what was called; `fail_create` makes create fail, with a handle (1) or without."""

    def __init__(self, fail_create=None):
        self.fail_create = fail_create
        self.calls = []
        self.alive = set()
        self.errors = {None: b"thread: no device"}
        self.next_rc = 0

    def iss_x_create(self, device, extra, out):
        self.calls.append(("create", device, extra))
        if self.fail_create == "no handle":
            return _native.E_HIP
        h = len(self.calls)
        out._obj.value = h
        self.alive.add(h)
        if self.fail_create == "handle":
            self.errors[h] = b"handle: no stream"
            return _native.E_HIP
        return 0

    def iss_x_destroy(self, h):
        self.calls.append(("destroy", h.value))
        self.alive.remove(h.value)
        self.errors.pop(h.value, None)

    def iss_x_last_error(self, h):
        return self.errors.get(h.value if h is not None else None)

    def iss_x_reset(self, h):
        self.calls.append(("reset", h.value))
        return self.next_rc

    def iss_x_kernel_ms(self, h, ms):
        ms._obj.value = 1.5
        return self.next_rc


class X(_native.Session):
    PREFIX = "iss_x"

    def __init__(self, device=0, extra=7):
        _native.Session.__init__(self, device, extra)


@pytest.fixture
def fake(monkeypatch):
    def install(**kw):
        lib = FakeLib(**kw)
        monkeypatch.setattr(_native, "lib", lambda: lib)
        return lib

    return install


def test_create_close_and_context_manager(fake):
    lib = fake()
    with X(3) as x:
        assert x._lib is lib and x._h.value == 1 and x.device == 3 and lib.calls == [("create", 3, 7)]
        x.reset()
        assert x.kernel_ms() == 1.5
    assert not x._h and not lib.alive and lib.calls[-1] == ("destroy", 1)
    n = len(lib.calls)
    x.close()
    x.close()
    del x
    assert len(lib.calls) == n  # close twice, and the finalizer after it: nothing is destroyed again


@pytest.mark.parametrize("how,message", [("handle", "handle: no stream"), ("no handle", "thread: no device")])
def test_failed_create_raises_with_the_message_and_leaves_a_closed_object(fake, how, message):
    lib = fake(fail_create=how)
    made = []

    class Kept(X):
        def __init__(self):
            made.append(self)
            X.__init__(self)

    with pytest.raises(_native.EngineError) as e:
        Kept()
    assert e.value.code == _native.E_HIP and e.value.message == message
    assert not made[0]._h and not lib.alive  # the error was read from the handle before it went
    assert [c[0] for c in lib.calls] == (["create", "destroy"] if how == "handle" else ["create"])
    made[0].close()
    assert [c[0] for c in lib.calls].count("destroy") == (1 if how == "handle" else 0)


def test_check_raises_with_the_sessions_last_error(fake):
    lib = fake()
    x = X()
    assert x._check(0) == 0 and x._check(5) == 5
    lib.errors[1], lib.next_rc = b"iss_x_reset: bad arguments", _native.E_INVALID
    with pytest.raises(_native.EngineError) as e:
        x.reset()
    assert e.value.code == _native.E_INVALID and e.value.message == "iss_x_reset: bad arguments"
    assert "iss_x_reset: bad arguments (iss error -1)" in str(e.value)
    lib.errors.pop(1)
    with pytest.raises(_native.EngineError) as e:
        x.kernel_ms()
    assert e.value.message == "unknown error"
    assert x._h.value == 1  # a failed call leaves the session open
    x.close()


def test_library_without_the_entries(monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda: object())
    with pytest.raises(_native.NativeLibraryError) as e:
        X()
    assert "has no iss_x_* entries: rebuild it" in str(e.value) and _native.LIB_PATH in str(e.value)


def test_the_four_contexts_derive_from_it():
    from insilicoseq_amd.bam_report import BamReadTally
    from insilicoseq_amd.engine import BamTally
    from insilicoseq_amd.fastq_report import FastqTally
    from insilicoseq_amd.inflate import BgzfInflater

    classes = (BamTally, FastqTally, BgzfInflater, BamReadTally)
    assert all(issubclass(c, _native.Session) for c in classes)
    assert sorted(c.PREFIX for c in classes) == sorted(_native.SESSIONS)
    for prefix in _native.SESSIONS:
        assert all("%s_%s" % (prefix, tail) in _native.EXPORTS for tail in ("create", "destroy", "last_error", "reset"))
