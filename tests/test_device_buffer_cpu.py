"""hip.DeviceBuffer against a stand-in library whose device memory is host
memory: what it allocates, copies and frees, in which order, and what it
refuses before any call.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from tmlibrary_amd import hip


class FakeLib(object):
    """tmh_malloc_device / tmh_memcpy / tmh_free_device over ctypes string
    buffers; every call is recorded.  ``fail[name]``: the calls of that entry
    (0-based, counted per entry) that return ``TMH_ENOMEM`` / ``TMH_EDEVICE``."""

    def __init__(self, fail=None):
        self.calls = []
        self.live = {}
        self.fail = fail or {}
        self.count = {}

    def _failing(self, name):
        k = self.count.get(name, 0)
        self.count[name] = k + 1
        return k in self.fail.get(name, ())

    def tmh_malloc_device(self, ref, nbytes):
        self.calls.append(("malloc", nbytes))
        if self._failing("malloc"):
            ref._obj.value = None
            return hip.TMH_ENOMEM
        if nbytes == 0:
            ref._obj.value = None       # as hipMalloc of no bytes
            return hip.TMH_OK
        mem = C.create_string_buffer(nbytes)
        self.live[C.addressof(mem)] = mem
        ref._obj.value = C.addressof(mem)
        return hip.TMH_OK

    def tmh_memcpy(self, dst, src, nbytes, kind, stream):
        self.calls.append(("memcpy", nbytes, kind))
        if self._failing("memcpy"):
            return hip.TMH_EDEVICE
        C.memmove(dst.value, src.value, nbytes)
        return hip.TMH_OK

    def tmh_free_device(self, p):
        self.calls.append(("free", p.value))
        del self.live[p.value]          # a double free is a KeyError
        return hip.TMH_OK

    def tmh_last_error(self):
        return b"stand-in failure"

    def named(self, name):
        return [c for c in self.calls if c[0] == name]


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(hip, "_lib", lib)
    return lib


def test_put_get_round_trip_with_and_without_offsets(fake):
    a = np.arange(64, dtype=np.uint16)
    with hip.DeviceBuffer(a.nbytes) as buf:
        assert buf.nbytes == 128 and fake.calls == [("malloc", 128)]
        buf.put(a)
        assert np.array_equal(buf.get(64, np.uint16), a)
        assert np.array_equal(buf.get((2, 8), np.uint16, offset=32), a[16:32].reshape(2, 8))
        buf.put(np.array([7, 8], np.uint16), offset=124)
        got = buf.get(64, np.uint16)
        assert got[-2:].tolist() == [7, 8] and np.array_equal(got[:-2], a[:-2])
        assert buf.get(0, np.uint8, offset=128).size == 0       # the end itself is in range
    assert [c[1:] for c in fake.named("memcpy")] == [(128, 0), (128, 1), (32, 1), (4, 0), (128, 1),
                                                     (0, 1)]
    assert not fake.live


def test_put_takes_a_strided_array(fake):
    a = np.arange(24, dtype=np.int32).reshape(4, 6)
    with hip.DeviceBuffer(48) as buf:
        buf.put(a[:, ::2])
        assert np.array_equal(buf.get((4, 3), np.int32), a[:, ::2])


def test_from_array_uploads_the_bytes(fake):
    a = np.arange(30, dtype=np.float64).reshape(5, 6)[:, 1:4]       # not contiguous
    buf = hip.DeviceBuffer.from_array(a)
    assert buf.nbytes == a.size * 8
    assert fake.calls == [("malloc", a.size * 8), ("memcpy", a.size * 8, 0)]
    assert C.string_at(buf.ptr.value, buf.nbytes) == np.ascontiguousarray(a).tobytes()
    buf.free()


def test_out_of_range_raises_before_any_call(fake):
    buf = hip.DeviceBuffer(100)
    before = list(fake.calls)
    for offset in (-1, 101):
        with pytest.raises(ValueError):
            buf.at(offset)
    assert buf.at(0).value == buf.value == buf.ptr.value
    assert buf.at(100).value == buf.value + 100
    with pytest.raises(ValueError):
        buf.put(np.zeros(101, np.uint8))
    with pytest.raises(ValueError):
        buf.put(np.zeros(8, np.uint8), offset=93)
    with pytest.raises(ValueError):
        buf.put(np.zeros(8, np.uint8), offset=-8)
    with pytest.raises(ValueError):
        buf.get(26, np.int32)
    with pytest.raises(ValueError):
        buf.get(4, np.uint8, offset=97)
    assert fake.calls == before
    buf.free()


def test_zero_bytes_is_a_null_pointer_and_is_never_freed(fake):
    with hip.DeviceBuffer(0) as buf:
        assert buf.ptr.value is None and buf.value is None and buf.nbytes == 0
    buf.free()
    assert fake.calls == [("malloc", 0)]
    with pytest.raises(ValueError):
        hip.DeviceBuffer(-1)
    assert fake.calls == [("malloc", 0)]


def test_free_is_idempotent_and_use_after_free_raises(fake):
    buf = hip.DeviceBuffer(16)
    address = buf.ptr.value
    buf.free()
    buf.free()
    del buf                     # and the destructor does not free again
    assert fake.named("free") == [("free", address)]
    buf = hip.DeviceBuffer(16)
    buf.free()
    assert buf.ptr.value is None
    calls = list(fake.calls)
    for use in (lambda: buf.at(0), lambda: buf.put(np.zeros(4, np.uint8)),
                lambda: buf.get(4, np.uint8)):
        with pytest.raises(ValueError, match="buffer is freed"):
            use()
    assert fake.calls == calls


def test_with_frees_on_a_raised_exception_and_the_destructor_frees(fake):
    with pytest.raises(KeyError):
        with hip.DeviceBuffer(32):
            raise KeyError("inside")
    assert len(fake.named("free")) == 1 and not fake.live
    hip.DeviceBuffer(32)        # dropped at once
    assert len(fake.named("free")) == 2 and not fake.live


def test_failed_allocation_is_a_memory_error(monkeypatch):
    lib = FakeLib(fail={"malloc": (0,)})
    monkeypatch.setattr(hip, "_lib", lib)
    with pytest.raises(MemoryError, match="stand-in failure"):
        hip.DeviceBuffer(1 << 20)
    assert lib.calls == [("malloc", 1 << 20)]


def test_failed_upload_in_from_array_frees_the_allocation(monkeypatch):
    lib = FakeLib(fail={"memcpy": (0,)})
    monkeypatch.setattr(hip, "_lib", lib)
    with pytest.raises(hip.HipError):
        hip.DeviceBuffer.from_array(np.zeros(10))
    assert [c[0] for c in lib.calls] == ["malloc", "memcpy", "free"] and not lib.live


def test_passes_where_argtypes_say_c_void_p(fake):
    memmove = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)(("memmove", C.CDLL(None)))
    a = np.arange(16, dtype=np.uint8)
    out = np.zeros(16, dtype=np.uint8)
    with hip.DeviceBuffer.from_array(a) as buf:
        memmove(hip.ptr(out), buf, 16)
        assert np.array_equal(out, a)
    null = C.CFUNCTYPE(C.c_size_t, C.c_void_p)(lambda p: p or 0)
    with hip.DeviceBuffer(0) as buf:
        assert null(buf) == 0


def test_device_table_frees_the_first_upload_when_the_second_fails(monkeypatch):
    from tmlibrary_amd.tools.base import DeviceTable, RobustScaler
    lib = FakeLib(fail={"memcpy": (1,)})
    monkeypatch.setattr(hip, "_lib", lib)
    scaler = RobustScaler()
    scaler.center_, scaler.scale_ = np.zeros(3), np.ones(3)
    table = DeviceTable(np.ones((5, 3)), scaler)
    with pytest.raises(hip.HipError):
        table.__enter__()
    assert [c[0] for c in lib.calls] == ["malloc", "memcpy", "malloc", "memcpy", "free", "free"]
    assert not lib.live


def test_device_table_keeps_its_interface(fake):
    from tmlibrary_amd.tools.base import DeviceTable
    X = np.arange(12, dtype=np.float64).reshape(4, 3)
    with DeviceTable(X) as t:
        assert (t.n, t.d) == (4, 3) and t.center is None and t.scale is None
        assert np.array_equal(t.x.get((4, 3), np.float64), X)
        extra = t.alloc(40)
        assert extra.nbytes == 40 and len(fake.live) == 2
        # x and what alloc returns read as the c_void_p they were
        assert t.x.value == t.x.ptr.value and extra.value == extra.ptr.value
        assert C.c_void_p(extra.value + 16).value == extra.at(16).value
    assert not fake.live
