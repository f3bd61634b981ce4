"""CPU: capi.DeviceCall, the one statement of a device call on host arrays, against a fake lib() that records every allocation,
copy, sync and free and never touches a device."""
import numpy as np
import pytest

from of_dis_amd import capi


class FakeLib:
    """the memory and sync functions of the library on host bytearrays; `log` has every event in order"""

    def __init__(self):
        self.log, self.mem, self.next = [], {}, 0x1000

    def ofdis_dev_alloc(self, nbytes):
        ptr, self.next = self.next, self.next + 0x1000 + nbytes
        self.mem[ptr] = bytearray(nbytes)
        self.log.append(("alloc", ptr, nbytes))
        return ptr

    def ofdis_dev_free(self, ptr):
        del self.mem[ptr]   # (a second free of a pointer is an error here)
        self.log.append(("free", ptr))

    def ofdis_memcpy_h2d(self, dst, src, nbytes):
        import ctypes
        self.mem[dst][:nbytes] = ctypes.string_at(src, nbytes)
        self.log.append(("h2d", dst, nbytes))
        return 0

    def ofdis_memcpy_d2h(self, dst, src, nbytes):
        import ctypes
        ctypes.memmove(dst, bytes(self.mem[src][:nbytes]), nbytes)
        self.log.append(("d2h", src, nbytes))
        return 0

    def ofdis_sync(self, stream):
        self.log.append(("sync", stream))
        return 0

    def ofdis_last_error(self):
        return b"refused by the fake"

    def call(self, *args, rc=0):
        """a C entry point: records its arguments and returns the status `rc`"""
        self.log.append(("call",) + args)
        return rc

    def events(self, kind):
        return [e for e in self.log if e[0] == kind]

    def index(self, kind, nth=0):
        return [i for i, e in enumerate(self.log) if e[0] == kind][nth]


@pytest.fixture
def fake(monkeypatch):
    L = FakeLib()
    monkeypatch.setattr(capi, "lib", lambda: L)
    return L


STREAM = 0xBEEF


def test_inputs_outputs_and_the_order_of_completion(fake):
    a = np.arange(6, dtype=np.float32).reshape(2, 3)
    seed = np.arange(4, dtype=np.int64)
    with capi.DeviceCall(STREAM) as c:
        pa, pnone = c.input(a), c.input(None)
        po1, po2, po3 = c.output((2, 2), np.int32), c.output((5,), np.uint8, want=False), c.output((4,), np.int64, fill=seed)
        pw = c.work(100)
        capi.check(fake.call(pa, pnone, po1, po2, po3, pw))
        fake.mem[po1][:16] = np.array([[1, 2], [3, 4]], np.int32).tobytes()   # what the kernel wrote
        got = c.results()
    # None in is NULL; an unwanted output is NULL and None
    assert pnone is None and po2 is None and got[1] is None and len(got) == 3
    assert len({pa, po1, po3, pw}) == 4
    np.testing.assert_array_equal(got[0], [[1, 2], [3, 4]])
    assert got[0].dtype == np.int32 and got[2].dtype == np.int64
    np.testing.assert_array_equal(got[2], seed)   # an output starts from its fill
    # the uploads happen before the call
    call = fake.index("call")
    assert [e[1] for e in fake.events("h2d")] == [pa, po3] and fake.index("h2d", 1) < call
    assert fake.log[call] == ("call", pa, None, po1, None, po3, pw)
    # exactly one sync, on the given stream, after the call and before the first download
    assert fake.events("sync") == [("sync", STREAM)]
    assert call < fake.index("sync") < fake.index("d2h")
    # downloads in declaration order, of the shapes' sizes
    assert fake.events("d2h") == [("d2h", po1, 16), ("d2h", po3, 32)]
    # every buffer freed, once, after the sync and the downloads
    assert sorted(e[1] for e in fake.events("free")) == sorted([pa, po1, po3, pw])
    assert fake.index("free") > fake.index("d2h", 1) and not fake.mem


def test_the_least_allocation_is_one_value(fake):
    with capi.DeviceCall() as c:
        c.output((0, 3), np.float32), c.output((1,), np.uint8), c.work(0), c.output((3,), np.float64)
        assert [e[2] for e in fake.events("alloc")] == [capi.DeviceCall.MIN_BYTES] * 3 + [24]
        assert [a.shape for a in c.results()] == [(0, 3), (1,), (3,)]
    assert fake.events("sync") == [("sync", None)] and not fake.mem


def test_an_output_over_an_input_is_the_inputs_device_array(fake):
    a = np.arange(4, dtype=np.float32)
    with capi.DeviceCall() as c:
        pa = c.input(a)
        assert c.output(a.shape, over=pa) == pa and c.output(a.shape, want=False, over=pa) is None
        assert len(fake.events("alloc")) == 1
        got = c.results()
    np.testing.assert_array_equal(got[0], a)
    assert got[1] is None and fake.events("free") == [("free", pa)]


def test_a_refused_call_frees_every_buffer(fake):
    with pytest.raises(capi.OfdisError, match="refused by the fake"):
        with capi.DeviceCall(STREAM) as c:
            capi.check(fake.call(c.input(np.zeros(3, np.float32)), c.output((3,)), c.work(8), rc=capi.ERR_INVALID))
            c.results()
    assert len(fake.events("alloc")) == 3 and len(fake.events("free")) == 3 and not fake.mem
    assert not fake.events("d2h") and not fake.events("sync")   # nothing was enqueued, nothing is waited for


def test_a_failed_sync_frees_every_buffer(fake, monkeypatch):
    monkeypatch.setattr(fake, "ofdis_sync", lambda stream: capi.ERR_DEVICE)
    with pytest.raises(capi.OfdisError):
        with capi.DeviceCall() as c:
            c.input(np.zeros(3, np.float32)), c.output((3,))
            c.results()
    assert not fake.mem and not fake.events("d2h")


def test_the_pointer_form_passes_pointers_through_and_downloads_nothing(fake):
    with capi.DeviceCall(STREAM, own=False) as c:
        ptrs = [c.output((4, 4), np.uint8, 0xA000), c.output((4,), np.uint8, None), c.output((4,), np.uint8, False),
                c.output((4,), np.uint8, 0), c.output((4,), np.uint8, True)]
        assert ptrs == [0xA000, None, None, None, None]
        assert c.results() is None
    assert fake.log == []   # nothing allocated, nothing uploaded: no sync either


def test_the_pointer_form_syncs_exactly_when_something_was_uploaded(fake):
    models = np.ones((2, 6), np.float64)
    with capi.DeviceCall(STREAM, own=False) as c:
        pm = c.input(models)
        capi.check(fake.call(pm, c.output((2, 8, 8, 2), np.float32, 0xA000)))
        assert c.results() is None
    kinds = [e[0] for e in fake.log]
    assert kinds == ["alloc", "h2d", "call", "sync", "free"] and fake.events("sync") == [("sync", STREAM)]
    assert fake.events("free") == [("free", pm)]


def test_a_wrapper_through_the_object(fake, monkeypatch):
    """capi.fb_check end to end on the fake: two uploads, the call's arguments in the C order, one sync, one download"""
    monkeypatch.setattr(fake, "ofdis_fb_check", lambda *args: fake.call(*args), raising=False)
    flow = np.zeros((2, 3, 5, 2), np.float32)
    mask = capi.fb_check(flow, flow)
    assert mask.shape == (2, 3, 5) and mask.dtype == np.uint8
    (_, pf, po, pm, n, w, h, alpha, beta, stream), = fake.events("call")
    assert (n, w, h, alpha, beta, stream) == (2, 5, 3, capi.FB_ALPHA, capi.FB_BETA, None)
    assert [e[1] for e in fake.events("h2d")] == [pf, po] and fake.events("d2h") == [("d2h", pm, 30)]
    assert fake.events("sync") == [("sync", None)] and not fake.mem
