"""CPU checks of many byte-text records in one call (mm_run_text_batch_*): the argument checks that need no device, the
new symbols and error code in the Python mirror, and the Python input handling up to the C call."""
import ctypes as C

import numpy as np
import pytest

BATCH_SYMBOLS = ["mm_run_text_batch_device_async", "mm_run_text_batch_device", "mm_run_text_batch_host"]


def test_symbols_and_error_code(sm):
    L = sm.lib()
    for name in BATCH_SYMBOLS:
        assert name in sm.EXPORTED_SYMBOLS
        getattr(L, name)
    assert sm.ERR["UNSORTED"] == -24
    assert L.mm_strerror(sm.ERR["UNSORTED"]) == b"record starts must not decrease"


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))


def test_argument_checks_without_a_device(sm):
    """Every refusal that needs no workspace comes before the workspace is looked at (ws = NULL here)."""
    L = sm.lib()
    E = sm.ERR
    text_plan = sm.Plan(21, 11, False, 0, None, text=True)
    packed_plan = sm.Plan(21, 11, False, 0, None)
    sync_plan = sm.Plan(21, 11, False, 1, None, text=True)
    cnt = C.c_uint64()
    offs = np.zeros(8, dtype=np.uint64)
    pos = np.zeros(100, dtype=np.uint32)
    text = np.zeros(100, dtype=np.uint8)
    tp = text.ctypes.data_as(C.POINTER(C.c_uint8))
    pp = pos.ctypes.data_as(C.POINTER(C.c_uint32))
    op = offs.ctypes.data_as(C.POINTER(C.c_uint64))
    fake = C.c_void_p(0x1000)  # (never dereferenced: every call below is refused first)

    def dev(plan, n_records, n_chars, text_bytes=1 << 40, sk=None, offsets=fake, starts=fake):
        return L.mm_run_text_batch_device(plan.h, None, fake, text_bytes, n_records, starts, n_chars, fake, sk, 100,
                                          offsets, C.byref(cnt))

    assert dev(packed_plan, 1, 10) == E["BAD_MODE"]
    assert dev(text_plan, 1, 1 << 32) == E["LEN_TOO_LARGE"]
    assert dev(text_plan, 1 << 31, 10) == E["LEN_TOO_LARGE"]
    assert dev(sync_plan, 1, 10, sk=fake) == E["BAD_MODE"]
    assert dev(text_plan, 1, 10, offsets=None) == E["NULL"]
    assert dev(text_plan, 1, 10, starts=None) == E["NULL"]
    assert dev(text_plan, 1, 101, text_bytes=100) == E["CAPACITY"]
    assert dev(text_plan, 1, 10) == E["NULL"]  # (the workspace, last)
    assert L.mm_run_text_batch_device_async(packed_plan.h, None, fake, 0, 0, fake, 0, None, None, 0, fake,
                                            None) == E["BAD_MODE"]
    assert L.mm_run_text_batch_device_async(text_plan.h, None, fake, 0, 0, fake, 1 << 32, None, None, 0, fake,
                                            None) == E["LEN_TOO_LARGE"]

    def host(plan, starts, sk=None):
        return L.mm_run_text_batch_host(plan.h, None, tp, len(starts) - 1, _u64(starts), pp, sk, 100, op, C.byref(cnt))

    assert host(packed_plan, [0, 10]) == E["BAD_MODE"]
    assert host(sync_plan, [0, 10], sk=pp) == E["BAD_MODE"]
    assert host(text_plan, [0, 50, 40, 100]) == E["UNSORTED"]
    assert host(text_plan, [5, 4]) == E["UNSORTED"]
    assert host(text_plan, [0, 1 << 32]) == E["LEN_TOO_LARGE"]
    assert host(text_plan, [0, 0, 50, 50, 100]) == E["NULL"]  # (ordered: only the workspace is missing)
    # the single-text and packed entry points are unchanged: a text plan is still refused by the packed ones
    assert L.mm_run_packed_reads_host(text_plan.h, None, None, 0, None, 0, None, None, 0, op,
                                      C.byref(cnt)) == E["BAD_MODE"]


class _RecordingLib:
    """The real library, with the batch entry point replaced by a recorder that fills a plausible answer."""

    def __init__(self, real):
        self._real = real
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def mm_run_text_batch_host(self, plan, ws, text, n_records, starts, pos, sk, cap, offs, cnt):
        st = [starts[i] for i in range(n_records + 1)] if n_records else [0]
        self.calls.append((bytes(C.string_at(text, st[-1])) if st[-1] else b"", st, cap, bool(sk)))
        for r in range(n_records + 1):
            offs[r] = r  # (one position per record)
        for r in range(n_records):
            pos[r] = 100 + r
            if sk:
                sk[r] = 200 + r
        cnt._obj.value = n_records
        return 0


class _FakeWorkspace:
    h = C.c_void_p(0x1234)


def test_python_batch_input_handling(sm, monkeypatch):
    rec = _RecordingLib(sm.lib())
    monkeypatch.setattr(sm, "lib", lambda: rec)
    b = sm.minimizers(5, 11).workspace(_FakeWorkspace())
    records = [b"MKV", bytearray(b""), np.frombuffer(b"ACDEFG", dtype=np.uint8), memoryview(b"\x00\xff")]
    pos, offs, idx = sm.run_text_batch_host(b, records)
    text, starts, cap, has_sk = rec.calls[0]
    assert text == b"MKVACDEFG\x00\xff" and starts == [0, 3, 3, 9, 11] and cap == 11 and not has_sk
    assert list(pos) == [100, 101, 102, 103] and offs == [0, 1, 2, 3, 4] and idx is None
    pos, offs, idx = sm.run_text_batch_host(b, records, super_kmers=True)
    assert rec.calls[1][3] and list(idx) == [200, 201, 202, 203]
    pos, offs, idx = sm.run_text_batch_host(b, [])
    assert rec.calls[2][1] == [0] and offs == [0] and len(pos) == 0
    with pytest.raises(TypeError):
        sm.run_text_batch_host(b, ["a str is not byte text"])
    # run_reads_host still reads bytes as ASCII DNA (packed entry point), untouched by the batch text path
    assert len(rec.calls) == 3
