"""MM_FASTX_ONE_MINIMIZER of the DNA stream (mm_fastx_stream_create): what needs no GPU - the flag's value, the export,
and the refusals of create before any device is touched."""
import ctypes as C


def test_flag_and_entry_point(sm):
    L = sm.lib()
    assert sm.FASTX_ONE_MINIMIZER == 256
    assert hasattr(L, "mm_fastx_stream_one_minimizer")
    assert "mm_fastx_stream_one_minimizer" in sm.EXPORTED_SYMBOLS
    assert L.mm_fastx_stream_one_minimizer.argtypes is not None
    words, n = C.c_void_p(), C.c_uint64()
    fake = C.c_void_p(4096)  # (never dereferenced: the NULL arguments are refused first)
    assert L.mm_fastx_stream_one_minimizer(None, C.byref(words), C.byref(n)) == sm.ERR["NULL"]
    assert L.mm_fastx_stream_one_minimizer(fake, None, C.byref(n)) == sm.ERR["NULL"]
    assert L.mm_fastx_stream_one_minimizer(fake, C.byref(words), None) == sm.ERR["NULL"]


def test_refusals_of_create_before_any_device(sm):
    """The flag is known to the DNA stream only; 32, 64 and 128 stay unknown there; with MM_FASTX_LONG_RECORDS it is
    refused with a message that says why.  Device -1 stands for "everything else was accepted"."""
    L, E = sm.lib(), sm.ERR
    ONE, LONG, SKIP, U64, SK = (sm.FASTX_ONE_MINIMIZER, sm.FASTX_LONG_RECORDS, sm.FASTX_SKIP_AMBIGUOUS, sm.FASTX_VALUES_U64,
                                sm.FASTX_SK)
    canon, fwd, text = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.mm_plan_create(C.byref(canon), 21, 11, 1, 0, None) == 0
    assert L.mm_plan_create(C.byref(fwd), 21, 11, 0, 0, None) == 0
    th = sm.TextMulHasher(canonical=False)
    assert L.mm_plan_create_text(C.byref(text), 7, 11, 0, 0, C.byref(th)) == 0

    def create(plan, flags, chunk_bytes=1 << 16, device=-1):
        c = sm.FastxStreamConfig(device, 0, flags, 0, chunk_bytes, 100, 0, 0)
        h = C.c_void_p()
        r = L.mm_fastx_stream_create(C.byref(h), plan, C.byref(c))
        assert r != 0 and not h.value
        return r

    try:
        # accepted: only the missing device is left to refuse
        for plan, flags in ((canon, ONE), (fwd, ONE), (canon, ONE | SKIP), (canon, ONE | U64), (fwd, ONE | SK | U64),
                            (canon, ONE | SKIP | U64)):
            assert create(plan, flags) == E["NO_DEVICE"], flags
        # with long records: refused, and the message says why
        assert create(canon, ONE | LONG) == E["BAD_MODE"]
        msg = L.mm_last_error()
        assert b"MM_FASTX_ONE_MINIMIZER" in msg and b"MM_FASTX_LONG_RECORDS" in msg and b"not joined" in msg, msg
        assert create(canon, ONE | LONG | SKIP | U64) == E["BAD_MODE"]
        assert create(canon, ONE | LONG, chunk_bytes=64) == E["BAD_MODE"]  # (ahead of the long-records capacity check)
        assert create(canon, LONG, chunk_bytes=64) == E["CAPACITY"]
        # the values between stay unknown to the DNA stream, alone and beside the new flag
        for bad in (32, 64, 128, 512, 1 << 31):
            assert create(canon, bad) == E["BAD_MODE"], bad
            assert create(canon, ONE | bad) == E["BAD_MODE"], bad
        # the earlier refusals keep their places in front of it
        assert create(fwd, ONE | SKIP) == E["HASHER_NOT_CANONICAL"]
        assert create(canon, ONE | SK | SKIP) == E["BAD_MODE"]
        # a text stream refuses 256 (it has MM_FASTX_TEXT_ONE_MINIMIZER), the DNA stream refuses a text plan
        c = sm.FastxTextStreamConfig(-1, 0, ONE, 0, 1 << 16, 100, 0, 0, sm.TEXT_VALUES_BYTES)
        h = C.c_void_p()
        assert L.mm_fastx_text_stream_create(C.byref(h), text, C.byref(c)) == E["BAD_MODE"] and not h.value
        c = sm.FastxTextStreamConfig(-1, 0, sm.FASTX_TEXT_ONE_MINIMIZER, 0, 1 << 16, 100, 0, 0, sm.TEXT_VALUES_BYTES)
        assert L.mm_fastx_text_stream_create(C.byref(h), text, C.byref(c)) == E["NO_DEVICE"] and not h.value
        assert create(text, ONE) == E["BAD_MODE"]
    finally:
        for p in (canon, fwd, text):
            L.mm_plan_destroy(p)


def test_python_stream_takes_the_option(sm):
    import inspect
    assert "one_minimizer" in inspect.signature(sm.FastxStream.__init__).parameters
    assert "one_min" in inspect.signature(sm.FastxBatch.__init__).parameters
