"""The byte-text FASTA stream (mm_fastx_text_stream_create): what needs no GPU - the exports and the refusals of create
before any device is touched, in the order the header documents."""
import ctypes as C


def test_entry_points_exported_and_wrapped(sm):
    L = sm.lib()
    for name in ("mm_fastx_text_stream_create", "mm_fastx_text_stream_extras"):
        assert hasattr(L, name), name
        assert name in sm.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    for name in ("FastxTextStream", "stream_fasta_text", "FastxTextStreamConfig"):
        assert callable(getattr(sm, name)), name
    assert (sm.FASTX_TEXT_ONE_MINIMIZER, sm.FASTX_TEXT_SEQ) == (32, 64)
    out = sm._FastxTextExtrasC()
    assert L.mm_fastx_text_stream_extras(None, C.byref(out)) == sm.ERR["NULL"]


def _text_plan(sm, k=7, w=11, mode=0, canonical=False):
    th = sm.TextMulHasher(canonical=canonical)
    h = C.c_void_p()
    assert sm.lib().mm_plan_create_text(C.byref(h), k, w, 0, mode, C.byref(th)) == 0
    return h


def test_refusals_before_any_device_in_the_documented_order(sm):
    """NULL arguments, a plan that is no text plan, chunk_bytes / max_records out of range, super-k-mers with syncmers, the
    two flags byte text has not, both values flags, an unknown encoding, BYTES values with a canonical hasher, a value
    length beyond the encoding's limit, a plan the fused text kernel does not take, FASTQ, an unknown format / flag / slots,
    no device: each wins over everything behind it."""
    L, E = sm.lib(), sm.ERR
    SK, SKIP, U64, U128, LONG = (sm.FASTX_SK, sm.FASTX_SKIP_AMBIGUOUS, sm.FASTX_VALUES_U64, sm.FASTX_VALUES_U128,
                                 sm.FASTX_LONG_RECORDS)
    ONE, SEQ = sm.FASTX_TEXT_ONE_MINIMIZER, sm.FASTX_TEXT_SEQ
    BYTES, DNA = sm.TEXT_VALUES_BYTES, sm.TEXT_VALUES_DNA
    dna = C.c_void_p()
    assert L.mm_plan_create(C.byref(dna), 21, 11, 0, 0, None) == 0
    fwd = _text_plan(sm)                                   # value length 7
    sync = _text_plan(sm, k=5, w=9, mode=1)                # value length 13
    sync_canon = _text_plan(sm, k=5, w=9, mode=1, canonical=True)
    canon = _text_plan(sm, k=7, canonical=True)
    k12 = _text_plan(sm, k=12, w=5)                        # 12 > 8, <= 16
    k20 = _text_plan(sm, k=20, w=5)                        # 20 > 16
    k40_canon = _text_plan(sm, k=40, w=5, canonical=True)  # DNA: 40 > 32, <= 64
    k70 = _text_plan(sm, k=70, w=5)                        # DNA: 70 > 64
    wide = _text_plan(sm, w=129)
    no_device = L.mm_device_count() <= 0

    def create(plan, flags=0, chunk_bytes=1 << 16, max_records=100, device=0, cfg=True, out=True, fmt=0, slots=0, enc=BYTES):
        c = sm.FastxTextStreamConfig(device, fmt, flags, slots, chunk_bytes, max_records, 0, 0, enc)
        h = C.c_void_p()
        r = L.mm_fastx_text_stream_create(C.byref(h) if out else None, plan, C.byref(c) if cfg else None)
        if r == 0:
            L.mm_fastx_stream_destroy(h)
        else:
            assert not h.value
        return r

    try:
        every = SK | SKIP | LONG | U64 | U128 | 128
        FQ = sm.FASTX_FASTQ
        # every argument wrong at once: the first documented refusal wins, one fix at a time
        assert create(None, every, 1, 1 << 31, -1, fmt=FQ, enc=9) == E["NULL"]
        assert create(dna, every, 1, 1 << 31, -1, cfg=False) == E["NULL"]
        assert create(dna, every, 1, 1 << 31, -1, out=False) == E["NULL"]
        assert create(dna, every, 1, 1 << 31, -1, fmt=FQ, enc=9) == E["BAD_MODE"]       # (no text plan)
        assert b"mm_fastx_stream_create" in L.mm_last_error()
        assert create(sync_canon, every, 63, 1 << 31, -1, fmt=FQ, enc=9) == E["LEN_TOO_LARGE"]
        assert create(sync_canon, every, 1 << 31, 5, -1, fmt=FQ, enc=9) == E["LEN_TOO_LARGE"]
        assert create(sync_canon, every, 64, 1 << 31, -1, fmt=FQ, enc=9) == E["LEN_TOO_LARGE"]  # (max_records alone)
        assert create(sync_canon, every, 64, 5, -1, fmt=FQ, enc=9) == E["BAD_MODE"]     # (super-k-mers with syncmers)
        assert b"MM_FASTX_SK" in L.mm_last_error()
        assert create(canon, every, 64, 5, -1, fmt=FQ, enc=9) == E["BAD_MODE"]          # (the two refused flags)
        assert b"MM_FASTX_SKIP_AMBIGUOUS" in L.mm_last_error()
        assert create(canon, SK | LONG | U64 | U128 | 128, 64, 5, -1, fmt=FQ, enc=9) == E["BAD_MODE"]
        assert b"MM_FASTX_LONG_RECORDS" in L.mm_last_error()
        assert create(canon, SK | SKIP, 64, 5, -1) == E["BAD_MODE"]
        assert create(canon, SK | U64 | U128 | 128, 64, 5, -1, fmt=FQ, enc=9) == E["BAD_MODE"]  # (both values flags)
        assert b"both values flags" in L.mm_last_error()
        assert create(canon, SK | U64 | 128, 64, 5, -1, fmt=FQ, enc=9) == E["BAD_MODE"]  # (an unknown encoding)
        assert b"values_encoding" in L.mm_last_error()
        assert create(canon, SK | 128, 64, 5, -1, fmt=FQ, enc=-1) == E["BAD_MODE"]       # (... with no values flag too)
        assert b"values_encoding" in L.mm_last_error()
        assert create(k40_canon, U64 | 128, 64, 5, -1, fmt=FQ, enc=BYTES) == E["BAD_MODE"]  # (BYTES, canonical hasher)
        assert b"canonical" in L.mm_last_error()
        assert create(k12, U64 | 128, 64, 5, -1, fmt=FQ, enc=BYTES) == E["VALUE_LEN"]    # (12 > 8)
        assert create(k20, U128 | 128, 64, 5, -1, fmt=FQ, enc=BYTES) == E["VALUE_LEN"]   # (20 > 16)
        assert create(sync, U64 | 128, 64, 5, -1, fmt=FQ, enc=BYTES) == E["VALUE_LEN"]   # (syncmers: k + w - 1 = 13 > 8)
        assert create(k40_canon, U64 | 128, 64, 5, -1, fmt=FQ, enc=DNA) == E["VALUE_LEN"]  # (40 > 32)
        assert create(k70, U128 | 128, 64, 5, -1, fmt=FQ, enc=DNA) == E["VALUE_LEN"]     # (70 > 64)
        assert create(wide, U64 | 128, 64, 5, -1, fmt=FQ) == E["BAD_MODE"]               # (w = 129: no fused text kernel)
        assert b"mm_run_text_batch_counts_device" in L.mm_last_error()
        assert create(fwd, U64 | 128, 64, 5, -1, fmt=FQ) == E["FORMAT"]
        assert create(k12, U128 | ONE | SEQ, 64, 5, -1, fmt=FQ) == E["FORMAT"]
        assert create(fwd, U64 | 128, 64, 5, -1) == E["BAD_MODE"]                        # (an unknown flag)
        assert create(fwd, U64, 64, 5, -1, fmt=3) == E["BAD_MODE"]
        assert create(fwd, U64, 64, 5, -1, fmt=-1) == E["BAD_MODE"]
        assert create(fwd, U64, 64, 5, -1, slots=1) == E["BAD_MODE"]
        assert create(fwd, U64, 64, 5, -1, slots=9) == E["BAD_MODE"]
        assert create(k40_canon, U128 | SK | ONE | SEQ, 64, 5, -1, enc=DNA) == E["NO_DEVICE"]  # (device -1, or none at all)
        assert create(fwd, SK | U64, 64, 5, 1 << 20) == E["NO_DEVICE"]
        if no_device:
            assert create(fwd, 0) == E["NO_DEVICE"]
        # the DNA stream still refuses a text plan, and does not know the new flags
        c = sm.FastxStreamConfig(0, 0, 0, 0, 1 << 16, 100, 0, 0)
        h = C.c_void_p()
        assert L.mm_fastx_stream_create(C.byref(h), fwd, C.byref(c)) == E["BAD_MODE"] and not h.value
        c = sm.FastxStreamConfig(0, 0, ONE, 0, 1 << 16, 100, 0, 0)
        assert L.mm_fastx_stream_create(C.byref(h), dna, C.byref(c)) == E["BAD_MODE"] and not h.value
    finally:
        for h in (dna, fwd, sync, sync_canon, canon, k12, k20, k40_canon, k70, wide):
            L.mm_plan_destroy(h)
