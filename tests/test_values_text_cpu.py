"""K-mer values of byte text (single text and record batches): what needs no GPU - the exports, the size of the LDS
stage, the refusals that come before the device is touched, the kernels' one-value arithmetic run on the host
(mm_debug_values_text) against the oracle and against numpy, and the C++ example's compile."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE = ("mm_values_u64_text_device_async", "mm_values_u128_text_device_async")
SINGLE_HOST = ("mm_values_u64_text_host", "mm_values_u128_text_host")
BATCH = ("mm_values_u64_text_batch_device_async", "mm_values_u128_text_batch_device_async")
BATCH_HOST = ("mm_values_u64_text_batch_host", "mm_values_u128_text_batch_host")
BYTES, DNA = 0, 1
U64_LENS = (1, 5, 15, 16, 17, 21, 31, 32)
U128_LENS = (33, 47, 63, 64, 21)
N_TEXT = 3000


def test_entry_points_exported_and_wrapped(sm):
    L = sm.lib()
    for name in SINGLE + SINGLE_HOST + BATCH + BATCH_HOST + ("mm_values_text_lds_stage", "mm_debug_values_text"):
        assert hasattr(L, name), name
        assert name in sm.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    for name in ("values_text_device", "values_text_batch_device", "values_text_batch_host", "values_text_lds_stage"):
        assert callable(getattr(sm, name)), name
    assert (sm.TEXT_VALUES_BYTES, sm.TEXT_VALUES_DNA) == (BYTES, DNA)
    stage = sm.values_text_lds_stage()
    assert 2 <= stage
    assert stage * 8 <= 64 * 1024  # one 64-bit offset per entry, in a workgroup's 64 KiB


def _callers(sm):
    """Every entry as f(ws, encoding, len, canonical, **kw) with well-formed other arguments; (name, f, is_u128)."""
    L = sm.lib()
    fake = C.c_void_p(4096)  # (never dereferenced: the refusals come first)
    p64 = lambda a: sm._p(a, C.c_uint64)
    starts = np.array([0, 50, 100], dtype=np.uint64)
    offs = np.array([0, 2, 4], dtype=np.uint64)
    pos = np.zeros(4, dtype=np.uint32)
    text = np.zeros(100, dtype=np.uint8)
    vals = np.zeros(8, dtype=np.uint64)
    out = []
    for i, u128 in enumerate((False, True)):
        def single(ws, enc, ln, canon, n=100, text_bytes=100, f=getattr(L, SINGLE[i])):
            return f(ws, fake, text_bytes, n, enc, ln, canon, fake, 4, fake)

        def single_host(ws, enc, ln, canon, n=100, f=getattr(L, SINGLE_HOST[i])):
            return f(ws, sm._p(text, C.c_uint8), n, enc, ln, canon, sm._p(pos, C.c_uint32), 4, p64(vals))

        def batch(ws, enc, ln, canon, n=100, text_bytes=100, n_records=2, f=getattr(L, BATCH[i])):
            return f(ws, fake, text_bytes, n_records, fake, n, enc, ln, canon, fake, fake, 4, fake)

        def batch_host(ws, enc, ln, canon, starts=starts, offs=offs, f=getattr(L, BATCH_HOST[i])):
            return f(ws, sm._p(text, C.c_uint8), len(starts) - 1, p64(starts), enc, ln, canon, sm._p(pos, C.c_uint32),
                     p64(offs), p64(vals))

        out += [(SINGLE[i], single, u128), (SINGLE_HOST[i], single_host, u128), (BATCH[i], batch, u128),
                (BATCH_HOST[i], batch_host, u128)]
    return out


def test_refusals_need_no_device(sm):
    E = sm.ERR
    ws = C.c_void_p(4096)  # (a workspace that is never looked into: every call below is refused first)
    for name, f, u128 in _callers(sm):
        # a NULL workspace is MM_ERR_NULL whatever else is wrong
        assert f(None, DNA, 21, 1) == E["NULL"], name
        assert f(None, DNA, 0, 1) == E["NULL"], name
        assert f(None, 7, 0, 1) == E["NULL"], name
        # the encoding
        for enc in (2, -1, 7):
            assert f(ws, enc, 5, 0) == E["BAD_MODE"], (name, enc)
        assert f(ws, BYTES, 5, 1) == E["BAD_MODE"], name  # general text has no reverse complement
        # len, per encoding and width
        assert f(ws, DNA, 0, 0) == E["VALUE_LEN"], name
        assert f(ws, BYTES, 0, 0) == E["VALUE_LEN"], name
        most = {(BYTES, False): 8, (BYTES, True): 16, (DNA, False): 32, (DNA, True): 64}
        for enc in (BYTES, DNA):
            assert f(ws, enc, most[enc, u128] + 1, 0) == E["VALUE_LEN"], (name, enc)
            if "device" in name:  # (the limit itself passes this check: the next refusal is a later one)
                assert f(ws, enc, most[enc, u128], 0, n=1 << 32, text_bytes=1 << 33) == E["LEN_TOO_LARGE"], (name, enc)
        if "device" in name:
            assert f(ws, DNA, 21, 1, n=1 << 32, text_bytes=1 << 33) == E["LEN_TOO_LARGE"], name
            assert f(ws, DNA, 21, 1, n=101, text_bytes=100) == E["CAPACITY"], name
        if "batch_device" in name:
            assert f(ws, DNA, 21, 1, n_records=1 << 31) == E["LEN_TOO_LARGE"], name
        if "batch_host" in name:
            down = np.array([0, 60, 50], dtype=np.uint64)
            assert f(ws, DNA, 21, 1, starts=down) == E["UNSORTED"], name
            assert f(ws, DNA, 21, 1, offs=np.array([0, 3, 2], dtype=np.uint64)) == E["UNSORTED"], name
    L = sm.lib()
    one = np.zeros(1, dtype=np.uint64)
    buf = np.zeros(8, dtype=np.uint8)
    dbg = lambda enc, ln, canon, u128: L.mm_debug_values_text(C.c_void_p(buf.ctypes.data), 8, enc, ln, canon, u128,
                                                              sm._p(one, C.c_uint64), 1, sm._p(np.zeros(2, np.uint64), C.c_uint64))
    assert dbg(3, 5, 0, 0) == E["BAD_MODE"] and dbg(BYTES, 5, 1, 0) == E["BAD_MODE"]
    assert dbg(BYTES, 9, 0, 0) == E["VALUE_LEN"] and dbg(BYTES, 17, 0, 1) == E["VALUE_LEN"]
    assert dbg(DNA, 33, 0, 0) == E["VALUE_LEN"] and dbg(DNA, 65, 0, 1) == E["VALUE_LEN"] and dbg(DNA, 0, 0, 0) == E["VALUE_LEN"]
    assert dbg(BYTES, 8, 0, 0) == 0 and dbg(BYTES, 16, 0, 1) == 0 and dbg(DNA, 32, 1, 0) == 0 and dbg(DNA, 64, 1, 1) == 0


@pytest.fixture(scope="module")
def dna_text():
    rng = np.random.default_rng(20261018)
    return bytes(rng.choice(np.frombuffer(b"ACGTacgt", dtype=np.uint8), N_TEXT))


@pytest.fixture(scope="module")
def dna_packed(oracle, dna_text):
    return oracle.pack_ascii(dna_text)


def _ints128(a):
    return [int(lo) | (int(hi) << 64) for lo, hi in np.asarray(a).reshape(-1, 2)]


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("length", U64_LENS)
def test_debug_values_dna_u64_match_the_oracle(sm, oracle, dna_text, dna_packed, length, canonical):
    pos = np.arange(0, N_TEXT - length + 1)
    want = oracle.values_u64(dna_packed, length, pos, canonical)
    for shift in range(4):
        got = sm.debug_values_text(dna_text, DNA, length, canonical, abs_pos=pos, address_shift=shift)
        assert np.array_equal(got, want), (length, canonical, shift)


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("length", U128_LENS)
def test_debug_values_dna_u128_match_the_oracle(sm, oracle, dna_text, dna_packed, length, canonical):
    pos = np.arange(0, N_TEXT - length + 1)
    want = _ints128(oracle.values_u128(dna_packed, length, pos, canonical))
    for shift in range(4):
        got = sm.debug_values_text(dna_text, DNA, length, canonical, u128=True, abs_pos=pos, address_shift=shift)
        assert got == want, (length, canonical, shift)


def _little_endian(text: bytes, pos, length):
    """sum text[p + j] << 8j of the zero-padded text, as Python ints."""
    padded = text + bytes(length)
    return [int.from_bytes(padded[p:p + length], "little") for p in pos]


@pytest.fixture(scope="module")
def byte_text():
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, 1500, dtype=np.uint8)
    a[::97] = 0x00
    a[5::89] = 0xFF
    a[-3:] = (0xFF, 0x00, 0xFF)
    return bytes(a)


@pytest.mark.parametrize("length", range(1, 17))
def test_debug_values_bytes_are_little_endian_integers(sm, byte_text, length):
    pos = np.arange(0, len(byte_text) - length + 1)
    want = _little_endian(byte_text, pos, length)
    for shift in range(4):
        got = sm.debug_values_text(byte_text, BYTES, length, u128=True, abs_pos=pos, address_shift=shift)
        assert got == want, (length, shift)
        if length <= 8:
            got = sm.debug_values_text(byte_text, BYTES, length, abs_pos=pos, address_shift=shift)
            assert [int(v) for v in got] == want, (length, shift)


def test_values_past_the_end_are_those_of_the_zero_padded_text(sm, oracle, dna_text, byte_text):
    """text_bytes == n: the last len - 1 positions (and positions past the text) read the missing characters as byte 0."""
    for shift in range(4):
        for length in (8, 16):
            tail = np.arange(len(byte_text) - length + 1, len(byte_text) + 3)
            got = sm.debug_values_text(byte_text, BYTES, length, u128=True, abs_pos=tail, address_shift=shift)
            assert got == _little_endian(byte_text + bytes(8), tail, length), (length, shift)
        padded = oracle.pack_ascii(dna_text + bytes(80))
        for length, canonical in ((21, True), (32, False), (16, True)):
            tail = np.arange(N_TEXT - length + 1, N_TEXT + 3)
            got = sm.debug_values_text(dna_text, DNA, length, canonical, abs_pos=tail, address_shift=shift)
            assert np.array_equal(got, oracle.values_u64(padded, length, tail, canonical)), (length, shift)
        for length, canonical in ((64, True), (47, False)):
            tail = np.arange(N_TEXT - length + 1, N_TEXT + 3)
            got = sm.debug_values_text(dna_text, DNA, length, canonical, u128=True, abs_pos=tail, address_shift=shift)
            assert got == _ints128(oracle.values_u128(padded, length, tail, canonical)), (length, shift)


def test_tiny_buffers_never_read_outside(sm):
    """Texts shorter than a dword at every address shift: the view has no whole dword, every byte goes the edge path."""
    for n in range(0, 6):
        text = bytes(range(0x41, 0x41 + n))
        for shift in range(4):
            got = sm.debug_values_text(text, BYTES, 8, abs_pos=np.arange(0, n + 2), address_shift=shift)
            assert [int(v) for v in got] == _little_endian(text + bytes(4), range(0, n + 2), 8), (n, shift)


def test_cxx_values_text_example_compiles(sm):
    """tests/cxx/values_text_example.cpp builds against the header-only mirror and the in-tree library."""
    cxx = os.path.join(ROOT, "tests", "cxx")
    subprocess.run(["make", "-C", cxx, "-f", "values_text_example.mk"], check=True, capture_output=True)
    assert os.path.exists(os.path.join(cxx, "values_text_example"))
