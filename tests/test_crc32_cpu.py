"""The BGZF CRC32 check without a device: the host function of csrc/mm_crc32.h (mm_debug_crc32 - the arithmetic the verify
kernel runs) against zlib.crc32, the scan that also hands out the trailers' CRC32s (mm_bgzf_scan_crc_host) against
mm_bgzf_scan_host and zlib, the refusals of the new entry points that need no device, the new stream flag beside the flags
that stay unknown, and the header alone under AddressSanitizer + UBSan (tests/cxx/crc32_check.cpp, a stand-alone host
program: bit-wise, byte-wise, sliced and segment-combined forms against each other and against zlib's values)."""
import ctypes as C
import gzip
import os
import random
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_cases as bc

HERE = os.path.dirname(os.path.abspath(__file__))

LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65280, 65535, 65536)


def _messages(lengths):
    rng = random.Random(20261021)
    out = []
    for n in lengths:
        out += [bytes(n), b"\xff" * n, rng.randbytes(n)]
    return out


def _fails(sm, fn, name, text=None):
    with pytest.raises(sm.MinimizerError) as e:
        fn()
    assert e.value.code == sm.ERR[name], e.value
    if text:
        assert text in sm.lib().mm_last_error().decode()


def test_entry_points_exported_and_wrapped(sm):
    L = sm.lib()
    for name in ("mm_debug_crc32", "mm_bgzf_scan_crc_host", "mm_bgzf_crc32_device_async", "mm_bgzf_inflate_verify_host"):
        assert hasattr(L, name), name
        assert name in sm.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    for name in ("crc32", "bgzf_crc32_device"):
        assert callable(getattr(sm, name)), name
    assert sm.FASTX_BGZF_CRC == 1024  # (512 is pinned as an unknown bit of the DNA stream by tests/test_fastx_one_minimizer_cpu.py)


def test_host_crc32_equals_zlib(sm):
    msgs = _messages(LENGTHS)
    assert len(msgs) == 3 * len(LENGTHS)
    for m in msgs:
        assert sm.crc32(m) == zlib.crc32(m), (len(m), m[:4])
    # all-zero data of different lengths must differ: a combine that loses the length gives them one value
    zeros = [sm.crc32(bytes(n)) for n in LENGTHS]
    assert len(set(zeros)) == len(LENGTHS)
    assert sm.crc32(np.frombuffer(b"123456789", np.uint8)) == 0xCBF43926
    L = sm.lib()
    out = C.c_uint32(7)
    buf = np.zeros(4, np.uint8)
    assert L.mm_debug_crc32(None, 4, C.byref(out)) == sm.ERR["NULL"]
    assert L.mm_debug_crc32(buf.ctypes.data, 4, None) == sm.ERR["NULL"]
    assert L.mm_debug_crc32(None, 0, C.byref(out)) == 0 and out.value == 0


def _scan_both(sm, data, **kw):
    plain, with_crc = sm.bgzf_scan(data, **kw), sm.bgzf_scan(data, crc=True, **kw)
    assert "crc" not in plain and with_crc["crc"].dtype == np.uint32
    assert np.array_equal(plain["blocks"], with_crc["blocks"])
    assert (plain["consumed"], plain["out_bytes"]) == (with_crc["consumed"], with_crc["out_bytes"])
    assert len(with_crc["crc"]) == len(with_crc["blocks"])
    return with_crc


def test_scan_crc_lists_every_trailer(sm):
    valid = bc.valid_blocks()
    listed = [raw for _, raw, _ in valid if raw]
    data = b"".join(bc.member(p, raw) for _, raw, p in valid) + bc.EOF_BLOCK
    r = _scan_both(sm, data)
    assert r["consumed"] == len(data) and len(r["blocks"]) == len(listed)
    assert [int(c) for c in r["crc"]] == [zlib.crc32(raw) for raw in listed]
    # a file made by bgzf(): the same through the helper, and with empty members in the middle (the seams of concatenated files)
    raws = [bc.fastq_bytes(n, n) for n in (700, 900, 1100, 1300)]
    data = bc.bgzf(b"".join(raws), [1000, 333, 2000])
    r = _scan_both(sm, data)
    text = gzip.decompress(data)
    assert text == b"".join(raws)
    assert [int(c) for c in r["crc"]] == [zlib.crc32(text[int(b["out_off"]):int(b["out_off"]) + int(b["isize"])]) for b in r["blocks"]]
    blocks = [bc.block(x) for x in raws]
    data = blocks[0] + bc.EOF_BLOCK + blocks[1] + bc.EOF_BLOCK + bc.EOF_BLOCK + blocks[2] + blocks[3] + bc.EOF_BLOCK
    r = _scan_both(sm, data)
    assert r["consumed"] == len(data)
    assert [int(c) for c in r["crc"]] == [zlib.crc32(x) for x in raws]


def test_scan_crc_stops_where_the_scan_stops(sm):
    """the cases of test_bgzf_cpu.py::test_scan_stops_where_it_must"""
    raws = [bc.fastq_bytes(n, n) for n in (700, 900, 1100, 1300)]
    blocks = [bc.block(r) for r in raws]
    two = bc.member(bc.deflate(raws[1]), raws[1], extra_first=b"XY" + (3).to_bytes(2, "little") + b"abc")
    data = blocks[0] + bc.EOF_BLOCK + two + blocks[2] + blocks[3]
    want = [zlib.crc32(r) for r in raws]
    r = _scan_both(sm, data)
    assert [int(x) for x in r["blocks"]["isize"]] == [700, 900, 1100, 1300] and r["consumed"] == len(data)
    assert int(r["blocks"]["comp_off"][1]) == len(blocks[0]) + len(bc.EOF_BLOCK) + 12 + 7 + 6
    assert [int(c) for c in r["crc"]] == want
    for cut in (5, 17, 40, len(blocks[3]) - 1):
        r = _scan_both(sm, data[:len(data) - len(blocks[3]) + cut])
        assert len(r["blocks"]) == 3 and r["consumed"] == len(data) - len(blocks[3])
        assert [int(c) for c in r["crc"]] == want[:3]
    r = _scan_both(sm, data, max_blocks=2)
    assert len(r["blocks"]) == 2 and r["consumed"] == len(blocks[0]) + len(bc.EOF_BLOCK) + len(two) and r["out_bytes"] == 1600
    assert [int(c) for c in r["crc"]] == want[:2]
    r = _scan_both(sm, data, max_out_bytes=2699)
    assert len(r["blocks"]) == 2 and r["out_bytes"] == 1600
    r = _scan_both(sm, data, max_out_bytes=2700)
    assert len(r["blocks"]) == 3 and r["out_bytes"] == 2700 and [int(c) for c in r["crc"]] == want[:3]
    r = _scan_both(sm, b"")
    assert len(r["blocks"]) == 0 and r["consumed"] == 0


def test_scan_crc_refuses_what_the_scan_refuses(sm):
    """the cases of test_bgzf_cpu.py::test_scan_refuses_plain_gzip_and_bad_headers"""
    scan = lambda d: sm.bgzf_scan(d, crc=True)
    raw = bc.fastq_bytes(500, 1)
    _fails(sm, lambda: scan(gzip.compress(raw)), "FORMAT", "plain gzip is one serial stream; recompress with bgzip")
    good = bc.block(raw)
    no_bc = bytearray(good)
    no_bc[12:14] = b"XX"
    _fails(sm, lambda: scan(bytes(no_bc)), "FORMAT", "plain gzip")
    for at, value in ((0, 0x1e), (1, 0x8c), (2, 7)):
        bad = bytearray(good)
        bad[at] = value
        _fails(sm, lambda: scan(bytes(bad)), "FORMAT", "no BGZF block header")
    _fails(sm, lambda: scan(good + b"@read\n"), "FORMAT", "no BGZF block header at byte %d" % len(good))
    big = bytearray(good)
    big[-4:] = (65537).to_bytes(4, "little")
    _fails(sm, lambda: scan(bytes(big)), "FORMAT", "ISIZE")


def test_refusals_without_a_device(sm):
    L = sm.lib()
    null = sm.ERR["NULL"]
    n, used, out = C.c_uint64(), C.c_uint64(), C.c_uint64()
    table = (sm.BgzfBlock * 4)()
    crcs = (C.c_uint32 * 4)()
    data = np.frombuffer(bc.block(b"ACGT"), np.uint8)
    args = (data.ctypes.data, data.size, 4, 100, table)
    assert L.mm_bgzf_scan_crc_host(*args, None, C.byref(used), C.byref(out), crcs) == null
    assert L.mm_bgzf_scan_crc_host(*args, C.byref(n), None, C.byref(out), crcs) == null
    assert L.mm_bgzf_scan_crc_host(*args, C.byref(n), C.byref(used), None, crcs) == null
    assert L.mm_bgzf_scan_crc_host(None, data.size, 4, 100, table, C.byref(n), C.byref(used), C.byref(out), crcs) == null
    assert L.mm_bgzf_scan_crc_host(data.ctypes.data, data.size, 4, 100, None, C.byref(n), C.byref(used), C.byref(out), crcs) == null
    assert L.mm_bgzf_scan_crc_host(*args, C.byref(n), C.byref(used), C.byref(out), None) == null
    assert (n.value, used.value, out.value) == (0, 0, 0)
    assert L.mm_bgzf_scan_crc_host(data.ctypes.data, data.size, 0, 100, None, C.byref(n), C.byref(used), C.byref(out), None) == 0
    assert (n.value, used.value) == (0, 0)
    assert L.mm_bgzf_scan_crc_host(*args, C.byref(n), C.byref(used), C.byref(out), crcs) == 0
    assert (n.value, used.value, out.value, table[0].isize, crcs[0]) == (1, data.size, 4, 4, zlib.crc32(b"ACGT"))
    # a NULL workspace comes first, whatever else is given
    buf = np.zeros(8, np.uint8)
    words = np.zeros(4, np.uint32)
    assert L.mm_bgzf_crc32_device_async(None, None, 0, None, 1, None, None, None) == null
    assert L.mm_bgzf_crc32_device_async(None, buf.ctypes.data, 8, table, 1, words.ctypes.data, words.ctypes.data, None) == null
    assert L.mm_bgzf_inflate_verify_host(None, data.ctypes.data, data.size, buf.ctypes.data, 8, C.byref(out)) == null
    if L.mm_device_count() == 0:
        with pytest.raises(sm.MinimizerError) as e:
            sm.bgzf_inflate_host(data.tobytes(), verify=True)
        assert e.value.code == sm.ERR["NO_DEVICE"]


def test_stream_creates_take_the_flag_and_no_unknown_one(sm):
    """The flag (1024) is known to both creates; every other unknown bit stays refused - 512 among them, 32 for the DNA
    create and 128 for the text create as the existing tests pin them - before any device is touched (device -1)."""
    L, E = sm.lib(), sm.ERR
    CRC = sm.FASTX_BGZF_CRC
    dna, text = C.c_void_p(), C.c_void_p()
    assert L.mm_plan_create(C.byref(dna), 21, 11, 0, 0, None) == 0
    th = sm.TextMulHasher(canonical=False)
    assert L.mm_plan_create_text(C.byref(text), 7, 11, 0, 0, C.byref(th)) == 0

    def create_dna(flags):
        c = sm.FastxStreamConfig(-1, 0, flags, 0, 1 << 16, 100, 0, 0)
        h = C.c_void_p()
        r = L.mm_fastx_stream_create(C.byref(h), dna, C.byref(c))
        assert r != 0 and not h.value
        return r

    def create_text(flags):
        c = sm.FastxTextStreamConfig(-1, 0, flags, 0, 1 << 16, 100, 0, 0, sm.TEXT_VALUES_BYTES)
        h = C.c_void_p()
        r = L.mm_fastx_text_stream_create(C.byref(h), text, C.byref(c))
        assert r != 0 and not h.value
        return r

    try:
        # the flag alone passes every refusal: only the device (there is no device -1) is left to object
        assert create_dna(CRC) == E["NO_DEVICE"] and create_text(CRC) == E["NO_DEVICE"]
        assert create_dna(CRC | sm.FASTX_VALUES_U64 | sm.FASTX_ONE_MINIMIZER) == E["NO_DEVICE"]
        assert create_text(CRC | sm.FASTX_TEXT_ONE_MINIMIZER | sm.FASTX_TEXT_SEQ) == E["NO_DEVICE"]
        assert create_dna(512 | 1024) == E["BAD_MODE"] and create_text(512 | 1024) == E["BAD_MODE"]
        assert create_dna(512 | 32) == E["BAD_MODE"] and create_text(512 | 128) == E["BAD_MODE"]
        assert create_dna(512) == E["BAD_MODE"] and create_text(512) == E["BAD_MODE"]
        assert create_dna(CRC | 2048) == E["BAD_MODE"] and create_text(CRC | 2048) == E["BAD_MODE"]
        assert create_dna(CRC | 32) == E["BAD_MODE"] and create_text(CRC | 128) == E["BAD_MODE"]
        assert create_dna(32) == E["BAD_MODE"] and create_text(128) == E["BAD_MODE"]
        for bit in (9, *range(11, 32)):
            assert create_dna(CRC | 1 << bit) == E["BAD_MODE"] and create_text(CRC | 1 << bit) == E["BAD_MODE"], bit
        assert create_dna(CRC | 64) == E["BAD_MODE"] and create_dna(CRC | 128) == E["BAD_MODE"]
        assert create_text(CRC | 256) == E["BAD_MODE"]
    finally:
        L.mm_plan_destroy(dna)
        L.mm_plan_destroy(text)


def test_header_under_sanitizers(tmp_path):
    """csrc/mm_crc32.h alone, as a child process: built exactly as test_bgzf_cpu.py::test_decoder_under_sanitizers builds its
    program.  The constants come from zlib, through a file."""
    exe = str(tmp_path / "crc32_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "cxx", "crc32_check.cpp")], check=True)
    msgs = _messages(LENGTHS + (70,)) + [b"123456789", b"@read\nACGT\n+\nIIII\n" * 100]
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(msgs)))
        for m in msgs:
            f.write(struct.pack("<II", len(m), zlib.crc32(m)))
            f.write(m)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "crc32_check OK: %d cases, 3 split in every way" % len(msgs) in r.stdout
    # the program is a check: a wrong constant makes it fail
    with open(path, "r+b") as f:
        f.seek(8)
        f.write(struct.pack("<I", zlib.crc32(msgs[0]) ^ 1))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "zlib" in r.stderr
