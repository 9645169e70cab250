"""BGZF without a device: the scanner (mm_bgzf_scan_host), the decoder on the host (mm_debug_bgzf_inflate - the code the
kernel runs, csrc/mm_inflate.h) against Python's zlib on valid, malformed and mutated payloads, the refusals of the new
entry points, and the decoder alone under AddressSanitizer + UBSan (tests/cxx/bgzf_inflate_check.cpp, a stand-alone host
program: exactly-sized heap allocations make any access outside a payload or an output slot a report)."""
import ctypes as C
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_cases as bc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def valid():
    return bc.valid_blocks()


def _err(sm, name):
    return sm.ERR[name]


def _fails(sm, fn, name, text=None):
    with pytest.raises(sm.MinimizerError) as e:
        fn()
    assert e.value.code == _err(sm, name), e.value
    if text:
        assert text in sm.lib().mm_last_error().decode()


def test_helper_makes_gzip_python_reads(valid):
    data = b"".join(bc.member(p, raw) for _, raw, p in valid) + bc.EOF_BLOCK
    assert gzip.decompress(data) == b"".join(raw for _, raw, _ in valid)
    kinds = set()
    for _, _, p in valid:
        if p:
            kinds.add((p[0] >> 1) & 3)
    assert kinds == {0, 1, 2}  # stored, fixed and dynamic first blocks are all there


def test_scan_lists_every_block(sm, valid):
    data = b"".join(bc.member(p, raw) for _, raw, p in valid) + bc.EOF_BLOCK
    r = sm.bgzf_scan(data)
    listed = [(raw, p) for _, raw, p in valid if raw]
    assert r["consumed"] == len(data) and r["out_bytes"] == sum(len(raw) for raw, _ in listed)
    assert len(r["blocks"]) == len(listed)
    out_off = 0
    for b, (raw, p) in zip(r["blocks"], listed):
        assert (int(b["comp_len"]), int(b["isize"]), int(b["out_off"])) == (len(p), len(raw), out_off)
        assert data[int(b["comp_off"]):int(b["comp_off"]) + len(p)] == p
        out_off += len(raw)


def test_scan_stops_where_it_must(sm):
    raws = [bc.fastq_bytes(n, n) for n in (700, 900, 1100, 1300)]
    blocks = [bc.block(r) for r in raws]
    # an EOF marker between blocks (concatenated files) and a second extra subfield in front of BC
    two = bc.member(bc.deflate(raws[1]), raws[1], extra_first=b"XY" + (3).to_bytes(2, "little") + b"abc")
    data = blocks[0] + bc.EOF_BLOCK + two + blocks[2] + blocks[3]
    r = sm.bgzf_scan(data)
    assert [int(x) for x in r["blocks"]["isize"]] == [700, 900, 1100, 1300] and r["consumed"] == len(data)
    assert int(r["blocks"]["comp_off"][1]) == len(blocks[0]) + len(bc.EOF_BLOCK) + 12 + 7 + 6
    # a truncated last block, cut in its header and in its payload
    for cut in (5, 17, 40, len(blocks[3]) - 1):
        r = sm.bgzf_scan(data[:len(data) - len(blocks[3]) + cut])
        assert len(r["blocks"]) == 3 and r["consumed"] == len(data) - len(blocks[3])
    r = sm.bgzf_scan(data, max_blocks=2)
    assert len(r["blocks"]) == 2 and r["consumed"] == len(blocks[0]) + len(bc.EOF_BLOCK) + len(two) and r["out_bytes"] == 1600
    r = sm.bgzf_scan(data, max_out_bytes=2699)
    assert len(r["blocks"]) == 2 and r["out_bytes"] == 1600
    r = sm.bgzf_scan(data, max_out_bytes=2700)
    assert len(r["blocks"]) == 3 and r["out_bytes"] == 2700
    r = sm.bgzf_scan(b"")
    assert len(r["blocks"]) == 0 and r["consumed"] == 0


def test_scan_refuses_plain_gzip_and_bad_headers(sm):
    raw = bc.fastq_bytes(500, 1)
    _fails(sm, lambda: sm.bgzf_scan(gzip.compress(raw)), "FORMAT", "plain gzip is one serial stream; recompress with bgzip")
    # an extra field without a BC subfield is plain gzip too
    good = bc.block(raw)
    no_bc = bytearray(good)
    no_bc[12:14] = b"XX"
    _fails(sm, lambda: sm.bgzf_scan(bytes(no_bc)), "FORMAT", "plain gzip")
    for at, value in ((0, 0x1e), (1, 0x8c), (2, 7)):
        bad = bytearray(good)
        bad[at] = value
        _fails(sm, lambda: sm.bgzf_scan(bytes(bad)), "FORMAT", "no BGZF block header")
    _fails(sm, lambda: sm.bgzf_scan(good + b"@read\n"), "FORMAT", "no BGZF block header at byte %d" % len(good))
    big = bytearray(good)
    big[-4:] = (65537).to_bytes(4, "little")
    _fails(sm, lambda: sm.bgzf_scan(bytes(big)), "FORMAT", "ISIZE")


def test_host_decoder_inflates_every_valid_block(sm, valid):
    assert len(valid) >= 55
    for name, raw, payload in valid:
        assert zlib.decompressobj(-15).decompress(payload) == raw, name
        assert sm.debug_bgzf_inflate(payload, len(raw)) == raw, name
        # bytes behind the final block are ignored
        assert sm.debug_bgzf_inflate(payload + b"\xff\x00\xff", len(raw)) == raw, name


def test_host_decoder_refuses_every_malformed_payload(sm):
    cases = bc.malformed()
    assert len(cases) >= 30 and {name for name, _, _ in cases} == set(bc.MALFORMED_CODES)
    assert set(bc.MALFORMED_CODES.values()) == set(range(1, 15))  # every error of the decoder's list
    for name, payload, isize in cases:
        # (the error the case is built for, not any error: mm_last_error() carries the decoder's code)
        _fails(sm, lambda: sm.debug_bgzf_inflate(payload, isize), "FORMAT", "BGZF block: inflate error %d" % bc.MALFORMED_CODES[name])
        assert sm.lib().mm_last_error().decode().endswith("inflate error %d" % bc.MALFORMED_CODES[name]), name


def test_host_decoder_agrees_with_zlib_on_mutated_payloads(sm):
    cases = bc.mutations()
    assert len(cases) == 20 * 200
    L = sm.lib()
    inflated = 0
    for payload, isize, want in cases:
        buf = np.frombuffer(payload, np.uint8)
        out = np.zeros(isize, np.uint8)
        code = L.mm_debug_bgzf_inflate(buf.ctypes.data, buf.size, out.ctypes.data, isize)
        if want is not None:
            assert code == 0 and out.tobytes() == want
            inflated += 1
        else:
            assert code == sm.ERR["FORMAT"]
    assert 0 < inflated < len(cases)


def test_refusals(sm):
    L = sm.lib()
    n, used, out = C.c_uint64(), C.c_uint64(), C.c_uint64()
    table = (sm.BgzfBlock * 4)()
    data = np.frombuffer(bc.block(b"ACGT"), np.uint8)
    null, fmt = sm.ERR["NULL"], sm.ERR["FORMAT"]
    assert L.mm_bgzf_scan_host(data.ctypes.data, data.size, 4, 100, table, None, C.byref(used), C.byref(out)) == null
    assert L.mm_bgzf_scan_host(data.ctypes.data, data.size, 4, 100, table, C.byref(n), None, C.byref(out)) == null
    assert L.mm_bgzf_scan_host(data.ctypes.data, data.size, 4, 100, table, C.byref(n), C.byref(used), None) == null
    assert L.mm_bgzf_scan_host(None, data.size, 4, 100, table, C.byref(n), C.byref(used), C.byref(out)) == null
    assert L.mm_bgzf_scan_host(data.ctypes.data, data.size, 4, 100, None, C.byref(n), C.byref(used), C.byref(out)) == null
    assert L.mm_bgzf_scan_host(data.ctypes.data, data.size, 0, 100, None, C.byref(n), C.byref(used), C.byref(out)) == 0
    assert (n.value, used.value) == (0, 0)
    assert L.mm_bgzf_scan_host(data.ctypes.data, data.size, 4, 100, table, C.byref(n), C.byref(used), C.byref(out)) == 0
    assert (n.value, used.value, out.value, table[0].isize) == (1, data.size, 4, 4)
    buf = np.zeros(8, np.uint8)
    assert L.mm_debug_bgzf_inflate(None, 3, buf.ctypes.data, 4) == null
    assert L.mm_debug_bgzf_inflate(data.ctypes.data, 3, None, 4) == null
    assert L.mm_debug_bgzf_inflate(data.ctypes.data, 3, buf.ctypes.data, 65537) == fmt
    assert L.mm_debug_bgzf_inflate(None, 0, None, 0) == fmt  # (no input: exhausted)
    # a NULL workspace comes first, whatever else is given
    assert L.mm_bgzf_inflate_device_async(None, None, 0, None, 1, None, 0, None) == null
    assert L.mm_bgzf_inflate_host(None, data.ctypes.data, data.size, buf.ctypes.data, 8, C.byref(out)) == null
    # a NULL stream
    assert L.mm_fastx_stream_feed_bgzf(None, data.ctypes.data, data.size, C.byref(used)) == null
    if L.mm_device_count() == 0:
        with pytest.raises(sm.MinimizerError) as e:
            sm.bgzf_inflate_host(data.tobytes())
        assert e.value.code == sm.ERR["NO_DEVICE"]
        with pytest.raises(sm.MinimizerError) as e:
            list(sm.stream_fastx(sm.canonical_minimizers(21, 11), [data.tobytes()], chunk_bytes=4096, max_records=64))
        assert e.value.code == sm.ERR["NO_DEVICE"]


def test_is_bgzf(sm):
    assert sm.is_bgzf(bc.block(b"ACGT")) and sm.is_bgzf(bc.EOF_BLOCK)
    assert not sm.is_bgzf(gzip.compress(b"ACGT")) and not sm.is_bgzf(b"@r\nA\n+\nI\n") and not sm.is_bgzf(b"\x1f\x8b")


def test_decoder_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bgzf_inflate_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "cxx", "bgzf_inflate_check.cpp")], check=True)
    cases = bc.all_check_cases()
    assert len(cases) > 4000
    path = str(tmp_path / "cases.bin")
    bc.write_check_file(path, cases)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "bgzf_inflate_check OK" in r.stdout
