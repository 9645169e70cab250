"""The CRC32 of BGZF blocks on the device: the verify kernel (mm_bgzf_crc32_device_async) over hand-laid tables of every
length and alignment and behind the inflate, what only the CRC32 catches (a changed text byte in a stored block, a changed
trailer), malformed blocks and bad table entries beside it, mm_bgzf_inflate_verify_host, and the streams with
MM_FASTX_BGZF_CRC.  Expected values come from Python's zlib and from the text the files were made from, never from the code
under test."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_cases as bc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PATTERN = 0x5a
LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65280, 65535, 65536)


def _table(sm, entries):
    t = np.zeros(len(entries), sm.BGZF_BLOCK_DTYPE)
    for i, e in enumerate(entries):
        t[i] = e
    return t


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _check(sm, ws):
    try:
        ws.check()
    except sm.MinimizerError as e:
        return e, sm.lib().mm_last_error().decode()
    return None, ""


@pytest.fixture(scope="module")
def laid():
    """(text, [(offset, length)]): every length at start offsets whose low four bits run over 0..15 - 72 segments, the
    offsets' low bits running on from segment to segment, so each length meets four of them and each of the sixteen is met
    - in one buffer of random bytes; a third of the segments are zeros, a third 0xFF.  Between two segments lie 1..16 bytes
    that belong to neither; segments 17 and 18 (and the two appended at the end) touch."""
    rng = np.random.default_rng(2026)
    order = [LENGTHS[(i * 7) % len(LENGTHS)] for i in range(4 * len(LENGTHS))]
    assert sorted(order) == sorted(LENGTHS * 4)
    segs, at = [], 3
    for i, n in enumerate(order):
        want = (5 * i + 1) % 16
        if i != 18:  # (segment 18 begins where 17 ends)
            at += 1
            at += (want - at) % 16
        segs.append((at, n))
        at += n
    assert {o % 16 for o, _ in segs} == set(range(16))
    segs += [(at + 9, 17), (at + 26, 255)]
    text = rng.integers(1, 255, at + 26 + 255 + 40, dtype=np.uint8)
    for i, (o, n) in enumerate(segs):
        if i % 3 == 0:
            text[o:o + n] = 0
        elif i % 3 == 1:
            text[o:o + n] = 255
    return text.tobytes(), segs


def test_one_launch_over_a_hand_laid_table(sm, gpu, laid):
    import torch

    text, segs = laid
    assert len(segs) == 74 and segs[18][0] == sum(segs[17]) and segs[-1][0] == sum(segs[-2])
    want = np.array([zlib.crc32(text[o:o + n]) for o, n in segs], np.uint32)
    d_text = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    assert d_text.data_ptr() % 16 == 0  # (so the offsets' low bits are the addresses')
    table = _table(sm, [(0, 0, n, o) for o, n in segs])
    d_crc = sm.bgzf_crc32_device(d_text, table, ws=gpu)
    assert _check(sm, gpu)[0] is None
    got = _u32(d_crc)
    assert [(s, hex(g), hex(w)) for s, g, w in zip(segs, got, want) if g != w] == []
    # the same table with the right values to compare with: clean, and no status word set
    d_status = torch.zeros(len(segs), dtype=torch.int32, device="cuda")
    d_crc = sm.bgzf_crc32_device(d_text, table, expect=want, d_status=d_status, ws=gpu)
    assert _check(sm, gpu)[0] is None
    assert not d_status.cpu().numpy().any() and np.array_equal(_u32(d_crc), want)
    # ... and with one wrong value: that block alone
    wrong = want.copy()
    wrong[40] ^= 0x80
    d_crc = sm.bgzf_crc32_device(d_text, table, expect=wrong, d_status=d_status, ws=gpu)
    err, text_of = _check(sm, gpu)
    assert err is not None and err.code == sm.ERR["FORMAT"] and "CRC32" in text_of
    assert list(np.nonzero(d_status.cpu().numpy())[0]) == [40] and int(d_status[40]) == 15
    assert np.array_equal(_u32(d_crc), want)


def _upload_file(sm, data):
    import torch

    r = sm.bgzf_scan(data, crc=True)
    assert r["consumed"] == len(data)
    d_comp = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    return r, d_comp


def _inflate(sm, ws, data, verify, front=37):
    """The whole file in one inflate launch behind `front` bytes of pattern (so that blocks take odd alignments), with a
    status array; with `verify` the verify launch behind it, with the scan's CRCs.  (text, status, error, error text)"""
    import torch

    r, d_comp = _upload_file(sm, data)
    table = r["blocks"].copy()
    table["out_off"] += front
    d_out = torch.full((front + r["out_bytes"] + 100,), PATTERN, dtype=torch.uint8, device="cuda")
    d_status = torch.full((len(table),), 77, dtype=torch.int32, device="cuda")
    sm.bgzf_inflate_device(d_comp, table, d_out, d_status, ws=ws)
    if verify:
        sm.bgzf_crc32_device(d_out, table, expect=r["crc"], d_status=d_status, ws=ws)
    err, text_of = _check(sm, ws)
    out = d_out.cpu().numpy().tobytes()
    assert out[:front] == bytes([PATTERN]) * front and out[front + r["out_bytes"]:] == bytes([PATTERN]) * 100
    return out[front:front + r["out_bytes"]], d_status.cpu().numpy(), err, text_of


def test_valid_set_inflated_then_verified(sm, gpu):
    valid = bc.valid_blocks()
    data = b"".join(bc.member(p, raw) for _, raw, p in valid) + bc.EOF_BLOCK
    text, status, err, _ = _inflate(sm, gpu, data, True)
    assert err is None and not status.any()
    assert text == b"".join(raw for _, raw, _ in valid)


@pytest.fixture(scope="module")
def corrupt_files():
    """(raws, good file, file with one text byte of the stored block flipped, file with one bit of that block's trailer CRC
    flipped, index of the block): a stored block (deflate level 0) among compressed neighbours"""
    raws = [bc.fastq_bytes(n, 30 + i) for i, n in enumerate((3000, 4100, 2500, 5000, 3700))]
    blocks = [bc.block(r, level=0) if i == 2 else bc.block(r) for i, r in enumerate(raws)]
    good = b"".join(blocks) + bc.EOF_BLOCK
    start = len(blocks[0]) + len(blocks[1])
    payload = start + 18
    assert blocks[2][18] == 1 and blocks[2][payload - start + 5:payload - start + 5 + 2500] == raws[2]  # (BFINAL, stored; LEN, NLEN; text)
    flipped = bytearray(good)
    flipped[payload + 5 + 1234] ^= 0x02
    trailer = bytearray(good)
    trailer[start + len(blocks[2]) - 8 + 1] ^= 0x10
    return raws, good, bytes(flipped), bytes(trailer), 2


def test_what_only_the_crc_catches(sm, gpu, corrupt_files):
    raws, good, flipped, trailer, bad = corrupt_files
    want = b"".join(raws)
    text, status, err, _ = _inflate(sm, gpu, good, True)
    assert err is None and not status.any() and text == want
    off = sum(len(r) for r in raws[:bad])
    for data, text_is_wrong in ((flipped, True), (trailer, False)):
        # the inflate alone: MM_OK (structure and ISIZE are right), and with the flipped byte the wrong text
        text, status, err, _ = _inflate(sm, gpu, data, False)
        assert err is None and not status.any()
        assert (text != want) == text_is_wrong
        if text_is_wrong:
            assert text[off + 1234] == want[off + 1234] ^ 0x02
        # inflate + verify
        text, status, err, text_of = _inflate(sm, gpu, data, True)
        assert err is not None and err.code == sm.ERR["FORMAT"] and "CRC32" in text_of
        assert list(status) == [15 if i == bad else 0 for i in range(len(raws))]
        assert text[:off] == want[:off] and text[off + len(raws[bad]):] == want[off + len(raws[bad]):]
        assert _check(sm, gpu)[0] is None  # (the error was taken: a second check is clean)


def test_malformed_block_keeps_its_inflate_code(sm, gpu):
    import torch

    valid = bc.valid_blocks()
    good = [(raw, p) for _, raw, p in valid if 0 < len(raw) <= 12000][:4]
    name, bad_payload, bad_isize = next(c for c in bc.malformed() if c[0] == "ends_short")
    payloads = [good[0][1], good[1][1], bad_payload, good[2][1], good[3][1]]
    isizes = [len(good[0][0]), len(good[1][0]), bad_isize, len(good[2][0]), len(good[3][0])]
    raws = [good[0][0], good[1][0], None, good[2][0], good[3][0]]
    comp, entries, out_off = bytearray(), [], 5
    for p, n in zip(payloads, isizes):
        entries.append((len(comp), len(p), n, out_off))
        comp += p + b"\xee"
        out_off += n
    table = _table(sm, entries)
    d_comp = torch.from_numpy(np.frombuffer(bytes(comp), np.uint8).copy()).cuda()
    d_out = torch.full((out_off + 64,), PATTERN, dtype=torch.uint8, device="cuda")
    d_status = torch.full((5,), 77, dtype=torch.int32, device="cuda")
    expect = np.array([zlib.crc32(r) if r is not None else 0 for r in raws], np.uint32)
    sm.bgzf_inflate_device(d_comp, table, d_out, d_status, ws=gpu)
    sm.bgzf_crc32_device(d_out, table, expect=expect, d_status=d_status, ws=gpu)
    err, text_of = _check(sm, gpu)
    assert err is not None and err.code == sm.ERR["FORMAT"]
    assert "did not inflate" in text_of and "CRC32" not in text_of
    assert list(d_status.cpu().numpy()) == [0, 0, bc.MALFORMED_CODES[name], 0, 0]
    # without values to compare with the call only writes CRC32s and raises nothing
    d_crc = sm.bgzf_crc32_device(d_out, table, ws=gpu)
    assert _check(sm, gpu)[0] is None
    got = _u32(d_crc)
    assert [int(got[i]) for i in (0, 1, 3, 4)] == [int(expect[i]) for i in (0, 1, 3, 4)]


def test_bad_table_entry_given_to_the_verify_call(sm, gpu):
    import torch

    raw = bc.fastq_bytes(3000, 9)
    d_text = torch.from_numpy(np.frombuffer(raw + bytes(10), np.uint8).copy()).cuda()
    table = _table(sm, [(0, 0, 1000, 0), (0, 0, 3000, 11), (0, 0, 1000, 3011), (0, 0, 65537, 0), (0, 0, 2000, 1000)])
    d_blocks = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    d_crc = torch.full((5,), 0x1234567, dtype=torch.int32, device="cuda")
    d_status = torch.zeros(5, dtype=torch.int32, device="cuda")
    code = sm.lib().mm_bgzf_crc32_device_async(gpu.h, sm._ptr(d_text), d_text.numel(), sm._ptr(d_blocks), 5, None, sm._ptr(d_crc),
                                               sm._ptr(d_status))
    assert code == 0
    err, text_of = _check(sm, gpu)
    assert err is not None and err.code == sm.ERR["CAPACITY"] and "table entry" in text_of
    assert list(d_status.cpu().numpy()) == [0, 100, 100, 100, 0]
    got = _u32(d_crc)
    assert [int(x) for x in got] == [zlib.crc32(raw[:1000]), 0x1234567, 0x1234567, 0x1234567, zlib.crc32(raw[1000:3000])]
    # a queue with a mismatch and a bad table entry reports the mismatch (the larger kernel error stays)
    expect = np.array([zlib.crc32(raw[:1000]) ^ 1, 0, 0, 0, zlib.crc32(raw[1000:3000])], np.uint32)
    d_status.zero_()
    sm.bgzf_crc32_device(d_text, d_blocks, expect=expect, d_status=d_status, ws=gpu)
    err, text_of = _check(sm, gpu)
    assert err is not None and err.code == sm.ERR["FORMAT"] and "CRC32" in text_of
    assert list(d_status.cpu().numpy()) == [15, 100, 100, 100, 0]
    # both outputs NULL is refused on the host
    assert sm.lib().mm_bgzf_crc32_device_async(gpu.h, sm._ptr(d_text), d_text.numel(), sm._ptr(d_blocks), 5, None, None,
                                               sm._ptr(d_status)) == sm.ERR["NULL"]
    assert _check(sm, gpu)[0] is None


def test_inflate_verify_host(sm, gpu, corrupt_files):
    raws, good, flipped, trailer, bad = corrupt_files
    want = b"".join(raws)
    assert sm.bgzf_inflate_host(good, ws=gpu, verify=True) == want
    for data in (flipped, trailer):
        with pytest.raises(sm.MinimizerError) as e:
            sm.bgzf_inflate_host(data, ws=gpu, verify=True)
        assert e.value.code == sm.ERR["FORMAT"] and "CRC32" in str(e.value)
    got = sm.bgzf_inflate_host(flipped, ws=gpu)  # (unchanged: the wrong text, and no error)
    off = sum(len(r) for r in raws[:bad])
    assert got != want and got[:off + 1234] == want[:off + 1234] and got[off + 1235:] == want[off + 1235:]
    assert sm.bgzf_inflate_host(trailer, ws=gpu) == want


# ---- the streams
def _fields(b):
    return {k: (None if getattr(b, k, None) is None else np.asarray(getattr(b, k)).tolist())
            for k in ("rec_text_pos", "rec_base", "offsets", "pos", "sk", "values", "one_min", "seq")} | {
                "n_records": b.n_records, "text_begin": b.text_begin, "text_end": b.text_end}


def _feed_bgzf(st, data, batches, pieces=(1000, 37, 4099, 1, 13001)):
    """feed_bgzf in calls of odd sizes; what a call leaves is fed again.  Batches go to `batches` as they come."""
    held, at, turn = b"", 0, 0

    def push(buf):
        done, stalled = 0, False
        while done < len(buf):
            took = st.feed_bgzf(buf[done:])
            done += took
            stalled = stalled and took == 0
            if done < len(buf):
                b = st.next()
                if b is not None:
                    batches.append(b.copy())
                elif took == 0:
                    if stalled:
                        break
                    stalled = True
        return done

    while at < len(data):
        n = pieces[turn % len(pieces)]
        turn += 1
        buf = held + data[at:at + n]
        at += n
        held = buf[push(buf):]
    if held:
        assert push(held) == 0
    st.finish()
    batches += [b.copy() for b in st]


def _stream_file(text, sizes, stored, line_starts_with):
    """(good file, file with the first byte of a sequence line inside stored block `stored` changed to another letter, the
    offset of that byte in the text): blocks of `sizes`, block `stored` with deflate level 0"""
    blocks, at, i, flip = [], 0, 0, None
    while at < len(text):
        n = sizes[min(i, len(sizes) - 1)]
        raw = text[at:at + n]
        blk = bc.block(raw, level=0) if i == stored else bc.block(raw)
        if i == stored:
            p = raw.index(line_starts_with)
            p = raw.index(b"\n", p + 1) + 1  # (the line behind a header line: sequence)
            assert p < len(raw) - 2 and blk[18 + 5 + p] == raw[p]
            flip = (sum(len(x) for x in blocks) + 18 + 5 + p, at + p, b"C"[0] if raw[p] != b"C"[0] else b"A"[0])
        blocks.append(blk)
        at += n
        i += 1
    assert flip is not None
    good = b"".join(blocks) + bc.EOF_BLOCK
    bad = bytearray(good)
    bad[flip[0]] = flip[2]
    return good, bytes(bad), flip[1]


def _run(make_stream, data):
    batches = []
    with make_stream() as st:
        try:
            _feed_bgzf(st, data, batches)
        except Exception as e:
            # like every stream error it stays
            with pytest.raises(type(e)) as again:
                st.next()
            assert again.value.code == e.code and "CRC32" in str(again.value)
            return batches, e
    return batches, None


def _sizes(seed, lo, hi, n=400):
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(lo, hi + 1, n)]


def test_stream_fastq_with_the_flag(sm, gpu):
    text = bc.fastq(1000, 150, 21)
    assert 300_000 < len(text) < 400_000
    b = sm.canonical_minimizers(21, 11)
    plain = lambda: sm.FastxStream(b, 16384, 200, slots=3, values="u64")
    checked = lambda: sm.FastxStream(b, 16384, 200, slots=3, values="u64", bgzf_crc=True)
    good, bad, flip_at = _stream_file(text, _sizes(1, 3000, 5000), 40, b"\n@read")
    assert flip_at > 5 * 16384
    want, err = _run(plain, good)
    assert err is None and len(want) > 10 and want[-1].text_end == len(text)
    got, err = _run(checked, good)
    assert err is None and [_fields(x) for x in got] == [_fields(x) for x in want]
    # one base of a LATER block changed: the device path
    got, err = _run(checked, bad)
    assert err is not None and err.code == sm.ERR["FORMAT"] and "CRC32" in str(err)
    begin = next(x.text_begin for x in want if x.text_begin <= flip_at < x.text_end)
    assert all(x.text_end <= begin for x in got)  # (no batch made from the bad chunk)
    assert [_fields(x) for x in got] == [_fields(x) for x in want[:len(got)]]
    # without the flag the stream finishes, as it did: the changed base is taken for text
    unchecked, err = _run(plain, bad)
    assert err is None and len(unchecked) == len(want) and unchecked[-1].text_end == len(text)
    # the FIRST block, inflated on the host while the format is unknown: the same failure
    good, bad, flip_at = _stream_file(text, _sizes(1, 3000, 5000), 0, b"@read")
    assert flip_at < 200
    got, err = _run(checked, bad)
    assert err is not None and err.code == sm.ERR["FORMAT"] and "CRC32" in str(err) and got == []
    got, err = _run(checked, good)
    assert err is None and [_fields(x) for x in got] == [_fields(x) for x in want]


def test_stream_byte_text_with_the_flag(sm, gpu):
    rng = np.random.default_rng(5)
    amino = list(b"ACDEFGHIKLMNPQRSTVWY")
    recs = []
    for i in range(300):
        s = rng.choice(amino, size=int(rng.integers(20, 600))).astype(np.uint8).tobytes()
        recs.append(b">prot%d some description\n" % i + b"\n".join(s[j:j + 60] for j in range(0, len(s), 60)) + b"\n")
    text = b"".join(recs)
    assert 80_000 < len(text) < 130_000
    b = sm.minimizers(7, 11).hasher(sm.TextMulHasher(canonical=False))
    opt = dict(values="u64", one_minimizer=True, seq=True, slots=3)
    plain = lambda: sm.FastxTextStream(b, 16384, 200, **opt)
    checked = lambda: sm.FastxTextStream(b, 16384, 200, bgzf_crc=True, **opt)
    good, bad, flip_at = _stream_file(text, _sizes(6, 3000, 5000), 15, b"\n>prot")
    assert flip_at > 3 * 16384
    want, err = _run(plain, good)
    assert err is None and len(want) >= 3 and sum(x.n_records for x in want) == 300
    got, err = _run(checked, good)
    assert err is None and [_fields(x) for x in got] == [_fields(x) for x in want]
    got, err = _run(checked, bad)
    assert err is not None and err.code == sm.ERR["FORMAT"] and "CRC32" in str(err)
    begin = next(x.text_begin for x in want if x.text_begin <= flip_at < x.text_end)
    assert all(x.text_end <= begin for x in got)
    # the generators pass the option on
    got = list(sm.stream_fasta_text(b, [good[i:i + 5003] for i in range(0, len(good), 5003)], chunk_bytes=16384, max_records=200,
                                    bgzf_crc=True, **opt))
    assert sum(x.n_records for x in got) == 300
    with pytest.raises(sm.MinimizerError) as e:
        list(sm.stream_fastx(sm.canonical_minimizers(21, 11), [bc.block(b"@r\nACGT\n+\nIIII\n")[:-8] + bytes(4) + (15).to_bytes(4, "little")],
                             chunk_bytes=16384, max_records=200, bgzf_crc=True))
    assert e.value.code == sm.ERR["FORMAT"] and "CRC32" in str(e.value)


def test_cxx_bgzf_crc_example_runs(gpu, tmp_path):
    exe = str(tmp_path / "bgzf_crc_example")
    libdir = os.path.join(ROOT, "simd-minimizers_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(HERE, "cxx", "bgzf_crc_example.cpp"), "-L" + libdir, "-lsimd_minimizers_amd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "bgzf_crc_example: OK" in r.stdout
