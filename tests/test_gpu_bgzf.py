"""BGZF on the device: the inflate kernel (one launch over the whole valid set, malformed blocks among valid neighbours)
against the raw bytes the blocks were made from, and the stream fed with BGZF (FastxStream.feed_bgzf, stream_fastx /
stream_fasta_text with bgzf=None) against the same stream fed with the inflated text, per record keyed by rec_text_pos.
Expected bytes come from the original text or from Python's zlib (tests/bgzf_cases.py), never from the code under test."""
import os
import subprocess

import numpy as np
import pytest

import bgzf_cases as bc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PATTERN = 0x5a


@pytest.fixture(scope="module")
def valid():
    return bc.valid_blocks()


def _table(sm, entries):
    t = np.zeros(len(entries), sm.BGZF_BLOCK_DTYPE)
    for i, e in enumerate(entries):
        t[i] = e
    return t


def _launch(sm, ws, payloads, isizes, front=1000, behind=3000):
    """One launch: the payloads back to back (three bytes of padding between them, so that offsets take every alignment), the
    slots back to back behind `front` bytes of a pattern-filled buffer.  Returns (out bytes, status, check's exception)."""
    import torch

    comp, entries, at, out_off = bytearray(), [], 0, front
    for p, n in zip(payloads, isizes):
        comp += p + b"\xee\xee\xee"
        entries.append((at, len(p), n, out_off))
        at += len(p) + 3
        out_off += n
    d_comp = torch.from_numpy(np.frombuffer(bytes(comp), np.uint8).copy()).cuda()
    d_out = torch.full((out_off + behind,), PATTERN, dtype=torch.uint8, device="cuda")
    d_status = torch.full((len(entries),), 77, dtype=torch.int32, device="cuda")
    assert sm.bgzf_inflate_device(d_comp, _table(sm, entries), d_out, d_status, ws=ws) == len(entries)
    err = None
    try:
        ws.check()
    except sm.MinimizerError as e:
        err = e
    return d_out.cpu().numpy().tobytes(), d_status.cpu().numpy(), err, [e[3] for e in entries]


def test_inflate_device_whole_valid_set_in_one_launch(sm, gpu, valid):
    out, status, err, offs = _launch(sm, gpu, [p for _, _, p in valid], [len(raw) for _, raw, _ in valid])
    assert err is None
    assert not status.any()
    for (name, raw, _), off in zip(valid, offs):
        assert out[off:off + len(raw)] == raw, name
    end = offs[-1] + len(valid[-1][1])
    assert out[:1000] == bytes([PATTERN]) * 1000 and out[end:] == bytes([PATTERN]) * 3000


def test_inflate_host_whole_file(sm, gpu, valid):
    data = b"".join(bc.member(p, raw) for _, raw, p in valid) + bc.EOF_BLOCK
    assert sm.bgzf_inflate_host(data, ws=gpu) == b"".join(raw for _, raw, _ in valid)
    with pytest.raises(sm.MinimizerError) as e:
        sm.bgzf_inflate_host(data[:-40], ws=gpu)
    assert e.value.code == sm.ERR["FORMAT"] and "truncated" in str(e.value)


def test_malformed_blocks_among_valid_neighbours(sm, gpu, valid):
    # (every one of these went through the sanitized host program of tests/test_bgzf_cpu.py: one per error family)
    bad = {name: (p, isize) for name, p, isize in bc.malformed()}
    chosen = ["input_exhausted", "output_passes_isize_match", "ends_short", "distance_too_far", "litlen_code_286",
              "oversubscribed_litlen", "stored_len_nlen"]
    good = [(raw, p) for _, raw, p in valid if 0 < len(raw) <= 12000][:8]
    payloads, isizes, is_bad = [], [], []
    for i, (raw, p) in enumerate(good):
        payloads.append(p), isizes.append(len(raw)), is_bad.append(False)
        if i < len(chosen):
            payloads.append(bad[chosen[i]][0]), isizes.append(bad[chosen[i]][1]), is_bad.append(True)
    out, status, err, offs = _launch(sm, gpu, payloads, isizes)
    assert err is not None and err.code == sm.ERR["FORMAT"]
    assert "BGZF block" in sm.lib().mm_last_error().decode()
    assert [bool(s) for s in status] == is_bad
    it = iter(good)
    for off, n, b in zip(offs, isizes, is_bad):
        if not b:
            assert out[off:off + n] == next(it)[0]
    end = offs[-1] + isizes[-1]
    assert out[:1000] == bytes([PATTERN]) * 1000 and out[end:] == bytes([PATTERN]) * 3000
    # a table entry beyond the buffers is refused on the device, the blocks around it are inflated
    import torch

    raw, p = good[0]
    d_comp = torch.from_numpy(np.frombuffer(p, np.uint8).copy()).cuda()
    d_out = torch.full((len(raw) + 10,), PATTERN, dtype=torch.uint8, device="cuda")
    d_status = torch.zeros(3, dtype=torch.int32, device="cuda")
    sm.bgzf_inflate_device(d_comp, _table(sm, [(0, len(p), len(raw), 11), (1, len(p), len(raw), 0), (0, len(p), len(raw), 0)]),
                           d_out, d_status, ws=gpu)
    with pytest.raises(sm.MinimizerError) as e:
        gpu.check()
    assert e.value.code == sm.ERR["CAPACITY"]
    assert list(d_status.cpu().numpy()) == [100, 100, 0]
    assert d_out.cpu().numpy().tobytes() == raw + bytes([PATTERN]) * 10
    # a launch with both kinds of failure reports the table's (the larger kernel error stays)
    d_out.fill_(PATTERN)
    sm.bgzf_inflate_device(d_comp, _table(sm, [(0, len(p) // 2, len(raw), 0), (1, len(p), len(raw), 0)]), d_out, d_status[:2], ws=gpu)
    with pytest.raises(sm.MinimizerError) as e:
        gpu.check()
    assert e.value.code == sm.ERR["CAPACITY"]
    got = list(d_status.cpu().numpy())
    assert 0 < got[0] < 100 and got[1] == 100
    assert d_out.cpu().numpy().tobytes()[len(raw):] == bytes([PATTERN]) * 10
    # the workspace runs a valid launch afterwards
    out, status, err, offs = _launch(sm, gpu, [p for _, p in good], [len(raw) for raw, _ in good])
    assert err is None and not status.any()
    for (raw, _), off in zip(good, offs):
        assert out[off:off + len(raw)] == raw


# ---- the stream
def _records(batches, joined=False):
    """{rec_text_pos: (bases, positions, values, one_min)} over all batches"""
    out = {}
    for b in batches:
        per = 2 if b.u128 else 1
        for r in range(b.n_records):
            o0, o1 = int(b.offsets[r]), int(b.offsets[r + 1])
            key = int(b.rec_text_pos[r])
            assert key not in out
            out[key] = (int(b.rec_base[r + 1]) - int(b.rec_base[r]), b.pos[o0:o1].tolist(),
                        None if b.values is None else b.values[o0 * per:o1 * per].tolist(),
                        None if b.one_min is None else int(b.one_min[r]),
                        None if b.seq is None else b.seq[int(b.rec_base[r]):int(b.rec_base[r + 1])].tobytes())
    return out


def _feed_bgzf(st, data, pieces=(1000, 37, 4099, 1, 13001)):
    """feed_bgzf in calls of odd sizes (they end inside headers and payloads); what a call leaves is fed again"""
    batches, held, at, turn = [], b"", 0, 0

    def push(buf):
        # (a call that takes nothing, twice in a row with a next() that wanted input in between: an incomplete block)
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
    return batches


def _block_sizes(seed, lo, hi, n=400):
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(lo, hi + 1, n)]


@pytest.fixture(scope="module")
def fastq_text():
    return bc.fastq(1000, 150, 21)


@pytest.mark.parametrize("options", [dict(values="u64"), dict(skip_ambiguous=True, one_minimizer=True)], ids=["u64", "skip_amb_one_min"])
def test_stream_fastq(sm, gpu, fastq_text, options):
    text = bc.fastq(1000, 150, 22, with_n=True) if options.get("skip_ambiguous") else fastq_text
    data = bc.bgzf(text, _block_sizes(1, 3000, 5000))
    b = sm.canonical_minimizers(21, 11)
    want = _records(sm.stream_fastx(b, [text], chunk_bytes=16384, max_records=200, slots=3, bgzf=False, **options))
    assert len(want) == 1000
    with sm.FastxStream(b, 16384, 200, slots=3, **options) as st:
        batches = _feed_bgzf(st, data)
    assert len(batches) > 10
    assert batches[0].text_begin == 0 and batches[-1].text_end == len(text)
    assert all(x.text_end == y.text_begin for x, y in zip(batches, batches[1:]))
    assert _records(batches) == want
    # the generator finds the format of the source by its first bytes
    assert _records(sm.stream_fastx(b, [data[i:i + 7001] for i in range(0, len(data), 7001)], chunk_bytes=16384, max_records=200,
                                    **options)) == want


def test_stream_leading_blank_lines(sm, gpu, fastq_text):
    text = b"\n \r\n" + fastq_text[:60000]
    b = sm.canonical_minimizers(21, 11)
    want = _records(sm.stream_fastx(b, [text], chunk_bytes=16384, max_records=200, bgzf=False))
    assert min(want) == 4
    # (blank bytes alone in the first block, then a block that ends the blank run, then text)
    data = bc.block(text[:2]) + bc.block(text[2:9]) + bc.bgzf(text[9:], _block_sizes(2, 3000, 5000))
    with sm.FastxStream(b, 16384, 200) as st:
        got = _records(_feed_bgzf(st, data))
    assert got == want


def test_stream_fasta_long_records(sm, gpu):
    rng = np.random.default_rng(3)

    def rec(name, n):
        s = rng.choice(list(b"ACGT"), size=n).astype(np.uint8).tobytes()
        return b">" + name + b"\n" + b"\n".join(s[i:i + 70] for i in range(0, n, 70)) + b"\n"

    text = rec(b"s1 short", 300) + rec(b"chr_long", 100_000) + rec(b"s2", 1000) + rec(b"s3", 77)
    b = sm.canonical_minimizers(21, 11)
    opt = dict(chunk_bytes=8192, max_records=64, long_records=True, values="u64")
    want = [(p, n, pos.tolist(), v.tolist()) for p, n, pos, _, v in sm.fastx_join(sm.stream_fastx(b, [text], bgzf=False, **opt))]
    assert len(want) == 4 and want[1][1] == 100_000
    data = bc.bgzf(text, _block_sizes(4, 1500, 4000))
    got = [(p, n, pos.tolist(), v.tolist()) for p, n, pos, _, v in sm.fastx_join(sm.stream_fastx(b, [data], read_bytes=1 << 20, **opt))]
    assert got == want


def test_stream_byte_text(sm, gpu):
    rng = np.random.default_rng(5)
    amino = list(b"ACDEFGHIKLMNPQRSTVWY")
    recs = []
    for i in range(300):
        s = rng.choice(amino, size=int(rng.integers(20, 600))).astype(np.uint8).tobytes()
        recs.append(b">prot%d some description\n" % i + b"\n".join(s[j:j + 60] for j in range(0, len(s), 60)) + b"\n")
    text = b"".join(recs)
    assert 80_000 < len(text) < 130_000
    b = sm.minimizers(7, 11).hasher(sm.TextMulHasher(canonical=False))
    opt = dict(chunk_bytes=16384, max_records=200, values="u64", one_minimizer=True, seq=True)
    want = _records(sm.stream_fasta_text(b, [text], bgzf=False, **opt))
    assert len(want) == 300
    data = bc.bgzf(text, _block_sizes(6, 3000, 5000))
    got = _records(sm.stream_fasta_text(b, [data[i:i + 5003] for i in range(0, len(data), 5003)], **opt))
    assert got == want


def test_stream_errors(sm, gpu, fastq_text):
    b = sm.canonical_minimizers(21, 11)
    data = bc.bgzf(fastq_text[:40000], [4000], eof=False)
    # a truncated file: finish names it, and the stream stays failed
    with sm.FastxStream(b, 16384, 200) as st:
        took = st.feed_bgzf(data[:-100])
        assert 0 < took < len(data) - 100
        assert st.feed_bgzf(data[took:-100]) == 0
        for call in (st.finish, st.finish, st.next, lambda: st.feed_bgzf(data[took:])):
            with pytest.raises(sm.MinimizerError) as e:
                call()
            assert e.value.code == sm.ERR["FORMAT"] and "truncated" in str(e.value)
    # a block with more text than a chunk
    with sm.FastxStream(b, 4096, 200) as st:
        with pytest.raises(sm.MinimizerError) as e:
            st.feed_bgzf(bc.block(fastq_text[:4097]))
        assert e.value.code == sm.ERR["CAPACITY"] and "chunk_bytes" in str(e.value)
    # plain gzip, by name
    import gzip

    with sm.FastxStream(b, 16384, 200) as st:
        with pytest.raises(sm.MinimizerError) as e:
            st.feed_bgzf(gzip.compress(fastq_text[:5000]))
        assert e.value.code == sm.ERR["FORMAT"] and "recompress with bgzip" in str(e.value)
    # text behind BGZF blocks is refused
    with sm.FastxStream(b, 16384, 200) as st:
        st.feed_bgzf(data[:took])
        with pytest.raises(sm.MinimizerError) as e:
            st.feed(b"@r\nACGT\n+\nIIII\n")
        assert e.value.code == sm.ERR["BAD_MODE"]
    # a block that does not inflate (its deflate stream ends short of ISIZE), on the device path: MM_ERR_FORMAT, and it stays
    raw = fastq_text[40000:43000]
    bad = bc.member(bc.deflate(raw[:-7]), raw)
    with sm.FastxStream(b, 16384, 200) as st:
        with pytest.raises(sm.MinimizerError) as e:
            _feed_bgzf(st, data + bad + bc.bgzf(fastq_text[43000:90000], [4000]))
        assert e.value.code == sm.ERR["FORMAT"] and "BGZF block" in str(e.value)
        with pytest.raises(sm.MinimizerError) as e:
            st.next()
        assert e.value.code == sm.ERR["FORMAT"]


def test_cxx_bgzf_stream_example_runs(gpu, tmp_path):
    exe = str(tmp_path / "bgzf_stream_example")
    libdir = os.path.join(ROOT, "simd-minimizers_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(HERE, "cxx", "bgzf_stream_example.cpp"), "-L" + libdir, "-lsimd_minimizers_amd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "bgzf_stream_example: OK" in r.stdout
