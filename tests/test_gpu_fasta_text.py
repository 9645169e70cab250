"""FASTA text -> records of byte text on the device (mm_fasta_text_device, fasta2_text_kernel in mm_fasta2.hip): the loader
step in front of mm_run_text_batch_* / mm_values_*_text_batch_*.  The checker is the oracle's restatement of the reader
(oracle.fasta_records): seq = the sequences back to back, starts = the running sum of their lengths, the text positions
and both counts.  Every call gets buffers pre-filled with 0xA5: a kernel that relied on a cleared output, or wrote a
byte at or beyond the characters it found (or the capacity), fails."""
import ctypes as C

import numpy as np
import pytest

import text_checker as tc

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL64 = int.from_bytes(bytes([FILL]) * 8, "little")
# protein letters plus '*', NUL, TAB and 0xFF: none is a line end or '>', all must pass through as they are
ALPHABET = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYacdxy*\x00\t\xff", dtype=np.uint8)


def _seq(rng, n):
    return ALPHABET[rng.integers(0, len(ALPHABET), n)].tobytes()


def _device_text(text):
    import torch
    if isinstance(text, (bytes, bytearray)):
        a = np.frombuffer(bytes(text), dtype=np.uint8).copy()
        return torch.from_numpy(a).cuda() if a.size else torch.zeros(0, dtype=torch.uint8, device="cuda")
    return text


def call(sm, gpu, text, cap=None, max_records=1 << 12, asynchronous=False, seq_shift=0):
    """One call on 0xA5-filled buffers.  Returns (code, counts, seq buffer, starts table, text_pos table) as numpy arrays
    of the WHOLE buffers, slack included."""
    import torch
    t = _device_text(text)
    n = int(t.numel())
    cap = n if cap is None else cap
    seq = torch.full(((cap + 3) // 4 * 4 + 64,), FILL, dtype=torch.uint8, device="cuda")
    starts = torch.full((8 * (max_records + 1 + 4),), FILL, dtype=torch.uint8, device="cuda")
    pos = torch.full((8 * (max_records + 4),), FILL, dtype=torch.uint8, device="cuda")
    counts = torch.full((16,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    args = (gpu.h, C.c_void_p(t.data_ptr()) if n else None, n, C.c_void_p(seq.data_ptr() + seq_shift), cap,
            C.c_void_p(starts.data_ptr()), C.c_void_p(pos.data_ptr()), max_records, C.c_void_p(counts.data_ptr()))
    out = (C.c_uint64 * 2)()
    if asynchronous:
        code = sm.lib().mm_fasta_text_device_async(*args)
        gpu.sync()
        got = counts.cpu().numpy().view(np.uint64)
        out[0], out[1] = int(got[0]), int(got[1])
    else:
        code = sm.lib().mm_fasta_text_device(*args, out)
    torch.cuda.synchronize()
    return (code, (int(out[0]), int(out[1])), seq.cpu().numpy(), starts.cpu().numpy().view(np.uint64),
            pos.cpu().numpy().view(np.uint64))


def expect(oracle, text):
    recs = oracle.fasta_records(bytes(text))
    seq = np.frombuffer(b"".join(s for _, _, s in recs), dtype=np.uint8)
    base = np.cumsum([0] + [len(s) for _, _, s in recs]).astype(np.uint64)
    return recs, seq, base, np.array([p for p, _, _ in recs], dtype=np.uint64)


def check(sm, oracle, gpu, text, dev=None, **kw):
    recs, want, base, where = expect(oracle, text)
    code, counts, seq, starts, pos = call(sm, gpu, text if dev is None else dev, **kw)
    assert code == 0, code
    assert counts == (len(want), len(recs)), (counts, len(want), len(recs))
    assert np.array_equal(seq[: len(want)], want)
    assert (seq[len(want):] == FILL).all(), "a byte at or beyond the characters was written"
    n = len(recs)
    assert np.array_equal(starts[: n + 1], base)
    assert (starts[n + 1:] == FILL64).all()
    assert np.array_equal(pos[:n], where)
    assert (pos[n:] == FILL64).all()
    return recs, want, base


def test_known_cases(sm, oracle, gpu):
    rng = np.random.default_rng(1)
    s = lambda n: _seq(rng, n)  # noqa: E731
    for text in [
        b">sp|P1 test\n" + s(4) + b"\n" + s(2) + b"\n",
        b">a\r\n" + s(4) + b"\r\n" + s(2) + b"\r\n>b\r\n" + s(2),             # CRLF, no newline at the end
        b"junk before\n>p1\n" + s(8) + b"\n\n\n" + s(4) + b"\n>c2\n>c3\nGG>T\nA",  # blank lines, empty records, '>' inside a line
        b"",
        b"\n",
        s(4) + b"\n" + s(4) + b"\n",                                          # no header at all: nothing
        b">only a header",
        b">h\n",
        b">\n>\n>\nA",
        b">x\n" + s(20_000),                                                  # one long line
        b">" + b"h" * 100_000 + b"\n" + s(4) + b"\n",                         # a header longer than six chunks
        b">x\n" + b"\n".join(s(1 + i % 8) for i in range(9000)) + b"\n>y\n" + s(7) + b"\n",  # 1-8-byte lines
        b">abcdefghijklmnopqrst\n" * 3000 + s(4) + b"\n",                     # 3 000 records, 744 in a chunk
        b">r\n" + b"".join(s(30) + b"\r\n" for _ in range(4000)),             # CRLF, 30-byte lines
    ]:
        check(sm, oracle, gpu, text)


def random_text(rng, n):
    """n bytes of every value, with '\\n', '\\r' and '>' only where the rates put them; ends wherever byte n falls,
    mostly inside a line."""
    a = rng.integers(0, 256, n, dtype=np.uint8)
    a[(a == 10) | (a == 13) | (a == 62)] = 0x80
    p_nl = float(rng.choice([1 / 3, 1 / 20, 1 / 61, 1 / 1000]))
    nl = rng.random(n) < p_nl
    a[rng.random(n) < p_nl / 8] = 13          # '\r' anywhere: in front of a '\n', inside lines and inside headers
    a[rng.random(n) < 1 / 200] = 62           # '>' inside lines
    a[nl] = 10
    after = np.flatnonzero(nl) + 1
    after = after[after < n]
    a[after[rng.random(len(after)) < float(rng.choice([0.02, 0.3]))]] = 62   # header lines
    if n and rng.random() < 0.5:
        a[0] = 62
    return a.tobytes()


def test_random_texts(sm, oracle, gpu):
    rng = np.random.default_rng(2025)
    sizes = [1, 15, 16, 17, 4095, 4096, 4097, 16383, 16384, 16385, 32767, 32768, 32769, 65536 + 3, 200_000, 1_000_000]
    for i in range(64):
        check(sm, oracle, gpu, random_text(rng, sizes[i % len(sizes)]), max_records=1 << 17)


def test_seam_phase_of_every_chunk_boundary(sm, oracle, gpu):
    """A header of 1..8 bytes in front of one 50 KB sequence of 60-byte lines: the output index at the chunk boundaries
    takes every value mod 4, so the chunks' partial first / last dwords meet at every byte phase."""
    rng = np.random.default_rng(3)
    body = b"".join(_seq(rng, 60) + b"\n" for _ in range(820))
    phases = set()
    for h in range(1, 9):
        text = b">" + b"h" * (h - 1) + b"\n" + body
        check(sm, oracle, gpu, text)
        a = np.frombuffer(text, dtype=np.uint8)
        kept = np.cumsum((a != 10) & (np.arange(len(a)) > h))
        phases |= {int(kept[c - 1]) % 4 for c in (16384, 32768, 49152)}
    assert phases == {0, 1, 2, 3}


def test_seam_chunks_that_give_one_byte_or_none(sm, oracle, gpu):
    """Twelve records with a header of about 16 380 bytes and one sequence byte: consecutive chunks give 0 or 1 byte each,
    several of them into the same output dword."""
    rng = np.random.default_rng(4)
    for drift in (0, 3, 9):
        text = b"".join(b">" + b"h" * (16_376 + (i * drift) % 11) + b"\n" + _seq(rng, 1) + b"\n" for i in range(12))
        recs, want, _ = check(sm, oracle, gpu, text)
        assert len(recs) == 12 and len(want) == 12


@pytest.mark.parametrize("j", [1, 2, 3, 4, 5])
def test_seam_chunk_that_gives_exactly_j_bytes(sm, oracle, gpu, j):
    """The second chunk holds the end of one long header, j sequence bytes and the start of the next long header; the
    chunk in front ends at every byte phase."""
    rng = np.random.default_rng(50 + j)
    for pre in (100, 101, 102, 103):
        text = (b">a\n" + _seq(rng, pre) + b"\n>" + b"h" * 20_000 + b"\n" + _seq(rng, j) + b"\n>" + b"g" * 20_000 + b"\n"
                + _seq(rng, 50) + b"\n")
        a = np.frombuffer(text, dtype=np.uint8)
        first = 3 + pre + 1 + 20_002
        assert 16384 < first and first + j + 1 < 32768 < first + j + 1 + 20_000  # (the j bytes are all chunk 1 gives)
        assert a[first - 1] == 10
        check(sm, oracle, gpu, text)


def test_state_across_groups(sm, oracle, gpu):
    """The header / record state carried over more than a group of 256 chunks (4 MB), and 100 000 short records."""
    rng = np.random.default_rng(31)
    big = 4_500_000
    check(sm, oracle, gpu, b">" + b"h" * big + b"\n" + _seq(rng, 1000) + b"\n>b\n" + _seq(rng, 77) + b"\n")
    check(sm, oracle, gpu, _seq(rng, big) + b"\n>a\n" + _seq(rng, 100) + b"\n")
    check(sm, oracle, gpu, (b">r\n" + _seq(rng, 40) + b"\n") * 100_000, max_records=1 << 17)


def _protein_fasta(rng, n_rec, max_len=2000, lens=None):
    parts = []
    lens = [int(x) for x in rng.integers(0, max_len + 1, n_rec)] if lens is None else lens
    for i, m in enumerate(lens):
        nl = b"\r\n" if i % 5 == 3 else b"\n"
        s = _seq(rng, m)
        parts.append(b">sp|Q%05d|NAME_%d some protein\n" % (i, i) + nl.join(s[q:q + 60] for q in range(0, m, 60)) + (nl if m else b""))
    return b"".join(parts), lens


def test_capacity_and_limits(sm, oracle, gpu):
    rng = np.random.default_rng(6)
    text, _ = _protein_fasta(rng, 40)
    recs, want, base, where = expect(oracle, text)
    chars, n = len(want), len(recs)
    assert chars > 20_003
    E = sm.ERR
    # capacity above the characters: bytes at and beyond `chars` keep the fill (check() asserts it)
    check(sm, oracle, gpu, text, cap=chars + 37)
    check(sm, oracle, gpu, text, cap=chars)
    # capacity below: the true counts, and nothing at or beyond the capacity
    for cap in (20_000, 20_003, chars - 1, 5, 3, 0):
        code, counts, seq, starts, pos = call(sm, gpu, text, cap=cap)
        assert code == E["CAPACITY"], cap
        assert counts == (chars, n)
        assert np.array_equal(seq[:cap], want[:cap]), cap
        assert (seq[cap:] == FILL).all(), cap
        assert np.array_equal(starts[: n + 1], base) and np.array_equal(pos[:n], where)
    # too few table entries: counted, not tabulated
    code, counts, seq, starts, pos = call(sm, gpu, text, max_records=7)
    assert code == E["CAPACITY"] and counts == (chars, n)
    assert np.array_equal(starts[:7], base[:7]) and np.array_equal(pos[:7], where[:7])
    assert (starts[7:] == FILL64).all() and (pos[7:] == FILL64).all()
    assert np.array_equal(seq[:chars], want) and (seq[chars:] == FILL).all()
    # exactly as many entries as records: fits
    check(sm, oracle, gpu, text, max_records=n)
    # FASTQ: refused by the synchronous form, nothing written
    code, counts, seq, starts, pos = call(sm, gpu, b"\n  @read1\nACGT\n+\n>>>>\n")
    assert code == E["FORMAT"]
    assert (seq == FILL).all() and (starts == FILL64).all() and (pos == FILL64).all()
    # a sequence buffer that is not 4-byte aligned
    code, _, seq, starts, _ = call(sm, gpu, text, seq_shift=1)
    assert code == E["NULL"] and (seq == FILL).all() and (starts == FILL64).all()
    with pytest.raises(sm.MinimizerError):
        sm.fasta_text_device(b">a\nA\n>b\nC\n>c\nG\n", max_records=2)
    with pytest.raises(sm.MinimizerError):
        sm.fasta_text_device(b"@r\nACGT\n+\nIIII\n")


def test_unaligned_text_pointer(sm, oracle, gpu):
    import torch
    rng = np.random.default_rng(7)
    text = random_text(rng, 100_000)
    buf = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    for off in (1, 3, 8, 15):
        buf[off: off + len(text)] = src
        check(sm, oracle, gpu, text, dev=buf[off: off + len(text)], max_records=1 << 15)


def test_agrees_with_the_packed_loader(sm, oracle, gpu):
    """On an ASCII-DNA FASTA both loaders read the same records: same starts, same text positions, and the 2-bit packing
    of the byte records is the packed loader's buffer."""
    import torch
    rng = np.random.default_rng(8)
    parts = []
    for i in range(200):
        m = int(rng.integers(0, 3000))
        s = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)[rng.integers(0, 9, m)].tobytes()
        parts.append(b">contig%d\n" % i + b"\n".join(s[q:q + 70] for q in range(0, m, 70)) + b"\n")
    text = b"".join(parts)
    packed = sm.fasta_pack_device(text)
    got = sm.fasta_text_device(text)
    assert len(got) == len(packed) == 200
    assert np.array_equal(got.starts.cpu().numpy().view(np.uint64), packed.base)
    assert np.array_equal(got.text_pos, packed.text_pos)
    assert got.n_chars == int(packed.base[-1]) and got.seq.numel() == got.n_chars
    m = got.n_chars
    exp = torch.zeros((m + 3) // 4 + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sm._check(sm.lib().mm_pack_ascii_device_async(gpu.h, C.c_void_p(got.seq.data_ptr()), m, C.c_void_p(exp.data_ptr())))
    gpu.sync()
    assert torch.equal(exp[: (m + 3) // 4], packed.packed[: (m + 3) // 4])
    assert got.header(text, 17) == b"contig17" and got.lengths() == packed.lengths()


def test_64_mb_against_torch(sm, gpu):
    """64 MB (4 096 chunks, 16 groups), built on the device: seq == t[keep], the starts follow from the running sum of
    keep."""
    import torch
    n, width, n_rec = 64 << 20, 60, 24
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    t = torch.from_numpy(ALPHABET.copy()).cuda()[torch.randint(0, len(ALPHABET), (n,), device="cuda", generator=g)]
    i = torch.arange(n, device="cuda")
    t[i % (width + 1) == width] = 10
    del i
    keep = t != 10
    where = []
    for r in range(n_rec):
        p = (n // n_rec) * r + (r * 7919) % 50
        hdr = b">record %d\n" % r
        if p:
            t[p - 1] = 10
            keep[p - 1] = False
        t[p: p + len(hdr)] = torch.tensor(list(hdr), dtype=torch.uint8, device="cuda")
        keep[p: p + len(hdr)] = False
        where.append(p)
    keep &= t != 10
    want = t[keep]
    m = int(want.numel())
    before = torch.cumsum(keep.to(torch.int64), 0)
    base = [int(before[p].item()) for p in where] + [m]
    del before
    seq = torch.full((n + 64,), FILL, dtype=torch.uint8, device="cuda")
    starts = torch.full((64,), -1, dtype=torch.int64, device="cuda")
    pos = torch.full((64,), -1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = (C.c_uint64 * 2)()
    torch.cuda.synchronize()
    sm._check(sm.lib().mm_fasta_text_device(gpu.h, C.c_void_p(t.data_ptr()), n, C.c_void_p(seq.data_ptr()), n,
                                            C.c_void_p(starts.data_ptr()), C.c_void_p(pos.data_ptr()), 63,
                                            C.c_void_p(counts.data_ptr()), out))
    assert (int(out[0]), int(out[1])) == (m, n_rec)
    assert torch.equal(seq[:m], want)
    assert bool((seq[m:] == FILL).all())
    assert starts[: n_rec + 1].tolist() == base and pos[:n_rec].tolist() == where
    assert bool((starts[n_rec + 1:] == -1).all())


def test_file_to_minimizers_and_values(sm, oracle, gpu):
    """A protein FASTA in device memory -> records -> forward minimizers k=7 w=11 -> their k-mer values, with no parsing on
    the host: per record against text_checker on the oracle reader's sequence, values against the bytes themselves."""
    import torch
    rng = np.random.default_rng(9)
    k, w = 7, 11
    l = k + w - 1
    lens = [0, 1, l - 1, l, l + 1, 2000, 0, 0, 60, 61, 120] + [int(x) for x in rng.integers(0, 2001, 289)]
    text, lens = _protein_fasta(rng, len(lens), lens=lens)
    recs = oracle.fasta_records(text)
    assert [len(s) for _, _, s in recs] == lens and len(lens) == 300
    th = sm.TextMulHasher(canonical=False)
    b = sm.minimizers(k, w).hasher(th)
    got = sm.fasta_text_device(text)
    assert len(got) == 300 and got.lengths() == lens
    out = torch.full((max(got.n_chars, 1),), -1, dtype=torch.int32, device="cuda")
    offs = torch.full((301,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cnt = sm.run_fasta_text_device(b, got, out, offs)
    assert gpu.last_path() == sm.PATH_FUSED
    vals = sm.values_text_batch_device(b, got.seq, got.starts, got.n_chars, out, offs, cnt, sm.TEXT_VALUES_BYTES)
    b._ws().sync()
    b._ws().check()
    pos, o, vals = out[:cnt].cpu().numpy().view(np.uint32), offs.cpu().numpy(), vals.cpu().numpy().view(np.uint64)
    assert o[0] == 0 and o[-1] == cnt
    for r, (_, hdr, s) in enumerate(recs):
        want = tc.run(s, k, w, th)
        mine = pos[o[r]:o[r + 1]]
        assert np.array_equal(mine, want), r
        a = np.frombuffer(s, dtype=np.uint8).astype(np.uint64)
        exp = np.zeros(len(mine), dtype=np.uint64)
        for j in range(k):
            exp |= a[mine.astype(np.int64) + j] << np.uint64(8 * j)
        assert np.array_equal(vals[o[r]:o[r + 1]], exp), r
        assert got.header(text, r) == hdr


def test_asynchronous_entry(sm, oracle, gpu):
    import torch
    rng = np.random.default_rng(10)
    text, _ = _protein_fasta(rng, 60)
    dev_before = torch.cuda.current_device()
    sync = call(sm, gpu, text)
    asyn = call(sm, gpu, text, asynchronous=True)
    assert asyn[0] == 0 and sync[0] == 0
    assert asyn[1] == sync[1]
    for a, b in zip(asyn[2:], sync[2:]):
        assert np.array_equal(a, b)
    assert sm.lib().mm_workspace_check(gpu.h) == 0
    assert torch.cuda.current_device() == dev_before
    check(sm, oracle, gpu, text, asynchronous=True)
    # an empty text: counts 0, starts[0] = 0, nothing else
    for asynchronous in (False, True):
        code, counts, seq, starts, pos = call(sm, gpu, b"", asynchronous=asynchronous)
        assert code == 0 and counts == (0, 0) and starts[0] == 0
        assert (seq == FILL).all() and (starts[1:] == FILL64).all() and (pos == FILL64).all()
