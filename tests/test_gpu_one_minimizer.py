"""One minimizer per record on the GPU (mm_one_minimizer_*): every output against the oracle
(tests/one_minimizer_cases.py), a guard word behind d_out_pos in every case."""
import ctypes as C

import numpy as np
import pytest

import hasher_cases
import one_minimizer_cases as oc
import stream_queue
import text_checker

pytestmark = pytest.mark.gpu
GUARD = 4


def _reads(sm, gpu, hasher, k, packed, n, starts=None, stride=0, length=0, base_offset=0, shift=0):
    """The device call with a guarded output; ``shift``: d_packed starts that many bytes past its allocation."""
    import torch
    raw = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8), packed])).cuda()
    d_starts = torch.from_numpy(np.ascontiguousarray(starts).view(np.int64)).cuda() if starts is not None else None
    out = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sm.one_minimizer_reads_device(hasher, k, raw[shift:], n, out, read_starts=d_starts, read_stride=stride, read_len=length,
                                  base_offset=base_offset, ws=gpu)
    gpu.sync()
    got = out.cpu().numpy()
    assert (got[n:] == -7).all(), "the guard behind d_out_pos was written"
    return got[:n].view(np.uint32)


def _text(sm, gpu, hasher, k, text, starts):
    import torch
    n = len(starts) - 1
    d_text = torch.from_numpy(text).cuda()
    d_starts = torch.from_numpy(np.ascontiguousarray(starts).view(np.int64)).cuda()
    out = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sm.one_minimizer_text_batch_device(hasher, k, d_text, d_starts, n, out, ws=gpu)
    gpu.sync()
    got = out.cpu().numpy()
    assert (got[n:] == -7).all(), "the guard behind d_out_pos was written"
    return got[:n].view(np.uint32)


def _hashers(sm, oracle, k):
    """(product, oracle) pairs: NtHasher forward and canonical, MulHasher, AntiLexHasher."""
    return [(sm.NtHasher(k, False), oracle.default_hasher(False)), (sm.NtHasher(k, True), oracle.default_hasher(True)),
            (sm.MulHasher(k, True), oracle.mul_hasher(True)), (sm.AntiLexHasher(k, False), oracle.antilex_hasher(k, False))]


@pytest.mark.parametrize("canonical", [False, True])
def test_one_record_over_four_tiles(sm, oracle, gpu, canonical):
    T, k = sm.one_minimizer_tile(), 21
    lens = [3 * T + T // 3 + k]
    packed, starts, _ = oc.packed_records(lens, 11, 1, 7)
    want = oc.expect_packed(oracle, packed, starts, k, oracle.default_hasher(canonical), 1)
    got = _reads(sm, gpu, sm.NtHasher(k, canonical), k, packed, 1, starts, base_offset=1)
    assert np.array_equal(got, want), (got, want)


@pytest.mark.parametrize("k", oc.KS)
def test_record_shapes(sm, oracle, gpu, k):
    """Records that end on a tile edge, k-mers that straddle one, runs of empty and too-short records; base offsets 0-3,
    starts[0] > 0, a hasher family per base offset."""
    T = sm.one_minimizer_tile()
    lens = oc.shape_lengths(T, k)
    for bo, (hp, ho) in enumerate(_hashers(sm, oracle, k)):
        packed, starts, _ = oc.packed_records(lens, 100 * k + bo, bo, 5 + bo)
        want = oc.expect_packed(oracle, packed, starts, k, ho, bo)
        assert (want[[5, 7, 8, 9]] == oc.NO_MINIMIZER).all() and (want[10] == oc.NO_MINIMIZER) == (k > 1)
        got = _reads(sm, gpu, hp, k, packed, len(lens), starts, base_offset=bo, shift=bo % 2)
        bad = np.nonzero(got != want)[0]
        assert not len(bad), (k, bo, bad[:8], got[bad[:8]], want[bad[:8]])


def test_second_route_single_window(sm, oracle, gpu):
    """Expected values by the independent route: a minimizer run with the one window w = len - k + 1."""
    lens = [150, 40, 31, 500, 700, 129, 3, 0, 33]
    for bo in range(4):
        packed, starts, _ = oc.packed_records(lens, 3 + bo, bo, 2)
        for k in (21, 5, 31, 32, 33, 1):
            for canonical in (False, True):
                ho = oracle.default_hasher(canonical)
                want = oc.expect_windows(oracle, packed, starts, k, ho, bo)
                assert np.array_equal(want, oc.expect_packed(oracle, packed, starts, k, ho, bo))
                got = _reads(sm, gpu, sm.NtHasher(k, canonical), k, packed, len(lens), starts, base_offset=bo)
                assert np.array_equal(got, want), (bo, k, canonical)


def test_hasher_rotation(sm, oracle, gpu):
    """Every table family and rot of tests/hasher_cases.py, const and low16 included: where every key ties the answer is 0."""
    T, k = sm.one_minimizer_tile(), 21
    draw, tally = hasher_cases.Draw(seed=5), hasher_cases.Tally()
    lens = oc.shape_lengths(T, k, 60)
    for i in range(24):
        case = draw(None)
        packed, starts, _ = oc.packed_records(lens, 40 + i, i % 4, i)
        want = oc.expect_packed(oracle, packed, starts, k, case.oracle(oracle), i % 4)
        if case.family == "const":
            assert (want[np.asarray(lens) >= k] == 0).all()
        got = _reads(sm, gpu, case.product(sm), k, packed, len(lens), starts, base_offset=i % 4)
        assert np.array_equal(got, want), case
        tally.add(case, int(starts[-1]), len(lens))
    tally.check("one_minimizer_reads")


def test_as_many_records_as_a_tile_holds(sm, oracle, gpu):
    T = sm.one_minimizer_tile()
    lens = [1] * (4 * T)
    packed, starts, codes = oc.packed_records(lens, 9, 3, 1)
    got = _reads(sm, gpu, sm.NtHasher(1, False), 1, packed, len(lens), starts, base_offset=3)
    assert np.array_equal(got, oc.expect_packed(oracle, packed, starts, 1, oracle.default_hasher(False), 3))
    assert (got == 0).all()
    got = _reads(sm, gpu, sm.NtHasher(2, False), 2, packed, len(lens), starts, base_offset=3)
    assert (got == oc.NO_MINIMIZER).all()


@pytest.mark.parametrize("canonical", [False, True])
def test_leftmost_across_tiles(sm, oracle, gpu, canonical):
    """One record of a random unit of 1 500 bases repeated over at least three tiles: every key repeats with period 1 500,
    so a tile that reports its own minimum without the position tie-break gives an answer at or above 1 500."""
    T, k, unit = sm.one_minimizer_tile(), 21, 1500
    reps = -(-3 * T // unit) + 1
    codes = np.tile(np.random.default_rng(17).integers(0, 4, size=unit, dtype=np.uint8), reps)
    packed = text_checker.pack_codes(codes)
    starts = np.array([0, len(codes)], dtype=np.uint64)
    ho = oracle.default_hasher(canonical)
    h = oracle.hash_kmers(packed, len(codes), k, ho)[: len(codes) - k + 1] & np.uint32(0xFFFF0000)
    assert int((h == h.min()).sum()) >= reps - 1  # (the minimum is tied once per repeat)
    want = oc.expect_packed(oracle, packed, starts, k, ho)
    assert want[0] < unit
    got = _reads(sm, gpu, sm.NtHasher(k, canonical), k, packed, 1, starts)
    assert np.array_equal(got, want), (got, want)


@pytest.mark.parametrize("length,stride", [(100, 128), (150, 150)])
def test_fixed_stride_layout(sm, oracle, gpu, length, stride):
    n = 1000
    codes = np.random.default_rng(length).integers(0, 4, size=2 + (n - 1) * stride + length, dtype=np.uint8)
    packed = text_checker.pack_codes(codes)[: (len(codes) + 3) // 4]  # (the last read ends with the buffer)
    starts = np.arange(n + 1, dtype=np.uint64) * np.uint64(stride)
    for k, canonical in ((21, False), (31, True), (length, False), (length + 1, False)):
        want = oc.expect_packed(oracle, np.concatenate([packed, np.zeros(16, np.uint8)]), starts, k,
                                oracle.default_hasher(canonical), 2, lens=[length] * n)
        got = _reads(sm, gpu, sm.NtHasher(k, canonical), k, packed, n, None, stride, length, base_offset=2)
        assert np.array_equal(got, want), (k, canonical)


@pytest.mark.parametrize("k", oc.TEXT_KS)
def test_text_record_shapes(sm, gpu, k):
    """All 256 byte values, the record shapes of the packed test, TextMulHasher forward and canonical and a custom table."""
    T = sm.one_minimizer_tile()
    lens = oc.shape_lengths(T, k, 200)
    text, starts = oc.text_records(lens, 50 + k, 3)
    assert len(np.unique(text)) == 256
    custom = hasher_cases.Case("random", 17, True, size=256, xor=True)
    for hp, hc in ((sm.TextMulHasher(k, False),) * 2, (sm.TextMulHasher(k, True),) * 2, (custom.product(sm), custom)):
        want = oc.expect_text(text, starts, k, hc)
        got = _text(sm, gpu, hp, k, text, starts)
        bad = np.nonzero(got != want)[0]
        assert not len(bad), (k, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("canonical", [False, True])
def test_text_equals_packed_on_dna(sm, oracle, gpu, canonical):
    """text_tables_from_dna over the code bytes 0..3: bit for bit the packed call on the same DNA."""
    T, k = sm.one_minimizer_tile(), 21
    lens = oc.shape_lengths(T, k, 100)
    packed, starts, codes = oc.packed_records(lens, 23, 0, 6)
    nt = sm.NtHasher(k, canonical)
    fw, rc = text_checker.text_tables_from_dna(nt)
    th = sm.TextHasher.from_tables(fw, rc, nt.rot, canonical)
    a = _reads(sm, gpu, nt, k, packed, len(lens), starts)
    b = _text(sm, gpu, th, k, codes[: int(starts[-1]) + 2].copy(), starts)
    assert np.array_equal(a, b)
    assert np.array_equal(a, oc.expect_packed(oracle, packed, starts, k, oracle.default_hasher(canonical)))


def test_k_larger_than_a_tile(sm, oracle, gpu):
    """k above a tile's size: the tile's symbols no longer fit its LDS copy and are read from global memory."""
    T = sm.one_minimizer_tile()
    k = 2 * T
    lens = [3 * T + 5, k - 1, k, 0, k + T + 1, 150]
    packed, starts, _ = oc.packed_records(lens, 61, 3, 2)
    want = oc.expect_packed(oracle, packed, starts, k, oracle.default_hasher(True), 3)
    got = _reads(sm, gpu, sm.NtHasher(k, True), k, packed, len(lens), starts, base_offset=3, shift=1)
    assert np.array_equal(got, want), (got, want)
    k = T + T // 4
    lens = [2 * T + 5, k - 1, k, 0, k + T + 1, 150]
    text, tstarts = oc.text_records(lens, 62, 1)
    th = sm.TextMulHasher(k, True)
    assert np.array_equal(_text(sm, gpu, th, k, text, tstarts), oc.expect_text(text, tstarts, k, th))


def _fasta(n_records, seed):
    rng = np.random.default_rng(seed)
    out, seqs = [], []
    for i in range(n_records):
        ln = int(rng.integers(0, 400)) if i % 7 else (0 if i % 2 else 20)
        s = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=ln))
        seqs.append(s)
        out.append(b">r%d\n" % i + b"".join(s[j:j + 60] + b"\n" for j in range(0, ln, 60)))
    return b"".join(out), seqs


def test_loader_to_positions(sm, oracle, gpu):
    """A FASTA in device memory -> records -> one position per record in two calls, packed and byte text."""
    k = 21
    fasta, seqs = _fasta(24, 4)
    ho = oracle.default_hasher(True)
    want = np.full(len(seqs), oc.NO_MINIMIZER, dtype=np.uint32)
    for r, s in enumerate(seqs):
        if len(s) >= k:
            h = oracle.hash_kmers(oracle.pack_ascii(s), len(s), k, ho)[: len(s) - k + 1]
            want[r] = int(np.argmin(h & np.uint32(0xFFFF0000)))
    rec = sm.fasta_pack_device(fasta, max_records=64)
    assert len(rec) == len(seqs)
    got = sm.one_minimizer_reads_device(sm.NtHasher(k, True), k, rec, ws=gpu)
    gpu.sync()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
    trec = sm.fasta_text_device(fasta, max_records=64)
    got = sm.one_minimizer_text_batch_device(sm.TextHasher.from_dna(sm.NtHasher(k, True)), k, trec, ws=gpu)
    gpu.sync()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)


def test_compose_with_values(sm, oracle, gpu):
    """Positions into values_reads_device with offsets 0..n: the k-mer value of every read's minimizer."""
    import torch
    k, n = 21, 300
    lens = [int(x) for x in np.random.default_rng(8).integers(k, 400, size=n)]
    packed, starts, _ = oc.packed_records(lens, 31, 0, 0)
    b = sm.minimizers(k, 11)
    d_packed = torch.from_numpy(packed).cuda()
    d_starts = torch.from_numpy(starts.view(np.int64)).cuda()
    pos = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ws = b._ws()
    sm.one_minimizer_reads_device(sm.NtHasher(k, False), k, d_packed, n, pos, read_starts=d_starts, ws=ws)
    offsets = torch.arange(n + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    vals = sm.values_reads_device(b, d_packed, n, pos, offsets, read_starts=d_starts, n_pos_max=n)
    ws.sync()
    got_pos = pos.cpu().numpy()
    assert (got_pos[n:] == -7).all()
    want_pos = oc.expect_packed(oracle, packed, starts, k, oracle.default_hasher(False))
    assert np.array_equal(got_pos[:n].view(np.uint32), want_pos)
    want = oracle.values_u64(packed, k, (starts[:-1] + want_pos).astype(np.uint32), bool(b.canonical))[:n]
    assert np.array_equal(vals.cpu().numpy().view(np.uint64)[:n], want)


def test_host_forms_equal_device_forms(sm, oracle, gpu):
    T, k = sm.one_minimizer_tile(), 21
    lens = oc.shape_lengths(T, k, 50)
    packed, starts, codes = oc.packed_records(lens, 77, 0, 0)
    reads = [sm.PackedSeq(packed, int(starts[r]), lens[r]) for r in range(len(lens))]
    hp = sm.NtHasher(k, True)
    dev = _reads(sm, gpu, hp, k, packed, len(lens), starts)
    assert np.array_equal(sm.one_minimizer_reads_host(reads, hp, k), dev)
    assert np.array_equal(dev, oc.expect_packed(oracle, packed, starts, k, oracle.default_hasher(True)))
    assert sm.one_minimizer(reads[3], hp, k) == int(dev[3])
    with pytest.raises(ValueError):
        sm.one_minimizer(reads[5], hp, k)  # (k - 1 bases: the reference panics)
    text, tstarts = oc.text_records(lens, 78)
    th = sm.TextMulHasher(k, True)
    tdev = _text(sm, gpu, th, k, text, tstarts)
    records = [text[int(tstarts[r]):int(tstarts[r + 1])] for r in range(len(lens))]
    assert np.array_equal(sm.one_minimizer_text_batch_host(records, th, k), tdev)
    assert np.array_equal(tdev, oc.expect_text(text, tstarts, k, th))
    assert sm.one_minimizer(bytes(records[1]), th, k) == int(tdev[1])
    ascii_read = bytes(np.frombuffer(b"ACTG", dtype=np.uint8)[codes[: lens[0]]])
    assert sm.one_minimizer(sm.AsciiSeq(ascii_read), hp, k) == int(_reads(sm, gpu, hp, k, packed, 1, starts[:2])[0])


def test_no_records_and_return_codes(sm, gpu):
    import torch
    L, E = sm.lib(), sm.ERR
    hp, th = sm.NtHasher(21, False), sm.TextMulHasher(21, False)
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    out = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    vp = stream_queue.vp
    reads = lambda ws, h, k, pk, nb, bo, n, s, stride, ln, o: L.mm_one_minimizer_reads_device_async(
        ws, C.byref(h) if h is not None else None, k, pk, nb, bo, n, s, stride, ln, o)
    assert reads(gpu.h, hp, 21, vp(d), 64, 0, 0, None, 0, 0, None) == 0
    assert reads(None, hp, 0, vp(d), 64, 0, 1, vp(st), 0, 0, vp(out)) == E["NULL"]
    assert reads(gpu.h, None, 0, vp(d), 64, 0, 1, vp(st), 0, 0, vp(out)) == E["NULL"]
    assert reads(gpu.h, hp, 0, vp(d), 64, 0, 1, vp(st), 0, 0, None) == E["NULL"]
    assert reads(gpu.h, hp, 0, vp(d), 64, 257, 1, vp(st), 0, 0, vp(out)) == E["K_ZERO"]  # (before the layout)
    assert reads(gpu.h, hp, 21, vp(d), 64, 257, 1, vp(st), 0, 0, vp(out)) == E["CAPACITY"]
    assert reads(gpu.h, hp, 21, vp(d), 64, 0, 3, None, 100, 57, vp(out)) == E["CAPACITY"]  # (the last read ends at 257)
    assert reads(gpu.h, hp, 21, vp(d), 64, 0, 3, None, 100, 56, vp(out)) == 0
    assert L.mm_one_minimizer_text_batch_device_async(gpu.h, C.byref(th), 21, vp(d), 64, 0, None, None) == 0
    assert L.mm_one_minimizer_text_batch_device_async(gpu.h, C.byref(th), 0, vp(d), 64, 1, vp(st), vp(out)) == E["K_ZERO"]
    gpu.sync()
    assert (out.cpu().numpy()[3:] == -7).all()
    assert len(sm.one_minimizer_reads_host([], hp, 21)) == 0 and len(sm.one_minimizer_text_batch_host([], th, 21)) == 0


def test_queued_on_a_callers_stream(sm, oracle):
    """The call queued on a caller's non-blocking stream behind the copies that fill its inputs, one wait at the end."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    T, k = sm.one_minimizer_tile(), 21
    lens = oc.shape_lengths(T, k, 100)
    packed, starts, _ = oc.packed_records(lens, 91, 2, 9)
    text, tstarts = oc.text_records(lens, 92, 1)
    hp, th = sm.NtHasher(k, True), sm.TextMulHasher(k, False)
    want = oc.expect_packed(oracle, packed, starts, k, oracle.default_hasher(True), 2)
    twant = oc.expect_text(text, tstarts, k, th)
    q = stream_queue.Queue(sm)
    try:
        i_packed, i_starts = q.input(packed, shift=1), q.input(starts, index=True)
        i_text, i_tstarts = q.input(text), q.input(tstarts, index=True)
        o_reads, o_text = q.output(len(lens)), q.output(len(lens))
        for name, inp in (("packed", i_packed), ("starts", i_starts), ("text", i_text), ("tstarts", i_tstarts)):
            q.upload(name, inp)
        q.add("reads", lambda: sm.one_minimizer_reads_device(hp, k, i_packed.d, len(lens), o_reads.d, read_starts=i_starts.d,
                                                             base_offset=2, ws=q.ws),
              after=("packed", "starts"), verify=lambda: stream_queue.check_exact("reads", o_reads, want, "positions"))
        q.add("text", lambda: sm.one_minimizer_text_batch_device(th, k, i_text.d, i_tstarts.d, len(lens), o_text.d, ws=q.ws),
              after=("text", "tstarts"), verify=lambda: stream_queue.check_exact("text", o_text, twant, "positions"))
        for seed in (None, 3):
            q.run(q.order(seed), delay=True, no_wait=True)
            q.finish(label=f"order {seed}: ")
    finally:
        q.close()
