"""One minimizer per read that skips ambiguous bases, on the device (mm_one_minimizer_reads_skip_ambiguous_*): the shapes of
tests/test_one_minimizer_amb_cpu.py at the kernel's own tile against the expectation built from the oracle's hashes
(tests/one_minimizer_amb_cases.py), a guard behind every output."""
import numpy as np
import pytest

import one_minimizer_amb_cases as ac
import one_minimizer_cases as oc
import stream_queue

pytestmark = pytest.mark.gpu
GUARD, EXTRA = 4, 37
JUNK = (1 << 63) - 1


def _dev(a, shift=0):
    """A device copy; ``shift``: the view starts that many bytes into its allocation (a pointer that is not aligned)."""
    import torch
    a = np.ascontiguousarray(a)
    if shift:
        base = torch.zeros(shift + a.size, dtype=torch.uint8, device="cuda")
        base[shift:] = torch.from_numpy(a).cuda()
        return base[shift:]
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _device(sm, gpu, hasher, k, packed, amb, n, starts=None, stride=0, length=0, bo=0, ao=0, shifts=(0, 0)):
    import torch
    out = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda")
    d_packed, d_amb = _dev(packed, shifts[0]), _dev(amb, shifts[1])
    d_starts = _dev(starts) if starts is not None else None
    torch.cuda.synchronize()
    sm.one_minimizer_reads_device(hasher, k, d_packed, n, out, read_starts=d_starts, read_stride=stride, read_len=length,
                                  base_offset=bo, ws=gpu, amb=d_amb, amb_offset=ao)
    gpu.check()
    got = out.cpu().numpy()
    assert (got[n:] == -7).all(), "the guard behind d_out_pos was written"
    return got[:n].view(np.uint32)


def _counts(sm, gpu, hasher, k, packed, amb, starts, counts, bo=0, ao=0, extra=EXTRA, max_bases=None):
    import torch
    n_max = len(starts) - 1 + extra
    out = torch.full((n_max + GUARD,), -7, dtype=torch.int32, device="cuda")
    d_packed, d_amb = _dev(packed), _dev(amb)
    d_starts = _dev(np.concatenate([starts, np.full(extra, JUNK, dtype=np.uint64)]))
    d_counts = _dev(np.asarray(counts, dtype=np.uint64))
    torch.cuda.synchronize()
    sm.one_minimizer_reads_counts_device(hasher, k, d_packed, d_starts, d_counts, n_max, max_bases, out, base_offset=bo, ws=gpu,
                                         amb=d_amb, amb_offset=ao)
    err = None
    try:
        gpu.check()
    except sm.MinimizerError as e:
        err = e
    got = out.cpu().numpy()
    assert (got[n_max:] == -7).all(), "the guard behind d_out_pos was written"
    return got[:n_max].view(np.uint32), err


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", (1, 21, 32, 33, 65))
def test_record_shapes(sm, oracle, gpu, k, canonical):
    T = sm.one_minimizer_tile()
    ho, hp = oracle.default_hasher(canonical), sm.NtHasher(k, canonical)
    for i, (bo, ao) in enumerate(ac.OFFSETS):
        packed, starts, amb, knocked, plain = ac.shape_case(oracle, T, k, ho, 700 * k + 10 * i + int(canonical), bo, ao, tail=60)
        n = len(starts) - 1
        want = ac.expect_packed_amb(oracle, packed, starts, k, ho, amb, bo, ao)
        assert len(knocked) and all(want[r] != plain[r] for r in knocked)
        got = _device(sm, gpu, hp, k, packed, amb, n, starts, bo=bo, ao=ao, shifts=(i % 4, (i + 1) % 4))
        bad = np.nonzero(got != want)[0]
        assert not len(bad), (k, canonical, bo, ao, bad[:8], got[bad[:8]], want[bad[:8]])
        # the counts form: at the record count and below it
        for m in (n, 9):
            got, err = _counts(sm, gpu, hp, k, packed, amb, starts, (int(starts[-1]), m), bo, ao)
            assert err is None
            assert np.array_equal(got[:m], want[:m]) and (got[m:] == oc.NO_MINIMIZER).all(), (k, canonical, bo, ao, m)


def test_one_record_over_four_tiles(sm, oracle, gpu):
    """The plain minimum knocked out by a bit in another tile than the new answer."""
    T, k = sm.one_minimizer_tile(), 21
    for canonical in (False, True):
        ho, hp = oracle.default_hasher(canonical), sm.NtHasher(k, canonical)
        lens = [4 * T - 5]
        packed, starts, codes = oc.packed_records(lens, 17 + int(canonical), 1, 7)
        mask = np.zeros(len(codes) - 1, dtype=bool)
        mask[:7] = True
        mask[int(starts[-1]):] = True
        first = int(oc.expect_packed(oracle, packed, starts, k, ho, 1)[0])
        for _ in range(40):  # knock the current answer out until the answer lies in another tile than the plain one
            mask[7 + (first if not mask[7 + first] else int(want[0]))] = True
            amb = ac.pack_bits(mask, 5)
            want = ac.expect_packed_amb(oracle, packed, starts, k, ho, amb, 1, 5)
            if int(want[0]) // T != first // T:
                break
        assert int(want[0]) // T != first // T, (first, int(want[0]))
        got = _device(sm, gpu, hp, k, packed, amb, 1, starts, bo=1, ao=5)
        assert got[0] == want[0] and got[0] != first


def test_more_records_in_a_tile_than_slots(sm, oracle, gpu):
    k, n, T = 2, 1500, sm.one_minimizer_tile()
    assert 2 * n <= T
    packed, starts, codes = oc.packed_records([2] * n, 5, 1, 7)
    rng = np.random.default_rng(6)
    mask = rng.random(len(codes) - 1) < 1.0 / 50
    mask[:7] = True
    mask[int(starts[-1]):] = True
    amb = ac.pack_bits(mask, 5)
    for canonical in (False, True):
        want = ac.expect_packed_amb(oracle, packed, starts, k, oracle.default_hasher(canonical), amb, 1, 5)
        assert (want == oc.NO_MINIMIZER).sum() > 10
        got = _device(sm, gpu, sm.NtHasher(k, canonical), k, packed, amb, n, starts, bo=1, ao=5)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
        got, err = _counts(sm, gpu, sm.NtHasher(k, canonical), k, packed, amb, starts, (int(starts[-1]), n), 1, 5)
        assert err is None and np.array_equal(got[:n], want) and (got[n:] == oc.NO_MINIMIZER).all()


def test_k_above_the_tile_reads_global_memory(sm, oracle, gpu):
    """k = 5000: symbols and bits are not staged."""
    k, bo, ao = 5000, 3, 37
    lens = [12000, 4999, 5000, 5001, 9000]
    packed, starts, codes = oc.packed_records(lens, 21, bo, 7)
    s = [int(x) for x in starts]
    mask = np.zeros(len(codes) - bo, dtype=bool)
    mask[s[0] + 3000] = True        # record 0: clean positions 3001 .. 7000
    mask[s[3] + 2500] = True        # 5001 bases with an N in the middle: none
    mask[s[4] + 8999] = True        # the last base: positions 0 .. 3999
    mask[:s[0]] = True
    mask[s[-1]:] = True
    amb = ac.pack_bits(mask, ao)
    for canonical in (False, True):
        ho = oracle.default_hasher(canonical)
        want = ac.expect_packed_amb(oracle, packed, starts, k, ho, amb, bo, ao)
        assert want[0] > 3000 and want[1] == oc.NO_MINIMIZER and want[2] == 0 and want[3] == oc.NO_MINIMIZER and want[4] < 4000
        got = _device(sm, gpu, sm.NtHasher(k, canonical), k, packed, amb, len(lens), starts, bo=bo, ao=ao, shifts=(1, 3))
        assert np.array_equal(got, want), (got, want)


def test_fixed_stride_layouts(sm, oracle, gpu):
    n = 300
    for length, stride in ((100, 128), (150, 150)):
        packed, _, codes = oc.packed_records([stride] * n, length, 1, 0)
        fixed = np.arange(n + 1, dtype=np.uint64) * np.uint64(stride)
        rng = np.random.default_rng(length)
        mask = rng.random(len(codes) - 1) < 1.0 / 200
        for r in range(0, n, 7):
            mask[r * stride + length:(r + 1) * stride + 1] = True
        mask[5 * stride:5 * stride + length] = True
        amb = ac.pack_bits(mask, 37)
        for k in (21, length, length + 1):
            for canonical in (False, True):
                want = ac.expect_packed_amb(oracle, packed, fixed, k, oracle.default_hasher(canonical), amb, 1, 37,
                                            lens=[length] * n)
                got = _device(sm, gpu, sm.NtHasher(k, canonical), k, packed, amb, n, None, stride, length, bo=1, ao=37)
                assert np.array_equal(got, want), (length, stride, k, canonical, np.nonzero(got != want)[0][:8])


def test_all_zero_bits_equal_the_plain_call_and_host_equals_device(sm, oracle, gpu):
    import torch
    T = sm.one_minimizer_tile()
    for k in (21, 33):
        lens = oc.shape_lengths(T, k, 60)
        n = len(lens)
        packed, starts, codes = oc.packed_records(lens, 31 + k, 2, 7)
        zero = np.zeros((5 + len(codes)) // 8 + 2, dtype=np.uint8)
        for canonical in (False, True):
            hp = sm.NtHasher(k, canonical)
            plain = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            sm.one_minimizer_reads_device(hp, k, _dev(packed), n, plain, read_starts=_dev(starts), base_offset=2, ws=gpu)
            gpu.check()
            plain = plain.cpu().numpy().view(np.uint32)
            assert np.array_equal(plain, oc.expect_packed(oracle, packed, starts, k, oracle.default_hasher(canonical), 2))
            assert np.array_equal(_device(sm, gpu, hp, k, packed, zero, n, starts, bo=2, ao=5), plain)
    # the host form: reads laid back to back from base 0, bits over them
    rng = np.random.default_rng(9)
    reads = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=ln)) for ln in (150, 20, 0, 21, 4100, 300, 22)]
    total = sum(len(r) for r in reads)
    mask = rng.random(total) < 1.0 / 60
    mask[150:170] = True  # the read of 20 and the first base of the one after it
    amb = ac.pack_bits(mask, 3)
    k = 21
    for canonical in (False, True):
        hp = sm.NtHasher(k, canonical)
        host = sm.one_minimizer_reads_host(reads, hp, k, ws=gpu, amb=amb, amb_offset=3)
        packed, starts = sm._pack_reads(reads)
        want = ac.expect_packed_amb(oracle, packed, starts, k, oracle.default_hasher(canonical), amb, 0, 3)
        assert np.array_equal(host, want), (host, want)
        assert np.array_equal(_device(sm, gpu, hp, k, packed, amb, len(reads), starts, ao=3), host)


def _fastq_with_n(n_reads, seed):
    rng = np.random.default_rng(seed)
    out, seqs = [], []
    for i in range(n_reads):
        ln = int(rng.integers(1, 30)) if i % 11 == 0 else int(rng.integers(30, 400))
        s = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=ln).tobytes())
        if i % 5 == 0 and ln:
            for p in rng.integers(0, ln, size=1 + i % 3):
                s[int(p)] = ord("N")
        if i == 7:
            s = bytearray(b"N" * ln)
        seqs.append(bytes(s))
        out.append(b"@r%d\n" % i + bytes(s) + b"\n+\n" + b"I" * ln + b"\n")
    return b"".join(out), seqs


def test_loader_to_positions_with_no_host_wait(sm, oracle, gpu):
    """ASCII FASTQ with N -> mm_fastq_pack_n_device_async -> the counts form with max_records above the real count, one
    check at the end; expected from the oracle's own packer."""
    import torch
    k, max_records = 21, 300
    fastq, seqs = _fastq_with_n(211, 4)
    n = len(seqs)
    t = _dev(np.frombuffer(fastq, dtype=np.uint8).copy())
    nb = int(t.numel())
    packed = torch.zeros((nb // 4 + 8 + 3) // 4 * 4 + 64, dtype=torch.uint8, device="cuda")
    amb = torch.zeros((nb // 8 + 8 + 3) // 4 * 4 + 64, dtype=torch.uint8, device="cuda")
    starts = torch.zeros(max_records + 1, dtype=torch.int64, device="cuda")
    rec_pos = torch.zeros(max_records, dtype=torch.int64, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = torch.full((max_records + GUARD,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    vp = stream_queue.vp
    opacked, oamb = oracle.pack_ascii_n(b"".join(seqs))
    ostarts = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    for canonical in (False, True):
        hp = sm.NtHasher(k, canonical)
        assert sm.lib().mm_fastq_pack_n_device_async(gpu.h, vp(t), nb, vp(packed), int(packed.numel()), vp(amb), int(amb.numel()),
                                                     vp(starts), vp(rec_pos), max_records, vp(counts)) == 0
        sm.one_minimizer_reads_counts_device(hp, k, packed, starts, counts, max_records, nb, out, ws=gpu, amb=amb)
        gpu.check()  # (the one wait)
        got = out.cpu().numpy()
        assert (got[max_records:] == -7).all()
        got = got[:max_records].view(np.uint32)
        assert [int(x) for x in counts.cpu().numpy()] == [int(ostarts[-1]), n]
        want = ac.expect_packed_amb(oracle, opacked, ostarts, k, oracle.default_hasher(canonical), oamb)
        assert want[7] == oc.NO_MINIMIZER and (want != oc.NO_MINIMIZER).sum() > 150
        assert np.array_equal(got[:n], want), np.nonzero(got[:n] != want)[0][:8]
        assert (got[n:] == oc.NO_MINIMIZER).all()


def test_counts_beyond_the_bounds(sm, oracle, gpu):
    """The whole output is "none", Workspace.check reports MM_ERR_CAPACITY once, the workspace is usable afterwards."""
    T, k, bo, ao = sm.one_minimizer_tile(), 21, 2, 5
    ho, hp = oracle.default_hasher(True), sm.NtHasher(k, True)
    packed, starts, amb, _, _ = ac.shape_case(oracle, T, k, ho, 99, bo, ao, tail=30)
    n = len(starts) - 1
    want = ac.expect_packed_amb(oracle, packed, starts, k, ho, amb, bo, ao)
    junk = np.full(len(starts), JUNK, dtype=np.uint64)
    max_bases = min(4 * len(packed) - bo, 8 * len(amb) - ao)
    for counts in ((max_bases + 1, n), (int(starts[-1]), n + EXTRA + 1)):
        got, err = _counts(sm, gpu, hp, k, packed, amb, junk, counts, bo, ao)
        assert err is not None and err.code == sm.ERR["CAPACITY"], counts
        assert (got == oc.NO_MINIMIZER).all(), counts
        gpu.check()  # (reported once)
        got, err = _counts(sm, gpu, hp, k, packed, amb, starts, (int(starts[-1]), n), bo, ao)
        assert err is None and np.array_equal(got[:n], want) and (got[n:] == oc.NO_MINIMIZER).all()


def test_queued_on_a_callers_non_blocking_stream(sm, oracle, gpu):
    """One host-n call and one counts call queued behind their uploads on a stream of the caller's, one check."""
    T, k, bo, ao = sm.one_minimizer_tile(), 21, 2, 5
    ho, hp = oracle.default_hasher(True), sm.NtHasher(k, True)
    packed, starts, amb, _, _ = ac.shape_case(oracle, T, k, ho, 123, bo, ao, tail=30)
    n = len(starts) - 1
    want = ac.expect_packed_amb(oracle, packed, starts, k, ho, amb, bo, ao)
    m = 17
    want_m = np.concatenate([want[:m], np.full(n - m, oc.NO_MINIMIZER, dtype=np.uint32)])
    q = stream_queue.Queue(sm)
    try:
        i_packed, i_amb = q.input(packed, shift=1), q.input(amb, shift=3)
        i_starts, i_counts = q.input(starts, index=True), q.input(np.array([int(starts[-1]), m], dtype=np.uint64), index=True)
        o_reads, o_counts = q.output(n), q.output(n)
        for name, inp in (("packed", i_packed), ("amb", i_amb), ("starts", i_starts), ("counts", i_counts)):
            q.upload(name, inp)
        q.add("reads", lambda: sm.one_minimizer_reads_device(hp, k, i_packed.d, n, o_reads.d, read_starts=i_starts.d,
                                                             base_offset=bo, ws=q.ws, amb=i_amb.d, amb_offset=ao),
              after=("packed", "amb", "starts"), verify=lambda: stream_queue.check_exact("reads", o_reads, want, "positions"))
        q.add("counts", lambda: sm.one_minimizer_reads_counts_device(hp, k, i_packed.d, i_starts.d, i_counts.d, n,
                                                                     None, o_counts.d, base_offset=bo, ws=q.ws, amb=i_amb.d,
                                                                     amb_offset=ao),
              after=("packed", "amb", "starts", "counts"),
              verify=lambda: stream_queue.check_exact("counts", o_counts, want_m, "positions"))
        for seed in (None, 3):
            q.run(q.order(seed), delay=True, no_wait=True)
            q.finish(label=f"order {seed}: ")
    finally:
        q.close()
