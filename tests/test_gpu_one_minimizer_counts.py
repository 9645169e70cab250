"""One minimizer per record with the counts read on the device (mm_one_minimizer_*_counts_device_async): out[0 .. n)
against the host-n call and the oracle (tests/one_minimizer_cases.py), MM_NO_MINIMIZER behind it up to max_records, a
guard word behind that in every case."""
import ctypes as C

import numpy as np
import pytest

import one_minimizer_cases as oc

pytestmark = pytest.mark.gpu
GUARD, EXTRA = 4, 37
JUNK = (1 << 63) - 1  # what the starts behind starts[n] hold: nobody may look at them


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _text_counts(sm, gpu, hasher, k, text, starts, counts, extra=EXTRA, max_chars=None):
    """(out[0 .. max_records) as uint32, what Workspace.check raised or None); starts padded to max_records + 1 words."""
    import torch
    n_max = len(starts) - 1 + extra
    d_text = _dev(text)
    d_starts = _dev(np.concatenate([starts, np.full(extra, JUNK, dtype=np.uint64)]))
    d_counts = _dev(np.asarray(counts, dtype=np.uint64))
    out = torch.full((n_max + GUARD,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sm.one_minimizer_text_batch_counts_device(hasher, k, d_text, d_starts, d_counts, n_max, max_chars, out, ws=gpu)
    err = None
    try:
        gpu.check()
    except sm.MinimizerError as e:
        err = e
    got = out.cpu().numpy()
    assert (got[n_max:] == -7).all(), "the guard behind d_out_pos was written"
    return got[:n_max].view(np.uint32), err


def _reads_counts(sm, gpu, hasher, k, packed, starts, counts, base_offset=0, extra=EXTRA, max_bases=None):
    import torch
    n_max = len(starts) - 1 + extra
    d_packed = _dev(packed)
    d_starts = _dev(np.concatenate([starts, np.full(extra, JUNK, dtype=np.uint64)]))
    d_counts = _dev(np.asarray(counts, dtype=np.uint64))
    out = torch.full((n_max + GUARD,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sm.one_minimizer_reads_counts_device(hasher, k, d_packed, d_starts, d_counts, n_max, max_bases, out,
                                         base_offset=base_offset, ws=gpu)
    err = None
    try:
        gpu.check()
    except sm.MinimizerError as e:
        err = e
    got = out.cpu().numpy()
    assert (got[n_max:] == -7).all(), "the guard behind d_out_pos was written"
    return got[:n_max].view(np.uint32), err


def _host_n_text(sm, gpu, hasher, k, text, starts, n):
    import torch
    out = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sm.one_minimizer_text_batch_device(hasher, k, _dev(text), _dev(starts), n, out, ws=gpu)
    gpu.sync()
    return out.cpu().numpy()[:n].view(np.uint32)


def _host_n_reads(sm, gpu, hasher, k, packed, starts, n, base_offset):
    import torch
    out = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sm.one_minimizer_reads_device(hasher, k, _dev(packed), n, out, read_starts=_dev(starts), base_offset=base_offset, ws=gpu)
    gpu.sync()
    return out.cpu().numpy()[:n].view(np.uint32)


def _lengths(T, k):
    """shape_lengths (records shorter than k, empty runs, a record spanning three tiles) and more than 1024 records
    inside one tile."""
    return oc.shape_lengths(T, k, 60) + [1, 0, 2] * 400 + [150] * 20


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", (1, 7, 31))
def test_text_counts_form(sm, gpu, k, canonical):
    T = sm.one_minimizer_tile()
    lens = _lengths(T, k)
    n = len(lens)
    text, starts = oc.text_records(lens, 70 + k, 3)
    hp = sm.TextMulHasher(k, canonical)
    want = oc.expect_text(text, starts, k, hp)
    got, err = _text_counts(sm, gpu, hp, k, text, starts, (int(starts[-1]), n))
    assert err is None
    bad = np.nonzero(got[:n] != want)[0]
    assert not len(bad), (bad[:8], got[bad[:8]], want[bad[:8]])
    assert (got[n:] == oc.NO_MINIMIZER).all()
    assert np.array_equal(got[:n], _host_n_text(sm, gpu, hp, k, text, starts, n))
    # fewer records than the starts describe: the host-n call for n_reads = m, "none" behind it
    m = 11
    got, err = _text_counts(sm, gpu, hp, k, text, starts, (int(starts[-1]), m))
    assert err is None
    assert np.array_equal(got[:m], _host_n_text(sm, gpu, hp, k, text, starts, m)) and np.array_equal(got[:m], want[:m])
    assert (got[m:] == oc.NO_MINIMIZER).all()
    # counts {0, 0}
    got, err = _text_counts(sm, gpu, hp, k, text, starts, (0, 0))
    assert err is None and (got == oc.NO_MINIMIZER).all()


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", (1, 7, 31))
def test_reads_counts_form(sm, oracle, gpu, k, canonical):
    T = sm.one_minimizer_tile()
    lens = _lengths(T, k)
    n = len(lens)
    bo = 1 + 2 * int(canonical)
    packed, starts, _ = oc.packed_records(lens, 80 + k, bo, 6)
    hp = sm.NtHasher(k, canonical)
    want = oc.expect_packed(oracle, packed, starts, k, oracle.default_hasher(canonical), bo)
    got, err = _reads_counts(sm, gpu, hp, k, packed, starts, (int(starts[-1]), n), bo)
    assert err is None
    bad = np.nonzero(got[:n] != want)[0]
    assert not len(bad), (bad[:8], got[bad[:8]], want[bad[:8]])
    assert (got[n:] == oc.NO_MINIMIZER).all()
    assert np.array_equal(got[:n], _host_n_reads(sm, gpu, hp, k, packed, starts, n, bo))
    m = 11
    got, err = _reads_counts(sm, gpu, hp, k, packed, starts, (int(starts[-1]), m), bo)
    assert err is None
    assert np.array_equal(got[:m], want[:m]) and (got[m:] == oc.NO_MINIMIZER).all()
    got, err = _reads_counts(sm, gpu, hp, k, packed, starts, (0, 0), bo)
    assert err is None and (got == oc.NO_MINIMIZER).all()


def test_symbol_count_below_the_last_start(sm, gpu):
    """n_sym inside the last record: the k-mers that end below it, as the host-n call gives them on a text cut there."""
    T, k = sm.one_minimizer_tile(), 7
    lens = oc.shape_lengths(T, k, 30)
    n = len(lens)
    text, starts = oc.text_records(lens, 5, 2)
    hp = sm.TextMulHasher(k, False)
    cut = int(starts[-1]) - 150 + k + 2
    cut_starts = starts.copy()
    cut_starts[-1] = cut
    got, err = _text_counts(sm, gpu, hp, k, text, starts, (cut, n))
    assert err is None
    assert np.array_equal(got[:n], oc.expect_text(text, cut_starts, k, hp)) and (got[n:] == oc.NO_MINIMIZER).all()
    assert got[n - 1] != oc.NO_MINIMIZER and got[n - 1] < 3


def test_counts_beyond_the_bounds(sm, oracle, gpu):
    """The whole output is "none", Workspace.check reports MM_ERR_CAPACITY once, the next call on the workspace succeeds.
    The starts are junk from word 0: a kernel that read them would not give "none" everywhere."""
    T, k = sm.one_minimizer_tile(), 7
    lens = oc.shape_lengths(T, k, 30)
    n = len(lens)
    text, starts = oc.text_records(lens, 6, 1)
    hp = sm.TextMulHasher(k, True)
    want = oc.expect_text(text, starts, k, hp)
    junk = np.full(len(starts), JUNK, dtype=np.uint64)
    for counts in ((len(text) + 1, n), (int(starts[-1]), n + EXTRA + 1), ((1 << 64) - 1, (1 << 64) - 1)):
        got, err = _text_counts(sm, gpu, hp, k, text, junk, counts)
        assert err is not None and err.code == sm.ERR["CAPACITY"], counts
        assert (got == oc.NO_MINIMIZER).all(), counts
        gpu.check()  # (reported once)
        got, err = _text_counts(sm, gpu, hp, k, text, starts, (int(starts[-1]), n))
        assert err is None and np.array_equal(got[:n], want) and (got[n:] == oc.NO_MINIMIZER).all()
    # a bound below the buffer: max_chars is the bound, not text_bytes
    got, err = _text_counts(sm, gpu, hp, k, text, junk, (int(starts[-1]), n), max_chars=int(starts[-1]) - 1)
    assert err is not None and err.code == sm.ERR["CAPACITY"] and (got == oc.NO_MINIMIZER).all()
    # max_chars below k: no workgroup of the main kernel, the refusal is raised all the same
    got, err = _text_counts(sm, gpu, hp, k, text, junk, (k, 1), max_chars=k - 1)
    assert err is not None and err.code == sm.ERR["CAPACITY"] and (got == oc.NO_MINIMIZER).all()
    bo = 2
    packed, pstarts, _ = oc.packed_records(lens, 7, bo, 3)
    nt = sm.NtHasher(k, True)
    pwant = oc.expect_packed(oracle, packed, pstarts, k, oracle.default_hasher(True), bo)
    for counts in ((4 * len(packed) - bo + 1, n), (int(pstarts[-1]), n + EXTRA + 1)):
        got, err = _reads_counts(sm, gpu, nt, k, packed, junk, counts, bo)
        assert err is not None and err.code == sm.ERR["CAPACITY"], counts
        assert (got == oc.NO_MINIMIZER).all(), counts
        got, err = _reads_counts(sm, gpu, nt, k, packed, pstarts, (int(pstarts[-1]), n), bo)
        assert err is None and np.array_equal(got[:n], pwant) and (got[n:] == oc.NO_MINIMIZER).all()


def _fasta(n_records, seed, alphabet=b"ACDEFGHIKLMNPQRSTVWY"):
    rng = np.random.default_rng(seed)
    out, seqs = [], []
    for i in range(n_records):
        ln = int(rng.integers(0, 400)) if i % 7 else (0 if i % 2 else 20)
        s = bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=ln))
        seqs.append(s)
        out.append(b">r%d\n" % i + b"".join(s[j:j + 60] + b"\n" for j in range(0, ln, 60)))
    return b"".join(out), seqs


def test_queued_behind_the_loader_with_no_host_wait(sm, gpu):
    """mm_fasta_text_device_async and the counts call back to back on the workspace's stream, one check at the end: equal
    to the synchronous route (fasta_text_device, then the host-n call) and to the checker."""
    import torch
    k, max_records = 7, 100
    fasta, seqs = _fasta(61, 12)
    n = len(seqs)
    hp = sm.TextMulHasher(k, False)
    t = _dev(np.frombuffer(fasta, dtype=np.uint8).copy())
    nb = int(t.numel())
    seq = torch.empty(nb, dtype=torch.uint8, device="cuda")
    starts = torch.zeros(max_records + 1, dtype=torch.int64, device="cuda")
    rec_pos = torch.zeros(max_records, dtype=torch.int64, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = torch.full((max_records + GUARD,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    vp = lambda x: C.c_void_p(x.data_ptr())
    assert sm.lib().mm_fasta_text_device_async(gpu.h, vp(t), nb, vp(seq), nb, vp(starts), vp(rec_pos), max_records,
                                               vp(counts)) == 0
    sm.one_minimizer_text_batch_counts_device(hp, k, seq, starts, counts, max_records, nb, out, ws=gpu)
    gpu.check()  # (the one wait)
    got = out.cpu().numpy()
    assert (got[max_records:] == -7).all()
    got = got[:max_records].view(np.uint32)
    assert [int(x) for x in counts.cpu().numpy()] == [sum(len(s) for s in seqs), n]
    rec = sm.fasta_text_device(fasta, max_records=max_records)
    sync = sm.one_minimizer_text_batch_device(hp, k, rec, ws=gpu)
    gpu.sync()
    assert np.array_equal(got[:n], sync.cpu().numpy().view(np.uint32))
    assert (got[n:] == oc.NO_MINIMIZER).all()
    hstarts = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    assert np.array_equal(got[:n], oc.expect_text(np.frombuffer(b"".join(seqs), dtype=np.uint8), hstarts, k, hp))


def test_no_records_and_return_codes(sm, gpu):
    import torch
    L, E = sm.lib(), sm.ERR
    th, hp = sm.TextMulHasher(7, False), sm.NtHasher(21, False)
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    cn = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    vp = lambda x: C.c_void_p(x.data_ptr())
    text, reads = L.mm_one_minimizer_text_batch_counts_device_async, L.mm_one_minimizer_reads_counts_device_async
    assert text(gpu.h, C.byref(th), 7, vp(d), 64, 64, 0, None, vp(cn), None) == 0
    assert text(gpu.h, C.byref(th), 7, vp(d), 64, 64, 3, vp(st), None, vp(out)) == E["NULL"]
    assert text(gpu.h, C.byref(th), 0, vp(d), 64, 65, 3, vp(st), vp(cn), vp(out)) == E["K_ZERO"]
    assert text(gpu.h, C.byref(th), 7, vp(d), 64, 65, 3, vp(st), vp(cn), vp(out)) == E["CAPACITY"]
    assert text(gpu.h, C.byref(th), 7, vp(d), 64, 64, 3, vp(st), vp(cn), vp(out)) == 0
    gpu.check()
    got = out.cpu().numpy()
    assert (got[:3].view(np.uint32) == oc.NO_MINIMIZER).all() and (got[3:] == -7).all()
    assert reads(gpu.h, C.byref(hp), 21, vp(d), 64, 1, 256, 3, vp(st), vp(cn), vp(out)) == E["CAPACITY"]
    assert reads(gpu.h, C.byref(hp), 21, vp(d), 64, 1, 255, 0, None, vp(cn), None) == 0
    assert reads(gpu.h, C.byref(hp), 21, vp(d), 64, 1, 255, 3, vp(st), vp(cn), vp(out)) == 0
    gpu.check()
    assert (out.cpu().numpy()[3:] == -7).all()
