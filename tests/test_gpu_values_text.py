"""K-mer values of byte text on the GPU (mm_values_*_text_device_async, mm_values_*_text_batch_device_async and their
host forms).  DNA encoding is pinned by the oracle's values of PackedSeqVec::from_ascii(text); BYTES by the little-endian
integer built here; the batch calls also by the single-text call on every record alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BYTES, DNA = 0, 1
U64_LENS = (1, 5, 15, 16, 17, 21, 31, 32)
U128_LENS = (33, 47, 63, 64, 21)
N_TEXT = 3000
ACGT = np.frombuffer(b"ACGTacgt", dtype=np.uint8)


def _builder(sm, length, canonical):
    """A builder whose values are `length` characters long (minimizers: len = k)."""
    return (sm.canonical_minimizers if canonical else sm.minimizers)(length, 2 if length % 2 == 0 else 3)


def _ints128(a):
    return [int(lo) | (int(hi) << 64) for lo, hi in np.asarray(a).reshape(-1, 2)]


def _little_endian(text: bytes, pos, length):
    padded = bytes(text) + bytes(length)
    return [int.from_bytes(padded[p:p + length], "little") for p in pos]


def _dev_pos(pos):
    import torch
    return torch.from_numpy(np.ascontiguousarray(pos, dtype=np.uint32).view(np.int32)).cuda()


def _values(sm, b, d_text, n, pos, encoding, u128):
    """The single-text device call on `pos`; a uint64 array (u128: (n, 2))."""
    d_pos = _dev_pos(pos)
    out = sm.values_text_device(b, d_text, n, d_pos, len(pos), encoding, u128=u128)
    b._ws().check()
    got = out.cpu().numpy().view(np.uint64)
    return got.reshape(-1, 2) if u128 else got


@pytest.fixture(scope="module")
def dna(oracle):
    import torch
    rng = np.random.default_rng(20261018)
    text = rng.choice(ACGT, N_TEXT)
    shifted = []
    for shift in range(4):  # the text at byte `shift` of a fresh allocation, exactly N_TEXT readable bytes
        big = torch.zeros(N_TEXT + 8, dtype=torch.uint8, device="cuda")
        big[shift:shift + N_TEXT] = torch.from_numpy(text).cuda()
        assert (big.data_ptr() + shift) % 4 == shift
        shifted.append(big[shift:shift + N_TEXT])
    torch.cuda.synchronize()
    return {"text": text.tobytes(), "packed": oracle.pack_ascii(text.tobytes()),
            "padded": oracle.pack_ascii(text.tobytes() + bytes(80)), "dev": shifted}


def _position_sets(length, seed):
    rng = np.random.default_rng(seed)
    last = N_TEXT - length
    sets = [np.arange(0, last + 1)]
    for m in (1, 3, 5, 1023, 1025):
        sets.append(rng.integers(0, last + 1, m))
    return sets


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("length", U64_LENS + U128_LENS)
def test_single_text_dna(sm, oracle, gpu, dna, length, canonical):
    """Every byte phase of the buffer, every position (both buffer ends: both edge paths), tails that are no multiple
    of four; u64 for len <= 32 and u128 for the U128_LENS."""
    import torch
    dev = torch.cuda.current_device()
    b = _builder(sm, length, canonical)
    widths = ([False] if length in U64_LENS else []) + ([True] if length in U128_LENS else [])
    for u128 in widths:
        f = oracle.values_u128 if u128 else oracle.values_u64
        for pos in _position_sets(length, 100 * length + canonical):
            want = f(dna["packed"], length, pos, canonical)
            want = np.asarray(want).reshape(-1, 2)[:len(pos)] if u128 else np.asarray(want)[:len(pos)]
            for shift in range(4):
                got = _values(sm, b, dna["dev"][shift], N_TEXT, pos, DNA, u128)
                assert np.array_equal(got, want), (length, canonical, u128, shift, len(pos))
    assert torch.cuda.current_device() == dev


def test_single_text_dna_past_the_end_reads_zeros(sm, oracle, gpu, dna):
    """text_bytes == n: the last len - 1 positions and positions past the text get the missing characters as byte 0."""
    for length, canonical, u128 in ((21, True, False), (32, False, False), (16, True, False), (64, True, True), (47, False, True)):
        pos = np.arange(N_TEXT - length + 1, N_TEXT + 3)
        f = oracle.values_u128 if u128 else oracle.values_u64
        want = np.asarray(f(dna["padded"], length, pos, canonical))
        want = want.reshape(-1, 2)[:len(pos)] if u128 else want[:len(pos)]
        for shift in range(4):
            got = _values(sm, _builder(sm, length, canonical), dna["dev"][shift], N_TEXT, pos, DNA, u128)
            assert np.array_equal(got, want), (length, shift)


def test_single_text_dna_many_workgroups(sm, oracle, gpu):
    """2^20 random positions over a 4 Mchar text: a thousand workgroups (u64), four thousand (u128)."""
    import torch
    rng = np.random.default_rng(5)
    n = 4 << 20
    text = rng.choice(ACGT, n)
    packed = oracle.pack_ascii(text.tobytes())
    d_text = torch.from_numpy(text).cuda()
    for length, canonical, u128 in ((21, True, False), (33, True, True)):
        pos = rng.integers(0, n - length + 1, 1 << 20)
        got = _values(sm, _builder(sm, length, canonical), d_text, n, pos, DNA, u128)
        want = np.asarray((oracle.values_u128 if u128 else oracle.values_u64)(packed, length, pos, canonical))
        assert np.array_equal(got, want.reshape(-1, 2) if u128 else want), (length, u128)


@pytest.mark.parametrize("length", [1, 3, 7, 8, 9, 15, 16])
def test_single_text_bytes(sm, gpu, length):
    """Random bytes with 0x00 and 0xFF among them; every position of the text, so the last len - 1 are zero-extended."""
    import torch
    rng = np.random.default_rng(40 + length)
    a = rng.integers(0, 256, N_TEXT, dtype=np.uint8)
    a[::97], a[5::89], a[-3:] = 0x00, 0xFF, (0xFF, 0x00, 0xFF)
    pos = np.arange(0, N_TEXT)
    want = _little_endian(a.tobytes(), pos, length)
    b = _builder(sm, length, False)
    for shift in range(4):
        big = torch.zeros(N_TEXT + 8, dtype=torch.uint8, device="cuda")
        big[shift:shift + N_TEXT] = torch.from_numpy(a).cuda()
        d_text = big[shift:shift + N_TEXT]
        torch.cuda.synchronize()
        if length <= 8:
            got = _values(sm, b, d_text, N_TEXT, pos, BYTES, False)
            assert [int(v) for v in got] == want, (length, shift)
        got = _values(sm, b, d_text, N_TEXT, pos, BYTES, True)
        assert _ints128(got) == want, (length, shift)
    for m in (1, 3, 5, 1023, 1025):
        sub = rng.integers(0, N_TEXT, m)
        got = _values(sm, b, d_text, N_TEXT, sub, BYTES, True)
        assert _ints128(got) == _little_endian(a.tobytes(), sub, length), (length, m)


@pytest.fixture(scope="module")
def records(sm, oracle):
    """More than 4000 records of ASCII DNA, lengths 0 .. 600: empty ones, ones shorter than l, a run of more empty records
    than the LDS stage holds between two long ones (the global path), and 5 bytes of other text before the first."""
    import torch
    rng = np.random.default_rng(77)
    stage = sm.values_text_lds_stage()
    lens = [int(x) for x in rng.integers(0, 601, 1200)]
    lens[3:3] = [0, 0, 7, 0, 30, 31, 8]
    lens += [600] + [0] * (stage + 50) + [600]
    lens += [int(x) for x in rng.integers(0, 601, 900)] + [0, 0]
    starts = np.concatenate([[5], 5 + np.cumsum(lens)]).astype(np.uint64)
    assert len(lens) > 4000
    n_chars = int(starts[-1])
    text = rng.choice(ACGT, n_chars + 3)  # (three readable bytes behind the last record)
    text[:5] = np.frombuffer(b"\xff\x00>id", dtype=np.uint8)
    return {"text": text, "starts": starts, "n_chars": n_chars, "packed": oracle.pack_ascii(text.tobytes()),
            "d_text": torch.from_numpy(text).cuda(), "d_starts": torch.from_numpy(starts.view(np.int64)).cuda()}


def _plans(sm):
    return {
        "fwd_21_11": sm.minimizers(21, 11).hasher(sm.TextHasher.from_dna(sm.NtHasher(canonical=False))),
        "canon_21_11": sm.canonical_minimizers(21, 11).hasher(sm.TextHasher.from_dna(sm.NtHasher(canonical=True))),
        "min_5_4": sm.minimizers(5, 4),                 # len 5
        "closed_5_4": sm.closed_syncmers(5, 4),         # len 8: the longest `&[u8]` value of 64 bits
    }


def _run_batch(sm, b, rec):
    import torch
    n_rec = len(rec["starts"]) - 1
    d_pos = torch.zeros(rec["n_chars"], dtype=torch.int32, device="cuda")
    d_offs = torch.zeros(n_rec + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cnt = sm.run_text_batch_device(b, rec["d_text"], rec["d_starts"], rec["n_chars"], d_pos, d_offs)
    return d_pos, d_offs, cnt


@pytest.mark.parametrize("plan", ["fwd_21_11", "canon_21_11", "min_5_4", "closed_5_4"])
def test_batch_against_per_record_loop_and_oracle(sm, oracle, gpu, records, plan):
    import torch
    rec = records
    b = _plans(sm)[plan]
    length = b.k if b.mode == sm.MM_MINIMIZERS else b.k + b.w - 1
    d_pos, d_offs, cnt = _run_batch(sm, b, rec)
    offs = d_offs.cpu().numpy().astype(np.uint64)
    pos = d_pos[:cnt].cpu().numpy().view(np.uint32)
    starts = rec["starts"]
    n_rec = len(starts) - 1
    assert cnt == int(offs[-1]) and cnt > 10_000
    owner = np.searchsorted(offs, np.arange(cnt), side="right") - 1
    absolute = (starts[owner] + pos).astype(np.uint64)
    assert int(absolute.max()) + length <= rec["n_chars"]
    L, ws = sm.lib(), b._ws().h
    dev = torch.cuda.current_device()
    encodings = [DNA] + ([BYTES] if plan in ("min_5_4", "closed_5_4") else [])
    for encoding in encodings:
        for u128 in (False, True):
            per = 2 if u128 else 1
            got = sm.values_text_batch_device(b, rec["d_text"], rec["d_starts"], rec["n_chars"], d_pos, d_offs, cnt,
                                              encoding, u128=u128)
            # the single-text call on every record alone: its bytes only (text_bytes = its length), its slice of positions
            loop = torch.zeros(per * cnt, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            f = L.mm_values_u128_text_device_async if u128 else L.mm_values_u64_text_device_async
            for r in range(n_rec):
                m = int(offs[r + 1] - offs[r])
                if m == 0:
                    continue
                n = int(starts[r + 1] - starts[r])
                assert f(ws, C.c_void_p(rec["d_text"].data_ptr() + int(starts[r])), n, n, encoding, length,
                         int(b.canonical), C.c_void_p(d_pos.data_ptr() + 4 * int(offs[r])), m,
                         C.c_void_p(loop.data_ptr() + 8 * per * int(offs[r]))) == 0
            b._ws().check()
            assert torch.equal(got, loop), (plan, encoding, u128)
            g = got.cpu().numpy().view(np.uint64)
            if encoding == DNA:
                want = np.asarray((oracle.values_u128 if u128 else oracle.values_u64)(rec["packed"], length, absolute,
                                                                                     bool(b.canonical)))
                assert np.array_equal(g, want.reshape(-1)[:per * cnt]), (plan, u128)
            else:
                chars = rec["text"][absolute[:, None] + np.arange(length, dtype=np.uint64)[None, :]].astype(np.uint64)
                want = (chars << (8 * np.arange(length, dtype=np.uint64))[None, :]).sum(axis=1, dtype=np.uint64)
                assert np.array_equal(g.reshape(-1, per)[:, 0], want), (plan, u128)
                if u128:
                    assert not g.reshape(-1, 2)[:, 1].any()
    assert torch.cuda.current_device() == dev


def test_true_count_is_read_on_the_device(sm, oracle, gpu, records):
    """The batch run and its values queued back to back with no synchronisation in between; n_pos_max is what the buffers
    hold, far above the count: nothing at or past the count is written."""
    import torch
    rec = records
    b = _plans(sm)["canon_21_11"]
    n_rec = len(rec["starts"]) - 1
    cap = rec["n_chars"]
    sentinel = 0x5A5A5A5A5A5A5A5A
    L, ws = sm.lib(), gpu.h
    dev = torch.cuda.current_device()
    for u128 in (False, True):
        per = 2 if u128 else 1
        d_pos = torch.zeros(cap, dtype=torch.int32, device="cuda")
        d_offs = torch.zeros(n_rec + 1, dtype=torch.int64, device="cuda")
        d_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        vals = torch.full((per * cap,), sentinel, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        f = L.mm_values_u128_text_batch_device_async if u128 else L.mm_values_u64_text_batch_device_async
        text_args = (C.c_void_p(rec["d_text"].data_ptr()), rec["d_text"].numel(), n_rec, C.c_void_p(rec["d_starts"].data_ptr()),
                     rec["n_chars"])
        assert L.mm_run_text_batch_device_async(b.text_plan().h, ws, *text_args, C.c_void_p(d_pos.data_ptr()), None, cap,
                                                C.c_void_p(d_offs.data_ptr()), C.c_void_p(d_cnt.data_ptr())) == 0
        assert f(ws, *text_args, DNA, 21, 1, C.c_void_p(d_pos.data_ptr()), C.c_void_p(d_offs.data_ptr()), cap,
                 C.c_void_p(vals.data_ptr())) == 0
        assert L.mm_workspace_check(ws) == 0
        assert torch.cuda.current_device() == dev
        cnt = int(d_cnt.item())
        assert 0 < cnt < cap and int(d_offs[-1].item()) == cnt
        assert bool((vals[per * cnt:] == sentinel).all())
        offs = d_offs.cpu().numpy().astype(np.uint64)
        owner = np.searchsorted(offs, np.arange(cnt), side="right") - 1
        absolute = rec["starts"][owner] + d_pos[:cnt].cpu().numpy().view(np.uint32)
        want = np.asarray((oracle.values_u128 if u128 else oracle.values_u64)(rec["packed"], 21, absolute, True))
        assert np.array_equal(vals[:per * cnt].cpu().numpy().view(np.uint64), want.reshape(-1)[:per * cnt])
        # a smaller n_pos_max than the count: nothing past n_pos_max is written either
        vals.fill_(sentinel)
        torch.cuda.synchronize()
        short = cnt - 1001
        assert f(ws, *text_args, DNA, 21, 1, C.c_void_p(d_pos.data_ptr()), C.c_void_p(d_offs.data_ptr()), short,
                 C.c_void_p(vals.data_ptr())) == 0
        assert L.mm_workspace_check(ws) == 0
        assert bool((vals[per * short:] == sentinel).all())
        assert np.array_equal(vals[:per * short].cpu().numpy().view(np.uint64), want.reshape(-1)[:per * short])


def test_front_doors(sm, gpu, records):
    import torch
    dev = torch.cuda.current_device()
    rng = np.random.default_rng(3)
    text = rng.integers(0, 256, 500, dtype=np.uint8).tobytes()
    for seq in (text, bytearray(text), np.frombuffer(text, dtype=np.uint8)):
        pos = []
        out = sm.minimizers(5, 4).run(seq, pos)
        assert len(pos) > 50
        assert [int(v) for v in out.values_u64()] == _little_endian(text, pos, 5)
        assert out.values_u128() == _little_endian(text, pos, 5)
        p64, v64 = out.pos_and_values_u64()
        assert list(p64) == pos and [int(v) for v in v64] == _little_endian(text, pos, 5)
    pos = []
    out = sm.closed_syncmers(9, 8).run(text, pos)  # len 16: u128 only
    assert out.values_u128() == _little_endian(text, pos, 16)
    with pytest.raises(sm.MinimizerError) as e:
        out.values_u64()
    assert e.value.code == sm.ERR["VALUE_LEN"]
    for values in ("values_u64", "values_u128", "pos_and_values_u64", "pos_and_values_u128"):
        with pytest.raises(sm.MinimizerError) as e:
            getattr(sm.canonical_minimizers(5, 5).run(text, []), values)()
        assert e.value.code == sm.ERR["BAD_MODE"], values
    assert torch.cuda.current_device() == dev
    # the host batch form against the device path
    rec = records
    starts = rec["starts"]
    recs = [rec["text"][int(starts[r]):int(starts[r + 1])] for r in range(len(starts) - 1)]
    for b, encoding in ((_plans(sm)["canon_21_11"], DNA), (_plans(sm)["closed_5_4"], BYTES)):
        pos, offs, _ = sm.run_text_batch_host(b, recs)
        d_pos, d_offs, cnt = _run_batch(sm, b, rec)
        assert cnt == len(pos) and d_offs.cpu().tolist() == offs
        for u128 in (False, True):
            dev_vals = sm.values_text_batch_device(b, rec["d_text"], rec["d_starts"], rec["n_chars"], d_pos, d_offs, cnt,
                                                   encoding, u128=u128)
            b._ws().check()
            host_vals = sm.values_text_batch_host(b, recs, pos, offs, encoding, u128=u128)
            g = dev_vals.cpu().numpy().view(np.uint64)
            assert (_ints128(g) if u128 else [int(v) for v in g]) == [int(v) for v in host_vals], (encoding, u128)
    assert torch.cuda.current_device() == dev


def test_cxx_values_text_example_runs(gpu):
    """Builder::values_u64 / values_u128 (TextSeq) and their _many forms through the header-only C++ mirror: the example
    checks every record against the single-text call and the definitions."""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx", "values_text_example")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe), "-f", "values_text_example.mk"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "values_text_example: ok" in r.stdout
