"""K-mer values of every read's minimizers in one launch (mm_values_u64_reads_* / mm_values_u128_reads_*): every
expectation is the oracle's values_u64 / values_u128 per read, bit-exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT = -0x0123456789ABCDEF  # what the value buffers hold before a call


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _expected(oracle, host, starts_abs, pos, offs, ln, canonical, u128):
    """The oracle per read: host = the packed bytes, starts_abs[r] = read r's first base in them."""
    f = oracle.values_u128 if u128 else oracle.values_u64
    parts = []
    for r in np.flatnonzero(np.diff(offs) > 0):
        parts.append(f(host, ln, pos[offs[r]: offs[r + 1]], canonical, base_offset=int(starts_abs[r])))
    if not parts:
        return np.zeros((0, 2) if u128 else (0,), dtype=np.uint64)
    return np.concatenate(parts)


def _call(sm, ws, d, packed_bytes, base_offset, n_reads, d_starts, stride, ln, canonical, d_pos, d_offs, n_pos_max, d_out,
          u128=False):
    f = sm.lib().mm_values_u128_reads_device_async if u128 else sm.lib().mm_values_u64_reads_device_async
    return f(ws.h if ws is not None else None, _vp(d), packed_bytes, base_offset, n_reads, _vp(d_starts), stride, ln,
             int(canonical), _vp(d_pos), _vp(d_offs), n_pos_max, _vp(d_out))


def _device_values(sm, ws, d, base_offset, n_reads, d_starts, stride, ln, canonical, d_pos, d_offs, tot, u128=False,
                   slack=9, packed_bytes=None):
    """One launch with n_pos_max = tot + slack into a sentinel-filled buffer; returns the tot values after checking that
    nothing behind them was written."""
    import torch
    per = 2 if u128 else 1
    n_pos_max = tot + slack
    assert d_pos.numel() >= n_pos_max
    out = torch.full((per * n_pos_max + 3,), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    sm._check(_call(sm, ws, d, d.numel() if packed_bytes is None else packed_bytes, base_offset, n_reads, d_starts, stride,
                    ln, canonical, d_pos, d_offs, n_pos_max, out, u128))
    ws.sync()
    ws.check()
    got = out.cpu().numpy()
    assert np.all(got[per * tot:] == SENT), "values past the true count were written"
    got = got[: per * tot].view(np.uint64)
    return got.reshape(-1, 2) if u128 else got


def _synthetic(rng, read_lens, counts, ln):
    """Read-local positions with pos + ln inside the read, back to back, and their offsets"""
    offs = np.zeros(len(counts) + 1, dtype=np.int64)
    offs[1:] = np.cumsum(counts)
    pos = np.zeros(int(offs[-1]), dtype=np.uint32)
    for r in np.flatnonzero(np.asarray(counts) > 0):
        assert read_lens[r] >= ln
        pos[offs[r]: offs[r + 1]] = np.sort(rng.integers(0, read_lens[r] - ln + 1, counts[r]))
    return pos, offs


PLANS = [  # (k, w, canonical, mode, u128): the value length is k for minimizers, k + w - 1 for syncmers
    (21, 11, True, 0, False),
    (5, 7, False, 0, False),
    (15, 17, False, 1, False),   # closed syncmers: len 31
    (32, 8, True, 0, False),     # len 32: the u64 mask edge
    (31, 33, True, 1, True),     # len 63
    (64, 8, True, 0, True),      # len 64
]


@pytest.fixture(scope="module")
def strided(sm, oracle, gpu):
    """3 000 reads of up to 150 bases every 151 bases (every 2-bit and dword phase) from base 37 on; lengths a mix of 0,
    a few bases, and up to 150."""
    import torch
    rng = np.random.default_rng(21)
    n_reads, read_len, stride, base_offset = 3000, 150, 151, 37
    lens = rng.integers(0, read_len + 1, n_reads)
    lens[rng.random(n_reads) < 0.15] = 0
    short = rng.random(n_reads) < 0.15
    lens[short] = rng.integers(1, 31, int(short.sum()))
    lens[-1] = read_len
    span = base_offset + (n_reads - 1) * stride + read_len
    d = sm.generate_device(span, 77)
    return dict(n_reads=n_reads, read_len=read_len, stride=stride, base_offset=base_offset, lens=lens, d=d,
                host=d.cpu().numpy(), d_lens=torch.from_numpy(lens.astype(np.int32)).cuda(),
                starts_abs=base_offset + np.arange(n_reads, dtype=np.int64) * stride)


@pytest.mark.parametrize("plan", PLANS, ids=lambda p: f"k{p[0]}w{p[1]}{'c' if p[2] else 'f'}m{p[3]}{'u128' if p[4] else ''}")
def test_strided_reads(sm, oracle, gpu, strided, plan):
    import torch
    k, w, canonical, mode, u128 = plan
    s = strided
    b = sm.Builder(k, w, canonical, mode)
    ln = k if mode == 0 else k + w - 1
    cap = s["n_reads"] * s["read_len"]
    d_pos = torch.zeros(cap + 16, dtype=torch.int32, device="cuda")
    d_offs = torch.zeros(s["n_reads"] + 1, dtype=torch.int64, device="cuda")
    tot = sm.run_reads_device(b, s["d"], s["n_reads"], s["stride"], s["read_len"], d_pos[:cap], d_offs,
                              read_lens=s["d_lens"], base_offset=s["base_offset"])
    assert tot > 1024
    pos, offs = d_pos[:tot].cpu().numpy().view(np.uint32), d_offs.cpu().numpy()
    want = _expected(oracle, s["host"], s["starts_abs"], pos, offs, ln, canonical, u128)
    got = _device_values(sm, gpu, s["d"], s["base_offset"], s["n_reads"], None, s["stride"], ln, canonical, d_pos, d_offs,
                         tot, u128)
    assert np.array_equal(got, want), plan
    # the wrapper takes len and canonical from the builder
    out = sm.values_reads_device(b, s["d"], s["n_reads"], d_pos, d_offs, read_stride=s["stride"],
                                 base_offset=s["base_offset"], n_pos_max=tot, u128=u128)
    gpu.sync()
    got2 = out.cpu().numpy().view(np.uint64)
    assert np.array_equal(got2.reshape(-1, 2) if u128 else got2, want), plan


@pytest.fixture(scope="module")
def packed_reads(sm, oracle, gpu):
    """2 000 reads of 0 .. 2 000 bases back to back, the first one starting at base 13"""
    rng = np.random.default_rng(22)
    lens = rng.integers(0, 2001, 2000)
    lens[:4] = [0, 2000, 0, 1]
    starts = np.zeros(len(lens) + 1, dtype=np.int64)
    starts[0] = 13
    starts[1:] = 13 + np.cumsum(lens)
    d = sm.generate_device(int(starts[-1]), 78)
    return dict(lens=lens, starts=starts, d=d, host=d.cpu().numpy())


@pytest.mark.parametrize("plan", [PLANS[0], PLANS[2], PLANS[4]], ids=["k21w11c", "sync31", "u128len63"])
def test_packed_reads(sm, oracle, gpu, packed_reads, plan):
    import torch
    k, w, canonical, mode, u128 = plan
    p = packed_reads
    b = sm.Builder(k, w, canonical, mode)
    ln = k if mode == 0 else k + w - 1
    n = len(p["lens"])
    total = int(p["starts"][-1])
    d_starts = torch.from_numpy(p["starts"]).cuda()
    d_pos = torch.zeros(total + 16, dtype=torch.int32, device="cuda")
    d_offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    cnt = C.c_uint64()
    sm._check(sm.lib().mm_run_packed_reads_device(b.plan().h, gpu.h, _vp(p["d"]), p["d"].numel(), 0, n, _vp(d_starts), total,
                                                  2000, _vp(d_pos), None, total, _vp(d_offs), C.byref(cnt)))
    tot = int(cnt.value)
    assert tot > 1024
    pos, offs = d_pos[:tot].cpu().numpy().view(np.uint32), d_offs.cpu().numpy()
    want = _expected(oracle, p["host"], p["starts"], pos, offs, ln, canonical, u128)
    got = _device_values(sm, gpu, p["d"], 0, n, d_starts, 0, ln, canonical, d_pos, d_offs, tot, u128)
    assert np.array_equal(got, want), plan
    out = sm.values_reads_device(b, p["d"], n, d_pos, d_offs, read_starts=d_starts, n_pos_max=tot, u128=u128)
    gpu.sync()
    got2 = out.cpu().numpy().view(np.uint64)
    assert np.array_equal(got2.reshape(-1, 2) if u128 else got2, want), plan


def test_packed_reads_with_n_skip_ambiguous(sm, oracle, gpu):
    """FASTQ with N through the packer that writes ambiguity bits and the skip-ambiguous packed run; the values of its
    positions (no k-mer there holds an N) against the oracle on the packed bases."""
    import torch
    rng = np.random.default_rng(23)
    recs, lens = [], []
    for r in range(600):
        n = int(rng.integers(0, 400))
        seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n)
        seq[rng.random(n) < 0.01] = ord("N")
        recs.append(b"@r%d\n" % r + seq.tobytes() + b"\n+\n" + b"I" * n + b"\n")
        lens.append(n)
    records = sm.fasta_pack_n_device(b"".join(recs), max_records=1024)
    assert records.lengths() == lens
    n = len(records)
    total = int(records.base[-1])
    b = sm.canonical_minimizers(21, 11)
    d_pos = torch.zeros(total + 16, dtype=torch.int32, device="cuda")
    d_offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    tot = sm.run_packed_reads_skip_ambiguous_device(b, records, d_pos[:total], d_offs)
    assert tot > 1024
    d_starts = torch.from_numpy(records.base.astype(np.int64)).cuda()
    pos, offs = d_pos[:tot].cpu().numpy().view(np.uint32), d_offs.cpu().numpy()
    want = _expected(oracle, records.packed.cpu().numpy(), records.base.astype(np.int64), pos, offs, 21, True, False)
    got = _device_values(sm, gpu, records.packed, 0, n, d_starts, 0, 21, True, d_pos, d_offs, tot)
    assert np.array_equal(got, want)


def _lookup_case(sm, name):
    """(read lengths, values per read) of the layouts that steer the lookup"""
    stage = sm.values_reads_lds_stage()
    n_empty = max(5000, 2 * stage)
    if name == "empty_run_global_path":  # one long read, a run of empty reads longer than the LDS stage, one long read
        return [30000] + [0] * n_empty + [30000], [1500] + [0] * n_empty + [1501]
    if name == "empty_run_lds_path":  # the same with a run the stage still holds
        m = stage - 8
        return [30000] + [0] * m + [30000], [1500] + [0] * m + [1501]
    if name == "all_empty":
        return [0] * 300, [0] * 300
    if name == "one_read_many_workgroups":
        return [50000], [4099]
    if name == "seams_and_odd_totals":  # reads whose values straddle the 1024- and 256-value seams; total % 4 == 3
        return [4000] * 9, [1000, 48, 1, 0, 2047, 3, 1021, 5, 2]
    if name == "leading_and_trailing_empty":
        return [0] * 700 + [900, 0, 0, 60, 77] + [0] * 700, [0] * 700 + [333, 0, 0, 1, 2] + [0] * 700
    raise KeyError(name)


LOOKUP_CASES = ["empty_run_global_path", "empty_run_lds_path", "all_empty", "one_read_many_workgroups",
                "seams_and_odd_totals", "leading_and_trailing_empty"]


@pytest.mark.parametrize("u128", [False, True], ids=["u64", "u128"])
@pytest.mark.parametrize("name", LOOKUP_CASES)
def test_lookup_paths(sm, oracle, gpu, name, u128):
    """Both lookup paths and their edges on chosen layouts: positions are drawn inside every read (the values kernel takes
    any position), reads back to back from base 5 on, then the same reads as a fixed-stride layout where they fit."""
    import torch
    rng = np.random.default_rng(24)
    read_lens, counts = _lookup_case(sm, name)
    read_lens, counts = np.asarray(read_lens, dtype=np.int64), np.asarray(counts, dtype=np.int64)
    ln, canonical = (47, True) if u128 else (21, True)
    n = len(read_lens)
    starts = np.zeros(n + 1, dtype=np.int64)
    starts[0] = 5
    starts[1:] = 5 + np.cumsum(read_lens)
    d = sm.generate_device(int(starts[-1]) + 64, 79)
    host = d.cpu().numpy()
    pos, offs = _synthetic(rng, read_lens, counts, ln)
    tot = int(offs[-1])
    if name == "seams_and_odd_totals":
        assert tot % 4 == 3 and offs[1] < 1024 < offs[5] and offs[4] < 2048 < offs[5]
    if name == "empty_run_global_path":
        assert n + 1 > sm.values_reads_lds_stage() and 1024 < offs[1] < 2048  # the run lies inside one workgroup's values
    d_starts = torch.from_numpy(starts).cuda()
    d_offs = torch.from_numpy(offs).cuda()
    want = _expected(oracle, host, starts, pos, offs, ln, canonical, u128)
    # positions one element off a 16-byte boundary, and on it
    for shift in (1, 0):
        buf = torch.zeros(tot + 16 + shift, dtype=torch.int32, device="cuda")
        assert buf.data_ptr() % 16 == 0
        d_pos = buf[shift:]
        d_pos[:tot] = torch.from_numpy(pos.view(np.int32)).cuda()
        got = _device_values(sm, gpu, d, 0, n, d_starts, 0, ln, canonical, d_pos, d_offs, tot, u128)
        assert np.array_equal(got, want), (name, shift)
    # n_pos_max SMALLER than the true count: nothing past n_pos_max is written
    if tot > 10:
        out = torch.full(((2 if u128 else 1) * tot,), SENT, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        sm._check(_call(sm, gpu, d, d.numel(), 0, n, d_starts, 0, ln, canonical, d_pos, d_offs, tot - 7, out, u128))
        gpu.sync()
        got = out.cpu().numpy()
        per = 2 if u128 else 1
        assert np.all(got[per * (tot - 7):] == SENT)
        assert np.array_equal(got[: per * (tot - 7)].view(np.uint64), want.reshape(-1)[: per * (tot - 7)])


def test_no_reads_and_no_room(sm, gpu):
    """n_reads == 0 and n_pos_max == 0 return MM_OK and launch nothing: the value buffer keeps its sentinel."""
    import torch
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    d_pos = torch.zeros(16, dtype=torch.int32, device="cuda")
    d_offs = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    out = torch.full((16,), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for u128 in (False, True):
        assert _call(sm, gpu, d, 64, 0, 0, None, 10, 21, 1, d_pos, d_offs, 4, out, u128) == 0
        assert _call(sm, gpu, d, 64, 0, 1, None, 10, 21, 1, d_pos, d_offs, 0, out, u128) == 0
        assert _call(sm, gpu, None, 0, 0, 0, None, 0, 21, 1, None, None, 0, None, u128) == 0
    gpu.sync()
    assert bool((out == SENT).all())


def test_reads_beyond_base_2_pow_32(sm, oracle, gpu):
    """Two reads whose second one starts past base 2^32 of a buffer of just over 1 GiB, allocated uninitialised, only the
    two reads' bytes written: fixed stride (a product that does not fit 32 bits with the base offset added) and starts."""
    import torch
    rng = np.random.default_rng(25)
    nbytes = (1 << 30) + 256
    d = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    lo, hi = rng.integers(0, 256, 128, dtype=np.uint8), rng.integers(0, 256, 128, dtype=np.uint8)
    d[:128] = torch.from_numpy(lo).cuda()
    d[1 << 30: (1 << 30) + 128] = torch.from_numpy(hi).cuda()
    read_len = 150
    for u128, ln in ((False, 31), (True, 64)):
        counts = np.array([37, 41])
        pos, offs = _synthetic(rng, [read_len, read_len], counts, ln)
        tot = int(offs[-1])
        d_pos = torch.zeros(tot + 16, dtype=torch.int32, device="cuda")
        d_pos[:tot] = torch.from_numpy(pos.view(np.int32)).cuda()
        d_offs = torch.from_numpy(offs).cuda()
        f = oracle.values_u128 if u128 else oracle.values_u64
        for layout in ("stride", "starts"):
            base_offset = 37
            if layout == "stride":
                stride, d_starts = (1 << 32) - 1, None
                second = base_offset + stride  # 2^32 + 36
            else:
                stride = 0
                starts = np.array([3, (1 << 32) + 21, (1 << 32) + 21 + read_len], dtype=np.int64)
                d_starts = torch.from_numpy(starts).cuda()
                second = base_offset + int(starts[1])
            first = base_offset + (3 if layout == "starts" else 0)
            assert second >= 1 << 32
            want = np.concatenate([f(lo, ln, pos[: offs[1]], True, base_offset=first),
                                   f(hi, ln, pos[offs[1]:], True, base_offset=second - (1 << 32))])
            got = _device_values(sm, gpu, d, base_offset, 2, d_starts, stride, ln, True, d_pos, d_offs, tot, u128)
            assert np.array_equal(got, want), (u128, layout)
    del d
    torch.cuda.empty_cache()


def test_file_to_values_on_one_stream_without_a_host_wait(sm, oracle, gpu):
    """FASTQ text -> mm_fastq_pack_device_async -> mm_run_packed_reads_device_async -> mm_values_u64_reads_device_async
    queued on the workspace's stream, ONE synchronize at the end; the values equal the per-read oracle."""
    import torch
    rng = np.random.default_rng(26)
    seqs = [rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(n)).tobytes() for n in rng.integers(0, 300, 900)]
    text = b"".join(b"@q%d\n" % i + s + b"\n+\n" + b"F" * len(s) + b"\n" for i, s in enumerate(seqs))
    n_rec, total = len(seqs), sum(len(s) for s in seqs)
    L, ws = sm.lib(), gpu
    b = sm.canonical_minimizers(21, 11)
    plan = b.plan()
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    packed = torch.zeros((total // 4 + 64) // 4 * 4, dtype=torch.uint8, device="cuda")
    rb = torch.zeros(n_rec + 1, dtype=torch.int64, device="cuda")
    rp = torch.zeros(n_rec, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    cap = total + 16
    d_pos = torch.zeros(cap, dtype=torch.int32, device="cuda")
    d_offs = torch.zeros(n_rec + 1, dtype=torch.int64, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    vals = torch.full((cap,), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    sm._check(L.mm_fastq_pack_device_async(ws.h, _vp(t), t.numel(), _vp(packed), packed.numel(), _vp(rb), _vp(rp), n_rec,
                                           _vp(cnt)))
    sm._check(L.mm_run_packed_reads_device_async(plan.h, ws.h, _vp(packed), packed.numel(), 0, n_rec, _vp(rb), total, 300,
                                                 _vp(d_pos), None, cap, _vp(d_offs), _vp(d_cnt)))
    sm._check(L.mm_values_u64_reads_device_async(ws.h, _vp(packed), packed.numel(), 0, n_rec, _vp(rb), 0, 21, 1, _vp(d_pos),
                                                 _vp(d_offs), cap, _vp(vals)))
    ws.sync()  # the only wait
    ws.check()
    assert [int(x) for x in cnt.cpu()] == [total, n_rec]
    tot = int(d_cnt.item())
    offs = d_offs.cpu().numpy()
    assert tot == offs[-1] and tot > 1024
    got = vals.cpu().numpy()
    assert np.all(got[tot:] == SENT)
    pos = d_pos[:tot].cpu().numpy().view(np.uint32)
    at = 0
    for r, s in enumerate(seqs):
        p = oracle.pack_ascii(s) if s else np.zeros(1, dtype=np.uint8)
        want_pos = oracle.run(p, len(s), 21, 11, canonical=True)
        assert np.array_equal(pos[offs[r]: offs[r + 1]], want_pos), r
        want = oracle.values_u64(p, 21, want_pos, True)
        assert np.array_equal(got[offs[r]: offs[r + 1]].view(np.uint64), want), r
        at += len(want)
    assert at == tot


def test_host_entries_equal_the_oracle(sm, oracle, gpu):
    """values_reads_host over run_reads_host's output == the oracle per read, ASCII reads and PackedSeq views."""
    rng = np.random.default_rng(27)
    seqs = [rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(n)).tobytes() for n in rng.integers(0, 500, 700)]
    seqs[0], seqs[5] = b"", b"ACGT"
    for (k, w, canonical, mode, u128) in (PLANS[0], PLANS[2], PLANS[4]):
        b = sm.Builder(k, w, canonical, mode)
        ln = k if mode == 0 else k + w - 1
        pos, offs, _ = sm.run_reads_host(b, seqs)
        assert len(pos) > 1024
        got = sm.values_reads_host(b, seqs, pos, offs, u128=u128)
        want = []
        for r, s in enumerate(seqs):
            if offs[r + 1] > offs[r]:
                p = oracle.pack_ascii(s)
                if u128:
                    v = oracle.values_u128(p, ln, pos[offs[r]: offs[r + 1]], canonical)
                    want += [int(a) | (int(c) << 64) for a, c in v]
                else:
                    want += [int(x) for x in oracle.values_u64(p, ln, pos[offs[r]: offs[r + 1]], canonical)]
        assert [int(x) for x in got] == want, (k, w, mode, u128)
    # PackedSeq views at odd offsets give what their ASCII gives
    b = sm.canonical_minimizers(21, 11)
    views = []
    for s in seqs[:60]:
        v = sm.PackedSeqVec.from_ascii(b"GT" + s)
        views.append(v.slice(2, 2 + len(s)))
    pos, offs, _ = sm.run_reads_host(b, seqs[:60])
    assert np.array_equal(sm.values_reads_host(b, views, pos, offs), sm.values_reads_host(b, seqs[:60], pos, offs))
    assert len(sm.values_reads_host(b, [], np.zeros(0, dtype=np.uint32), [0])) == 0


def test_error_codes(sm, gpu):
    import torch
    E, L = sm.ERR, sm.lib()
    d = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    d_pos = torch.zeros(16, dtype=torch.int32, device="cuda")
    d_offs = torch.tensor([0, 2, 4], dtype=torch.int64, device="cuda")
    out = torch.zeros(32, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for u128, too_long in ((False, 33), (True, 65)):
        assert _call(sm, None, d, 1024, 0, 2, None, 100, 21, 1, d_pos, d_offs, 4, out, u128) == E["NULL"]
        for ln in (0, too_long):
            assert _call(sm, gpu, d, 1024, 0, 2, None, 100, ln, 1, d_pos, d_offs, 4, out, u128) == E["VALUE_LEN"]
        assert _call(sm, gpu, d, 1024, 0, 2, None, 100, too_long - 1, 1, d_pos, d_offs, 4, out, u128) == 0
        for missing in range(4):
            args = [d, d_pos, d_offs, out]
            args[missing] = None
            assert _call(sm, gpu, args[0], 1024, 0, 2, None, 100, 21, 1, args[1], args[2], 4, args[3], u128) == E["NULL"]
        # the second read of a fixed-stride layout starts past the buffer's 4 096 bases
        assert _call(sm, gpu, d, 1024, 0, 2, None, 4097, 21, 1, d_pos, d_offs, 4, out, u128) == E["CAPACITY"]
        assert _call(sm, gpu, d, 1024, 1, 2, None, 4096, 21, 1, d_pos, d_offs, 4, out, u128) == E["CAPACITY"]
        assert _call(sm, gpu, d, 1024, 4097, 2, None, 0, 21, 1, d_pos, d_offs, 4, out, u128) == E["CAPACITY"]
        assert _call(sm, gpu, d, 1024, 0, 2, None, 4096, 21, 1, d_pos, d_offs, 4, out, u128) == 0
    gpu.sync()
    gpu.check()
    # host entries
    packed = np.zeros(64, dtype=np.uint8)
    pos = np.zeros(4, dtype=np.uint32)
    vals = np.zeros(8, dtype=np.uint64)
    p8, p32, p64 = (lambda a: sm._p(a, C.c_uint8)), (lambda a: sm._p(a, C.c_uint32)), (lambda a: sm._p(a, C.c_uint64))
    good_starts, good_offs = np.array([0, 100, 200], dtype=np.uint64), np.array([0, 2, 4], dtype=np.uint64)
    for f, too_long in ((L.mm_values_u64_reads_host, 33), (L.mm_values_u128_reads_host, 65)):
        def host(starts=good_starts, offs=good_offs, ln=21, ws=gpu.h, pk=p8(packed), stride=0, nbytes=64):
            return f(ws, pk, nbytes, 0, 2, p64(starts) if starts is not None else None, stride, ln, 1, p32(pos), p64(offs),
                     p64(vals))
        assert host() == 0
        assert host(ws=None) == E["NULL"]
        assert host(ln=0) == E["VALUE_LEN"] and host(ln=too_long) == E["VALUE_LEN"]
        assert host(starts=np.array([0, 100, 50], dtype=np.uint64)) == E["UNSORTED"]
        assert host(offs=np.array([0, 3, 2], dtype=np.uint64)) == E["UNSORTED"]
        assert host(pk=None) == E["NULL"]
        assert host(starts=np.array([0, 100, 257], dtype=np.uint64)) == E["CAPACITY"]  # 64 bytes hold 256 bases
        assert host(starts=None, stride=257) == E["CAPACITY"]
        assert host(starts=None, stride=100) == 0
        assert host(offs=np.array([0, 0, 0], dtype=np.uint64), pk=None) == 0  # nothing to do


def test_cxx_values_many_example_runs(gpu):
    """Builder::values_u64_many / values_u128_many == Output::values_* per read through the header-only C++ mirror."""
    exe = os.path.join(os.path.dirname(__file__), "cxx", "values_many_example")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe), "-f", "values_many_example.mk"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
