"""Reads-mode launches on layouts outside address order and small spans: fixed-stride reads that OVERLAP (read_len >
read_stride), lanes of one tile more than 2^31 bases apart (a large stride, a long first record cut to max_read_len, a contig
batch scattered over a 700 MB buffer in no address order), and contig batches in any order or aliasing each other.  Every
layout runs three ways - MM_LANE_TABLE unset (the policy), =1 (the lane table forced) and =0 (one lane per read, or the
per-sequence tiles of a batch) - every read / contig is compared element by element with the oracle on its own bases, and
every run asserts which path it took, so that a change of the policy cannot quietly stop a layout from reaching its code."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
MODES = (None, "1", "0")  # MM_LANE_TABLE: the policy, the table forced, the table off


class _Env:
    """MM_LANE_TABLE for the duration of a block (tests/conftest.py makes the library read switches every time)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("MM_LANE_TABLE")
        if self.value is None:
            os.environ.pop("MM_LANE_TABLE", None)
        else:
            os.environ["MM_LANE_TABLE"] = self.value

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("MM_LANE_TABLE", None)
        else:
            os.environ["MM_LANE_TABLE"] = self.old


def _free():
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _host_slices(buf, spans, unit=4):
    """The bytes of every (first base, length) span of a packed buffer - 2-bit bases (unit 4) or ambiguity bits (unit 8) -
    as (host array, offset of the first base in it).  A device buffer is copied once, span by span, never as a whole."""
    import torch
    if isinstance(buf, np.ndarray):
        return [(buf[s // unit:], s % unit) for s, _ in spans]
    idx = [(s // unit, min((s + n) // unit + 2, buf.numel())) for s, n in spans]
    flat = torch.cat([buf[a:b] for a, b in idx]).cpu().numpy() if idx else np.zeros(0, dtype=np.uint8)
    out, at = [], 0
    for (a, b), (s, _) in zip(idx, spans):
        out.append((np.concatenate([flat[at: at + b - a], np.zeros(16, dtype=np.uint8)]), s % unit))
        at += b - a
    return out


def _want(oracle, seq, spans, k, w, canonical, sk=False, amb=None):
    """The oracle's answer for every (first base, length) span: [positions] or [(positions, super-k-mer indices)]"""
    bases = _host_slices(seq, spans)
    bits = _host_slices(amb, spans, unit=8) if amb is not None else None
    res = []
    for i, (_, ln) in enumerate(spans):
        p, off = bases[i]
        if amb is not None:
            a, aoff = bits[i]
            res.append(oracle.run_skip_ambiguous(p, a, int(ln), k, w, base_offset=off, amb_offset=aoff))
        else:
            res.append(oracle.run(p, int(ln), k, w, canonical=canonical, super_kmers=sk, base_offset=off))
    return res


def _check_reads(want, flat, ho, fsk=None, what=()):
    assert len(ho) == len(want) + 1 and ho[0] == 0 and ho[-1] == len(flat)
    for r, res in enumerate(want):
        wp = res[0] if fsk is not None else res
        assert np.array_equal(flat[ho[r]: ho[r + 1]], wp), (what, r, len(wp), int(ho[r + 1] - ho[r]))
        if fsk is not None:
            assert np.array_equal(fsk[ho[r]: ho[r + 1]], res[1]), (what, r, "super-k-mer indices")


def _expect_path(ws, launches, path, what):
    """path: "table" (one lane-table launch), "lane" (one launch, one lane per read), "off" (no lane table: one lane per read
    or one launch per read / per-sequence tiles)"""
    if path == "table":
        assert ws.last_lane_table() and launches == 1, (what, path, launches)
    elif path == "lane":
        assert not ws.last_lane_table() and launches == 1, (what, path, launches)
    else:
        assert not ws.last_lane_table() and launches >= 1, (what, path, launches)


def _run_stride(sm, ws, b, d, n_reads, stride, read_len, cap, read_lens=None, d_amb=None, sk=False):
    """mm_run_reads_device / _superkmers_ / _skip_ambiguous_ through the wrapper: (positions, offsets, indices, launches)"""
    import torch
    out = torch.full((cap + 8,), -7, dtype=torch.int32, device="cuda")
    osk = torch.zeros_like(out) if sk else None
    offs = torch.full((n_reads + 1,), -1, dtype=torch.int64, device="cuda")
    ws.enable_timing(True)
    ws.kernel_time(True)
    try:
        tot = sm.run_reads_device(b, d, n_reads, stride, read_len, out[:cap], offs, read_lens=read_lens, d_amb=d_amb,
                                  out_sk=osk[:cap] if sk else None)
        _, launches = ws.kernel_time(True)
    finally:
        ws.enable_timing(False)
    ho = offs.cpu().numpy()
    assert ho[0] == 0 and ho[-1] == tot and np.all(np.diff(ho) >= 0)
    assert int(out[tot].item()) == -7  # nothing written past the count
    return out[:tot].cpu().numpy().view(np.uint32), ho, (osk[:tot].cpu().numpy().view(np.uint32) if sk else None), launches


def _run_packed(sm, ws, b, d, starts, mx, sk=False):
    """mm_run_packed_reads_device: (positions, offsets, indices, launches)"""
    import torch
    n = len(starts) - 1
    total = int(starts[-1])
    ds = torch.from_numpy(np.asarray(starts, dtype=np.int64)).cuda()
    cap = n * int(mx) // 3 + 64
    out = torch.full((cap + 8,), -7, dtype=torch.int32, device="cuda")
    osk = torch.zeros_like(out) if sk else None
    offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    cnt = C.c_uint64()
    ws.enable_timing(True)
    ws.kernel_time(True)
    try:
        sm._check(sm.lib().mm_run_packed_reads_device(b.plan().h, ws.h, C.c_void_p(d.data_ptr()), d.numel(), 0, n,
                                                      C.c_void_p(ds.data_ptr()), total, int(mx), C.c_void_p(out.data_ptr()),
                                                      C.c_void_p(osk.data_ptr()) if sk else None, cap,
                                                      C.c_void_p(offs.data_ptr()), C.byref(cnt)))
        _, launches = ws.kernel_time(True)
    finally:
        ws.enable_timing(False)
    tot = int(cnt.value)
    ho = offs.cpu().numpy()
    assert ho[0] == 0 and ho[-1] == tot and np.all(np.diff(ho) >= 0)
    assert int(out[tot].item()) == -7
    return out[:tot].cpu().numpy().view(np.uint32), ho, (osk[:tot].cpu().numpy().view(np.uint32) if sk else None), launches


def _batch(sm, ws, b, seqs, lens, boffs, out, osk=None):
    """mm_run_batch_device: (offsets, positions, indices, launches)"""
    ws.enable_timing(True)
    ws.kernel_time(True)
    try:
        offs = sm.run_batch_device(b, seqs, lens, out, osk, base_offsets=boffs)
        _, launches = ws.kernel_time(True)
    finally:
        ws.enable_timing(False)
    flat = out[: offs[-1]].cpu().numpy().view(np.uint32).copy()
    return offs, flat, (osk[: offs[-1]].cpu().numpy().view(np.uint32).copy() if osk is not None else None), launches


def _lane_plan(sm, k, w, canonical, mode, n_reads, total_bases):
    plan = (C.c_uint64 * 6)()
    assert sm.lib().mm_debug_lane_plan(k, w, int(canonical), mode, n_reads, total_bases, 0, plan) == 0
    return [int(x) for x in plan]


def _last_table(sm, ws):
    """the workspace's last lane table: rows of {start, win0, count, read}"""
    n = C.c_uint64()
    sm._check(sm.lib().mm_debug_last_lane_table(ws.h, None, 0, C.byref(n)))
    tab = np.zeros((int(n.value), 4), dtype=np.uint32)
    sm._check(sm.lib().mm_debug_last_lane_table(ws.h, tab.ctypes.data_as(C.POINTER(C.c_uint32)), len(tab), C.byref(n)))
    return tab


def _check_table(tab, starts, nw, S):
    """every read's windows are covered exactly once by consecutive lanes that start where the read does + win0"""
    want_lanes = np.where(nw > 0, -(-nw // S), 1)
    first = np.concatenate([[0], np.cumsum(want_lanes)])
    assert first[-1] <= len(tab), (first[-1], len(tab))
    for r in range(len(nw)):
        rows = tab[first[r]: first[r + 1]]
        assert np.all(rows[:, 3] == r), r
        assert rows[0, 1] == 0 and int(rows[:, 2].astype(np.int64).sum()) == int(nw[r]), (r, rows[:3])
        assert np.array_equal(rows[:, 1], np.concatenate([[0], np.cumsum(rows[:-1, 2])])), r
        assert int(rows[:, 2].max()) <= S, r
        if nw[r]:
            assert np.array_equal(rows[:, 0].astype(np.int64), int(starts[r]) + rows[:, 1].astype(np.int64)), r
    pad = tab[int(first[-1]):]
    assert np.all(pad[:, 2] == 0)


def _max_tile_spread(tab):
    """the largest distance between the first bases of two walking lanes of one tile"""
    best = 0
    for t in range(0, len(tab), 256):
        rows = tab[t: t + 256]
        s = rows[rows[:, 2] > 0, 0].astype(np.int64)
        if len(s):
            best = max(best, int(s.max() - s.min()))
    return best


# ---------------------------------------------------------------------------------------------- 1. overlapping fixed-stride reads
@pytest.mark.parametrize("n_reads,read_len,stride", [(1000, 5000, 1000), (300, 30_000, 997)])
def test_overlapping_long_reads(sm, oracle, gpu, n_reads, read_len, stride):
    """Long reads that overlap (5 kbp windows every 1 kbp along a chromosome): the lane table needs about n_reads x read_len / S
    lanes, not (n_reads - 1) x stride + read_len over S.  Canonical k/w 21/11 and 31/51, forward 21/11 with super-k-mer
    indices; the policy and the forced table take ONE lane-table launch, =0 does without; every read == the oracle."""
    span = (n_reads - 1) * stride + read_len
    d = sm.generate_device(span, 31 + stride)
    host = d.cpu().numpy()
    spans = [(r * stride, read_len) for r in range(n_reads)]
    cap = n_reads * read_len // 3 + 64
    for (k, w, canonical, sk) in ((21, 11, True, False), (31, 51, True, False), (21, 11, False, True)):
        want = _want(oracle, host, spans, k, w, canonical, sk=sk)
        b = sm.Builder(k, w, canonical, 0)
        for mode, path in zip(MODES, ("table", "table", "off")):
            with _Env(mode):
                flat, ho, fsk, launches = _run_stride(sm, gpu, b, d, n_reads, stride, read_len, cap, sk=sk)
                _expect_path(gpu, launches, path, (k, w, mode))
            _check_reads(want, flat, ho, fsk, (k, w, canonical, sk, mode))
    del d
    _free()


@pytest.mark.parametrize("n_reads,read_len,stride", [(20_000, 150, 50), (50_000, 101, 1)])
def test_overlapping_short_reads(sm, oracle, gpu, n_reads, read_len, stride):
    """Short reads that overlap (150 bp every 50, 101 bp every base): one lane per read under the policy and with the table
    off, the forced table gives every read one lane of its own; every read == the oracle."""
    span = (n_reads - 1) * stride + read_len
    d = sm.generate_device(span, 41 + stride)
    host = d.cpu().numpy()
    spans = [(r * stride, read_len) for r in range(n_reads)]
    cap = n_reads * read_len // 2 + 64
    for (k, w, canonical, sk) in ((21, 11, True, False), (21, 11, False, True), (9, 5, True, False)):
        want = _want(oracle, host, spans, k, w, canonical, sk=sk)
        b = sm.Builder(k, w, canonical, 0)
        for mode, path in zip(MODES, ("lane", "table", "lane")):
            with _Env(mode):
                flat, ho, fsk, launches = _run_stride(sm, gpu, b, d, n_reads, stride, read_len, cap, sk=sk)
                _expect_path(gpu, launches, path, (k, w, mode))
            _check_reads(want, flat, ho, fsk, (k, w, canonical, sk, mode))
    del d
    _free()


def test_overlapping_reads_lengths_ambiguous_and_table(sm, oracle, gpu):
    """Overlapping reads (4 kbp every 700 bases) with d_read_lens below read_len - 0, k + w - 2, k + w - 1 among them - through
    mm_run_reads_device and the skip-ambiguous entry over an N-sprinkled buffer; the lane table itself covers every read's
    windows exactly once (mm_debug_last_lane_table)."""
    import torch
    rng = np.random.default_rng(701)
    n_reads, read_len, stride = 600, 4000, 700
    span = (n_reads - 1) * stride + read_len + 64
    a = ACGT[rng.integers(0, 4, size=span)].copy()
    a[rng.integers(0, span, size=span // 700)] = ord("N")
    for s0 in rng.integers(0, span - 400, 20):
        a[s0: s0 + int(rng.integers(1, 300))] = ord("N")
    packed, amb = oracle.pack_ascii_n(a.tobytes())
    d_p, d_m = torch.from_numpy(packed).cuda(), torch.from_numpy(amb).cuda()
    k, w = 21, 11
    l = k + w - 1
    lens_r = rng.integers(0, read_len + 1, size=n_reads)
    lens_r[:8] = [read_len, 0, l - 1, l, l + 1, 1, read_len - 1, 2 * l]
    d_lens = torch.from_numpy(lens_r.astype(np.int32)).cuda()
    starts = np.arange(n_reads, dtype=np.int64) * stride
    spans = [(int(starts[r]), int(lens_r[r])) for r in range(n_reads)]
    cap = n_reads * read_len // 3 + 64
    S = _lane_plan(sm, k, w, True, 0, n_reads, n_reads * read_len)[1]
    nw = np.maximum(lens_r.astype(np.int64) - l + 1, 0)
    for (kk, ww) in ((21, 11), (31, 51)):
        b = sm.canonical_minimizers(kk, ww)
        for use_amb in (False, True):
            want = _want(oracle, packed, spans, kk, ww, True, amb=amb if use_amb else None)
            for mode, path in zip(MODES, ("table", "table", "off")):
                with _Env(mode):
                    flat, ho, _, launches = _run_stride(sm, gpu, b, d_p, n_reads, stride, read_len, cap, read_lens=d_lens,
                                                        d_amb=d_m if use_amb else None)
                    _expect_path(gpu, launches, path, (kk, ww, use_amb, mode))
                _check_reads(want, flat, ho, None, (kk, ww, use_amb, mode))
                if (kk, ww, use_amb, mode) == (k, w, False, "1"):
                    _check_table(_last_table(sm, gpu), starts, nw, S)


# ----------------------------------------------------------------------------------- 2. lanes of one tile more than 2^31 bases apart
def test_far_apart_fixed_stride_reads(sm, oracle, gpu):
    """400 reads of 150 bp every 9 Mbp (a 3.6 Gbase span): one lane per read puts read 239 on at 2^31 bases from its tile's
    origin, and the forced lane table (one lane per read) does the same.  Canonical and forward with super-k-mer indices;
    every read == the oracle."""
    n_reads, read_len, stride = 400, 150, 9_000_000
    span = (n_reads - 1) * stride + read_len
    ws = sm.Workspace(0)
    d = sm.generate_device(span, 51)
    spans = [(r * stride, read_len) for r in range(n_reads)]
    try:
        for (k, w, canonical, sk) in ((21, 11, True, False), (21, 11, False, True), (31, 19, True, False)):
            want = _want(oracle, d, spans, k, w, canonical, sk=sk)
            b = sm.Builder(k, w, canonical, 0, workspace=ws)
            for mode, path in zip(MODES, ("lane", "table", "lane")):
                with _Env(mode):
                    flat, ho, fsk, launches = _run_stride(sm, ws, b, d, n_reads, stride, read_len, n_reads * read_len, sk=sk)
                    _expect_path(ws, launches, path, (k, w, mode))
                if mode == "1":
                    assert _max_tile_spread(_last_table(sm, ws)) >= 2 ** 31
                _check_reads(want, flat, ho, fsk, (k, w, canonical, sk, mode))
    finally:
        del d
        ws.close()
        _free()


def test_far_apart_fixed_stride_reads_skip_ambiguous(sm, oracle, gpu):
    """The skip-ambiguous reads entry over 300 reads of 150 bp every 9 Mbp (2.7 Gbase, ambiguity bits on the device): reads
    beyond 2^31 bases from the tile's origin, N bases sprinkled into them, whole reads of N; every read == the oracle."""
    import torch
    rng = np.random.default_rng(702)
    n_reads, read_len, stride = 300, 150, 9_000_000
    span = (n_reads - 1) * stride + read_len
    ws = sm.Workspace(0)
    d = sm.generate_device(span, 52)
    amb = torch.zeros(span // 8 + 64, dtype=torch.uint8, device="cuda")
    try:
        idx = (np.arange(n_reads, dtype=np.int64)[:, None] * stride + rng.integers(0, read_len, (n_reads, 3))).ravel()
        idx = np.concatenate([idx, np.arange(7 * stride, 7 * stride + read_len), np.arange(290 * stride + 40, 290 * stride + 90)])
        byte = np.unique(idx // 8)
        vals = np.zeros(len(byte), dtype=np.uint8)
        np.bitwise_or.at(vals, np.searchsorted(byte, idx // 8), (1 << (idx % 8)).astype(np.uint8))
        amb[torch.from_numpy(byte).cuda()] = torch.from_numpy(vals).cuda()
        spans = [(r * stride, read_len) for r in range(n_reads)]
        b = sm.Builder(21, 11, True, 0, workspace=ws)
        want = _want(oracle, d, spans, 21, 11, True, amb=amb)
        assert sum(len(x) for x in want) > 0 and len(want[7]) == 0
        for mode, path in zip(MODES, ("lane", "table", "lane")):
            with _Env(mode):
                flat, ho, _, launches = _run_stride(sm, ws, b, d, n_reads, stride, read_len, n_reads * read_len, d_amb=amb)
                _expect_path(ws, launches, path, mode)
            _check_reads(want, flat, ho, None, ("amb", mode))
    finally:
        del d, amb
        ws.close()
        _free()


def test_far_apart_lanes_of_long_reads(sm, oracle, gpu):
    """Reads of 2 000 bp, several lanes each, spaced so that one lane-table tile spans more than 2^31 bases (stride sized from
    the plans' lane lengths S, which differ between the canonical and the super-k-mer plan): the policy takes the table, and
    the table's tiles really are that wide; every read == the oracle under all three settings."""
    read_len = 2000
    configs = ((21, 11, True, False), (21, 11, False, True))
    S = {c: _lane_plan(sm, c[0], c[1], c[2], 3 if c[3] else 0, 60, 60 * read_len)[1] for c in configs}
    nw = read_len - (21 + 11 - 1) + 1
    per_read = max(-(-nw // s) for s in S.values())
    per_tile = 256 // per_read  # reads whose lanes lie in one tile (give or take the two cut at its ends)
    assert per_read >= 2 and per_tile >= 8, (S, per_read)
    stride = (2 ** 31 + 2 ** 27) // (per_tile - 3)
    n_reads = min(60, (2 ** 32 - read_len - 1) // stride + 1)
    assert n_reads > 256 // min(-(-nw // s) for s in S.values()), (n_reads, S)
    span = (n_reads - 1) * stride + read_len
    ws = sm.Workspace(0)
    d = sm.generate_device(span, 53)
    spans = [(r * stride, read_len) for r in range(n_reads)]
    try:
        for (k, w, canonical, sk) in configs:
            want = _want(oracle, d, spans, k, w, canonical, sk=sk)
            b = sm.Builder(k, w, canonical, 0, workspace=ws)
            for mode, path in zip(MODES, ("table", "table", "off")):
                with _Env(mode):
                    flat, ho, fsk, launches = _run_stride(sm, ws, b, d, n_reads, stride, read_len, n_reads * read_len, sk=sk)
                    _expect_path(ws, launches, path, (k, w, mode))
                if path == "table":
                    tab = _last_table(sm, ws)
                    assert _max_tile_spread(tab) >= 2 ** 31, (_max_tile_spread(tab), stride, S)
                    _check_table(tab, np.arange(n_reads, dtype=np.int64) * stride, np.full(n_reads, nw), S[(k, w, canonical, sk)])
                _check_reads(want, flat, ho, fsk, (k, w, canonical, sk, mode))
    finally:
        del d
        ws.close()
        _free()


def test_far_apart_packed_reads_after_a_cut_record(sm, oracle, gpu):
    """Reads packed back to back whose first record is 2.5 Gbases long and cut to max_read_len: the reads behind it lie 2.5e9
    bases from the tile's origin.  max_read_len 10 000 (the lane table) and 300 (one lane per read); the device entry, and
    the host entry on the same bases; the oracle of record 0 is its first max_read_len bases."""
    rng = np.random.default_rng(703)
    first = 2_500_000_000
    lens = np.concatenate([[first], rng.integers(100, 20_001, 300)]).astype(np.int64)
    lens[1:6] = [0, 30, 31, 10_000, 10_001]
    starts = np.zeros(len(lens) + 1, dtype=np.int64)
    starts[1:] = np.cumsum(lens)
    ws = sm.Workspace(0)
    d = sm.generate_device(int(starts[-1]), 54)
    host = None
    try:
        for (mx, paths) in ((10_000, ("table", "table", "off")), (300, ("lane", "table", "lane"))):
            spans = [(int(starts[r]), int(min(lens[r], mx))) for r in range(len(lens))]
            for (k, w, canonical, sk) in ((21, 11, True, False), (21, 11, False, True)):
                want = _want(oracle, d, spans, k, w, canonical, sk=sk)
                b = sm.Builder(k, w, canonical, 0, workspace=ws)
                for mode, path in zip(MODES, paths):
                    with _Env(mode):
                        flat, ho, fsk, launches = _run_packed(sm, ws, b, d, starts, mx, sk=sk)
                        _expect_path(ws, launches, path, (mx, k, w, mode))
                    _check_reads(want, flat, ho, fsk, (mx, k, w, canonical, sk, mode))
        # the host entry point on the same bases (one upload into the workspace's staging area, the same launch behind it)
        host = d[: (int(starts[-1]) + 3) // 4].cpu().numpy()
        del d
        _free()
        spans = [(int(starts[r]), int(min(lens[r], 10_000))) for r in range(len(lens))]
        want = _want(oracle, host, spans, 21, 11, True)
        b = sm.Builder(21, 11, True, 0, workspace=ws)
        hs = starts.astype(np.uint64)
        cap = len(lens) * 10_000 // 3
        for mode, path in zip(MODES, ("table", "table", "off")):
            pos = np.zeros(cap, dtype=np.uint32)
            offs = np.zeros(len(lens) + 1, dtype=np.uint64)
            cnt = C.c_uint64()
            with _Env(mode):
                sm._check(sm.lib().mm_run_packed_reads_host(b.plan().h, ws.h, host.ctypes.data_as(C.POINTER(C.c_uint8)), len(lens),
                                                            hs.ctypes.data_as(C.POINTER(C.c_uint64)), 10_000,
                                                            pos.ctypes.data_as(C.POINTER(C.c_uint32)), None, cap,
                                                            offs.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(cnt)))
                assert ws.last_lane_table() == (path == "table"), mode
            _check_reads(want, pos[: int(cnt.value)], offs.astype(np.int64), None, ("host", mode))
    finally:
        d = host = None
        ws.close()
        _free()


def test_far_apart_contig_batch_out_of_address_order(sm, oracle, gpu):
    """2 000 contigs of 1 - 20 kbp scattered over one 2.8 Gbase (700 MB) tensor, listed alternately from its low and its
    high end: one lane-table launch under the policy whose tiles mix contigs 2.8e9 bases apart; offsets and positions
    equal the per-sequence tiles (MM_LANE_TABLE=0) and the oracle, contig by contig."""
    import torch
    rng = np.random.default_rng(704)
    n_bases = 2_800_000_000
    n = 2000
    lens = rng.integers(1000, 20_001, n).astype(np.int64)
    lens[:4] = [1000, 31, 30, 20_000]
    pos = np.sort(rng.choice(n_bases // 32 - 1000, n, replace=False).astype(np.int64) * 32 + rng.integers(0, 32, n))
    order = np.empty(n, dtype=np.int64)
    order[0::2] = np.arange(n // 2)
    order[1::2] = np.arange(n - 1, n // 2 - 1, -1)
    starts = pos[order]
    ws = sm.Workspace(0)
    big = sm.generate_device(n_bases, 55)
    seqs = []
    try:
        seqs = [big[int(s) // 4:] for s in starts]
        boffs = [int(s) % 4 for s in starts]
        ln = [int(x) for x in lens]
        spans = [(int(starts[i]), ln[i]) for i in range(n)]
        out = torch.zeros(int(lens.sum()) // 4 + 64, dtype=torch.int32, device="cuda")
        for (k, w, canonical, sk) in ((21, 11, True, False), (21, 11, False, True), (31, 51, True, False)):
            want = _want(oracle, big, spans, k, w, canonical, sk=sk)
            b = sm.Builder(k, w, canonical, 0, workspace=ws)
            osk = torch.zeros_like(out) if sk else None
            res = {}
            for mode, path in zip(MODES, ("table", "table", "off")):
                out.fill_(-7)
                with _Env(mode):
                    offs, flat, fsk, launches = _batch(sm, ws, b, seqs, ln, boffs, out, osk)
                    _expect_path(ws, launches, path, (k, w, mode))
                if mode == "1":
                    assert _max_tile_spread(_last_table(sm, ws)) >= 2 ** 31
                _check_reads(want, flat, np.asarray(offs), fsk, (k, w, canonical, sk, mode))
                res[mode] = (offs, flat)
            assert res[None][0] == res["0"][0] and np.array_equal(res[None][1], res["0"][1])
    finally:
        del big, seqs
        ws.close()
        _free()


# ------------------------------------------------------------------------------------- 3. batch orders and aliasing at small span
def test_batch_permuted_repeated_and_overlapping_slices(sm, oracle, gpu):
    """The contig batch of test_lane_table_batch_of_short_contigs in a random permutation, with one contig listed twice and two
    slices that overlap in memory added: every listed sequence gets exactly the in-order run's positions, permuted back, under
    the policy, the forced table and the per-sequence tiles."""
    import torch
    rng = np.random.default_rng(705)
    lens = [int(x) for x in rng.integers(0, 30_000, 1500)]
    lens[:4] = [0, 30, 31, 100_000]
    gaps = rng.integers(0, 9, len(lens))
    starts = [int(x) for x in np.concatenate([[0], np.cumsum(np.array(lens) + gaps)])[: len(lens)]]
    big = sm.generate_device(starts[-1] + lens[-1] + 64, 12)
    host = big.cpu().numpy()
    # listed: a permutation of the contigs, contig 17 a second time, and two slices overlapping each other and contig 40
    ov = starts[40] + 5
    l_starts = [starts[i] for i in range(len(lens))] + [starts[17], ov, ov + 3001]
    l_lens = lens + [lens[17], 9000, 7000]
    perm = [int(x) for x in rng.permutation(len(l_lens))]
    out = torch.zeros(sum(l_lens) // 4 + 64, dtype=torch.int32, device="cuda")
    for (k, w, canonical, sk) in ((21, 11, True, False), (21, 11, False, True), (31, 51, True, False)):
        b = sm.Builder(k, w, canonical, 0)
        osk = torch.zeros_like(out) if sk else None
        seqs = [big[s // 4:] for s in l_starts]
        boffs = [s % 4 for s in l_starts]
        with _Env(None):
            ro, ref, rsk, launches = _batch(sm, gpu, b, seqs, l_lens, boffs, out, osk)
            _expect_path(gpu, launches, "table", (k, w, "in order"))
        want = _want(oracle, host, list(zip(l_starts, l_lens)), k, w, canonical, sk=sk)
        _check_reads(want, ref, np.asarray(ro), rsk, (k, w, "in order"))
        for mode, path in zip(MODES, ("table", "table", "off")):
            out.fill_(-7)
            with _Env(mode):
                offs, flat, fsk, launches = _batch(sm, gpu, b, [seqs[i] for i in perm], [l_lens[i] for i in perm],
                                                   [boffs[i] for i in perm], out, osk)
                _expect_path(gpu, launches, path, (k, w, mode))
            assert offs[-1] == ro[-1]
            for j, i in enumerate(perm):
                assert np.array_equal(flat[offs[j]: offs[j + 1]], ref[ro[i]: ro[i + 1]]), (k, w, mode, j, i)
                if sk:
                    assert np.array_equal(fsk[offs[j]: offs[j + 1]], rsk[ro[i]: ro[i + 1]]), (k, w, mode, j, i)
    del big
    _free()
