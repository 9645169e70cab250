"""Every window size 34 .. 128 without a prebuilt kernel, against the oracle (exact equality everywhere;
tests/test_jit_windows_cpu.py pins the oracle at these sizes first).

Each such w is a kernel of its own, compiled with hiprtc at first use from a source that branches on W at compile time.
test_every_window_size runs EVERY one of them with canonical minimizers (forward ones at 26 sizes) on input where the vote decides,
with lanes that start at every residue mod 16 and all three walk bodies (whole tiles, a partial tile, the direct-store redo
of a tile whose lists overflow) - the conditions under which w = 49 and w = 65 once read a zero at the edge of their last
view (wide_group_blocks_nd, mm_fused_impl.h).  test_flavours runs every other flavour - syncmers, super-k-mer indices,
window ranges, the batch call, reads at a fixed stride, the lane table, the skip-ambiguous walks - at one size per distinct
combination of the kernel's compile-time choices (jit_window_cases.REPS).  The conditions are asserted from the launch plan
and the input, never from the product's outputs.

What a cold hiprtc compile costs (MI355X box, empty disk caches, one at a time through Builder.prepare), seconds at
w = 35 / 121 / 128: canonical minimizers 1.9 / 4.0 / 4.4, forward minimizers 0.7 / 1.6 / 1.6, canonical closed syncmers
2.0 / 3.7 / 4.4, forward minimizers with super-k-mer indices 0.8 / 1.5 / 1.8, canonical reads-mode minimizers 1.4 / 2.8 /
3.5.  Compiles from several threads of one process do not overlap (8 threads, 8 kernels: 24.5 s; 2 kernels one after the
other: 6.2 s), so worker processes compile ahead (jit_window_cases.prepare_ahead).  The module, all 93 sizes on both strands:
7 min 13 s cold, 7 s with the kernels in the disk cache; since then the forward runs are thinned (_forward_too)."""
import ctypes as C

import numpy as np
import pytest

import jit_window_cases as jw
from jit_window_cases import K_MAIN, REPS, SENTINEL, feasible, pack_at, plan_k, tie_heavy_codes
from test_gpu_long_k import _device_seq

pytestmark = pytest.mark.gpu

LIST_STRIDE = 2 * (256 + 2)   # bytes between the entries of a lane's 16-bit list (kListStride, mm_fused_impl.h)
LANES = 256                   # lanes of a tile (kFusedThreads)


def _all():
    import simd_minimizers_amd as sm
    return jw.jit_windows(sm)


def _u32(t, n):
    return t[:n].cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------ compiling ahead
def _forward_too(w):
    """Every size runs its canonical walk - that is where the strand vote is.  The forward walk shares the loads and the
    views but has no vote, and its kernel is one more compile per size: it runs at the sizes around a multiple of 16
    (one base in the last view, a full last view, no wide loads) and at the representatives - 26 of the 93 sizes.  (All 93
    forward kernels as well put the cold module at 7 min 13 s, see the module's docstring.)"""
    return w % 16 in (0, 1, 15) or w in REPS


def _kernels_of(name, w):
    """The prepare calls that cover the kernels of one id: (canonical, mode, sequence, reads, super-k-mer indices)."""
    if name == "test_every_window_size":
        return [(True, 0, True, False, False)] + ([(False, 0, True, False, False)] if _forward_too(w) else [])
    c = REPS.index(w) % 2 == 1
    jobs = [(c, 1, True, False, False), (c, 0, True, False, True), (c, 0, False, True, True), (c, 1, False, True, False),
            (True, 0, True, True, False), (True, 1, True, False, False)]
    return jobs + ([(c, 2, True, False, False)] if w % 2 else [])


@pytest.fixture(scope="module")
def ahead(request, sm, gpu):
    """A cold hiprtc compile of one of these kernels takes seconds and the module needs about 300 of them: the kernels of
    the ids that were selected are prepared by worker processes (jit_window_cases.prepare_ahead), in the order of the
    ids, while earlier ids run; an id waits for the workers to be done with its kernels and then runs as any caller
    would.  Nothing depends on it but the time."""
    keys = [(item.originalname, item.callspec.params["w"]) for item in request.session.items
            if getattr(item, "module", None) is request.module and hasattr(item, "callspec")]
    jobs = [(key, (K_MAIN, key[1]) + job) for key in keys for job in _kernels_of(*key)]
    pool, futures = jw.prepare_ahead([job for _, job in jobs])
    try:
        yield lambda name, w: jw.wait([f for (key, _), f in zip(jobs, futures) if key == (name, w)])
    finally:
        pool.shutdown(wait=True, cancel_futures=True)


def _default_plan(sm, w, canonical, mode, nw):
    """(blocks per lane, tiles, entries per lane list) of a default-lanes run over nw windows (mode as mm_debug_launch_plan)."""
    L = sm.lib()
    out7, out2, arr = (C.c_uint64 * 7)(), (C.c_uint64 * 2)(), (C.c_uint64 * 1)(nw)
    sm._check(L.mm_debug_launch_plan(w, int(canonical), mode, 0, arr, out7, None, None, None, 0, None))
    sm._check(L.mm_debug_launch_lds(w, int(canonical), mode, nw, out2))
    return int(out7[0]), int(out7[1]), int(out2[0]) // LIST_STRIDE


def _run_and_compare(sm, gpu, torch, b, data, off, n, want, what, sk=None):
    nw_cap = len(want) + 8
    d, _keep = _device_seq(torch, data, off, n, off % 4)
    out = torch.full((nw_cap,), SENTINEL, dtype=torch.int32, device="cuda")
    osk = torch.full((nw_cap,), SENTINEL, dtype=torch.int32, device="cuda") if sk is not None else None
    cnt = b.run_device(d, n, out, out_sk=osk, base_offset=off)
    assert gpu.last_path() == sm.PATH_FUSED, (what, sm.lib().mm_last_error())
    assert cnt == len(want), (what, cnt, len(want))
    got = _u32(out, cnt)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, bad[:4], got[bad[:4]], want[bad[:4]])
    assert int(out[cnt].item()) == SENTINEL, what   # the word behind the count
    if sk is not None:
        assert np.array_equal(_u32(osk, cnt), sk) and int(osk[cnt].item()) == SENTINEL, what
    return d, out, osk


# ------------------------------------------------------------------------------------------ every window size
def _every(sm, oracle, gpu, torch, w, canonical):
    k = plan_k(K_MAIN, w, canonical)
    l = k + w - 1
    b = sm.Builder(k, w, canonical, 0)
    # ---- (a) short explicit lanes: two whole tiles and a partial one, lane starts at every residue
    nblk = 2 if w % 16 == 0 else 3
    S = w * nblk
    tile = LANES * S
    nw = 2 * tile + 37 * S + 11
    n = nw + l - 1
    assert nw // tile == 2 and nw % tile != 0 and n < 260_000
    codes = tie_heavy_codes(max(n, l + 60_000), 9100 + w)   # ((b) and (c) take the first l + 60 000 bases or fewer)
    assert len(codes) >= plan_k(1, w, canonical) + w - 1 + 60_000
    offs = jw.offsets_for_every_residue(S)
    assert jw.lane_start_residues(offs, S) == set(range(16)) and {r % 4 for r in jw.lane_start_residues(offs, S)} == {0, 1, 2, 3}
    gpu.set_blocks_per_lane(nblk)
    for off in offs:
        data = pack_at(codes[:n], off)
        want = oracle.run(data, n, k, w, canonical=canonical, base_offset=off)
        _run_and_compare(sm, gpu, torch, b, data, off, n, want, dict(w=w, k=k, canonical=canonical, nblk=nblk, off=off))
    gpu.set_blocks_per_lane(0)
    # ---- (b) default lanes, on the first l + 60 000 bases; there the vote decides
    n = l + 60_000
    data = pack_at(codes[:n])
    nb_d, tiles, _cap = _default_plan(sm, w, canonical, 0, 60_001)
    assert nb_d >= 6 and tiles >= 1
    if canonical:
        ties = jw.tied_windows(oracle, data, n, k, w)
        assert ties >= 1000, (w, ties)
    want = oracle.run(data, n, k, w, canonical=canonical)
    assert len(want) > 500
    _run_and_compare(sm, gpu, torch, b, data, 0, n, want, dict(w=w, k=k, canonical=canonical, nblk=0))
    # ---- (c) a tile whose lists overflow: k = 1 or 2, every k-mer of the homopolymer ties and nearly every window emits
    k1 = plan_k(1, w, canonical)
    n = k1 + w - 1 + 60_000
    data = pack_at(codes[:n])
    nb_d, tiles, cap = _default_plan(sm, w, canonical, 0, 60_001)
    want, win = oracle.run(data, n, k1, w, canonical=canonical, super_kmers=True)
    per_lane = np.bincount(win // (w * nb_d))   # (uniform tiles: window i belongs to lane i // S of the run)
    assert tiles >= 1 and cap >= 8 and per_lane.max() >= 2 * cap, (w, nb_d, cap, int(per_lane.max()))
    _run_and_compare(sm, gpu, torch, sm.Builder(k1, w, canonical, 0), data, 0, n, want,
                     dict(w=w, k=k1, canonical=canonical, nblk=0, dense=True))


@pytest.mark.parametrize("w", _all())
def test_every_window_size(sm, oracle, gpu, ahead, w):
    """Canonical (k = 21 or 22) minimizers of one sequence, and forward ones (k = 21) where _forward_too says so, position
    for position."""
    import torch
    before = sm.jit_stats()
    ahead("test_every_window_size", w)
    try:
        for canonical in ((True, False) if _forward_too(w) else (True,)):
            _every(sm, oracle, gpu, torch, w, canonical)
    finally:
        gpu.set_blocks_per_lane(0)
    assert sm.jit_stats()["failed"] == before["failed"]


# ------------------------------------------------------------------------------------------ every flavour at the representatives
def _by_window(want, win, a, e):
    return want[(win >= a) & (win < e)]


def _sequence_family(sm, oracle, gpu, torch, w, canonical, rng):
    """Closed syncmers, open syncmers (odd w), minimizers with super-k-mer indices: whole, and as three window-range shards."""
    k = plan_k(K_MAIN, w, canonical)
    l = k + w - 1
    n = l + 100_000
    off = int(rng.integers(0, 4))
    data = pack_at(jw.tie_input(w, k, 100_000), off)
    nw = n - l + 1
    cut2 = 3 * nw // 4 + (1 if (3 * nw // 4) % w == 0 else 0)
    cuts = [0, nw // 2 + 3, cut2, nw]
    assert cut2 % w != 0 and cuts == sorted(cuts)
    ran = 0
    for mode, sk in ((1, False), (2, False), (0, True)):
        if not feasible(k, w, canonical, mode):
            continue
        what = dict(w=w, k=k, canonical=canonical, mode=mode, sk=sk, off=off)
        if sk:
            want, win = oracle.run(data, n, k, w, canonical=canonical, base_offset=off, super_kmers=True)
        else:
            want = oracle.run(data, n, k, w, canonical=canonical, mode=mode, base_offset=off)
            win = want
        assert len(want) >= (1 if mode == 2 else 500), (what, len(want))
        b = sm.Builder(k, w, canonical, mode)
        d, out, osk = _run_and_compare(sm, gpu, torch, b, data, off, n, want, what, sk=win if sk else None)
        parts = []
        for a, e in zip(cuts[:-1], cuts[1:]):
            out.fill_(SENTINEL)
            cc = b.run_device(d, n, out, out_sk=osk, base_offset=off, win_begin=a, win_end=e)
            sub = _by_window(want, win, a, e)
            assert cc == len(sub) and np.array_equal(_u32(out, cc), sub) and int(out[cc].item()) == SENTINEL, (what, a, e)
            if sk:
                assert np.array_equal(_u32(osk, cc), _by_window(win, win, a, e)), (what, a, e)
            parts.append(_u32(out, cc).copy())
        assert np.array_equal(np.concatenate(parts), want), what
        ran += 1
    assert ran == 2 + w % 2


def _check_reads(hp, ho, tot, want, hs=None, wsk=None, what=None):
    assert ho[0] == 0 and ho[-1] == tot and np.all(np.diff(ho.astype(np.int64)) >= 0) and len(ho) == len(want) + 1, what
    for r, wr in enumerate(want):
        assert np.array_equal(hp[ho[r]:ho[r + 1]], wr), (what, r, len(wr))
        if hs is not None:
            assert np.array_equal(hs[ho[r]:ho[r + 1]], wsk[r]), (what, r)


def _batch(sm, oracle, gpu, torch, w, canonical, rng):
    """mm_run_batch_device with super-k-mer indices: four contigs of one buffer at base offsets 0 .. 3 - l - 1 bases, l
    bases, about three tiles of two-block lanes, a few hundred windows."""
    k = plan_k(K_MAIN, w, canonical)
    l = k + w - 1
    lens = [l - 1, l, 3 * LANES * 2 * w + l + 5, l + 300]
    starts, pos = [], 0
    for i, x in enumerate(lens):
        pos += (i - pos) % 4          # contig i begins at a base with start % 4 == i
        starts.append(pos)
        pos += x
    assert [s % 4 for s in starts] == [0, 1, 2, 3]
    codes = tie_heavy_codes(pos, 9300 + w)
    data = pack_at(codes)
    res = [oracle.run(data, x, k, w, canonical=canonical, base_offset=s, super_kmers=True) for x, s in zip(lens, starts)]
    want, wsk = [r[0] for r in res], [r[1] for r in res]
    tot = sum(len(x) for x in want)
    assert len(want[0]) == 0 and len(want[1]) == 1 and tot > 1000
    big = torch.from_numpy(data).cuda()
    d = [big[s // 4:] for s in starts]
    out = torch.full((tot + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    osk = torch.full((tot + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    what = dict(w=w, k=k, canonical=canonical, batch=True)
    gpu.set_blocks_per_lane(2)
    try:
        offs = sm.run_batch_device(sm.Builder(k, w, canonical, 0), d, lens, out[:tot], osk[:tot], base_offsets=[s % 4 for s in starts])
    finally:
        gpu.set_blocks_per_lane(0)
    assert gpu.last_path() == sm.PATH_FUSED, what
    assert offs[-1] == tot and int(out[tot].item()) == SENTINEL and int(osk[tot].item()) == SENTINEL, what
    _check_reads(_u32(out, tot), np.array(offs, dtype=np.uint64), tot, want, _u32(osk, tot), wsk, what)


def _reads_fixed_stride(sm, oracle, gpu, torch, w, canonical, rng):
    """300 reads at a stride that is no multiple of 4, read_lens between 0 and read_len: minimizers, minimizers with
    super-k-mer indices, closed syncmers."""
    k = plan_k(K_MAIN, w, canonical)
    l = k + w - 1
    n_reads, base = 300, 3
    read_len = l + int(rng.integers(150, 401))
    stride = read_len + 5
    stride += 1 if stride % 4 == 0 else 0
    assert stride % 4 != 0
    span = (n_reads - 1) * stride + read_len
    data = pack_at(tie_heavy_codes(span, 9400 + w), base)
    lens = rng.integers(0, read_len + 1, size=n_reads)
    lens[:4] = [0, l - 1, l, read_len]
    d = torch.from_numpy(data).cuda()
    d_lens = torch.from_numpy(lens.astype(np.int32)).cuda()
    cap = n_reads * read_len
    for mode, sk in ((0, False), (0, True), (1, False)):
        what = dict(w=w, k=k, canonical=canonical, mode=mode, sk=sk, reads=True)
        res = [oracle.run(data, int(lens[r]), k, w, canonical=canonical, mode=mode, base_offset=base + r * stride,
                          super_kmers=sk) for r in range(n_reads)]
        want = [x[0] for x in res] if sk else res
        wsk = [x[1] for x in res] if sk else None
        out = torch.full((cap + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        osk = torch.full((cap + 8,), SENTINEL, dtype=torch.int32, device="cuda") if sk else None
        offs = torch.full((n_reads + 1,), SENTINEL, dtype=torch.int64, device="cuda")
        tot = sm.run_reads_device(sm.Builder(k, w, canonical, mode), d, n_reads, stride, read_len, out[:cap], offs,
                                  read_lens=d_lens, base_offset=base, out_sk=osk[:cap] if sk else None)
        assert gpu.last_path() == sm.PATH_FUSED, what
        assert tot == sum(len(x) for x in want) > 200 and int(out[tot].item()) == SENTINEL, (what, tot)
        _check_reads(_u32(out, tot), offs.cpu().numpy(), tot, want, _u32(osk, tot) if sk else None, wsk, what)


def _lane_table(sm, oracle, gpu, torch, w, canonical, rng):
    """mm_run_packed_reads_device on 40 reads back to back: none, l - 1, l, l + 1 bases, around ten windows' worth, several
    lanes long (the lengths of tests/test_gpu_round6.py::test_lane_table_reads_of_any_lengths in units of l)."""
    k = plan_k(K_MAIN, w, canonical)
    l = k + w - 1
    lens = [0, l - 1, l, l + 1, 10 * l - 2, 10 * l - 1, 11 * l, 60 * l + 1] + [int(x) for x in rng.integers(0, 12 * l, size=32)]
    starts = np.zeros(len(lens) + 1, dtype=np.uint64)
    starts[1:] = np.cumsum(lens, dtype=np.uint64)
    total = int(starts[-1])
    plan6 = (C.c_uint64 * 6)()
    assert sm.lib().mm_debug_lane_plan(k, w, int(canonical), 0, len(lens), total, 0, plan6) == 0
    assert max(lens) - l + 1 > 2 * int(plan6[1]), (w, max(lens), int(plan6[1]))   # the longest read spans several lanes
    data = pack_at(tie_heavy_codes(total, 9500 + w))
    want = [oracle.run(data, x, k, w, canonical=canonical, base_offset=int(s)) for x, s in zip(lens, starts[:-1])]
    tot_want = sum(len(x) for x in want)
    d, _keep = _device_seq(torch, data, 0, total, 1)
    recs = sm.FastaRecords(d, starts, None)
    out = torch.full((tot_want + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    offs = torch.full((len(lens) + 1,), SENTINEL, dtype=torch.int64, device="cuda")
    what = dict(w=w, k=k, canonical=canonical, lane_table=True)
    tot = sm.run_packed_reads_device(sm.Builder(k, w, canonical, 0), recs, out[:tot_want], offs)
    assert gpu.last_lane_table() and gpu.last_path() == sm.PATH_FUSED, what
    assert tot == tot_want > 100 and int(out[tot].item()) == SENTINEL, (what, tot, tot_want)
    _check_reads(_u32(out, tot), offs.cpu().numpy(), tot, want, what=what)


def _n_mask(rng, n, l):
    """Isolated Ns every few thousand bases, a run longer than l, a short run, and one in the last window."""
    isn = np.zeros(n, dtype=bool)
    isn[rng.integers(0, n, size=max(3, n // 3000))] = True
    s = n // 3
    isn[s: s + l + 9] = True
    isn[2 * n // 3: 2 * n // 3 + 3] = True
    isn[n - 2] = True
    return isn


def _amb_bits(isn, amb_offset):
    bits = np.concatenate([np.zeros(amb_offset, dtype=bool), isn])
    return np.concatenate([np.packbits(bits, bitorder="little"), np.zeros(16, dtype=np.uint8)])


def _skip_ambiguous_sequence(sm, oracle, gpu, torch, w, rng):
    """mm_run_skip_ambiguous_device, canonical minimizers and closed syncmers, at base and bit offsets 0 and 3; where the
    window bits arrive in chunks (ambi_rows), lanes one block shorter than a chunk, equal to it and one block longer."""
    k = plan_k(K_MAIN, w, True)
    l = k + w - 1
    n = l + 100_000
    codes = jw.tie_input(w, k, 100_000)
    isn = _n_mask(rng, n, l)
    t = sm.walk_traits(w, True, 0, False, False, True)
    lanes = [0]
    if t["ambi_rows"]:
        per_chunk = (32 * t["amb_row_dwords"] - 31) // w
        assert per_chunk >= 2
        lanes += [per_chunk - 1, per_chunk, per_chunk + 1]
    try:
        for base_offset, amb_offset in ((0, 0), (3, 3), (3, 0)):
            data, amb = pack_at(codes, base_offset), _amb_bits(isn, amb_offset)
            d, _keep = _device_seq(torch, data, base_offset, n, 2)
            d_m = torch.from_numpy(amb).cuda()
            for mode in (0, 1):
                want = oracle.run_skip_ambiguous(data, amb, n, k, w, mode=mode, base_offset=base_offset, amb_offset=amb_offset)
                plain = oracle.run(data, n, k, w, canonical=True, mode=mode, base_offset=base_offset)
                assert len(want) > 500 and len(want) < len(plain)
                out = torch.full((len(want) + 8,), SENTINEL, dtype=torch.int32, device="cuda")
                b = sm.Builder(k, w, True, mode)
                for nb in (lanes if mode == 0 and base_offset == amb_offset else [0]):
                    what = dict(w=w, k=k, mode=mode, base_offset=base_offset, amb_offset=amb_offset, nblk=nb)
                    gpu.set_blocks_per_lane(nb)
                    out.fill_(SENTINEL)
                    cnt = b.run_skip_ambiguous_device(d, d_m, n, out, base_offset=base_offset, amb_offset=amb_offset)
                    assert gpu.last_path() == sm.PATH_FUSED, what
                    assert cnt == len(want), (what, cnt, len(want))
                    got = _u32(out, cnt)
                    bad = np.flatnonzero(got != want)
                    assert len(bad) == 0, (what, bad[:4], got[bad[:4]], want[bad[:4]])
                    assert int(out[cnt].item()) == SENTINEL, what
    finally:
        gpu.set_blocks_per_lane(0)


def _skip_ambiguous_reads(sm, oracle, gpu, torch, w, rng):
    """mm_run_reads_device with ambiguity bits on 300 reads, an N about every 150 bases
    (tests/test_gpu_round5.py::test_skip_ambiguous_chunked_window_bits is the model)."""
    k = plan_k(K_MAIN, w, True)
    l = k + w - 1
    n_reads, off = 300, 1
    read_len = l + 250
    stride = read_len + 1 + (1 if (read_len + 1) % 4 == 0 else 0)
    span = n_reads * stride + 64 + off
    a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=span)].copy()
    a[rng.integers(0, span, size=span // 150)] = ord("N")
    packed, amb = oracle.pack_ascii_n(a.tobytes())
    d_p, d_m = torch.from_numpy(packed).cuda(), torch.from_numpy(amb).cuda()
    out = torch.full((n_reads * read_len + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    offs = torch.zeros(n_reads + 1, dtype=torch.int64, device="cuda")
    want = [oracle.run_skip_ambiguous(packed, amb, read_len, k, w, base_offset=off + r * stride, amb_offset=off + r * stride)
            for r in range(n_reads)]
    tot = sm.run_reads_device(sm.Builder(k, w, True, 0), d_p, n_reads, stride, read_len, out[:n_reads * read_len], offs,
                              base_offset=off, d_amb=d_m, amb_offset=off)
    what = dict(w=w, k=k, skip_reads=True)
    assert gpu.last_path() == sm.PATH_FUSED, what
    assert tot == sum(len(x) for x in want) > 50 and int(out[tot].item()) == SENTINEL, (what, tot)
    _check_reads(_u32(out, tot), offs.cpu().numpy(), tot, want, what=what)


@pytest.mark.parametrize("w", REPS)
def test_flavours(sm, oracle, gpu, ahead, w):
    """Strand by the position of w in REPS (forward at even positions, canonical at odd ones; the skip-ambiguous calls are
    canonical), k from plan_k(21, ...), every record against the oracle."""
    import torch
    assert w in _all()
    canonical = REPS.index(w) % 2 == 1
    rng = np.random.default_rng(9200 + w)
    before = sm.jit_stats()
    ahead("test_flavours", w)
    _sequence_family(sm, oracle, gpu, torch, w, canonical, rng)
    _batch(sm, oracle, gpu, torch, w, canonical, rng)
    _reads_fixed_stride(sm, oracle, gpu, torch, w, canonical, rng)
    _lane_table(sm, oracle, gpu, torch, w, canonical, rng)
    _skip_ambiguous_sequence(sm, oracle, gpu, torch, w, rng)
    _skip_ambiguous_reads(sm, oracle, gpu, torch, w, rng)
    assert sm.jit_stats()["failed"] == before["failed"]
