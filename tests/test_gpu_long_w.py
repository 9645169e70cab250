"""w above 128 and runs past 2^24 windows: the generic family as the product, on every GPU entry point, against the
oracle's streaming flavour (exact equality everywhere; tests/test_long_w_cpu.py pins that flavour first).

The fused kernels and their run-time specialisation stop at w = 128 (kJitMaxW); a plan is valid for any w below 2^15.  For
w = 129 .. 32767 the three kernels of mm_generic.hip (hash, per-window argmin and vote, ordered compaction) are the only
path: single sequences run them in rounds of 2^24 windows, batches fall to one launch per sequence, reads to one launch per
read with the totals appended, the host entry points stage or pipeline around that, and the skip-ambiguous calls feed it
window_ambiguity_kernel's l >= 32 branch.  tests/test_gpu_long_k.py is the model; this is its counterpart for w and for
rounds.  Nothing here may compile a kernel: the module asserts that."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_long_k import _device_seq
from test_long_w_cpu import K_BASE, W_LONG, feasible, pack_at, plan_k, tie_heavy_codes

pytestmark = pytest.mark.gpu

SENTINEL = -7
OFFSETS = [0, 1, 2, 3, 17]
ROUND = 1 << 24          # windows of one round of the generic family (mm_api.hip)
WIN_BLOCK = 256          # windows of one block of generic_window_kernel
COMPACT_BLOCK = 256 * 16  # windows of one block of generic_compact_kernel
HASH_BLOCK = 256 * 64    # k-mers of one block of generic_hash_kernel
U8P, U32P, U64P = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


@pytest.fixture(scope="module", autouse=True)
def _nothing_compiled(sm, gpu):
    """No window size of this module has a fused kernel, prebuilt or compiled: the run-time compiler stays idle."""
    before = sm.jit_stats()
    yield
    after = sm.jit_stats()
    assert after["compiled"] - before["compiled"] == 0, (before, after)


def _u32(t, n):
    return t[:n].cpu().numpy().view(np.uint32)


def _p(a, t):
    return a.ctypes.data_as(t)


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _by_window(want, win, a, e):
    """The outputs of windows [a, e): `win` holds the window every output belongs to."""
    return want[(win >= a) & (win < e)]


def _plant_open_syncmer(oracle, k, w, canonical):
    """A block of l + 200 bases that holds an open syncmer whatever surrounds it: a homopolymer (every k-mer ties) with a
    short insert whose k-mers include one strict minimum of the upper 16 hash bits; the window that has it in the middle
    lies inside the block.  Found by asking the oracle about the candidates."""
    l = k + w - 1
    for h in range(4):
        for ins in ([a] for a in range(4)), ([a, b] for a in range(4) for b in range(4)):
            for x in ins:
                if all(v == h for v in x):
                    continue
                block = np.full(l + 200, h, dtype=np.uint8)
                block[w // 2 + 100: w // 2 + 100 + len(x)] = x
                if len(oracle.run(pack_at(block), len(block), k, w, canonical=canonical, mode=2)):
                    return block
    raise AssertionError(("no open syncmer could be planted", k, w, canonical))


# ------------------------------------------------------------------------------------------ 1. single sequences
def _small_kinds():
    """name -> length as a function of l and w (None: no such length for this w)."""
    kinds = {"0": lambda l, w: 0, "l-1": lambda l, w: l - 1, "l": lambda l, w: l, "l+1": lambda l, w: l + 1,
             "l+31": lambda l, w: l + 31}
    for nw in (WIN_BLOCK - 1, WIN_BLOCK, WIN_BLOCK + 1, COMPACT_BLOCK - 1, COMPACT_BLOCK, COMPACT_BLOCK + 1,
               2 * COMPACT_BLOCK + 1):
        kinds[f"nw={nw}"] = lambda l, w, nw=nw: l - 1 + nw
    for t in (HASH_BLOCK - 1, HASH_BLOCK, HASH_BLOCK + 1):  # (the k-mers of a run: its windows + w - 1, one more at a seam)
        kinds[f"nw+w={t}"] = lambda l, w, t=t: l - 1 + t - w if t > w else None
    return kinds


def _draw_cases(canonical, seed, per_combo=2):
    """A seeded sample as tests/test_gpu_long_k.py::_draw_cases deals it: every w of W_LONG x mode per_combo times on this
    strand, k from K_BASE, the length kinds, base offsets and pointer shifts in rotation so that each occurs."""
    rng = np.random.default_rng(seed)
    kinds = _small_kinds()
    combos = [(w, mode) for _ in range(per_combo) for w in W_LONG for mode in (0, 1, 2) if mode != 2 or w % 2]

    def deal(values):
        reps = -(-len(combos) // len(values))
        return [values[j] for j in rng.permutation(np.repeat(np.arange(len(values)), reps))[:len(combos)]]
    names, offs, shifts, ks = deal(list(kinds)), deal(OFFSETS), deal([0, 1, 2, 3]), deal(K_BASE)
    order = list(kinds)
    cases = []
    for i, (w, mode) in enumerate(combos):
        k = plan_k(ks[i], w, canonical)
        assert feasible(k, w, canonical, mode)
        l = k + w - 1
        name = names[i]
        while kinds[name](l, w) is None:  # (w = 32767 is longer than a block of the hash kernel: the next kind instead)
            name = order[(order.index(name) + 1) % len(order)]
        cases.append(dict(k=k, w=w, mode=mode, sk=mode == 0 and i % 2 == 0, kind=name, n=kinds[name](l, w), off=offs[i],
                          shift=shifts[i], ties=i % 3 == 1))
    return cases


def _input(oracle, rng, c):
    """Random bases from the oracle's generator, or the tie-heavy variant; `off` bases in front."""
    n, off = c["n"], c["off"]
    if c["ties"]:
        return pack_at(tie_heavy_codes(n, int(rng.integers(1 << 30))), off)
    return oracle.gen_packed(int(rng.integers(1 << 30)), off + n + 64)


def _run_whole(sm, oracle, gpu, torch, canonical, c, data):
    """One run of the whole sequence: count, every position, the element behind the count, indices; returns the reference
    (positions, the window of every output, indices or None) and what the ranges below need."""
    k, w, mode, n, off = c["k"], c["w"], c["mode"], c["n"], c["off"]
    l = k + w - 1
    nw = max(0, n - l + 1)
    d, keep = _device_seq(torch, data, off, n, c["shift"])
    b = sm.Builder(k, w, canonical, mode)
    out = torch.full((nw + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    sk = torch.full((nw + 8,), SENTINEL, dtype=torch.int32, device="cuda") if c["sk"] else None
    if mode == 0:
        want, win = oracle.run(data, n, k, w, canonical=canonical, mode=mode, base_offset=off, super_kmers=True)
    else:
        want = oracle.run(data, n, k, w, canonical=canonical, mode=mode, base_offset=off)
        win = want
    cnt = b.run_device(d, n, out, out_sk=sk, base_offset=off)
    assert nw == 0 or gpu.last_path() == sm.PATH_GENERIC, c
    assert cnt == len(want), (c, cnt, len(want))
    assert np.array_equal(_u32(out, cnt), want), c
    assert int(out[cnt].item()) == SENTINEL, c
    if c["sk"]:
        assert np.array_equal(_u32(sk, cnt), win), c
        assert int(sk[cnt].item()) == SENTINEL, c
    return b, d, keep, out, sk, want, win, nw


def _run_range(b, d, c, out, sk, want, win, a, e):
    out.fill_(SENTINEL)
    cc = b.run_device(d, c["n"], out, out_sk=sk, base_offset=c["off"], win_begin=a, win_end=e)
    sub = _by_window(want, win, a, e)
    assert cc == len(sub) and np.array_equal(_u32(out, cc), sub), (c, a, e, cc, len(sub))
    assert int(out[cc].item()) == SENTINEL, (c, a, e)
    if sk is not None:
        assert np.array_equal(_u32(sk, cc), _by_window(win, win, a, e)), (c, a, e)
    return _u32(out, cc).copy()


@pytest.mark.parametrize("canonical", [False, True])
def test_single_sequence_long_w(sm, oracle, gpu, canonical):
    """mm_run_device at the small lengths: none, one window, around one block of each of the three kernels."""
    import torch
    cases = _draw_cases(canonical, 5100 + canonical)
    assert {(c["w"], c["mode"]) for c in cases} == {(w, m) for w in W_LONG for m in (0, 1, 2) if m != 2 or w % 2}
    kinds = set(_small_kinds())
    assert {c["kind"] for c in cases} == kinds, kinds - {c["kind"] for c in cases}
    assert {c["off"] for c in cases} == set(OFFSETS) and {c["shift"] for c in cases} == {0, 1, 2, 3}
    assert any(c["sk"] for c in cases) and any(c["mode"] == 0 and not c["sk"] for c in cases)
    assert any(c["ties"] for c in cases) and not all(c["ties"] for c in cases)
    assert (len({c["k"] for c in cases}) >= 4 if canonical else {c["k"] for c in cases} == set(K_BASE)) and len(cases) == 42
    rng = np.random.default_rng(5200 + canonical)
    positions = 0
    for c in cases:
        want = _run_whole(sm, oracle, gpu, torch, canonical, c, _input(oracle, rng, c))[5]
        positions += len(want)
    print("long w single", canonical, dict(cases=len(cases), positions=positions))
    assert positions > 5_000


MAIN = [(w, mode) for w in W_LONG for mode in (0, 1, 2) if mode != 2 or w % 2]


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("w,mode", MAIN)
def test_main_length_long_w(sm, oracle, gpu, w, mode, canonical):
    """n = l + 150 000 on the tie-heavy input: the whole run, three window-range shards at random cuts that concatenate to
    it, and ranges of one window.  Floors on the reference alone: 1 000 minimizers or closed syncmers; open syncmers are
    sparse by nature (a few hundred at w = 129, a handful at w = 32767), so at least one - and one planted within a block
    of the compaction (4 096 windows) of either end."""
    import torch
    i = MAIN.index((w, mode)) + len(MAIN) * canonical
    rng = np.random.default_rng(5300 + i)
    # (w = 32767: random-like input at k = 21 selects about ten positions in 150 000 windows; k = 1 on the ties does)
    k = plan_k(1 if w == 32767 else K_BASE[i % 4], w, canonical)
    l = k + w - 1
    n = l + 150_000
    c = dict(k=k, w=w, mode=mode, sk=mode == 0 and i % 2 == 0, n=n, off=OFFSETS[i % 5], shift=i % 4)
    codes = tie_heavy_codes(n, 5400 + i)
    if mode == 2:
        block = _plant_open_syncmer(oracle, k, w, canonical)
        codes[:len(block)] = block
        codes[n - len(block):] = block
    data = pack_at(codes, c["off"])
    b, d, _keep, out, sk, want, win, nw = _run_whole(sm, oracle, gpu, torch, canonical, c, data)
    assert nw == 150_001
    if mode == 2:
        assert len(want) >= 1 and want[0] < COMPACT_BLOCK and want[-1] >= nw - COMPACT_BLOCK, (c, want[:3], want[-3:])
    else:
        assert len(want) >= 1000, (c, len(want))
    cuts = [0] + sorted(int(x) for x in rng.integers(1, nw, size=2)) + [nw]
    parts = [_run_range(b, d, c, out, sk, want, win, a, e) for a, e in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(parts), want), (c, cuts)
    # one window that selects and the one behind it; the first and the last window of the sequence
    hit = int(win[len(win) // 2])
    assert len(_run_range(b, d, c, out, sk, want, win, hit, hit + 1)) == 1
    for a in (hit + 1, 0, nw - 1):
        _run_range(b, d, c, out, sk, want, win, a, a + 1)
    print("long w main", dict(c, canonical=canonical, outputs=len(want)))


# ------------------------------------------------------------------------------------------ 2. more than one round
NW2 = ROUND + COMPACT_BLOCK + 1
SEED2 = 1  # (chosen so that every flavour below selects within w windows of window 2^24 on both sides: asserted)
FLAVOURS = {
    # name: (k, w, canonical, mode, indices, forced, base offset)
    "canonical minimizers k21 w11 sk": (21, 11, True, 0, True, True, 1),
    "closed syncmers k15 w17": (15, 17, False, 1, False, True, 2),
    "canonical open syncmers k5 w7": (5, 7, True, 2, False, True, 3),
    "minimizers k21 w129 sk": (21, 129, False, 0, True, False, 0),
}


@pytest.fixture(scope="module")
def two_rounds(oracle):
    """16.8 Mbases from the oracle's generator, shared by the flavours and left unchanged."""
    data = oracle.gen_packed(SEED2, NW2 + 160 + 64)
    return data


def _both_sides(win, w, lo=ROUND, hi=ROUND):
    """The reference selects within w windows in front of window `lo` and within w windows from window `hi` on."""
    return bool(np.any((win >= lo - w) & (win < lo))) and bool(np.any((win >= hi) & (win < hi + w)))


@pytest.mark.parametrize("name", list(FLAVOURS))
def test_more_than_one_round(sm, oracle, gpu, two_rounds, name):
    """2^24 + 4097 windows: a second round with the DNA stages - the extra window in front of it, win_first against
    win_begin in the compaction, block 0's carry from the running total, the per-round reset of status words and ticket,
    indices across the seam."""
    import torch
    k, w, canonical, mode, sk_wanted, forced, off = FLAVOURS[name]
    l = k + w - 1
    n = NW2 + l - 1
    data = two_rounds
    if mode == 0:
        want, win = oracle.run(data, n, k, w, canonical=canonical, mode=mode, base_offset=off, super_kmers=True)
    else:
        want = oracle.run(data, n, k, w, canonical=canonical, mode=mode, base_offset=off)
        win = want
    assert _both_sides(win, w), (name, win[np.searchsorted(win, ROUND) - 2: np.searchsorted(win, ROUND) + 2])
    d, _keep = _device_seq(torch, data, off, n, off)
    out = torch.full((len(want) + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    sk = torch.full((len(want) + 8,), SENTINEL, dtype=torch.int32, device="cuda") if sk_wanted else None
    b = sm.Builder(k, w, canonical, mode)
    c = dict(n=n, off=off, name=name)
    gpu.force_generic(forced)
    try:
        cnt = b.run_device(d, n, out, out_sk=sk, base_offset=off)
        assert gpu.last_path() == sm.PATH_GENERIC
        assert cnt == len(want), (name, cnt, len(want))
        got = _u32(out, cnt)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (name, bad[:4], got[bad[:4]], want[bad[:4]])
        assert int(out[cnt].item()) == SENTINEL
        if sk is not None:
            assert np.array_equal(_u32(sk, cnt), win), name
            assert int(sk[cnt].item()) == SENTINEL
        if name == "canonical minimizers k21 w11 sk":
            first = _run_range(b, d, c, out, sk, want, win, 0, ROUND)
            second = _run_range(b, d, c, out, sk, want, win, ROUND, NW2)
            assert np.array_equal(np.concatenate([first, second]), want)
            _run_range(b, d, c, out, sk, want, win, 5, NW2)  # (its seam is at window 2^24 + 5)
            _run_range(b, d, c, out, sk, want, win, ROUND - 1, ROUND + 1)
            assert _both_sides(win, w, ROUND + 5, ROUND + 5)
    finally:
        gpu.force_generic(False)


def test_more_than_one_round_skip_ambiguous(sm, oracle, gpu, two_rounds):
    """Skip-ambiguous canonical minimizers k = 21, w = 11 over the seam: wamb[i >> 5] indexed by absolute window in the
    second round.  An N run makes windows 2^24 - 5 .. 2^24 + 40 skipped (the last window of the first round, the extra
    window in front of the second and its first forty); isolated Ns every few thousand bases; one N in the last window.
    The reference selects within w windows in front of the skipped stretch and within w windows behind it."""
    import torch
    k, w = 21, 11
    l = k + w - 1
    n = NW2 + l - 1
    isn = np.zeros(n, dtype=bool)
    isn[ROUND - 5 + l - 1: ROUND + 40 + 1] = True   # windows i with i <= p <= i + l - 1 for a p of the run
    rng = np.random.default_rng(5500)
    isn[rng.integers(0, n, size=n // 3000)] = True
    isn[n - 3] = True
    amb = np.concatenate([np.packbits(isn, bitorder="little"), np.zeros(16, dtype=np.uint8)])
    data = two_rounds
    stream = oracle.window_positions_skip_ambiguous(data, amb, n, k, w)
    assert len(stream) == NW2 and stream[-1] == oracle.SKIPPED
    dirty = stream == oracle.SKIPPED
    assert dirty[ROUND - 5: ROUND + 41].all() and not dirty[ROUND - 6] and not dirty[ROUND + 41]
    emit = ~dirty & np.concatenate([[True], stream[1:] != stream[:-1]])
    win = np.flatnonzero(emit)
    want = oracle.run_skip_ambiguous(data, amb, n, k, w)
    assert np.array_equal(want, stream[emit])
    assert _both_sides(win, w, ROUND - 5, ROUND + 41)
    d, _keep = _device_seq(torch, data, 0, n, 2)
    d_m = torch.from_numpy(amb).cuda()
    out = torch.full((len(want) + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    b = sm.canonical_minimizers(k, w)
    gpu.force_generic(True)
    try:
        cnt = b.run_skip_ambiguous_device(d, d_m, n, out)
        assert gpu.last_path() == sm.PATH_GENERIC
        assert cnt == len(want), (cnt, len(want))
        got = _u32(out, cnt)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (bad[:4], got[bad[:4]], want[bad[:4]])
        assert int(out[cnt].item()) == SENTINEL
        parts = []
        for a, e in ((0, ROUND), (ROUND, NW2)):
            out.fill_(SENTINEL)
            cc = b.run_skip_ambiguous_device(d, d_m, n, out, win_begin=a, win_end=e)
            sub = _by_window(want, win, a, e)
            assert cc == len(sub) and np.array_equal(_u32(out, cc), sub), (a, e)
            parts.append(sub)
        assert np.array_equal(np.concatenate(parts), want)
    finally:
        gpu.force_generic(False)


# ------------------------------------------------------------------------------------------ 3. reads and batches
READ_W = {129: 21, 257: 31, 1000: 65}  # w: k (moved by one for a canonical plan where l would be even)


def _prime_lane_table(sm, oracle, gpu, torch):
    """One lane-table launch of a fused reads-mode kernel, so that the flag the runs below must clear is set."""
    n_reads, read_len = 6, 6000
    data = oracle.gen_packed(77, n_reads * read_len + 64)
    d = torch.from_numpy(data).cuda()
    out = torch.zeros(n_reads * read_len, dtype=torch.int32, device="cuda")
    offs = torch.zeros(n_reads + 1, dtype=torch.int64, device="cuda")
    sm.run_reads_device(sm.minimizers(21, 11), d, n_reads, read_len, read_len, out, offs)
    assert gpu.last_path() == sm.PATH_FUSED and gpu.last_lane_table()


def _read_lengths(rng, l):
    """About 40 reads from the menu, shuffled; a zero-length read first, one last and two in a row."""
    menu = [0, 1, l - 1, l, l + 1, l + 300, 3 * l]
    lens = [int(x) for x in rng.permutation(menu * 5)]
    return [0] + lens + [0, 0, l + 300, 0]


def _reads_floor(mode, lens, l):
    """What the reference must give at least: a read with a window selects one minimizer or more; a closed syncmer is not
    certain in any one read (2 / w of the windows: w = 1000 leaves a dozen in forty reads), open ones are rarer still."""
    return sum(x >= l for x in lens) if mode == 0 else (1 if mode == 1 else 0)


def _flavours(w):
    return [(False, 0), (True, 0), (True, 1)] + ([(False, 2)] if w % 2 else [(False, 1)])


def _check_reads(hp, ho, tot, want, hs=None, wsk=None, what=None):
    """Offsets whole (first 0, last the total, non-decreasing) and every read against the oracle."""
    assert ho[0] == 0 and ho[-1] == tot and np.all(np.diff(ho.astype(np.int64)) >= 0), what
    assert len(ho) == len(want) + 1
    for r, wr in enumerate(want):
        assert np.array_equal(hp[ho[r]:ho[r + 1]], wr), (what, r, len(wr))
        if hs is not None:
            assert np.array_equal(hs[ho[r]:ho[r + 1]], wsk[r]), (what, r)


def _generic_reads_run(sm, gpu, what):
    assert gpu.last_path() == sm.PATH_GENERIC and not gpu.last_lane_table(), what
    assert sm.lib().mm_workspace_last_lane_table(gpu.h) == 0, what


@pytest.mark.parametrize("w", list(READ_W))
def test_reads_fixed_stride_long_w(sm, oracle, gpu, w):
    """mm_run_reads_device (with and without d_read_lens, base offset 3, a read_len that cuts the longest reads),
    mm_run_reads_superkmers_device and mm_run_reads_skip_ambiguous_device: the host loop that runs one read per launch
    and appends."""
    import torch
    rng = np.random.default_rng(5600 + w)
    total_checked = 0
    for canonical, mode in _flavours(w):
        k = plan_k(READ_W[w], w, canonical)
        l = k + w - 1
        lens = _read_lengths(rng, l)
        n_reads = len(lens)
        stride, base, read_len = 3 * l + 7, 3, 2 * l + 5
        span = (n_reads - 1) * stride + read_len
        codes = rng.integers(0, 4, size=span).astype(np.uint8)
        # Ns in every third read that has a window, nowhere else (the skip-ambiguous run; the codes stay what they are)
        isn = np.zeros(span, dtype=bool)
        with_n = [r for r in range(n_reads) if lens[r] >= l and (r % 3 == 0 or lens[r] == l)]
        for r in with_n:
            isn[r * stride + int(rng.integers(0, min(lens[r], read_len)))] = True
        data = pack_at(codes, base)
        d, _keep = _device_seq(torch, data, base, span, 1)
        b = sm.Builder(k, w, canonical, mode)
        cap = n_reads * read_len
        offs = torch.full((n_reads + 2,), SENTINEL, dtype=torch.int64, device="cuda")
        d_lens = torch.from_numpy(np.array(lens, dtype=np.int32)).cuda()
        for use_lens in (True, False):
            for sk in ((False, True) if mode == 0 else (False,)):
                what = dict(w=w, k=k, canonical=canonical, mode=mode, use_lens=use_lens, sk=sk)
                _prime_lane_table(sm, oracle, gpu, torch)
                m = [min(x, read_len) if use_lens else read_len for x in lens]
                res = [oracle.run(data, m[r], k, w, canonical=canonical, mode=mode, base_offset=base + r * stride,
                                  super_kmers=sk) for r in range(n_reads)]
                want = [x[0] for x in res] if sk else res
                wsk = [x[1] for x in res] if sk else None
                out = torch.full((cap + 8,), SENTINEL, dtype=torch.int32, device="cuda")
                osk = torch.full((cap + 8,), SENTINEL, dtype=torch.int32, device="cuda") if sk else None
                offs.fill_(SENTINEL)
                tot = sm.run_reads_device(b, d, n_reads, stride, read_len, out[:cap], offs[:n_reads + 1],
                                          read_lens=d_lens if use_lens else None, base_offset=base,
                                          out_sk=osk[:cap] if sk else None)
                _generic_reads_run(sm, gpu, what)
                assert tot == sum(len(x) for x in want) and tot >= _reads_floor(mode, m, l), (what, tot)
                ho = offs.cpu().numpy()
                assert ho[n_reads + 1] == SENTINEL and int(out[tot].item()) == SENTINEL, what
                _check_reads(_u32(out, tot), ho[:n_reads + 1], tot, want, _u32(osk, tot) if sk else None, wsk, what)
                assert osk is None or int(osk[tot].item()) == SENTINEL
                total_checked += n_reads
                if use_lens and not sk and tot > 0:
                    # a capacity one short of the total is refused; a correct run follows on the same workspace
                    with pytest.raises(sm.MinimizerError) as e:
                        sm.run_reads_device(b, d, n_reads, stride, read_len, out[:tot - 1], offs[:n_reads + 1],
                                            read_lens=d_lens, base_offset=base)
                    assert e.value.code == sm.ERR["CAPACITY"], what
                    assert int(out[tot].item()) == SENTINEL, what
                    out.fill_(SENTINEL)
                    again = sm.run_reads_device(b, d, n_reads, stride, read_len, out[:tot], offs[:n_reads + 1],
                                                read_lens=d_lens, base_offset=base)
                    assert again == tot and int(out[tot].item()) == SENTINEL
                    _check_reads(_u32(out, tot), offs.cpu().numpy()[:n_reads + 1], tot, want, what=what)
        if canonical:
            # skip-ambiguous: bit j of the span at bit amb_offset + j, another alignment than the bases'
            amb_offset = 5
            bits = np.concatenate([np.zeros(amb_offset, dtype=bool), isn])
            amb = np.concatenate([np.packbits(bits, bitorder="little"), np.zeros(16, dtype=np.uint8)])
            d_m = torch.from_numpy(amb).cuda()
            m = [min(x, read_len) for x in lens]
            want = [oracle.run_skip_ambiguous(data, amb, m[r], k, w, mode=mode, base_offset=base + r * stride,
                                              amb_offset=amb_offset + r * stride) for r in range(n_reads)]
            plain = [oracle.run(data, m[r], k, w, canonical=True, mode=mode, base_offset=base + r * stride)
                     for r in range(n_reads)]
            assert all(np.array_equal(want[r], plain[r]) for r in range(n_reads) if r not in with_n)
            # (a read of l bases with an N has its one window skipped, and a minimizer with it)
            assert mode != 0 or all(len(want[r]) == 0 and len(plain[r]) == 1 for r in with_n if lens[r] == l)
            _prime_lane_table(sm, oracle, gpu, torch)
            out = torch.full((cap + 8,), SENTINEL, dtype=torch.int32, device="cuda")
            offs.fill_(SENTINEL)
            tot = sm.run_reads_device(b, d, n_reads, stride, read_len, out[:cap], offs[:n_reads + 1], read_lens=d_lens,
                                      base_offset=base, d_amb=d_m, amb_offset=amb_offset)
            what = dict(w=w, k=k, mode=mode, skip=True)
            _generic_reads_run(sm, gpu, what)
            ho = offs.cpu().numpy()
            assert ho[n_reads + 1] == SENTINEL and int(out[tot].item()) == SENTINEL, what
            _check_reads(_u32(out, tot), ho[:n_reads + 1], tot, want, what=what)
            assert tot == sum(len(x) for x in want) >= _reads_floor(mode, [m[r] for r in range(n_reads) if r not in with_n], l)
    assert total_checked > 200


def _pack_reads(codes_list):
    lens = [len(x) for x in codes_list]
    starts = np.zeros(len(lens) + 1, dtype=np.uint64)
    starts[1:] = np.cumsum(lens, dtype=np.uint64)
    flat = np.concatenate(codes_list).astype(np.uint8)
    return pack_at(flat), starts, flat


@pytest.mark.parametrize("w", list(READ_W))
def test_packed_reads_long_w(sm, oracle, gpu, w):
    """mm_run_packed_reads_device, mm_run_packed_reads_host and mm_run_packed_reads_skip_ambiguous_host: reads back to
    back, zero-length reads first, last and two in a row, max_read_len below the longest read."""
    import torch
    rng = np.random.default_rng(5700 + w)
    L = sm.lib()
    for canonical, mode in _flavours(w):
        k = plan_k(READ_W[w], w, canonical)
        l = k + w - 1
        lens = _read_lengths(rng, l)
        assert lens[0] == 0 and lens[-1] == 0 and any(a == b == 0 for a, b in zip(lens, lens[1:]))
        n_reads = len(lens)
        mx = 2 * l + 5
        assert mx < max(lens)
        reads = [rng.integers(0, 4, size=x).astype(np.uint8) for x in lens]
        packed, starts, flat = _pack_reads(reads)
        total = int(starts[-1])
        sk = mode == 0
        res = [oracle.run(packed, min(lens[r], mx), k, w, canonical=canonical, mode=mode, base_offset=int(starts[r]),
                          super_kmers=sk) for r in range(n_reads)]
        want = [x[0] for x in res] if sk else res
        wsk = [x[1] for x in res] if sk else None
        tot_want = sum(len(x) for x in want)
        assert tot_want >= _reads_floor(mode, lens, l)
        b = sm.Builder(k, w, canonical, mode)
        what = dict(w=w, k=k, canonical=canonical, mode=mode)
        # ---- device
        d, _keep = _device_seq(torch, packed, 0, total, 3)
        recs = sm.FastaRecords(d, starts, None)
        out = torch.full((tot_want + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        osk = torch.full((tot_want + 8,), SENTINEL, dtype=torch.int32, device="cuda") if sk else None
        offs = torch.full((n_reads + 2,), SENTINEL, dtype=torch.int64, device="cuda")
        _prime_lane_table(sm, oracle, gpu, torch)
        tot = sm.run_packed_reads_device(b, recs, out[:tot_want], offs[:n_reads + 1], out_sk=osk[:tot_want] if sk else None,
                                         max_read_len=mx)
        _generic_reads_run(sm, gpu, what)
        ho = offs.cpu().numpy()
        assert tot == tot_want and ho[n_reads + 1] == SENTINEL and int(out[tot].item()) == SENTINEL, what
        _check_reads(_u32(out, tot), ho[:n_reads + 1], tot, want, _u32(osk, tot) if sk else None, wsk, what)
        with pytest.raises(sm.MinimizerError) as e:
            sm.run_packed_reads_device(b, recs, out[:tot_want - 1], offs[:n_reads + 1], max_read_len=mx)
        assert e.value.code == sm.ERR["CAPACITY"], what
        out.fill_(SENTINEL)
        assert sm.run_packed_reads_device(b, recs, out[:tot_want], offs[:n_reads + 1], max_read_len=mx) == tot_want
        _check_reads(_u32(out, tot), offs.cpu().numpy()[:n_reads + 1], tot, want, what=what)
        # ---- host
        host = np.ascontiguousarray(packed[: (total + 3) // 4])
        pos = np.full(tot_want + 8, 0xFFFFFFF9, dtype=np.uint32)
        psk = np.full(tot_want + 8, 0xFFFFFFF9, dtype=np.uint32) if sk else None
        hoffs = np.full(n_reads + 2, 0xFFFFFFF9, dtype=np.uint64)
        cnt = C.c_uint64()
        _prime_lane_table(sm, oracle, gpu, torch)
        sm._check(L.mm_run_packed_reads_host(b.plan().h, gpu.h, _p(host, U8P), n_reads, _p(starts, U64P), mx, _p(pos, U32P),
                                             _p(psk, U32P) if sk else None, tot_want, _p(hoffs, U64P), C.byref(cnt)))
        _generic_reads_run(sm, gpu, dict(what, host=True))
        assert cnt.value == tot_want and pos[tot_want] == 0xFFFFFFF9 and hoffs[n_reads + 1] == 0xFFFFFFF9, what
        _check_reads(pos[:tot_want], hoffs[:n_reads + 1], tot_want, want, psk[:tot_want] if sk else None, wsk, what)
        code = L.mm_run_packed_reads_host(b.plan().h, gpu.h, _p(host, U8P), n_reads, _p(starts, U64P), mx, _p(pos, U32P),
                                          None, tot_want - 1, _p(hoffs, U64P), C.byref(cnt))
        assert code == sm.ERR["CAPACITY"], (what, code)
        if canonical:
            # ---- host, skip-ambiguous: Ns in every third read that has a window
            isn = np.zeros(total, dtype=bool)
            with_n = [r for r in range(n_reads) if lens[r] >= l and (r % 3 == 0 or lens[r] == l)]
            for r in with_n:
                isn[int(starts[r]) + int(rng.integers(0, min(lens[r], mx)))] = True
            amb = np.concatenate([np.packbits(isn, bitorder="little"), np.zeros(16, dtype=np.uint8)])
            swant = [oracle.run_skip_ambiguous(packed, amb, min(lens[r], mx), k, w, mode=mode, base_offset=int(starts[r]),
                                               amb_offset=int(starts[r])) for r in range(n_reads)]
            assert all(np.array_equal(swant[r], want[r]) for r in range(n_reads) if r not in with_n)
            assert mode != 0 or all(len(swant[r]) == 0 and len(want[r]) == 1 for r in with_n if lens[r] == l)
            stot = sum(len(x) for x in swant)
            pos.fill(0xFFFFFFF9)
            hoffs.fill(0xFFFFFFF9)
            _prime_lane_table(sm, oracle, gpu, torch)
            sm._check(L.mm_run_packed_reads_skip_ambiguous_host(b.plan().h, gpu.h, _p(host, U8P), _p(amb, U8P), n_reads,
                                                                _p(starts, U64P), mx, _p(pos, U32P), stot, _p(hoffs, U64P),
                                                                C.byref(cnt)))
            _generic_reads_run(sm, gpu, dict(what, host=True, skip=True))
            assert cnt.value == stot and pos[stot] == 0xFFFFFFF9 and hoffs[n_reads + 1] == 0xFFFFFFF9, what
            _check_reads(pos[:stot], hoffs[:n_reads + 1], stot, swant, what=what)


@pytest.mark.parametrize("w", list(READ_W))
def test_batch_long_w(sm, oracle, gpu, w):
    """mm_run_batch_device with sequences in allocations of their own and odd base offsets, one of them shorter than l:
    one launch of the generic family per sequence."""
    import torch
    rng = np.random.default_rng(5800 + w)
    for canonical, mode in _flavours(w):
        k = plan_k(READ_W[w], w, canonical)
        l = k + w - 1
        lens = [l + 5000, l - 1, l, 3 * l + 1, 0, l + 20_011]
        offs_b = [1, 3, 5, 7, 2, 17]
        sk = mode == 0
        datas = [oracle.gen_packed(int(rng.integers(1 << 30)), o + n + 64) for n, o in zip(lens, offs_b)]
        res = [oracle.run(dd, n, k, w, canonical=canonical, mode=mode, base_offset=o, super_kmers=sk)
               for dd, n, o in zip(datas, lens, offs_b)]
        want = [x[0] for x in res] if sk else res
        wsk = [x[1] for x in res] if sk else None
        tot_want = sum(len(x) for x in want)
        assert tot_want >= _reads_floor(mode, lens, l)
        pairs = [_device_seq(torch, dd, o, n, i % 4) for i, (dd, n, o) in enumerate(zip(datas, lens, offs_b))]
        d = [p[0] for p in pairs]
        b = sm.Builder(k, w, canonical, mode)
        what = dict(w=w, k=k, canonical=canonical, mode=mode)
        out = torch.full((tot_want + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        osk = torch.full((tot_want + 8,), SENTINEL, dtype=torch.int32, device="cuda") if sk else None
        _prime_lane_table(sm, oracle, gpu, torch)
        offs = sm.run_batch_device(b, d, lens, out[:tot_want], osk[:tot_want] if sk else None, base_offsets=offs_b)
        _generic_reads_run(sm, gpu, what)
        assert len(offs) == len(lens) + 1 and offs[-1] == tot_want and int(out[tot_want].item()) == SENTINEL, what
        _check_reads(_u32(out, tot_want), np.array(offs, dtype=np.uint64), tot_want, want,
                     _u32(osk, tot_want) if sk else None, wsk, what)
        with pytest.raises(sm.MinimizerError) as e:
            sm.run_batch_device(b, d, lens, out[:tot_want - 1], None, base_offsets=offs_b)
        assert e.value.code == sm.ERR["CAPACITY"], what
        assert int(out[tot_want].item()) == SENTINEL
        out.fill_(SENTINEL)
        offs = sm.run_batch_device(b, d, lens, out[:tot_want], None, base_offsets=offs_b)
        _check_reads(_u32(out, tot_want), np.array(offs, dtype=np.uint64), tot_want, want, what=what)


# ------------------------------------------------------------------------------------------ 4. skip-ambiguous at long l
def _n_sites(n, l):
    """Bases that are N: for groups of 32 windows far apart (window 32 T is bit 0 of a word of window bits), an N at
    every edge of window_ambiguity_kernel's views - bit 0, 1 and 31 of the group's first 32 bases, the first bases all
    32 windows share (32, 33), the last one they share (l - 1), the bases behind it (l, l + 1, l + 31) and the first one
    outside the group (l + 32) - then a run longer than l, isolated Ns, base l - 1, base l and the last base."""
    isn = np.zeros(n, dtype=bool)
    gap = -(-3 * l // 32)
    t = gap
    for dlt in (0, 1, 31, 32, 33, l - 33, l - 32, l - 31, l - 1, l, l + 1, l + 31, l + 32):
        isn[32 * t + dlt] = True
        t += gap
    end = 32 * t + 2 * l
    isn[end: end + l + 9] = True
    return isn, end + 3 * l


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("w", [129, 257, 4097])
def test_skip_ambiguous_long_w(sm, oracle, gpu, w, mode):
    """mm_run_skip_ambiguous_device, canonical, with base_offset and amb_offset that differ, and window-range shards."""
    import torch
    k = plan_k(READ_W.get(w, 21), w, True)
    l = k + w - 1
    rng = np.random.default_rng(5900 + w + mode)
    isn, used = _n_sites(40 * l + 2 * l + 100_000, l)
    n = len(isn)
    isn[rng.integers(used, n, size=12)] = True
    isn[[l - 1, l, n - 1]] = True
    codes = tie_heavy_codes(n, 6000 + w)
    for base_offset, amb_offset in ((3, 13), (0, 7)):
        data = pack_at(codes, base_offset)
        bits = np.concatenate([np.zeros(amb_offset, dtype=bool), isn])
        amb = np.concatenate([np.packbits(bits, bitorder="little"), np.zeros(16, dtype=np.uint8)])
        stream = oracle.window_positions_skip_ambiguous(data, amb, n, k, w, base_offset=base_offset, amb_offset=amb_offset)
        nw = n - l + 1
        assert len(stream) == nw
        dirty = stream == oracle.SKIPPED
        i = np.arange(nw, dtype=np.int64)
        s = stream.astype(np.int64)
        if mode == 0:
            emit = ~dirty & np.concatenate([[True], s[1:] != s[:-1]])
        else:
            emit = ~dirty & ((s == i) | (s == i + w - 1))
        win = np.flatnonzero(emit)
        want = oracle.run_skip_ambiguous(data, amb, n, k, w, mode=mode, base_offset=base_offset, amb_offset=amb_offset)
        assert np.array_equal(want, stream[emit] if mode == 0 else win.astype(np.uint32))
        assert len(want) > 200 and 1000 < int(dirty.sum()) < nw - 1000, (len(want), int(dirty.sum()))
        d, _keep = _device_seq(torch, data, base_offset, n, (base_offset + 1) % 4)
        d_m = torch.from_numpy(amb).cuda()
        out = torch.full((len(want) + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        b = sm.Builder(k, w, True, mode)
        what = dict(w=w, k=k, mode=mode, base_offset=base_offset, amb_offset=amb_offset)
        cnt = b.run_skip_ambiguous_device(d, d_m, n, out, base_offset=base_offset, amb_offset=amb_offset)
        assert gpu.last_path() == sm.PATH_GENERIC, what
        got = _u32(out, cnt)
        assert cnt == len(want), (what, cnt, len(want))
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (what, bad[:4], got[bad[:4]], want[bad[:4]])
        assert int(out[cnt].item()) == SENTINEL, what
        cuts = [0] + sorted(int(x) for x in rng.integers(1, nw, size=2)) + [nw]
        parts = []
        for a, e in list(zip(cuts[:-1], cuts[1:])) + [(int(win[len(win) // 2]), int(win[len(win) // 2]) + 1)]:
            out.fill_(SENTINEL)
            cc = b.run_skip_ambiguous_device(d, d_m, n, out, base_offset=base_offset, amb_offset=amb_offset, win_begin=a,
                                             win_end=e)
            sub = _by_window(want, win, a, e)
            assert cc == len(sub) and np.array_equal(_u32(out, cc), sub), (what, a, e)
            assert int(out[cc].item()) == SENTINEL
            parts.append(sub)
        assert np.array_equal(np.concatenate(parts[:3]), want) and len(parts[3]) == 1


# ------------------------------------------------------------------------------------------ 5. host entry points
ASCII = np.frombuffer(b"ACTG", dtype=np.uint8)  # (code c is (letter >> 1) & 3)


@pytest.mark.parametrize("w", [129, 1000])
def test_host_entry_points_long_w(sm, oracle, gpu, w):
    """mm_run_host (count only, then outputs and indices), mm_run_host_ascii, mm_run_skip_ambiguous_host and _host_ascii
    at l - 1, l, l + 1 and l + 150 000 bases."""
    L = sm.lib()
    rng = np.random.default_rng(6100 + w)
    checked = 0
    for canonical, mode in _flavours(w):
        k = plan_k(READ_W[w], w, canonical)
        l = k + w - 1
        b = sm.Builder(k, w, canonical, mode)
        sk = mode == 0
        for n in (l - 1, l, l + 1, l + 150_000):
            off = int(rng.integers(0, 4))
            codes = tie_heavy_codes(n, int(rng.integers(1 << 30)))
            data = pack_at(codes, off)
            host = np.ascontiguousarray(data[: (off + n + 3) // 4])
            res = oracle.run(data, n, k, w, canonical=canonical, mode=mode, base_offset=off, super_kmers=sk)
            want, wsk = res if sk else (res, None)
            what = dict(w=w, k=k, canonical=canonical, mode=mode, n=n, off=off)
            cnt = C.c_uint64(99)
            assert L.mm_run_host(b.plan().h, gpu.h, _p(host, U8P), off, n, None, None, 0, C.byref(cnt)) == 0, what
            assert cnt.value == len(want), (what, cnt.value, len(want))
            cap = len(want) + 8
            pos = np.full(cap, 0xFFFFFFF9, dtype=np.uint32)
            psk = np.full(cap, 0xFFFFFFF9, dtype=np.uint32) if sk else None
            sm._check(L.mm_run_host(b.plan().h, gpu.h, _p(host, U8P), off, n, _p(pos, U32P), _p(psk, U32P) if sk else None,
                                    cap, C.byref(cnt)))
            assert n < l or gpu.last_path() == sm.PATH_GENERIC, what
            assert cnt.value == len(want) and np.array_equal(pos[:len(want)], want) and pos[len(want)] == 0xFFFFFFF9, what
            if sk:
                assert np.array_equal(psk[:len(want)], wsk) and psk[len(want)] == 0xFFFFFFF9, what
            text = np.ascontiguousarray(ASCII[codes])
            pos.fill(0xFFFFFFF9)
            sm._check(L.mm_run_host_ascii(b.plan().h, gpu.h, _p(text, U8P), n, _p(pos, U32P), None, cap, C.byref(cnt)))
            want0 = oracle.run(pack_at(codes), n, k, w, canonical=canonical, mode=mode)
            assert cnt.value == len(want0) and np.array_equal(pos[:len(want0)], want0) and pos[len(want0)] == 0xFFFFFFF9, what
            checked += 1
            if not canonical:
                continue
            # Ns: isolated ones and a run longer than l (none at the three short lengths but one in the middle)
            isn = np.zeros(n, dtype=bool)
            isn[n // 2] = True
            if n > 3 * l:
                isn[rng.integers(0, n, size=20)] = True
                isn[n // 3: n // 3 + l + 3] = True
            amb_offset = 9
            bits = np.concatenate([np.zeros(amb_offset, dtype=bool), isn])
            amb = np.concatenate([np.packbits(bits, bitorder="little"), np.zeros(16, dtype=np.uint8)])
            swant = oracle.run_skip_ambiguous(data, amb, n, k, w, mode=mode, base_offset=off, amb_offset=amb_offset)
            assert n < 3 * l or (len(swant) > 0 and not np.array_equal(swant, want))
            pos.fill(0xFFFFFFF9)
            sm._check(L.mm_run_skip_ambiguous_host(b.plan().h, gpu.h, _p(host, U8P), off, _p(amb, U8P), amb_offset, n,
                                                   _p(pos, U32P), cap, C.byref(cnt)))
            assert cnt.value == len(swant) and np.array_equal(pos[:len(swant)], swant) and pos[len(swant)] == 0xFFFFFFF9, what
            text_n = text.copy()
            text_n[isn] = ord("N")
            # (the packer's lossy code of N is its own: the oracle packs the same text)
            p2, a2 = oracle.pack_ascii_n(text_n.tobytes())
            swant2 = oracle.run_skip_ambiguous(p2, a2, n, k, w, mode=mode)
            pos.fill(0xFFFFFFF9)
            sm._check(L.mm_run_skip_ambiguous_host_ascii(b.plan().h, gpu.h, _p(text_n, U8P), n, _p(pos, U32P), cap,
                                                         C.byref(cnt)))
            assert cnt.value == len(swant2) and np.array_equal(pos[:len(swant2)], swant2), what
            assert pos[len(swant2)] == 0xFFFFFFF9, what
    assert checked == 16


def test_pipelined_host_run_long_w(sm, oracle, gpu):
    """One pipelined mm_run_host (kPipeMinWindows = 48 * 2^20 windows): forward minimizers k = 21, w = 129 with indices on
    48 * 2^20 + 100 000 windows - the only case where chunked window ranges, `append` and the generic family's running
    total meet (every chunk is more than one round long)."""
    k, w = 21, 129
    l = k + w - 1
    nw = (48 << 20) + 100_000
    n = nw + l - 1
    data = oracle.gen_packed(6200, n + 64)
    want, wsk = oracle.run(data, n, k, w, super_kmers=True)
    assert len(want) > 500_000
    host = np.ascontiguousarray(data[: (n + 3) // 4])
    cap = len(want) + 8
    pos = np.full(cap, 0xFFFFFFF9, dtype=np.uint32)
    psk = np.full(cap, 0xFFFFFFF9, dtype=np.uint32)
    cnt = C.c_uint64()
    b = sm.minimizers(k, w)
    sm._check(sm.lib().mm_run_host(b.plan().h, gpu.h, _p(host, U8P), 0, n, _p(pos, U32P), _p(psk, U32P), cap, C.byref(cnt)))
    assert gpu.last_path() == sm.PATH_GENERIC
    assert cnt.value == len(want), (cnt.value, len(want))
    bad = np.flatnonzero(pos[:len(want)] != want)
    assert len(bad) == 0, (bad[:4], pos[bad[:4]], want[bad[:4]])
    assert np.array_equal(psk[:len(want)], wsk)
    assert pos[len(want)] == 0xFFFFFFF9 and psk[len(want)] == 0xFFFFFFF9


# ------------------------------------------------------------------------------------------ 6. small related checks
def test_values_long_w(sm, oracle, gpu):
    """A minimizer plan at w = 257 reads k bases per value, as at any w; a syncmer plan at w = 129 reads l = 149 > 64 and
    is refused by the single, reads and batch values calls with the value buffer untouched."""
    import torch
    k, w, n = 31, 257, 60_000
    data = oracle.gen_packed(6300, n + 64)
    seq = sm.PackedSeq(data, 0, n)
    b = sm.canonical_minimizers(k, w)
    o = b.run(seq, [])
    pos = np.array(o.min_pos, dtype=np.uint32)
    want = oracle.run(data, n, k, w, canonical=True)
    assert gpu.last_path() == sm.PATH_GENERIC and np.array_equal(pos, want) and len(want) > 300
    assert np.array_equal(o.values_u64(), oracle.values_u64(data, k, want, True))
    w128 = oracle.values_u128(data, k, want, True)
    assert o.values_u128() == [int(lo) | (int(hi) << 64) for lo, hi in w128]
    # the syncmer plan
    k, w = 21, 129
    b = sm.closed_syncmers(k, w)
    assert b.plan().value_len() == k + w - 1 == 149
    d = torch.from_numpy(data).cuda()
    out = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    cnt = b.run_device(d, n, out)
    assert cnt == len(oracle.run(data, n, k, w, mode=1)) > 100
    E = sm.ERR["VALUE_LEN"]
    L = sm.lib()
    for u128 in (False, True):
        vals = torch.full((2 * cnt + 2,), SENTINEL, dtype=torch.int64, device="cuda")
        f = L.mm_values_u128_device_async if u128 else L.mm_values_u64_device_async
        assert f(gpu.h, _vp(d), d.numel(), 0, n, 149, 0, _vp(out), cnt, _vp(vals)) == E
        offs = torch.tensor([0, cnt], dtype=torch.int64, device="cuda")
        with pytest.raises(sm.MinimizerError) as e:
            sm.values_reads_device(b, d, 1, out, offs, read_stride=n, n_pos_max=cnt, out=vals, u128=u128)
        assert e.value.code == E
        with pytest.raises(sm.MinimizerError) as e:
            sm.values_batch_device(b, [d], [n], out, [0, cnt], out=vals, u128=u128)
        assert e.value.code == E
        gpu.sync()
        assert bool((vals == SENTINEL).all())


def test_prepare_and_stream_long_w(sm, oracle, gpu):
    """mm_plan_prepare on a w = 129 plan: its kernels are the prebuilt generic family, nothing is unavailable, nothing is
    compiled, and the first run afterwards compiles nothing.  mm_fastx_stream_create refuses the plan as the counts calls
    do (no lane table) and leaves *out null."""
    import torch
    b = sm.canonical_minimizers(21, 129)
    before = sm.jit_stats()
    for what in (dict(sequence=True, reads=False), dict(sequence=False, reads=True), dict(sequence=True, reads=True)):
        rep = b.prepare(**what)
        assert rep["unavailable"] == 0 and rep["compiled"] == 0 and rep["from_disk"] == 0 and rep["kernels"] >= 3, (what, rep)
    n = 50_000
    data = oracle.gen_packed(6400, n + 64)
    d = torch.from_numpy(data).cuda()
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    cnt = b.run_device(d, n, out)
    assert gpu.last_path() == sm.PATH_GENERIC
    assert np.array_equal(_u32(out, cnt), oracle.run(data, n, 21, 129, canonical=True))
    after = sm.jit_stats()
    assert after["compiled"] == before["compiled"], (before, after)
    cfg = sm.FastxStreamConfig(0, 0, 0, 0, 1 << 20, 1 << 10, 0, 0)
    h = C.c_void_p(0xDEAD)
    assert sm.lib().mm_fastx_stream_create(C.byref(h), b.plan().h, C.byref(cfg)) == sm.ERR["BAD_MODE"]
    assert not h.value
    with pytest.raises(sm.MinimizerError) as e:
        sm.FastxStream(b, 1 << 20, 1 << 10)
    assert e.value.code == sm.ERR["BAD_MODE"]


def test_device_group_long_w(sm, oracle, gpu):
    """A device group on entries {0, 0} at w = 257: mm_run_sharded_host and the device-resident shards + gather on
    300 000 bases equal the oracle, indices included."""
    import torch
    k, w, n, off = 31, 257, 300_000, 1
    data = pack_at(tie_heavy_codes(n, 6500), off)
    want, wsk = oracle.run(data, n, k, w, canonical=True, base_offset=off, super_kmers=True)
    assert len(want) > 1000
    g = sm.DeviceGroup([0, 0])
    try:
        sk_list = []
        b = sm.canonical_minimizers(k, w).super_kmers(sk_list)
        pos, sk = g.run(b, data, n, base_offset=off)
        assert np.array_equal(pos, want) and np.array_equal(sk, wsk)
        g.upload(data[: (off + n + 3) // 4 + 1])
        counts = g.run_device(b, n, base_offset=off)
        assert sum(counts) == len(want) and all(c > 0 for c in counts), counts
        dst = torch.full((len(want) + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        dsk = torch.full((len(want) + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        tot = g.gather(0, dst, dsk)
        assert tot == len(want) and np.array_equal(_u32(dst, tot), want) and np.array_equal(_u32(dsk, tot), wsk)
        assert int(dst[tot].item()) == SENTINEL and int(dsk[tot].item()) == SENTINEL
        nw = n - (k + w - 1) + 1
        assert g.result(0)[3] == 0 and g.result(0)[4] == g.result(1)[3] and g.result(1)[4] == nw
    finally:
        g.close()
