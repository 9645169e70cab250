"""Custom hasher tables (``mm_hasher_t`` as data: any table, any rot, any xor terms) on every GPU entry point of the
packed path, against the oracle's definition-level flavour with the same tables: single sequences (fused and
generic), reads (one lane per read and the lane table), batches, the skip-ambiguous walk, packed reads and their
counts form, device groups, and the strand symmetry of canonical hashers on the reads and batch paths.

The hashers come from tests/hasher_cases.py in rotation; every function tallies which families and rot values
reached the path it is about and asserts at its end that none was left out.  Output buffers are prefilled with a
sentinel: a check is the count, every position, and the sentinel right behind the count.  Window sizes are prebuilt
ones; the only flavour without a prebuilt instance (forward windows with a canonical hasher) runs under
``force_generic`` except for one single-sequence case, and the module asserts that nothing else was compiled."""
import os

import numpy as np
import pytest

import hasher_cases as hc
import text_checker as tc

pytestmark = pytest.mark.gpu

SENT = -7
PLANS = [(21, 11), (5, 7), (31, 19), (32, 5), (33, 4), (64, 2), (65, 3), (100, 12)]
LANES = 256  # lanes of a tile: a tile holds LANES * w * blocks_per_lane windows


@pytest.fixture(scope="module", autouse=True)
def _at_most_one_flavour_compiled(sm, gpu):
    """Every plan here has a prebuilt kernel, but for the one unforced run of forward windows with a canonical hasher."""
    before = sm.jit_stats()
    for canonical in (False, True):
        assert {w for _, w in PLANS} <= set(sm.prebuilt_window_sizes(canonical))
        for mode, sk, ws in ((0, False, {5, 7, 11, 19}), (0, True, {11}), (1, False, {17})):
            assert ws <= set(sm.prebuilt_flavour_window_sizes(canonical, True, mode, sk)), (canonical, mode, sk)
    yield
    after = sm.jit_stats()
    assert after["failed"] == before["failed"]
    assert after["compiled"] - before["compiled"] <= 1, (before, after)


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


def _filled(n):
    import torch
    return torch.full((n,), SENT, dtype=torch.int32, device="cuda")


def _upload(data, shift=0):
    """The bytes on the device, ``shift`` bytes off the allocation's alignment."""
    import torch
    dev = torch.zeros(len(data) + 8, dtype=torch.uint8, device="cuda")
    dev[shift: shift + len(data)] = torch.from_numpy(data).cuda()
    return dev[shift:]


def _same(out, count, want, tag):
    """count, every position, the sentinel right behind the count"""
    assert count == len(want), (tag, count, len(want))
    host = out[: count + 1].cpu().numpy()
    assert np.array_equal(host[:count].view(np.uint32), want), tag
    assert host[count] == SENT, tag


def _modes(w):
    return (0, 1, 2) if w % 2 else (0, 1)


def _flavours(k, w):
    """(name, hasher canonical, canonical windows): the third has no prebuilt instance."""
    out = [("fwd", False, False)]
    if (k + w - 1) % 2:
        out.append(("canon", True, True))
    out.append(("mixed", True, False))
    return out


def _shapes(k, w):
    """(n, blocks per lane): around l, a few thousand, and around one and three tiles of one and two blocks per lane"""
    l = k + w - 1
    out = [(l - 1, 0), (l, 0), (l + 1, 0), (3001 + l, 0)]
    for nblk in (1, 2):
        for t in (1, 3):
            for d in (-1, 0, 1):
                out.append((LANES * w * nblk * t + l - 1 + d, nblk))
    return out


# ------------------------------------------------------------------ 1. single sequence


def test_single_sequence_fused_and_generic(sm, oracle, gpu):
    rng = np.random.default_rng(9101)
    draw = hc.Draw(seed=11)
    fused, generic, host_tally = hc.Tally(), hc.Tally(), hc.Tally(rots=hc.ROTS[:6])
    redo = ranges = sks = 0
    big_n = 400_003
    data = oracle.gen_packed(501, big_n + 128)

    def one(case, k, w, canon_w, mode, n, nblk, forced, off, shift, want_all):
        nonlocal ranges, sks
        l = k + w - 1
        nw = max(0, n - l + 1)
        tag = (case, k, w, canon_w, mode, n, nblk, forced, off, shift)
        d = _upload(data[: (off + n + 3) // 4 + 16], shift)
        b = sm.Builder(k, w, canon_w, mode, hasher=case.product(sm))
        out = _filled(nw + 8)
        sk = _filled(nw + 8) if mode == 0 else None
        gpu.set_blocks_per_lane(nblk)
        gpu.force_generic(forced)
        try:
            c = b.run_device(d, n, out, out_sk=sk, base_offset=off)
            path = gpu.last_path()
            if nw:
                assert path == (sm.PATH_GENERIC if forced else sm.PATH_FUSED), tag
            if mode == 0:
                want, wsk = want_all
                _same(out, c, want, tag)
                _same(sk, c, wsk, tag)
                sks += 1
            else:
                want = want_all
                _same(out, c, want, tag)
                if nw > 2:  # one window sub-range: the matching slice of the whole run
                    a, e = sorted(int(x) for x in rng.integers(0, nw + 1, size=2))
                    out.fill_(SENT)
                    cc = b.run_device(d, n, out, base_offset=off, win_begin=a, win_end=e)
                    _same(out, cc, want[(want >= a) & (want < e)], (tag, a, e))
                    ranges += 1
        finally:
            gpu.set_blocks_per_lane(0)
            gpu.force_generic(False)
        if nw:
            (generic if forced else fused).add(case, n, c)
        return c

    def expected(case, k, w, canon_w, mode, n, off):
        return oracle.run(data, n, k, w, hasher=case.oracle(oracle), canonical=canon_w, mode=mode,
                          flavour=oracle.NAIVE, base_offset=off, super_kmers=mode == 0)

    turn = 0
    for k, w in PLANS:
        shapes = _shapes(k, w)
        for mode in _modes(w):
            for name, hash_canon, canon_w in _flavours(k, w):
                picked = [shapes[(turn + 5 * j) % len(shapes)] for j in range(3)]
                if (k, w) == (21, 11):
                    picked.append((big_n - 40, 0))  # a second tile of the default geometry
                turn += 1
                for n, nblk in picked:
                    case = draw(hash_canon)
                    off, shift = int(rng.integers(0, 40)), int(rng.integers(0, 4))
                    want = expected(case, k, w, canon_w, mode, n, off)
                    for forced in ((True,) if name == "mixed" else (False, True)):
                        one(case, k, w, canon_w, mode, n, nblk, forced, off, shift, want)
    # every key ties: one output per window, far above the density the lane lists are sized for (the redo walk)
    for i, (k, w) in enumerate(PLANS):
        l = k + w - 1
        for name, hash_canon, canon_w in _flavours(k, w)[:-1]:
            for n, nblk in ((LANES * w * 3 + l, 1), (5000 + l, 0)):
                case = hc.Case("const", hc.ROTS[(i + nblk) % len(hc.ROTS)], hash_canon, seed=20 + i, xor=bool(i & 1))
                want = expected(case, k, w, canon_w, 0, n, 3)
                c = one(case, k, w, canon_w, 0, n, nblk, False, 3, 1, want)
                if hc.const_emits_every_window(w, canon_w):
                    assert c == n - l + 1, (case, k, w, canon_w, n)
                    redo += 1
    # the flavour without a prebuilt instance, unforced: the one run of this module that may compile
    n, ps = 50_000, sm.PackedSeq(data, 5, 50_000)
    case = hc.Case("random", 17, True, seed=31, xor=True)
    got, _ = sm.minimizers(21, 11).hasher(case.product(sm))._run_arrays(ps)
    want = oracle.run(data, n, 21, 11, hasher=case.oracle(oracle), canonical=False, flavour=oracle.NAIVE, base_offset=5)
    assert np.array_equal(got, want), case
    # the host entry points: a PackedSeq view (mm_run_host) and ASCII (mm_run_host_ascii), one case per family
    ascii_ = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=30_011)].tobytes()
    packed_ascii = oracle.pack_ascii(ascii_)
    for i, fam in enumerate(hc.FAMILIES):
        canon_w = bool(i & 1)
        case = hc.Case(fam, hc.ROTS[i], canon_w, seed=40 + i, xor=i % 3 == 0)
        k, w = PLANS[i % 3]
        b = sm.Builder(k, w, canon_w, 0, hasher=case.product(sm)).super_kmers([])
        n = 20_001 + i
        got, gsk = b._run_arrays(sm.PackedSeq(data, 7 + i, n))
        want, wsk = expected(case, k, w, canon_w, 0, n, 7 + i)
        assert np.array_equal(got, want) and np.array_equal(gsk, wsk), ("mm_run_host", case, k, w)
        got, gsk = b._run_arrays(sm.AsciiSeq(ascii_))
        want, wsk = oracle.run(packed_ascii, len(ascii_), k, w, hasher=case.oracle(oracle), canonical=canon_w,
                               flavour=oracle.NAIVE, super_kmers=True)
        assert np.array_equal(got, want) and np.array_equal(gsk, wsk), ("mm_run_host_ascii", case, k, w)
        host_tally.add(case, n + len(ascii_), 2 * len(want))
    print("ranges", ranges, "super-k-mer checks", sks, "one-output-per-window runs", redo)
    fused.check("single sequence, fused")
    generic.check("single sequence, generic")
    host_tally.check("host entry points")
    assert redo >= 2 * len(PLANS) and ranges >= 40 and sks >= 40


# ------------------------------------------------------------------ 2. reads

READ_PLANS = [  # (k, w, mode, super-k-mer indices)
    (21, 11, 0, False), (5, 7, 0, False), (31, 19, 0, False), (15, 17, 1, False), (65, 5, 0, False), (21, 11, 0, True)]


def _read_layout(rng, l, long_reads):
    if long_reads:  # lanes start inside reads
        n_reads, read_len = int(rng.integers(1, 41)), int(rng.integers(1000, 7001))
    else:
        n_reads, read_len = int(rng.integers(1, 301)), int(rng.integers(l, l + 261))
    stride = read_len + int(rng.integers(0, 9))
    lens = rng.integers(0, read_len + 1, size=n_reads)
    for j, v in enumerate((0, l - 1, l, read_len, l + 1)):
        if j < n_reads:
            lens[(j * 7) % n_reads] = min(v, read_len)
    return n_reads, read_len, stride, lens.astype(np.int64)


def _run_reads(sm, b, d, n_reads, stride, read_len, lens, base, sk, d_amb=None):
    """(positions, offsets, indices or None) on the host, the sentinel behind the total checked"""
    import torch
    out = _filled(n_reads * read_len + 8)
    osk = _filled(n_reads * read_len + 8) if sk else None
    offs = torch.zeros(n_reads + 1, dtype=torch.int64, device="cuda")
    d_lens = torch.from_numpy(lens.astype(np.int32)).cuda()
    tot = sm.run_reads_device(b, d, n_reads, stride, read_len, out, offs, read_lens=d_lens, base_offset=base,
                              out_sk=osk, d_amb=d_amb, amb_offset=base)
    ho = offs.cpu().numpy()
    hp = out[: tot + 1].cpu().numpy()
    assert ho[0] == 0 and ho[-1] == tot and hp[tot] == SENT
    hs = None
    if sk:
        hs = osk[: tot + 1].cpu().numpy()
        assert hs[tot] == SENT
        hs = hs[:tot].view(np.uint32)
    return hp[:tot].view(np.uint32), ho, hs


def test_reads_one_lane_per_read_and_lane_table(sm, oracle, gpu):
    rng = np.random.default_rng(9102)
    draw = hc.Draw(seed=12)
    per_read, table = hc.Tally(), hc.Tally()
    reads_checked = 0
    for rep in range(2):
        for pi, (k, w, mode, sk) in enumerate(READ_PLANS):
            for long_reads in (False, True):
                canon = bool((pi + rep + long_reads) & 1) and (k + w - 1) % 2 == 1
                l = k + w - 1
                n_reads, read_len, stride, lens = _read_layout(rng, l, long_reads)
                base = int(rng.integers(0, 4))
                data = oracle.gen_packed(int(rng.integers(1 << 30)), base + n_reads * stride + 64)
                d = _upload(data, int(rng.integers(0, 4)))
                case = draw(canon)
                oh = case.oracle(oracle)
                want = [oracle.run(data, int(m), k, w, hasher=oh, canonical=canon, mode=mode, flavour=oracle.NAIVE,
                                   base_offset=base + r * stride, super_kmers=sk) for r, m in enumerate(lens)]
                b = sm.Builder(k, w, canon, mode, hasher=case.product(sm))
                nblk = (0, 1, 2)[(pi + rep) % 3] if long_reads else 0
                for policy in ("0", "1", None):
                    tag = (case, k, w, mode, sk, n_reads, read_len, stride, policy, nblk)
                    gpu.set_blocks_per_lane(nblk)
                    try:
                        with _Env(policy):
                            hp, ho, hs = _run_reads(sm, b, d, n_reads, stride, read_len, lens, base, sk)
                            assert gpu.last_path() == sm.PATH_FUSED, tag
                            lane_table = gpu.last_lane_table()
                    finally:
                        gpu.set_blocks_per_lane(0)
                    if policy is not None:
                        assert lane_table == (policy == "1"), tag
                    for r in range(n_reads):
                        got = hp[ho[r]:ho[r + 1]]
                        if sk:
                            assert np.array_equal(got, want[r][0]), (tag, r, int(lens[r]))
                            assert np.array_equal(hs[ho[r]:ho[r + 1]], want[r][1]), (tag, r, int(lens[r]))
                        else:
                            assert np.array_equal(got, want[r]), (tag, r, int(lens[r]))
                    reads_checked += n_reads
                    (table if lane_table else per_read).add(case, int(lens.sum()), len(hp))
    print("reads checked", reads_checked)
    per_read.check("reads, one lane per read")
    table.check("reads, lane table")


# ------------------------------------------------------------------ 3. batches


def _batch_layout(rng, l, n_seq, long_one):
    """lengths from below l to 150 000 and their starts in one buffer, at base offsets 0..3"""
    kinds = [l - 1, l, l + 1, int(rng.integers(l, 3000)), int(rng.integers(3000, 40_000)), 0]
    lens = [kinds[int(rng.integers(0, len(kinds)))] for _ in range(n_seq)]
    if long_one:
        lens[int(rng.integers(0, n_seq))] = int(rng.integers(100_000, 150_001))
    elif max(lens) < l + 1000:  # every batch holds windows to compare
        lens[int(rng.integers(0, n_seq))] = int(rng.integers(l + 1000, 9000))
    starts, s = [], 0
    for j, m in enumerate(lens):
        s += (j - s) % 4  # base offset j % 4
        starts.append(s)
        s += m + int(rng.integers(0, 3)) * 4
    return lens, starts, s


def _run_batch(sm, b, big, lens, starts, sk):
    d = [big[s0 // 4:] for s0 in starts]
    out = _filled(sum(lens) + 8)
    osk = _filled(sum(lens) + 8) if sk else None
    offs = sm.run_batch_device(b, d, lens, out, osk, base_offsets=[s0 % 4 for s0 in starts])
    tot = offs[-1]
    hp = out[: tot + 1].cpu().numpy()
    assert offs[0] == 0 and hp[tot] == SENT
    hs = None
    if sk:
        hs = osk[: tot + 1].cpu().numpy()
        assert hs[tot] == SENT
        hs = hs[:tot].view(np.uint32)
    return hp[:tot].view(np.uint32), offs, hs


def test_batches_tiles_and_lane_table(sm, oracle, gpu):
    rng = np.random.default_rng(9103)
    draw = hc.Draw(seed=13)
    tiles, table = hc.Tally(), hc.Tally()
    stood_in = table_sk = 0
    plans = [(21, 11), (5, 7), (31, 19), (32, 5), (65, 3), (100, 12)]
    for rep in range(3):
        for pi, (k, w) in enumerate(plans):
            mode = _modes(w)[(pi + rep) % len(_modes(w))]
            canon = bool((pi + rep) & 1) and (k + w - 1) % 2 == 1
            flavour = (mode, mode == 0)  # with out_sk at mode 0
            l = k + w - 1
            n_seq = 1 + (pi + 2 * rep) % 6
            lens, starts, total = _batch_layout(rng, l, n_seq, long_one=(pi + rep) % 3 == 0)
            data = oracle.gen_packed(int(rng.integers(1 << 30)), total + 128)
            big = _upload(data)
            case = draw(canon)
            oh = case.oracle(oracle)
            nblk = (0, 1, 2)[(pi + rep) % 3]
            for policy in ("0", "1"):
                mode, sk = flavour
                # the lane table runs the reads-mode kernel: where this flavour has no prebuilt one at w, plain
                # minimizer positions (prebuilt for reads at every window size) stand for it
                if policy == "1" and w not in sm.prebuilt_flavour_window_sizes(canon, True, mode, sk):
                    mode, sk = 0, False
                    stood_in += 1
                want = [oracle.run(data, m, k, w, hasher=oh, canonical=canon, mode=mode, flavour=oracle.NAIVE,
                                   base_offset=s0, super_kmers=sk) for m, s0 in zip(lens, starts)]
                b = sm.Builder(k, w, canon, mode, hasher=case.product(sm))
                tag = (case, k, w, mode, lens, starts, policy, nblk)
                gpu.set_blocks_per_lane(nblk)
                try:
                    with _Env(policy):
                        hp, offs, hs = _run_batch(sm, b, big, lens, starts, sk)
                        lane_table = gpu.last_lane_table()
                        if offs[-1]:
                            assert gpu.last_path() == sm.PATH_FUSED, tag
                finally:
                    gpu.set_blocks_per_lane(0)
                assert lane_table == (policy == "1") or not any(m >= l for m in lens), tag
                for i in range(n_seq):
                    got = hp[offs[i]:offs[i + 1]]
                    if sk:
                        assert np.array_equal(got, want[i][0]), (tag, i)
                        assert np.array_equal(hs[offs[i]:offs[i + 1]], want[i][1]), (tag, i)
                    else:
                        assert np.array_equal(got, want[i]), (tag, i)
                if any(m >= l for m in lens):
                    (table if lane_table else tiles).add(case, sum(lens), len(hp))
                    table_sk += int(lane_table and sk)
    tiles.check("batches, tile table")
    table.check("batches, lane table")
    assert stood_in <= 6 and table_sk >= 3, (stood_in, table_sk)


# ------------------------------------------------------------------ 4. skip-ambiguous


def _ascii_with_n(rng, n, l):
    """ACGT with scattered N and one run of N longer than l"""
    a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n + 8)].copy()
    if n:
        a[rng.integers(0, n, size=max(1, n // 200))] = ord("N")
        s0 = int(rng.integers(0, max(1, n - 2 * l)))
        a[s0: s0 + l + int(rng.integers(1, 40))] = ord("N")
    return a


def test_skip_ambiguous_walk(sm, oracle, gpu):
    import torch
    rng = np.random.default_rng(9104)
    fused, generic, reads = hc.Tally(), hc.Tally(), hc.Tally()
    skipped_windows = 0
    plans = [(21, 11), (5, 7), (31, 19), (15, 17), (65, 3)]
    # the two families with the most ties come first in every pass: every plan sees them
    order = ("const", "two") + tuple(f for f in hc.FAMILIES if f not in ("const", "two"))
    draw = hc.Draw(seed=14, families=order)
    for rep in range(2):
        for pi, (k, w) in enumerate(plans):
            l = k + w - 1
            for mode in _modes(w):
                for n, nblk in ((3000 + l + pi, 0), (LANES * w * 3 + l + rep, 1), (LANES * w * 2 + l - 2 + rep, 2)):
                    case = draw(True)
                    a = _ascii_with_n(rng, n, l)
                    packed, amb = oracle.pack_ascii_n(a.tobytes())
                    want = oracle.run_skip_ambiguous(packed, amb, n, k, w, hasher=case.oracle(oracle), mode=mode)
                    d_p, d_m = torch.from_numpy(packed).cuda(), torch.from_numpy(amb).cuda()
                    b = sm.Builder(k, w, True, mode, hasher=case.product(sm))
                    for forced in (False, True):
                        tag = (case, k, w, mode, n, nblk, forced)
                        out = _filled(n + 8)
                        gpu.set_blocks_per_lane(nblk)
                        gpu.force_generic(forced)
                        try:
                            c = b.run_skip_ambiguous_device(d_p, d_m, n, out)
                            assert gpu.last_path() == (sm.PATH_GENERIC if forced else sm.PATH_FUSED), tag
                        finally:
                            gpu.set_blocks_per_lane(0)
                            gpu.force_generic(False)
                        _same(out, c, want, tag)
                        (generic if forced else fused).add(case, n, c)
                    if mode == 0 and case.family == "const" and w > 2:
                        # one output per window that holds no N (neighbours of a skipped window may repeat a position)
                        clean = oracle.window_positions_skip_ambiguous(packed, amb, n, k, w, hasher=case.oracle(oracle))
                        n_clean = int((clean != oracle.SKIPPED).sum())
                        assert 0 < n_clean < n - l + 1 and c == n_clean, (case, k, w, n, c, n_clean)
                        skipped_windows += n - l + 1 - n_clean
    assert skipped_windows > 0
    # reads with ambiguity bits (mm_run_reads_skip_ambiguous_device), both launches
    draw = hc.Draw(seed=15)
    for pi, (k, w, mode) in enumerate([(21, 11, 0), (5, 7, 0), (15, 17, 1), (31, 19, 2), (65, 5, 0), (21, 11, 0)]):
        for long_reads in (False, True):
            l = k + w - 1
            n_reads, read_len, stride, lens = _read_layout(rng, l, long_reads)
            a = _ascii_with_n(rng, n_reads * stride + 64, l)
            packed, amb = oracle.pack_ascii_n(a.tobytes())
            d_p, d_m = torch.from_numpy(packed).cuda(), torch.from_numpy(amb).cuda()
            case = draw(True)
            oh = case.oracle(oracle)
            want = [oracle.run_skip_ambiguous(packed, amb, int(m), k, w, hasher=oh, mode=mode, base_offset=r * stride,
                                              amb_offset=r * stride) for r, m in enumerate(lens)]
            b = sm.Builder(k, w, True, mode, hasher=case.product(sm))
            for policy in ("0", "1"):
                tag = (case, k, w, mode, n_reads, read_len, stride, policy)
                with _Env(policy):
                    hp, ho, _ = _run_reads(sm, b, d_p, n_reads, stride, read_len, lens, 0, False, d_amb=d_m)
                    assert gpu.last_path() == sm.PATH_FUSED and gpu.last_lane_table() == (policy == "1"), tag
                for r in range(n_reads):
                    assert np.array_equal(hp[ho[r]:ho[r + 1]], want[r]), (tag, r, int(lens[r]))
                reads.add(case, int(lens.sum()), len(hp))
    fused.check("skip-ambiguous, fused")
    generic.check("skip-ambiguous, generic")
    reads.check("skip-ambiguous reads")


# ------------------------------------------------------------------ 5. packed reads and counts


def _fastq(rng, n_reads, max_len, with_n):
    lens = rng.integers(0, max_len + 1, size=n_reads)
    lens[:4] = [0, max_len, 30, 31]
    out = bytearray()
    for i, m in enumerate(lens):
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(m))].copy()
        if with_n and m and i % 3 == 0:
            s[rng.integers(0, m, size=1 + int(m) // 100)] = ord("N")
        out += b"@r%d\n" % i + s.tobytes() + b"\n+\n" + b"I" * int(m) + b"\n"
    return bytes(out), [int(m) for m in lens]


def test_packed_reads_and_counts(sm, oracle, gpu):
    import torch
    rng = np.random.default_rng(9105)
    tally = hc.Tally()
    text, lens = _fastq(rng, 200, 400, with_n=True)
    rec = sm.fasta_pack_n_device(text, max_records=256)
    assert rec.lengths() == lens
    n = len(rec)
    total = int(rec.base[-1])
    packed, amb = rec.packed.cpu().numpy(), rec.amb.cpu().numpy()
    base = [int(x) for x in rec.base]
    d_starts = torch.from_numpy(np.ascontiguousarray(rec.base, dtype=np.uint64).view(np.int64)).cuda()
    d_counts = torch.tensor([total, n], dtype=torch.int64, device="cuda")

    def host(out, offs, tot):
        hp = out[: tot + 1].cpu().numpy()
        ho = offs.cpu().numpy()
        assert hp[tot] == SENT and ho[0] == 0 and ho[n] == tot
        return hp[:tot].view(np.uint32), ho

    def per_record(hp, ho, want, tag):
        for r in range(n):
            assert np.array_equal(hp[ho[r]:ho[r + 1]], want[r]), (tag, r, lens[r])

    three = [hc.Case("random", 17, None, seed=51, xor=True), hc.Case("const", 7, None, seed=52),
             hc.Case("paired", 0, None, seed=53)]
    more = [hc.nth(i, None, seed=54) for i in range(8)]  # the rotation through the plain run: every family, every rot
    for ci, proto in enumerate(three + more):
        for canon in (False, True):
            case = hc.Case(proto.family, proto.rot, canon, proto.seed, xor=bool(proto.fw_xor))
            oh = case.oracle(oracle)
            k, w = (21, 11) if ci % 2 == 0 else (5, 7)
            b = sm.Builder(k, w, canon, 0, hasher=case.product(sm))
            want = [oracle.run(packed, lens[r], k, w, hasher=oh, canonical=canon, flavour=oracle.NAIVE,
                               base_offset=base[r]) for r in range(n)]
            out, offs = _filled(total + 8), torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            tot = sm.run_packed_reads_device(b, rec, out, offs)
            assert gpu.last_path() == sm.PATH_FUSED
            per_record(*host(out, offs, tot), want, ("run_packed_reads_device", case, k, w))
            tally.add(case, total, tot)
            if ci >= len(three):
                continue
            out, offs = _filled(total + 8), torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            got = sm.run_packed_reads_counts_device(b, rec.packed, d_starts, d_counts, out, offs, max_records=n,
                                                    max_bases=len(text))
            assert got[1:] == (total, n) and gpu.last_lane_table()
            per_record(*host(out, offs, got[0]), want, ("run_packed_reads_counts_device", case, k, w))
            if canon:
                want_a = [oracle.run_skip_ambiguous(packed, amb, lens[r], k, w, hasher=oh, base_offset=base[r],
                                                    amb_offset=base[r]) for r in range(n)]
                assert sum(len(x) for x in want_a) < sum(len(x) for x in want)  # windows were skipped
                out, offs = _filled(total + 8), torch.zeros(n + 1, dtype=torch.int64, device="cuda")
                tot = sm.run_packed_reads_skip_ambiguous_device(b, rec, out, offs)
                per_record(*host(out, offs, tot), want_a, ("run_packed_reads_skip_ambiguous_device", case, k, w))
                out, offs = _filled(total + 8), torch.zeros(n + 1, dtype=torch.int64, device="cuda")
                got = sm.run_packed_reads_counts_device(b, rec.packed, d_starts, d_counts, out, offs, max_records=n,
                                                        max_bases=len(text), amb=rec.amb)
                assert got[1:] == (total, n)
                per_record(*host(out, offs, got[0]), want_a, ("counts, skip-ambiguous", case, k, w))
    tally.check("packed reads")


# ------------------------------------------------------------------ 6. device group


def test_device_group(sm, oracle, gpu):
    import torch
    rng = np.random.default_rng(9106)
    tally = hc.Tally()
    n = 200_003
    data = oracle.gen_packed(601, n + 64)
    lens8 = [0, 20, 31, 1000, 4097, 30_000, 7, 12_345]
    seqs = [oracle.gen_packed(610 + i, m + 3) for i, m in enumerate(lens8)]
    g = sm.DeviceGroup([0, 0])
    try:
        g.upload(data[: (n + 3) // 4 + 1])
        g.upload_batch([s_[: (m + 3) // 4 + 1] for s_, m in zip(seqs, lens8)])
        two = [hc.Case("random", 17, None, seed=61, xor=True), hc.Case("const", 16, None, seed=62)]
        for ci, proto in enumerate(two + [hc.nth(i, None, seed=63) for i in range(8)]):
            for canon in (False, True):
                case = hc.Case(proto.family, proto.rot, canon, proto.seed, xor=bool(proto.fw_xor))
                oh = case.oracle(oracle)
                k, w = (21, 11) if ci % 2 == 0 else (31, 19)
                m = n if ci < len(two) else 20_003 + ci  # the rotation runs on a prefix of the resident sequence
                b = sm.Builder(k, w, canon, 0, hasher=case.product(sm)).super_kmers([])
                want, wsk = oracle.run(data, m, k, w, hasher=oh, canonical=canon, flavour=oracle.NAIVE, super_kmers=True)
                counts = g.run_device(b, m)
                assert sum(counts) >= len(want) and all(c > 0 for c in counts), (case, counts)
                dst, dsk = _filled(len(want) + 8), _filled(len(want) + 8)
                root = int(rng.integers(0, 2))
                assert g.gather(root, dst, dsk) == len(want), case
                _same(dst, len(want), want, ("gather", case, k, w))
                _same(dsk, len(want), wsk, ("gather, indices", case, k, w))
                if case.family == "const":
                    assert len(want) == m - (k + w - 1) + 1
                tally.add(case, m, len(want))
                wants = [oracle.run(s_, mm_, k, w, hasher=oh, canonical=canon, flavour=oracle.NAIVE, super_kmers=True)
                         for s_, mm_ in zip(seqs, lens8)]
                cc = g.run_batch_device(b, lens8)
                assert cc == [len(x[0]) for x in wants], case
                dst, dsk = _filled(sum(cc) + 8), _filled(sum(cc) + 8)
                o = g.gather_batch(root, dst, dsk)
                assert o == [0] + list(np.cumsum(cc)), case
                _same(dst, o[-1], np.concatenate([x[0] for x in wants]), ("gather_batch", case, k, w))
                _same(dsk, o[-1], np.concatenate([x[1] for x in wants]), ("gather_batch, indices", case, k, w))
                tally.add(case, sum(lens8), o[-1])
    finally:
        g.close()
    tally.check("device group")


# ------------------------------------------------------------------ 7. strand symmetry


def test_strand_symmetry_on_reads_and_batches(sm, oracle, gpu):
    """A canonical hasher with rc[c] = fw[c ^ 2] and equal xor terms gives a k-mer and its reverse complement the same
    key, and an odd l an untied strand vote: the positions of a sequence are ``(n - k) -`` those of its reverse
    complement, as sets (the check of test_alternative_hashers, there on the single-sequence path only)."""
    rng = np.random.default_rng(9107)
    tally_r, tally_b = hc.Tally(families=("paired",)), hc.Tally(families=("paired",))
    for i, rot in enumerate(hc.ROTS):
        k, w = [(21, 11), (5, 7), (31, 19), (65, 5)][i % 4]
        l = k + w - 1
        case = hc.Case("paired", rot, True, seed=70 + i, xor=bool(i & 1))
        case.rc_xor = case.fw_xor
        b = sm.Builder(k, w, True, 0, hasher=case.product(sm))
        # reads: every read reversed and complemented in place
        n_reads, read_len, stride, lens = _read_layout(rng, l, long_reads=bool(i & 1))
        codes = rng.integers(0, 4, size=n_reads * stride + 64, dtype=np.uint8)
        rc = codes.copy()
        for r, m in enumerate(lens):
            rc[r * stride: r * stride + m] = codes[r * stride: r * stride + m][::-1] ^ 2
        for policy in ("0", "1"):
            with _Env(policy):
                fp, fo, _ = _run_reads(sm, b, _upload(tc.pack_codes(codes)), n_reads, stride, read_len, lens, 0, False)
                rp, ro, _ = _run_reads(sm, b, _upload(tc.pack_codes(rc)), n_reads, stride, read_len, lens, 0, False)
                assert gpu.last_lane_table() == (policy == "1")
            assert np.array_equal(fo, ro), (case, policy)
            for r, m in enumerate(lens):
                mirrored = np.sort((int(m) - k) - rp[ro[r]:ro[r + 1]].astype(np.int64))
                assert np.array_equal(np.sort(fp[fo[r]:fo[r + 1]].astype(np.int64)), mirrored), (case, policy, r, int(m))
            tally_r.add(case, int(lens.sum()), len(fp))
        # batches: the reverse complements in the same layout
        lens_b, starts, total = _batch_layout(rng, l, 1 + i % 6, long_one=i % 4 == 0)
        codes = rng.integers(0, 4, size=total + 128, dtype=np.uint8)
        rc = codes.copy()
        for s0, m in zip(starts, lens_b):
            rc[s0: s0 + m] = codes[s0: s0 + m][::-1] ^ 2
        for policy in ("0", "1"):
            with _Env(policy):
                fp, fo, _ = _run_batch(sm, b, _upload(tc.pack_codes(codes)), lens_b, starts, False)
                rp, ro, _ = _run_batch(sm, b, _upload(tc.pack_codes(rc)), lens_b, starts, False)
            assert fo == ro, (case, policy)
            for j, m in enumerate(lens_b):
                mirrored = np.sort((m - k) - rp[ro[j]:ro[j + 1]].astype(np.int64))
                assert np.array_equal(np.sort(fp[fo[j]:fo[j + 1]].astype(np.int64)), mirrored), (case, policy, j, m)
            tally_b.add(case, sum(lens_b), len(fp))
    tally_r.check("strand symmetry, reads")
    tally_b.check("strand symmetry, batches")
    assert tally_r.positions > 1000 and tally_b.positions > 1000
