"""w above 128 on the CPU: the oracle that judges the generic family at long w (tests/test_gpu_long_w.py) is pinned here
first, and the inputs both files share are built here.

Above w = 128 (kJitMaxW) no fused kernel exists and the generic family is the product on every entry point; a plan is
valid for any w below 2^15 (src/sliding_min.rs:91-95).  tests/test_oracle.py::test_sixteen_bit_position_wrap stops at
w = 200, forward only.  Here the oracle's streaming flavour - the one every GPU test compares with - equals its naive
flavour (a plain argmin per window) up to w = 32767, on input where most windows tie at their minimum, with more than
65 535 k-mers so that the streaming flavour's 16-bit positions are rebased (src/sliding_min.rs:117-125)."""
import numpy as np
import pytest

import text_checker as tc

W_LONG = [129, 130, 255, 256, 257, 1000, 4097, 32767]
K_BASE = [1, 21, 31, 65]
# the grid of the oracle pin: every w of W_LONG, k small, usual and above 64
KW_PIN = [(21, 129), (22, 130), (1, 255), (31, 256), (21, 257), (65, 1000), (21, 4097), (1, 32767), (21, 32767)]


def feasible(k, w, canonical, mode):
    """tests/test_gpu_long_k.py::_feasible: open syncmers have odd w, canonical plans odd l = k + w - 1."""
    if mode == 2 and w % 2 == 0:
        return False
    return not (canonical and (k + w - 1) % 2 == 0)


def plan_k(k, w, canonical):
    """k, moved by one where a canonical plan needs l = k + w - 1 odd."""
    return k + 1 if canonical and (k + w - 1) % 2 == 0 else k


def tie_heavy_codes(n, seed):
    """2-bit codes (A0 C1 T2 G3) built as tests/test_gpu_round5.py::test_strand_vote_at_every_lane_alignment builds its
    input, with stretches long enough for l up to 4 161: per 50 000 bases one stretch of 20 000 A / G only, one of 9 000
    C / T only and a homopolymer of 6 000 (each base in turn), random bases between them.  In the two-letter stretches
    most windows tie at their minimum (equal upper 16 bits) and a canonical window's vote sits near its threshold; in a
    homopolymer every k-mer of a window ties."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, size=n).astype(np.uint8)
    for j, s in enumerate(range(0, n, 50_000)):
        m = min(20_000, n - s)
        codes[s:s + m] = rng.integers(0, 2, size=m) * 3
        m = max(0, min(9_000, n - s - 24_000))
        codes[s + 24_000:s + 24_000 + m] = rng.integers(0, 2, size=m) + 1
        m = max(0, min(6_000, n - s - 38_000))
        codes[s + 38_000:s + 38_000 + m] = j % 4
    return codes


def pack_at(codes, off=0, slack=64):
    """The codes packed with `off` bases (all T) in front of them and `slack` zero bytes behind."""
    c = np.concatenate([np.full(off, 2, dtype=np.uint8), np.asarray(codes, dtype=np.uint8)])
    return np.concatenate([tc.pack_codes(c), np.zeros(slack, dtype=np.uint8)])


@pytest.mark.parametrize("k,w", KW_PIN)
def test_oracle_streaming_equals_naive_at_long_w(oracle, k, w):
    """Both strands where l is odd, every mode w admits, super-k-mer indices of minimizers.  n = l + 150 000; at
    w = 32767, where the naive flavour costs 3 s (forward) to 8 s (canonical) per 150 000 windows, 70 000 windows and
    k = 1 on both strands, k = 21 forward."""
    l = k + w - 1
    big = w == 32767
    nw = 70_000 if big else 150_001
    n = l - 1 + nw
    assert nw + w - 1 > 65_535  # k-mers: past the first rebase of the 16-bit positions
    packed = pack_at(tie_heavy_codes(n, 7 * w + k))
    done = 0
    # floors on the naive flavour's answers: random-like k = 21 at w = 32767 selects a handful of positions in 70 000
    # windows, and open syncmers are sparse by nature (none at all in 70 000 windows of w = 32767)
    floor = {0: 1 if big and k == 21 else 100, 1: 1 if big and k == 21 else 100, 2: 0 if big else 1}
    for canonical in (False, True):
        if big and canonical and k != 1:
            continue
        h = oracle.default_hasher(canonical)
        for mode in (0, 1, 2):
            if not feasible(k, w, canonical, mode):
                continue
            if mode == 0:
                wp, wsk = oracle.run(packed, n, k, w, h, canonical, mode, flavour=oracle.NAIVE, super_kmers=True)
                gp, gsk = oracle.run(packed, n, k, w, h, canonical, mode, flavour=oracle.STREAMING, super_kmers=True)
                assert len(wp) >= floor[0] and np.array_equal(gp, wp) and np.array_equal(gsk, wsk), (k, w, canonical)
                assert np.array_equal(oracle.run(packed, n, k, w, h, canonical, mode), gp), (k, w, canonical)
                assert np.all(np.diff(wsk.astype(np.int64)) > 0) and wsk[0] == 0 and wsk[-1] < nw
                if not big:
                    assert np.array_equal(oracle.run(packed, n, k, w, h, canonical, mode, flavour=oracle.NAIVE), wp)
            else:
                want = oracle.run(packed, n, k, w, h, canonical, mode, flavour=oracle.NAIVE)
                got = oracle.run(packed, n, k, w, h, canonical, mode, flavour=oracle.STREAMING)
                assert np.array_equal(got, want), (k, w, canonical, mode)
                assert len(want) >= floor[mode], (k, w, canonical, mode, len(want))
            done += 1
    want_done = sum(feasible(k, w, c, m) for c in (False, True) for m in (0, 1, 2) if not (big and c and k != 1))
    assert done == want_done >= 2


def test_the_pin_covers_the_grid():
    """44 (k, w, strand, mode) combinations are valid plans; every w of W_LONG is among them."""
    combos = [(k, w, c, m) for k, w in KW_PIN for c in (False, True) for m in (0, 1, 2) if feasible(k, w, c, m)]
    assert len(combos) == 44 and {w for _, w, _, _ in combos} == set(W_LONG)
    assert all(w < (1 << 15) for w in W_LONG)


def ascii_with_n(rng, n, l, isolated_every=5000):
    """ACGT with isolated Ns (about one per `isolated_every` bases) and one run of Ns longer than l."""
    a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
    if n:
        a[rng.integers(0, n, size=max(1, n // isolated_every))] = ord("N")
        s = int(rng.integers(n // 3, n // 2))
        a[s:s + l + 7] = ord("N")
    return a


@pytest.mark.parametrize("k,w", [(21, 129), (65, 1000)])
def test_oracle_skip_ambiguous_at_long_w(oracle, k, w):
    """oracle.run_skip_ambiguous against its parts and against numpy: the window stream is the NAIVE canonical stream
    with SKIPPED wherever a prefix sum of the ambiguity bits finds one in the window's l bases; minimizers are
    collect_and_dedup_skip of it, syncmers the windows whose position is at an end (closed) or in the middle (open)."""
    canonical = True
    k = plan_k(k, w, canonical)
    l = k + w - 1
    rng = np.random.default_rng(w)
    n = l + 60_000
    a = ascii_with_n(rng, n, l)
    packed, amb = oracle.pack_ascii_n(a.tobytes())
    nw = n - l + 1
    plain = oracle.window_positions(packed, n, k, w, oracle.default_hasher(True), True, flavour=oracle.NAIVE)
    isn = np.concatenate([[0], np.cumsum(a == ord("N"))])
    dirty = (isn[l:l + nw] - isn[:nw]) > 0
    assert 100 < int(dirty.sum()) < nw - 1000
    want_stream = np.where(dirty, np.uint32(oracle.SKIPPED), plain)
    stream = oracle.window_positions_skip_ambiguous(packed, amb, n, k, w)
    assert np.array_equal(stream, want_stream)
    i = np.arange(nw, dtype=np.int64)
    s = stream.astype(np.int64)
    for mode in (0, 1, 2):
        if not feasible(k, w, canonical, mode):
            continue
        got = oracle.run_skip_ambiguous(packed, amb, n, k, w, mode=mode)
        if mode == 0:
            keep = ~dirty & np.concatenate([[True], s[1:] != s[:-1]])
            want = stream[keep]
            assert np.array_equal(oracle.collect_and_dedup_skip(stream, True), want)
        elif mode == 1:
            want = i[~dirty & ((s == i) | (s == i + w - 1))].astype(np.uint32)
        else:
            want = i[~dirty & (s == i + w // 2)].astype(np.uint32)
        assert np.array_equal(got, want) and len(want) > (0 if mode == 2 else 50), (k, w, mode, len(want))
    # the same read at another base and bit offset (a PackedNSeq slice)
    sub = oracle.run_skip_ambiguous(packed, amb, n - 13, k, w, base_offset=13, amb_offset=13)
    keep = ~dirty[13:] & np.concatenate([[True], s[14:] != s[13:-1]])
    assert np.array_equal(sub, (stream[13:][keep] - np.uint32(13)))
