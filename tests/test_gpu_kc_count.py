"""The fixed-k canonical walk on sequence where its strand vote decides (DESIGN.md 4.1 "lazy vote").  That walk keeps no
running T|G count: where a window's leftmost and rightmost minimum differ it counts the window from its two sequence
buffers (kc_count_plan; tests/test_kc_count_cpu.py checks the plan on the host), and at a lane's start it counts the window
before the lane's first only where that one ties.  Here every wave-step takes that path - exact repeats, in which every
window ties, on either strand - or an isolated one does (random sequence with a k-mer copied a few bases on), at the
lengths, offsets and window ranges at which the walk changes its path.  Every case is compared with the CPU oracle."""
import numpy as np
import pytest

K, W = 21, 11
L = K + W - 1
TILE = 256 * 6 * W  # windows of a tile of a short run (6 blocks per lane: 66 windows a lane)
# ends inside the first block, inside the first load group, on a group, a lane and a tile boundary
WINDOWS = [1, 5, 11, 12, 30, 54, 55, 56, 66, 67, 99, 110, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 45, 5 * TILE + 54]
OFFSETS = (0, 1, 2, 3, 5)

# exact repeats; the T|G share of a unit below, at and above one half (a window holds 31 bases, so both strands win where
# the share is one half, and one strand everywhere else)
REPEATS = {
    "p2 CA (none)": b"CA", "p2 AG (half)": b"AG", "p2 GT (all)": b"GT",
    "p3 ACG (1/3)": b"ACG", "p3 GTA (2/3)": b"GTA",
    "p5 AACGC (1/5)": b"AACGC", "p5 ACGTT (3/5)": b"ACGTT",
    "p7 AACCAGT (2/7)": b"AACCAGT", "p7 GGTTACG (5/7)": b"GGTTACG",
    "p10 AACCACAGCT (1/5)": b"AACCACAGCT", "p10 ACGTACGTAG (half)": b"ACGTACGTAG", "p10 GGTTGATTCG (4/5)": b"GGTTGATTCG",
}


def _random_over(alphabet: bytes, n: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def _isolated_ties(n: int, seed: int) -> bytes:
    """random sequence with a k-mer copied to a distance of 1 .. w - 1 every few hundred bases: the two copies hash alike,
    so the windows that hold both as their minimum tie, and most wave-steps around them do not"""
    rng = np.random.default_rng(seed)
    s = bytearray(_random_over(b"ACGT", n, seed + 1))
    p = 40
    while p + K + W < n:
        d = int(rng.integers(1, W))
        for j in range(K):
            s[p + d + j] = s[p + j]
        p += int(rng.integers(200, 400))
    return bytes(s)


def _sequence(name: str, n: int) -> bytes:
    if name in REPEATS:
        u = REPEATS[name]
        return (u * (n // len(u) + 1))[:n]
    if name == "random over AC":
        return _random_over(b"AC", n, 5)
    if name == "random over GT":
        return _random_over(b"GT", n, 6)
    assert name == "isolated ties"
    return _isolated_ties(n, 7)


SEQUENCES = list(REPEATS) + ["random over AC", "random over GT", "isolated ties"]


def _dev(out, c):
    return out[:c].cpu().numpy().view(np.uint32)


def _check_kernel(sm, gpu):
    assert gpu.last_path() == sm.PATH_FUSED
    assert sm.lib().mm_debug_fixed_k_kernel(K, W, 1) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", SEQUENCES)
def test_lengths_and_offsets_vs_oracle(sm, oracle, gpu, name):
    import torch
    big = WINDOWS[-1] + L + 64
    data = oracle.pack_ascii(_sequence(name, big))
    d = torch.from_numpy(data).cuda()
    out = torch.zeros(big, dtype=torch.int32, device="cuda")
    b = sm.Builder(K, W, True, 0)
    for nw in WINDOWS:
        for off in OFFSETS:
            n = nw + L - 1
            want = oracle.run(data, n, K, W, canonical=True, base_offset=off)
            c = b.run_device(d, n, out, base_offset=off)
            _check_kernel(sm, gpu)
            assert c == len(want) and np.array_equal(_dev(out, c), want), (name, nw, off)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["p2 AG (half)", "p5 ACGTT (3/5)", "p7 AACCAGT (2/7)", "p10 ACGTACGTAG (half)", "isolated ties"])
def test_window_ranges_inside_tie_rich_sequence_vs_oracle(sm, oracle, gpu, name):
    """Window ranges that begin and end inside the repeat: the range-checked walk, and lanes whose first window's
    predecessor ties (the count of that window decides what the first window is compared with)."""
    import torch
    n = 3 * TILE + 500
    nw = n - L + 1
    data = oracle.pack_ascii(_sequence(name, n + 8))
    d = torch.from_numpy(data).cuda()
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    b = sm.Builder(K, W, True, 0)
    for off in (0, 3, 5):
        per_window = oracle.window_positions(data, n, K, W, oracle.default_hasher(True), True, base_offset=off)
        for a, e in ((1, nw), (7, 8), (66 * 3 + 5, 66 * 40 + 17), (TILE - 3, TILE + 300), (TILE + 66 * 7, 2 * TILE + 66 * 3 + 1),
                     (12_345, nw - 13), (2 * TILE + 1, nw)):
            sub = per_window[a:e]
            keep = np.ones(len(sub), dtype=bool)
            keep[1:] = sub[1:] != sub[:-1]
            keep[0] = sub[0] != per_window[a - 1]
            want = sub[keep]
            c = b.run_device(d, n, out, base_offset=off, win_begin=a, win_end=e)
            _check_kernel(sm, gpu)
            assert c == len(want) and np.array_equal(_dev(out, c), want), (name, off, a, e)


@pytest.mark.gpu
def test_poly_a_overflows_the_lists_beside_ties_vs_oracle(sm, oracle, gpu):
    """A poly-A stretch emits at every window, the lane lists overflow and the tile is walked again storing directly: the
    direct-store walk counts the same way, here with repeats on both sides of the stretch."""
    import torch
    seq = (_sequence("isolated ties", 20_000) + _sequence("p5 ACGTT (3/5)", 9_000) + b"A" * 60_000 +
           _sequence("p10 ACGTACGTAG (half)", 9_000) + b"T" * 30_000 + _sequence("p3 ACG (1/3)", 9_000) +
           _sequence("isolated ties", 20_000))
    data = oracle.pack_ascii(seq)
    d = torch.from_numpy(data).cuda()
    out = torch.zeros(len(seq), dtype=torch.int32, device="cuda")
    for off in (0, 2):
        n = len(seq) - off
        want = oracle.run(data, n, K, W, canonical=True, base_offset=off)
        c = sm.Builder(K, W, True, 0).run_device(d, n, out, base_offset=off)
        _check_kernel(sm, gpu)
        assert c == len(want) and np.array_equal(_dev(out, c), want), off


@pytest.mark.gpu
def test_full_lanes_with_repeats_on_tile_and_lane_boundaries_vs_oracle(sm, oracle, gpu):
    """64 Mbp: the launcher walks full 28-block lanes (308 windows a lane, 78 848 a tile) through the loop that unrolls whole
    load groups.  Repeats are planted across several tile boundaries - each also crosses a dozen lane boundaries - and
    across lane boundaries inside tiles, so that ties meet every block of a group, a lane's start and a tile's start."""
    import torch
    n = 67_108_864 + 3
    lane, tile = 28 * W, 256 * 28 * W
    data = oracle.gen_packed(65, n)
    units = [REPEATS[x] for x in ("p5 ACGTT (3/5)", "p10 ACGTACGTAG (half)", "p2 AG (half)", "p3 ACG (1/3)", "p7 GGTTACG (5/7)",
                                  "p5 AACGC (1/5)")]
    spots = [(t * tile - 2_000, 4_000) for t in (1, 2, 37, 400, 851)] + \
            [(t * tile + m * lane - 150, 400) for t, m in ((0, 1), (5, 100), (5, 101), (300, 255), (850, 17))]
    for i, (start, length) in enumerate(spots):
        u = units[i % len(units)]
        pat = oracle.pack_ascii(u * 4)[:len(u)]  # 4 periods are a whole number of bytes
        b0, nb = (start // 4), length // 4
        assert b0 > 0 and 4 * (b0 + nb) < n
        data[b0:b0 + nb] = np.resize(pat, nb)
    d = torch.from_numpy(data).cuda()
    out = torch.zeros(n // 4, dtype=torch.int32, device="cuda")
    want = oracle.run_fast(data, n, K, W, canonical=True, threads=8)
    c = sm.Builder(K, W, True, 0).run_device(d, n, out)
    _check_kernel(sm, gpu)
    assert c == len(want) and np.array_equal(_dev(out, c), want)
