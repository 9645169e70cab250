"""The two ends of a tile of the fixed-k fused kernel (canonical k=21 w=11; DESIGN.md 4.1 "Phase 2 ahead of the barrier"):
what a lane reads before it walks, and the copy-out, whose list reads and values are made in front of the workgroup
barrier.  Every case is compared with the CPU oracle, counts and positions exactly.  The shapes are the smallest that reach
that code: full tiles of the default lanes (28 blocks per lane, 256 x 308 = 78 848 windows a tile; a run this short would
get 6-block lanes, so the lane length is pinned) and of the short-run geometry."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, W = 21, 11
L = K + W - 1
NBLK = 28
TILE = 256 * NBLK * W  # 78 848 windows
N = 3 * TILE + L - 1 + 13_456  # three full tiles and a remainder: 250 030 bases
SEED = 808


def _dev(out, c):
    return out[:c].cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def seq(oracle):
    """The seeded three-tile sequence (64 spare bases behind it for the runs at a base offset) and its oracle positions."""
    data = oracle.gen_packed(SEED, N + 64)
    data.setflags(write=False)
    want = oracle.run(data, N, K, W, canonical=True)
    want.setflags(write=False)
    return data, want


@pytest.fixture()
def lanes28(gpu):
    gpu.set_blocks_per_lane(NBLK)
    yield gpu
    gpu.set_blocks_per_lane(0)


def _run(sm, d, n, out, **kw):
    c = sm.Builder(K, W, True, 0).run_device(d, n, out, **kw)
    assert sm.default_workspace(0).last_path() == sm.PATH_FUSED
    return c


def test_three_full_tiles_and_a_remainder(sm, oracle, lanes28, seq):
    """Lane 0 of tile 0 (the base before the buffer), interior tiles, a partial last tile; then the same sequence with the
    lanes a run of this length gets by default (6 blocks: fifteen tiles, the last one partial)."""
    import torch
    assert sm.lib().mm_debug_fixed_k_kernel(K, W, 1) == 1
    data, want = seq
    d = torch.from_numpy(np.array(data)).cuda()
    out = torch.zeros(N // 2, dtype=torch.int32, device="cuda")
    c = _run(sm, d, N, out)
    assert c == len(want) and np.array_equal(_dev(out, c), want)
    lanes28.set_blocks_per_lane(0)
    out.zero_()
    c = _run(sm, d, N, out)
    assert c == len(want) and np.array_equal(_dev(out, c), want)


@pytest.mark.parametrize("base_offset,shift", [(1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (3, 1), (1, 3)])
def test_base_offsets_and_unaligned_pointers(sm, oracle, lanes28, seq, base_offset, shift):
    """The byte-shift cases of the sequence view: a base offset whose byte part is not 0, and a device pointer 1 - 3 bytes
    off dword alignment (both move the tile's origin against the dword grid of the loads)."""
    import torch
    data, _ = seq
    want = oracle.run(data, N, K, W, canonical=True, base_offset=base_offset)
    buf = torch.zeros(shift + len(data), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    d = buf[shift:]
    d.copy_(torch.from_numpy(np.array(data)))
    assert d.data_ptr() % 4 == shift
    out = torch.zeros(N // 2, dtype=torch.int32, device="cuda")
    c = _run(sm, d, N, out, base_offset=base_offset)
    assert c == len(want) and np.array_equal(_dev(out, c), want)


def test_window_range_inside_the_buffer(sm, oracle, lanes28, seq):
    """win_begin = 12 345, win_end two tiles further: element 0 of every tile lies inside the buffer."""
    import torch
    data, _ = seq
    a, e = 12_345, 12_345 + 2 * TILE
    per_window = oracle.window_positions(data, N, K, W, oracle.default_hasher(True), True)
    sub = per_window[a:e]
    keep = np.ones(len(sub), dtype=bool)
    keep[1:] = sub[1:] != sub[:-1]
    keep[0] = sub[0] != per_window[a - 1]
    want = sub[keep]
    d = torch.from_numpy(np.array(data)).cuda()
    out = torch.zeros(N // 2, dtype=torch.int32, device="cuda")
    c = _run(sm, d, N, out, win_begin=a, win_end=e)
    assert c == len(want) and np.array_equal(_dev(out, c), want)


@pytest.mark.parametrize("extra_bytes", [0, 1, 25, 63])
def test_sequence_ends_right_behind_the_last_full_tile(sm, oracle, lanes28, seq, extra_bytes):
    """The buffer ends 0 - 63 bytes behind the span of the last full tile (and is exactly as long as the sequence): what the
    last lanes read past it comes back as zeros from the bounds-checked descriptor."""
    import torch
    data, _ = seq
    n = 3 * TILE + L - 1 + 4 * extra_bytes
    nbytes = (n + 3) // 4
    want = oracle.run(data, n, K, W, canonical=True)
    d = torch.from_numpy(np.array(data[:nbytes])).cuda()
    assert d.numel() == nbytes
    out = torch.zeros(N // 2, dtype=torch.int32, device="cuda")
    c = _run(sm, d, n, out)
    assert c == len(want) and np.array_equal(_dev(out, c), want)


def test_low_complexity_overflow_and_long_lists(sm, oracle, lanes28):
    """poly-A of two tiles (every window emits: every list overflows and the tile is walked again, storing directly, behind
    the reads made for the copy-out), then short tandem repeats and random sequence (lists of more than 64 entries that do
    not overflow: the entries from the 65th on are read behind the barrier)."""
    import torch
    rng = np.random.default_rng(5)
    rnd = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 30_000)].tobytes()
    text = b"A" * (2 * TILE) + b"ACGGTCA" * 6_000 + rnd + b"AC" * 20_000 + rnd + b"ACGTT" * 4_000
    n = len(text)
    data = oracle.pack_ascii(text)
    want = oracle.run(data, n, K, W, canonical=True)
    d = torch.from_numpy(data).cuda()
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    c = _run(sm, d, n, out)
    assert c == len(want) and np.array_equal(_dev(out, c), want)


def test_capacity_below_the_output(sm, oracle, lanes28, seq):
    """An output buffer smaller than the count: the capacity error with the true count, the slots that exist hold the
    right positions, nothing is written behind them (the capacity-checked copy-out reads the lists itself)."""
    import torch
    data, want = seq
    d = torch.from_numpy(np.array(data)).cuda()
    for cap in (len(want) - 1, len(want) // 2 + 7, 100):
        buf = torch.full((len(want) + 64,), -7, dtype=torch.int32, device="cuda")
        with pytest.raises(sm.MinimizerError) as err:
            _run(sm, d, N, buf[:cap])
        assert err.value.args and str(len(want)) in str(err.value)
        host = buf.cpu().numpy()
        assert np.array_equal(host[:cap].view(np.uint32), want[:cap]), cap
        assert (host[cap:] == -7).all(), cap


def test_neighbouring_kernels_are_unaffected(sm, oracle, lanes28, seq):
    """The instantiations beside the fixed-k one, on the same sequence: k=21 w=11 with super-k-mer indices, k=20 w=11
    (forward windows: canonical windows need k + w - 1 odd) and its canonical neighbour k=19, forward k=21 w=11."""
    import torch
    data, _ = seq
    d = torch.from_numpy(np.array(data)).cuda()
    out = torch.zeros(N // 2, dtype=torch.int32, device="cuda")
    sk = torch.zeros(N // 2, dtype=torch.int32, device="cuda")
    want, wsk = oracle.run(data, N, K, W, canonical=True, super_kmers=True)
    c = sm.canonical_minimizers(K, W).run_device(d, N, out, out_sk=sk)
    assert lanes28.last_path() == sm.PATH_FUSED
    assert c == len(want) and np.array_equal(_dev(out, c), want) and np.array_equal(_dev(sk, c), wsk)
    for k, canonical in ((20, False), (19, True), (21, False)):
        want = oracle.run(data, N, k, W, canonical=canonical)
        c = sm.Builder(k, W, canonical, 0).run_device(d, N, out)
        assert lanes28.last_path() == sm.PATH_FUSED
        assert c == len(want) and np.array_equal(_dev(out, c), want), (k, canonical)


def test_ticket_mode(sm, oracle, lanes28, seq, monkeypatch):
    """Tile ids from the atomic ticket: the tile id is known only behind the first barrier."""
    import torch
    data, want = seq
    d = torch.from_numpy(np.array(data)).cuda()
    out = torch.zeros(N // 2, dtype=torch.int32, device="cuda")
    monkeypatch.setenv("MM_FORCE_TICKET", "1")
    c = _run(sm, d, N, out)
    assert c == len(want) and np.array_equal(_dev(out, c), want)
