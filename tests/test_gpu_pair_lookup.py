"""The pair look-ups of the fixed-k canonical walk (canonical k=21 w=11; DESIGN.md 4.1 "Pair look-ups"): the blocks of that
walk take their rolling-hash contributions from a 256-entry table indexed by two consecutive bases of each stream - one LDS
read per two steps, the odd step made from the state the even one started from.  Every case goes through the C ABI as
canonical k=21 w=11, so that it reaches that kernel, and is compared with the CPU oracle element by element.  The shapes are
the smallest that reach each walk of the instance: a tile of the default lanes of a long run is 256 x 286 = 73 216 windows
(26 blocks per lane; a run this short would get 6-block lanes, so the lane length is pinned where tiles matter)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, W = 21, 11
L = K + W - 1
NBLK = 26
LANE = NBLK * W          # 286 windows
TILE = 256 * LANE        # 73 216 windows
N3 = 3 * TILE + 20_011 + L - 1  # three tiles and a partial one


def _dev(out, c):
    return out[:c].cpu().numpy().view(np.uint32)


def _run(sm, d, n, out, hasher=None, **kw):
    b = sm.Builder(K, W, True, 0, hasher=hasher) if hasher is not None else sm.Builder(K, W, True, 0)
    c = b.run_device(d, n, out, **kw)
    assert sm.default_workspace(0).last_path() == sm.PATH_FUSED
    return c


def _ranged(per_window, a, e):
    sub = per_window[a:e]
    keep = np.ones(len(sub), dtype=bool)
    keep[1:] = sub[1:] != sub[:-1]
    keep[0] = sub[0] != per_window[a - 1]
    return sub[keep]


@pytest.fixture(scope="module")
def seq(sm, oracle):
    """A seeded sequence of three tiles and a partial one (spare bases behind it for the runs at a base offset)."""
    assert sm.lib().mm_debug_fixed_k_kernel(K, W, 1) == 1
    data = oracle.gen_packed(2611, N3 + 64)
    data.setflags(write=False)
    return data


@pytest.fixture()
def lanes26(gpu):
    gpu.set_blocks_per_lane(NBLK)
    yield gpu
    gpu.set_blocks_per_lane(0)


@pytest.mark.parametrize("n_windows", [TILE + 5, 3 * TILE + 20_011], ids=["tile+5", "3 tiles+partial"])
def test_whole_tiles_and_a_partial_one(sm, oracle, lanes26, seq, n_windows):
    import torch
    n = n_windows + L - 1
    want = oracle.run(seq, n, K, W, canonical=True)
    d = torch.from_numpy(np.array(seq)).cuda()
    out = torch.zeros(n // 2, dtype=torch.int32, device="cuda")
    c = _run(sm, d, n, out)
    assert c == len(want) and np.array_equal(_dev(out, c), want)


@pytest.mark.parametrize("pinned", [True, False], ids=["26 blocks", "default lanes"])
def test_shorter_than_one_lane(sm, oracle, gpu, seq, pinned):
    """1 window, a few blocks, one window short of a lane: the partial walk's blocks behind the last whole load group."""
    import torch
    d = torch.from_numpy(np.array(seq[:4096])).cuda()
    out = torch.zeros(1024, dtype=torch.int32, device="cuda")
    gpu.set_blocks_per_lane(NBLK if pinned else 0)
    try:
        for nw in (1, 2, 10, 11, 12, 23, 45, 100, LANE - 1):
            for off in (0, 3):
                n = nw + L - 1
                want = oracle.run(seq, n, K, W, canonical=True, base_offset=off)
                c = _run(sm, d, n, out, base_offset=off)
                assert c == len(want) and np.array_equal(_dev(out, c), want), (nw, off)
    finally:
        gpu.set_blocks_per_lane(0)


def test_every_base_offset_and_pointer_alignment(sm, oracle, lanes26, seq):
    """About 100 kbp at base offsets 0 .. 15 and device pointers 0 .. 3 bytes off dword alignment: the tile's origin moves
    through every bit and byte position of the loads, and with it the pair bytes through every shift of the views."""
    import torch
    n = 100_003
    nbytes = (n + 15 + 3) // 4 + 8
    wants = [oracle.run(seq, n, K, W, canonical=True, base_offset=off) for off in range(16)]
    out = torch.zeros(n // 2, dtype=torch.int32, device="cuda")
    for shift in range(4):
        buf = torch.zeros(shift + nbytes, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        d = buf[shift:]
        d.copy_(torch.from_numpy(np.array(seq[:nbytes])))
        for off in range(16):
            c = _run(sm, d, n, out, base_offset=off)
            assert c == len(wants[off]) and np.array_equal(_dev(out, c), wants[off]), (shift, off)


def test_window_range_that_begins_and_ends_inside_tiles(sm, oracle, lanes26, seq):
    import torch
    n = N3
    per_window = oracle.window_positions(seq, n, K, W, oracle.default_hasher(True), True)
    d = torch.from_numpy(np.array(seq)).cuda()
    out = torch.zeros(n // 2, dtype=torch.int32, device="cuda")
    for a, e in ((12_345, 12_345 + 2 * TILE + 777), (TILE - 3, TILE + 300), (5, 6), (LANE * 7 + 1, 3 * TILE + 19_999)):
        want = _ranged(per_window, a, e)
        c = _run(sm, d, n, out, win_begin=a, win_end=e)
        assert c == len(want) and np.array_equal(_dev(out, c), want), (a, e)


def test_three_contigs_in_one_launch(sm, oracle, lanes26, seq):
    """A batch: every contig starts a tile of its own; one longer than a tile, one of a few lanes, one shorter than a lane."""
    import torch
    lens = [TILE + 4_321 + L - 1, 7 * LANE + 3 + L - 1, 57 + L - 1]
    starts = [0, 100_000, 200_000]  # bases of `seq`, multiples of 4
    hosts = [np.array(seq[s // 4: s // 4 + (m + 3) // 4 + 8]) for s, m in zip(starts, lens)]
    wants = [oracle.run(h, m, K, W, canonical=True) for h, m in zip(hosts, lens)]
    d_seqs = [torch.from_numpy(h).cuda() for h in hosts]
    out = torch.zeros(sum(lens) // 2, dtype=torch.int32, device="cuda")
    offs = sm.run_batch_device(sm.Builder(K, W, True, 0), d_seqs, lens, out)
    assert lanes26.last_path() == sm.PATH_FUSED
    assert [offs[i + 1] - offs[i] for i in range(3)] == [len(x) for x in wants]
    host = out[:offs[3]].cpu().numpy().view(np.uint32)
    for i in range(3):
        assert np.array_equal(host[offs[i]:offs[i + 1]], wants[i]), i


def test_poly_a_overflows_into_the_direct_store_walk(sm, oracle, lanes26):
    """poly-A of two tiles: every window emits, every list overflows, the tiles are walked again storing directly."""
    import torch
    rng = np.random.default_rng(26)
    rnd = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 9_000)].tobytes()
    text = rnd + b"A" * (2 * TILE) + rnd
    n = len(text)
    data = oracle.pack_ascii(text)
    want = oracle.run(data, n, K, W, canonical=True)
    assert len(want) > 2 * TILE
    d = torch.from_numpy(data).cuda()
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    c = _run(sm, d, n, out)
    assert c == len(want) and np.array_equal(_dev(out, c), want)


def test_custom_hasher_with_random_tables(sm, oracle, lanes26, seq):
    """Random per-base values, rot = 7, constant XOR terms: the table is made from the plan's own tables."""
    import torch
    rng = np.random.default_rng(77)
    fw, rc = [int(x) for x in rng.integers(0, 1 << 32, 4, dtype=np.uint64)], [int(x) for x in rng.integers(0, 1 << 32, 4, dtype=np.uint64)]
    fx, rx = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
    oh = oracle.Hasher()
    for i in range(4):
        oh.fw[i], oh.rc[i] = fw[i], rc[i]
    oh.rot, oh.canonical, oh.fw_xor, oh.rc_xor, oh.kind = 7, 1, fx, rx, 0
    ph = sm.Hasher.from_tables(fw, rc, rot=7, canonical=True, fw_xor=fx, rc_xor=rx)
    n = TILE + 9_000 + L - 1
    d = torch.from_numpy(np.array(seq)).cuda()
    out = torch.zeros(n // 2, dtype=torch.int32, device="cuda")
    for off in (0, 5):
        want = oracle.run(seq, n, K, W, hasher=oh, canonical=True, flavour=oracle.NAIVE, base_offset=off)
        c = _run(sm, d, n, out, hasher=ph, base_offset=off)
        assert c == len(want) and np.array_equal(_dev(out, c), want), off


def test_period_five_repeat_every_step_decides_a_tie(sm, oracle, lanes26):
    """The exact repeat ACGTT: every window ties, so every step's strand count reads the buffers the pair bytes come from."""
    import torch
    n = TILE + 3 * LANE + 17 + L - 1
    data = oracle.pack_ascii((b"ACGTT" * (n // 5 + 2))[:n + 16])
    d = torch.from_numpy(data).cuda()
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    for off in (0, 1, 2, 3, 4):
        want = oracle.run(data, n, K, W, canonical=True, base_offset=off)
        c = _run(sm, d, n, out, base_offset=off)
        assert c == len(want) and np.array_equal(_dev(out, c), want), off
