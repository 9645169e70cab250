"""k above 64 on every GPU path of the packed engine, against the oracle (exact equality everywhere).

The existing fuzz draws k from 1..64 (tests/test_gpu_fuzz.py::_plan); the reference's own grid reaches 65 and random k up
to 99 (src/test.rs:29-33), and the plans accept any k.  What differs at long k: the warm-up of a lane's first hash takes
k bases in 16-base view words with a two-base table and an odd last base (k mod 16 in {0, 1, 15}); the rotation constants
depend on R * k mod 32 (k mod 32 == 0 wraps); and the stream of bases entering the hash starts k bases ahead of the one
leaving it - with short lanes (set_blocks_per_lane) and k = 1000 or 4097 that is beyond the lane and beyond the whole
tile.  Window sizes come from the library's own lists of prebuilt kernels, so nothing is compiled at run time: the
module asserts that."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_LONG = [65, 80, 96, 97, 99, 127, 128, 129, 255, 256, 1000, 4097]
W_WANTED = [1, 5, 11, 16, 19, 31, 32, 33, 51]  # (W % 16 == 0: the third load stream of canonical walks)
READ_WS = [5, 7, 11, 15, 17, 19, 21, 31]
LANES = 256  # lanes of a workgroup: a tile is LANES * blocks per lane * w windows
SENTINEL = -7


@pytest.fixture(scope="module", autouse=True)
def _nothing_compiled(sm, gpu):
    """Every window size of this module has a prebuilt kernel for its flavour: the run-time compiler stays idle."""
    before = sm.jit_stats()
    yield
    after = sm.jit_stats()
    assert after["compiled"] - before["compiled"] == 0, (before, after)


def _feasible(k, w, canonical, mode):
    if mode == 2 and w % 2 == 0:
        return False
    return not (canonical and (k + w - 1) % 2 == 0)


def _windows(sm, k, canonical, mode, sk=False, reads=False):
    """The wanted window sizes that are prebuilt for this flavour and give a valid plan with k."""
    listed = set(sm.prebuilt_flavour_window_sizes(canonical, reads, mode, sk))
    wanted = sorted(set(W_WANTED + READ_WS)) if reads else W_WANTED
    return [w for w in wanted if w in listed and _feasible(k, w, canonical, mode)]


def _device_seq(torch, data, off, n, shift):
    """The sequence in a device allocation filled with 0xFF, `shift` bytes off a 16-byte boundary, sliced to exactly
    ceil((off + n) / 4) bytes: a load past the end that the kernel does not zero shows up as T bases."""
    nb = (off + n + 3) // 4
    dev = torch.full((nb + 512,), 0xFF, dtype=torch.uint8, device="cuda")
    a = 64 + shift
    if nb:
        dev[a: a + nb] = torch.from_numpy(data[:nb]).cuda()
    d = dev[a: a + nb]
    assert d.numel() == nb and (nb == 0 or d.data_ptr() % 16 == a % 16)
    return d, dev


# the lengths of (a): name -> (blocks per lane, length as a function of l, w and the generator)
def _length_kinds():
    kinds = {
        "0": (None, lambda l, w, rng: 0),
        "l-1": (None, lambda l, w, rng: l - 1),
        "l": (None, lambda l, w, rng: l),
        "l+1": (None, lambda l, w, rng: l + 1),
        "l+31": (None, lambda l, w, rng: l + 31),
        "300k": (0, lambda l, w, rng: 300_000 + int(rng.integers(-500, 500))),
    }
    for nblk in (1, 2):
        for t in (1, 2):
            for d in (-1, 0, 1):
                kinds[f"tile nblk={nblk} t={t} d={d}"] = (
                    nblk, lambda l, w, rng, nblk=nblk, t=t, d=d: LANES * nblk * w * t + l - 1 + d)
    return kinds


OFFSETS = [0, 1, 2, 3, 17]


def _draw_cases(sm, canonical, seed, per_combo=4):
    """A seeded sample of the product (k, mode) x window sizes x lengths x offsets x pointer shifts: every (k, mode)
    per_combo times, the length kinds, base offsets and pointer shifts in rotation so that each occurs."""
    rng = np.random.default_rng(seed)
    kinds = _length_kinds()
    combos = [(k, mode) for _ in range(per_combo) for k in K_LONG for mode in (0, 1, 2)
              if _windows(sm, k, canonical, mode)]

    def deal(values):  # every value about equally often, in random order
        reps = -(-len(combos) // len(values))
        return [values[j] for j in rng.permutation(np.repeat(np.arange(len(values)), reps))[:len(combos)]]
    names, offs, shifts = deal(list(kinds)), deal(OFFSETS), deal([0, 1, 2, 3])
    cases = []
    for i, (k, mode) in enumerate(combos):
        sk = mode == 0 and bool(rng.integers(0, 2))
        nblk, fn = kinds[names[i]]
        w = int(rng.choice(_windows(sm, k, canonical, mode, sk)))
        if nblk is None:
            nblk = int(rng.choice([0, 1, 2]))
        cases.append(dict(k=k, w=w, mode=mode, sk=sk, kind=names[i], nblk=nblk, n=max(0, fn(k + w - 1, w, rng)),
                          off=offs[i], shift=shifts[i]))
    # the smallest shapes whose hash-in stream starts outside every lane's own TILE: one block per lane and a window size
    # with 256 w < k (w = 5 for k = 4097: a tile of 1 280 windows; w = 1 or 2 for k = 1000), two and a bit tiles of it.
    # Here any prebuilt window size serves, not only the wanted ones.
    for k in (1000, 4097):
        for mode in (0, 1, 2):
            ws = [w for w in sm.prebuilt_flavour_window_sizes(canonical, False, mode, mode == 0)
                  if _feasible(k, w, canonical, mode) and LANES * w < k]
            if not ws:
                continue
            w = 5 if 5 in ws else min(ws)
            cases.append(dict(k=k, w=w, mode=mode, sk=mode == 0, kind="tile below k", nblk=1,
                              n=2 * LANES * w + 77 + k + w - 1, off=OFFSETS[(k + mode) % 5], shift=(k + mode) % 4))
    return cases


def _check_single(sm, oracle, gpu, torch, rng, canonical, c):
    k, w, mode, n, off = c["k"], c["w"], c["mode"], c["n"], c["off"]
    l = k + w - 1
    nw = max(0, n - l + 1)
    data = oracle.gen_packed(int(rng.integers(1 << 30)), off + n + 64)
    d, _keep = _device_seq(torch, data, off, n, c["shift"])
    b = sm.Builder(k, w, canonical, mode)
    out = torch.full((nw + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    sk = torch.full((nw + 8,), SENTINEL, dtype=torch.int32, device="cuda") if c["sk"] else None
    if c["sk"]:
        want, wsk = oracle.run(data, n, k, w, canonical=canonical, mode=mode, base_offset=off, super_kmers=True)
    else:
        want = oracle.run(data, n, k, w, canonical=canonical, mode=mode, base_offset=off)
    gpu.set_blocks_per_lane(c["nblk"])
    try:
        cnt = b.run_device(d, n, out, out_sk=sk, base_offset=off)
        assert nw == 0 or gpu.last_path() == sm.PATH_FUSED, c
        assert cnt == len(want), (c, cnt, len(want))
        assert np.array_equal(out[:cnt].cpu().numpy().view(np.uint32), want), c
        assert int(out[cnt].item()) == SENTINEL, c  # nothing written past the count
        if c["sk"]:
            assert np.array_equal(sk[:cnt].cpu().numpy().view(np.uint32), wsk), c
            assert int(sk[cnt].item()) == SENTINEL, c
        ranged = False
        if nw > 2 and mode != 0:  # a window sub-range equals the matching slice of the full answer
            a, e = sorted(int(x) for x in rng.integers(0, nw + 1, size=2))
            cc = b.run_device(d, n, out, base_offset=off, win_begin=a, win_end=e)
            sub = want[(want >= a) & (want < e)]
            assert np.array_equal(out[:cc].cpu().numpy().view(np.uint32), sub), (c, a, e)
            ranged = True
    finally:
        gpu.set_blocks_per_lane(0)
    return len(want), ranged


@pytest.mark.parametrize("canonical", [False, True])
def test_single_sequence_long_k(sm, oracle, gpu, canonical):
    """(a) Builder.run_device.  Canonical open syncmers need w odd and l = k + w - 1 odd, so they exist for odd k only:
    the coverage asserted below is every k with both strands and every mode that has a plan at all."""
    import torch
    cases = _draw_cases(sm, canonical, 4100 + canonical, per_combo=5 if canonical else 4)
    # ---- coverage, from the drawn list
    want_combos = {(k, mode) for k in K_LONG for mode in (0, 1, 2) if not (canonical and mode == 2 and k % 2 == 0)}
    assert {(c["k"], c["mode"]) for c in cases} == want_combos
    assert {c["kind"] for c in cases} == set(_length_kinds()) | {"tile below k"}
    assert {c["off"] for c in cases} == set(OFFSETS) and {c["shift"] for c in cases} == {0, 1, 2, 3}
    assert any(c["sk"] for c in cases) and {c["nblk"] for c in cases} == {0, 1, 2}
    assert {c["k"] for c in cases if c["kind"] == "tile below k"} == {1000, 4097}
    assert all(LANES * c["w"] < c["k"] for c in cases if c["kind"] == "tile below k")
    assert 140 <= len(cases) <= 165, len(cases)
    used_w = {c["w"] for c in cases}
    assert used_w <= set(sm.prebuilt_window_sizes(canonical)) and len(used_w) >= 4, used_w
    rng = np.random.default_rng(4200 + canonical)
    positions = ranges = 0
    for c in cases:
        p, r = _check_single(sm, oracle, gpu, torch, rng, canonical, c)
        positions += p
        ranges += r
    print("long k single", canonical, dict(cases=len(cases), positions=positions, ranges=ranges, w=sorted(used_w)))
    assert positions > 100_000 and ranges >= 20


@pytest.mark.parametrize("canonical", [False, True])
def test_generic_family_long_k(sm, oracle, gpu, canonical):
    """(b) mm_workspace_force_generic: every k of the list, three lengths, modes in rotation."""
    import torch
    rng = np.random.default_rng(4300 + canonical)
    seen = set()
    for i, k in enumerate(K_LONG):
        mode = i % 3
        if canonical and mode == 2 and k % 2 == 0:
            mode = 1
        w = int(rng.choice(_windows(sm, k, canonical, mode)))
        l = k + w - 1
        for j, n in enumerate((l, l + 1 + int(rng.integers(0, 40)), 20_000 + int(rng.integers(0, 50_000)))):
            c = dict(k=k, w=w, mode=mode, n=n, off=OFFSETS[(i + j) % 5], shift=(i + j) % 4)
            data = oracle.gen_packed(int(rng.integers(1 << 30)), c["off"] + n + 64)
            d, _keep = _device_seq(torch, data, c["off"], n, c["shift"])
            out = torch.full((n - l + 1 + 8,), SENTINEL, dtype=torch.int32, device="cuda")
            want = oracle.run(data, n, k, w, canonical=canonical, mode=mode, base_offset=c["off"])
            gpu.force_generic(True)
            try:
                cnt = sm.Builder(k, w, canonical, mode).run_device(d, n, out, base_offset=c["off"])
                assert gpu.last_path() == sm.PATH_GENERIC, c
            finally:
                gpu.force_generic(False)
            assert cnt == len(want) and np.array_equal(out[:cnt].cpu().numpy().view(np.uint32), want), c
            assert int(out[cnt].item()) == SENTINEL, c
        seen.add((k, mode))
    assert {k for k, _ in seen} == set(K_LONG) and {m for _, m in seen} == {0, 1, 2}


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [65, 99, 128, 1000])
def test_batch_long_k(sm, oracle, gpu, k, canonical):
    """(c) mm_run_batch_device: about 40 slices of one tensor (the lane-table route), then one 2 Mbp sequence beside two
    short ones (tiles per sequence); every slice against the oracle on that slice alone."""
    import torch
    rng = np.random.default_rng(4400 + k + canonical)
    # (canonical plans of even k need an even w, and in reads mode only minimizer positions are prebuilt at even w)
    mode = {65: 0, 99: 1, 128: 0, 1000: 0}[k] if canonical else {65: 0, 99: 1, 128: 2, 1000: 1}[k]
    # (the lane table runs the reads-mode kernel, the tiles the sequence-mode one: a window size prebuilt for both)
    seq_ws = set(sm.prebuilt_flavour_window_sizes(canonical, False, mode, False))
    w = int(rng.choice([w for w in _windows(sm, k, canonical, mode, reads=True) if w in seq_ws]))
    l = k + w - 1
    b = sm.Builder(k, w, canonical, mode)

    def run(lens, gaps):
        starts = np.concatenate([[0], np.cumsum(np.array(lens) + np.array(gaps))])[:len(lens)]
        total = int(starts[-1] + lens[-1])
        data = oracle.gen_packed(int(rng.integers(1 << 30)), total + 64)
        big = torch.from_numpy(data[: (total + 3) // 4]).cuda()  # exactly the bytes that hold bases
        d = [big[int(s) // 4:] for s in starts]
        offs_b = [int(s) % 4 for s in starts]
        out = torch.full((sum(lens) + 64,), SENTINEL, dtype=torch.int32, device="cuda")
        offs = sm.run_batch_device(b, d, lens, out, None, base_offsets=offs_b)
        assert gpu.last_path() == sm.PATH_FUSED
        host = out[: offs[-1] + 1].cpu().numpy()
        assert host[offs[-1]] == SENTINEL
        host = host.view(np.uint32)
        assert offs[0] == 0
        for i, n in enumerate(lens):
            want = oracle.run(data, n, k, w, canonical=canonical, mode=mode, base_offset=int(starts[i]))
            assert np.array_equal(host[offs[i]:offs[i + 1]], want), (k, w, canonical, mode, i, n, int(starts[i]))
        return offs[-1]

    lens = [0, l - 1, l, l + 1, 2 * l] * 2 + [int(x) for x in rng.integers(0, 20_001, size=30)]
    lens = [int(x) for x in rng.permutation(lens)]
    # gaps that walk the base offset of the starts through 0..3
    gaps = [int((4 - (n % 4)) % 4 + (i % 4)) for i, n in enumerate(lens)]
    assert {int(s) % 4 for s in np.concatenate([[0], np.cumsum(np.array(lens) + np.array(gaps))])[:len(lens)]} == {0, 1, 2, 3}
    total = run(lens, gaps)
    assert gpu.last_lane_table(), "a batch of short slices of one tensor takes the lane table"
    assert total > 1000
    # (the launcher keeps the lane table while the batch averages fewer than 750 000 windows per sequence that has one:
    # the long sequence is 2.5 Mbp so that three sequences pass that whatever the tile size)
    total = run([l + 3, 2_500_000 + int(rng.integers(0, 999)), 5000 + l], [1, 2, 0])
    assert not gpu.last_lane_table(), "a 2.5 Mbp sequence beside two short ones takes tiles of its own"
    assert total > 10_000


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [65, 99, 128, 1000])
def test_reads_long_k(sm, oracle, gpu, k, canonical):
    """(d) mm_run_reads_device: read_len in {l, l + 1, l + 200, 6 000} (the last one the lane-table launch), per-read
    lengths from 0..read_len, minimizers, both syncmers and super-k-mer indices at window sizes prebuilt for reads."""
    import torch
    rng = np.random.default_rng(4500 + k + canonical)
    flavours = [(0, False), (0, True), (1, False), (2, False)]
    checked = short = 0
    for mode, sk in flavours:
        ws = _windows(sm, k, canonical, mode, sk, reads=True)
        if not ws:
            # canonical plans of even k need an even w; closed and open syncmers and super-k-mer indices are prebuilt
            # for reads at odd w only (5 .. 31), so these flavours would compile: minimizer positions stand for them
            assert canonical and k % 2 == 0 and (mode, sk) != (0, False), (k, mode, sk)
            continue
        w = int(rng.choice(ws))
        l = k + w - 1
        b = sm.Builder(k, w, canonical, mode)
        for read_len in (l, l + 1, l + 200, 6000):
            n_reads = int(rng.integers(1, 60) if read_len == 6000 else rng.integers(150 if read_len == l + 200 else 1, 301))
            stride = read_len + int(rng.integers(0, 9))
            base = int(rng.integers(0, 4))
            span = base + n_reads * stride + 64
            data = oracle.gen_packed(int(rng.integers(1 << 30)), span)
            d = torch.from_numpy(data[: (base + n_reads * stride + 3) // 4]).cuda()
            lens_r = rng.integers(0, read_len + 1, size=n_reads)
            lens_r[rng.integers(0, n_reads)] = read_len  # (a full read, so that read_len = l has a window)
            d_lens = torch.from_numpy(lens_r.astype(np.int32)).cuda()
            outr = torch.full((n_reads * read_len + 8,), SENTINEL, dtype=torch.int32, device="cuda")
            outs = torch.full((n_reads * read_len + 8,), SENTINEL, dtype=torch.int32, device="cuda") if sk else None
            offr = torch.zeros(n_reads + 1, dtype=torch.int64, device="cuda")
            tot = sm.run_reads_device(b, d, n_reads, stride, read_len, outr, offr, read_lens=d_lens, base_offset=base,
                                      out_sk=outs)
            case = dict(k=k, w=w, canonical=canonical, mode=mode, sk=sk, read_len=read_len, n_reads=n_reads,
                        stride=stride, base=base)
            assert gpu.last_path() == sm.PATH_FUSED, case
            if read_len == 6000:
                assert gpu.last_lane_table(), case
            ho = offr.cpu().numpy()
            hp = outr[:tot + 1].cpu().numpy()
            assert ho[0] == 0 and ho[-1] == tot and hp[tot] == SENTINEL, case
            hp = hp.view(np.uint32)
            hs = outs[:tot].cpu().numpy().view(np.uint32) if sk else None
            which = range(n_reads) if n_reads <= 40 else rng.choice(n_reads, 40, replace=False)
            for r in which:
                m = int(lens_r[r])
                res = oracle.run(data, m, k, w, canonical=canonical, mode=mode, base_offset=base + int(r) * stride,
                                 super_kmers=sk)
                want, wsk = res if sk else (res, None)
                assert np.array_equal(hp[ho[r]:ho[r + 1]], want), (case, int(r), m)
                if sk:
                    assert np.array_equal(hs[ho[r]:ho[r + 1]], wsk), (case, int(r), m)
                checked += 1
                short += m < l
    assert checked > 40 and short > 0, (checked, short)  # (reads shorter than l occurred and gave nothing)


@pytest.mark.parametrize("k", [65, 99, 128, 1000])
def test_skip_ambiguous_long_k(sm, oracle, gpu, k):
    """(e) mm_run_skip_ambiguous_device, canonical: single Ns at about 1 / 200 and one run of 1-300 Ns, n up to 100 000;
    the same without any N.  With l up to 1 050 dense Ns skip almost every window: from the oracle's answers alone, one
    case keeps more than 100 positions and one keeps none."""
    import torch
    rng = np.random.default_rng(4600 + k)
    kept = []
    # (mode, n, one N per `density` bases; 0: none).  One N per 3 bases leaves no clean window of l >= 65 bases (a window is
    # clean with probability (2/3)^l < 4e-12); one per 2 000 leaves clean stretches far longer than l = 1 050.
    for i, (mode, n, density) in enumerate([(0, 100_000, 200), (1, 60_000, 2000), (0, 30_011, 0), (2, 40_000, 0),
                                            (0, 20_000, 3), (1, 0, 0)]):
        if mode == 2 and k % 2 == 0:
            mode = 1
        w = int(rng.choice(_windows(sm, k, True, mode)))
        l = k + w - 1
        if n == 0:
            n = l + 5
        a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n + 8)].copy()
        if density:
            a[rng.integers(0, n, size=max(1, n // density))] = ord("N")
            s0 = int(rng.integers(0, n))
            a[s0:s0 + int(rng.integers(1, 301))] = ord("N")
        a = a[:n]
        packed, amb = oracle.pack_ascii_n(a.tobytes())
        d_p, d_m = torch.from_numpy(packed).cuda(), torch.from_numpy(amb).cuda()
        out = torch.full((n + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        b = sm.Builder(k, w, True, mode)
        want = oracle.run_skip_ambiguous(packed, amb, n, k, w, mode=mode)
        c = b.run_skip_ambiguous_device(d_p, d_m, n, out)
        case = dict(k=k, w=w, mode=mode, n=n, density=density)
        assert gpu.last_path() == sm.PATH_FUSED, case
        assert c == len(want) and np.array_equal(out[:c].cpu().numpy().view(np.uint32), want), case
        assert int(out[c].item()) == SENTINEL, case
        if not density:  # no N at all: the plain canonical answer
            assert np.array_equal(want, oracle.run(packed, n, k, w, canonical=True, mode=mode)), case
        kept.append((density, len(want)))
    assert any(dn and c > 100 for dn, c in kept), kept
    assert any(dn and c == 0 for dn, c in kept), kept
