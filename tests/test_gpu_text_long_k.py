"""Byte text at k above 63 on the GPU, up to the fused text kernel's limit k = 1024 and across the hand-over to the
generic text family at k = 1025 / w = 129.  The checker is tests/text_checker.py on every case (pinned to the oracle and
to its own definition at these k by tests/test_long_k_cpu.py); batches are compared record by record with the checker
on that record alone, never with the single-text GPU path.  Exact equality everywhere.

What is new at long k: the k-character warm-up of every run of 33 k-mers, the staged span of kTextTile + 1 + w + k bytes,
the strand vote over l = k + w - 1 bytes, the t_out rotation R * k & 31 of the rolling tables (rot 8 and 16 make it zero
for the even k below), the batch collect stage's validity test with l up to 1 151, and the generic text family's plain
loads, which must stay inside a text of exactly n readable bytes."""
import numpy as np
import pytest

import text_checker as tc

pytestmark = pytest.mark.gpu

TILE = 8192  # windows of a tile of the fused text kernel (kTextTile)
SENTINEL = -7
KS = [64, 65, 100, 255, 256, 257, 511, 1000, 1023, 1024]
WS = [1, 2, 5, 11, 19, 37, 127, 128]  # 5, 11, 19: prebuilt W; the others: the run-time-w instance
ROTS = [1, 8, 16, 31]


def _ctor(sm, mode, canonical):
    if mode == 0:
        return sm.canonical_minimizers if canonical else sm.minimizers
    if mode == 1:
        return sm.canonical_closed_syncmers if canonical else sm.closed_syncmers
    return sm.canonical_open_syncmers if canonical else sm.open_syncmers


def _hasher(sm, which, canonical, seed=0):
    """'mul', 'dna', or 'rot<R>': random 256-entry tables, rotation R, non-zero xor constants."""
    if which == "mul":
        return sm.TextMulHasher(canonical=canonical)
    if which == "dna":
        return sm.TextHasher.from_dna(sm.NtHasher(canonical=canonical))
    rng = np.random.default_rng(1000 + seed)
    fw = rng.integers(0, 1 << 32, 256, dtype=np.uint64)
    rc = rng.integers(0, 1 << 32, 256, dtype=np.uint64)
    return sm.TextHasher.from_tables(fw, rc, rot=int(which[3:]), canonical=canonical,
                                     fw_xor=int(rng.integers(1, 1 << 32)), rc_xor=int(rng.integers(1, 1 << 32)))


HASHERS = ["mul", "dna"] + [f"rot{r}" for r in ROTS]
TEXTS = ["uniform", "two", "constant", "period3"]


def _text(kind, n, rng):
    if kind == "uniform":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "two":  # tie-heavy; 0xFF carries the strand vote's bit, 0x00 does not
        return np.where(rng.integers(0, 2, n) == 1, 255, 0).astype(np.uint8)
    if kind == "constant":
        return np.full(n, int(rng.integers(0, 256)), dtype=np.uint8)
    return np.resize(np.frombuffer(b"G\x00\xf3", dtype=np.uint8), n)


def _dev_text(torch, text, phase):
    """The text on the device with exactly len(text) readable bytes, `phase` bytes off a 16-byte boundary, in an
    allocation that holds 0xA5 in front of it and behind it."""
    n = len(text)
    dev = torch.full((n + 768,), 0xA5, dtype=torch.uint8, device="cuda")
    a = 256 + phase
    if n:
        dev[a: a + n] = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    d = dev[a: a + n]
    assert d.numel() == n and (n == 0 or d.data_ptr() % 16 == phase % 16)
    return d, dev


def _want(text, k, w, th, canonical, mode):
    r = tc.run(text, k, w, th, canonical, mode, super_kmers=mode == 0)
    return r if mode == 0 else (r, None)


def _run_and_compare(sm, gpu, torch, b, d, n, l, mode, want, wsk, path, tag):
    nw = max(0, n - l + 1)
    out = torch.full((nw + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    sk = torch.full((nw + 8,), SENTINEL, dtype=torch.int32, device="cuda") if mode == 0 else None
    cnt = b.run_text_device(d, n, out, out_sk=sk)
    if nw:  # (a text without a window launches nothing and leaves last_path as it was)
        assert gpu.last_path() == path, tag
    assert cnt == len(want), (tag, cnt, len(want))
    assert np.array_equal(out[:cnt].cpu().numpy().view(np.uint32), want), tag
    assert int(out[cnt].item()) == SENTINEL, tag  # nothing written past the count
    if sk is not None:
        assert np.array_equal(sk[:cnt].cpu().numpy().view(np.uint32), wsk), tag
        assert int(sk[cnt].item()) == SENTINEL, tag
    return cnt


# ------------------------------------------------------------------ (a) single text, fused


def _draw_single(canonical, seed, n_cases=60):
    """A seeded sample of k x w x mode x length x hasher x text: every k and every w that has a plan on this strand,
    the length kinds, hashers and texts dealt evenly."""
    rng = np.random.default_rng(seed)
    kinds = ["0", "l-1", "l", "l+1"] + [f"tile t={t} d={d}" for t in (1, 2) for d in (-1, 0, 1)] + ["random"]

    def deal(values, count):
        reps = -(-count // len(values))
        return [values[j] for j in rng.permutation(np.repeat(np.arange(len(values)), reps))[:count]]
    ks, ws = deal(KS, n_cases), deal(WS, n_cases)
    names, hs, ts = deal(kinds, n_cases), deal(HASHERS, n_cases), deal(TEXTS, n_cases)
    cases = []
    for i in range(n_cases):
        k, w = ks[i], ws[i]
        if canonical and (k + w - 1) % 2 == 0:  # keep l odd: another w of the other parity, dealt as evenly
            w = [x for x in WS if (k + x - 1) % 2 == 1][i % len([x for x in WS if (k + x - 1) % 2 == 1])]
        mode = int(rng.integers(0, 3))
        if mode == 2 and w % 2 == 0:
            mode = int(rng.integers(0, 2))
        l = k + w - 1
        name = names[i]
        if name == "random":
            n = int(rng.integers(10_000, 24_000 if k > 256 else 40_000))  # (k > 256: at most three tiles for the checker)
        elif name.startswith("tile"):
            t, d = int(name[7]), int(name.split("d=")[1])
            n = TILE * t + d + l - 1
        else:
            n = {"0": 0, "l-1": l - 1, "l": l, "l+1": l + 1}[name]
        cases.append(dict(k=k, w=w, mode=mode, kind=name, n=n, hasher=hs[i], text=ts[i], phase=int(rng.integers(0, 16))))
    return cases, kinds


@pytest.mark.parametrize("canonical", [False, True])
def test_single_text_long_k(sm, gpu, canonical):
    import torch
    cases, kinds = _draw_single(canonical, 5100 + canonical)
    assert {c["k"] for c in cases} == set(KS) and {c["w"] for c in cases} == set(WS)
    assert {c["kind"] for c in cases} == set(kinds) and {c["mode"] for c in cases} == {0, 1, 2}
    assert {c["hasher"] for c in cases} == set(HASHERS) and {c["text"] for c in cases} == set(TEXTS)
    rng = np.random.default_rng(5200 + canonical)
    total = 0
    for i, c in enumerate(cases):
        k, w, mode, n = c["k"], c["w"], c["mode"], c["n"]
        th = _hasher(sm, c["hasher"], canonical, seed=i)
        text = _text(c["text"], n, rng)
        want, wsk = _want(text, k, w, th, canonical, mode)
        d, _keep = _dev_text(torch, text, c["phase"])
        b = _ctor(sm, mode, canonical)(k, w).hasher(th)
        total += _run_and_compare(sm, gpu, torch, b, d, n, k + w - 1, mode, want, wsk, sm.PATH_FUSED, c)
    print("long k text single", canonical, dict(cases=len(cases), positions=total))
    assert total > 20_000


@pytest.mark.parametrize("k,w,canonical", [(1024, 128, False), (1024, 128, True), (1024, 5, False), (1023, 5, True)])
def test_every_alignment_at_the_k_limit(sm, gpu, k, w, canonical):
    """k = 1024 with w = 128 and w = 5 at a tile-boundary length (8 193 windows: a second tile of one window), the text at
    all 16 values of address & 15 (the kernel's sh / off0).  Canonical windows of w = 5 need an odd k: 1023."""
    import torch
    l = k + w - 1
    n = TILE + l
    rng = np.random.default_rng(5300 + w + canonical)
    text = _text("uniform", n, rng)
    text[3000:5000] = _text("two", 2000, rng)
    th = _hasher(sm, "rot16" if w == 128 else "rot31", canonical, seed=w)
    want, wsk = _want(text, k, w, th, canonical, 0)
    assert len(want) > 100
    b = _ctor(sm, 0, canonical)(k, w).hasher(th)
    for phase in range(16):
        d, _keep = _dev_text(torch, text, phase)
        assert d.data_ptr() & 15 == phase
        _run_and_compare(sm, gpu, torch, b, d, n, l, 0, want, wsk, sm.PATH_FUSED, (k, w, canonical, phase))


# ------------------------------------------------------------------ (b) window ranges


def _range_plan(k, w, canonical, mode):
    """Open syncmers need an odd w (128 -> 127) and canonical windows an odd l (k + 1, or k - 1 at the limit)."""
    if mode == 2 and w % 2 == 0:
        w -= 1
    if canonical and (k + w - 1) % 2 == 0:
        k = k + 1 if k < 1024 else k - 1
    return k, w


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k0,w0", [(1000, 11), (1024, 128)])
def test_window_ranges_long_k(sm, gpu, k0, w0, canonical):
    import torch
    rng = np.random.default_rng(5400 + k0 + canonical)
    for mode in (0, 1, 2):
        k, w = _range_plan(k0, w0, canonical, mode)
        l = k + w - 1
        nw = 3 * TILE - 517
        n = nw + l - 1
        text = _text("uniform" if mode != 1 else "two", n, rng)
        th = _hasher(sm, HASHERS[2 + mode + canonical], canonical, seed=mode)  # (random tables, rot 1 .. 31)
        want, wsk = _want(text, k, w, th, canonical, mode)
        d, _keep = _dev_text(torch, text, 3 + mode)
        b = _ctor(sm, mode, canonical)(k, w).hasher(th)
        _run_and_compare(sm, gpu, torch, b, d, n, l, mode, want, wsk, sm.PATH_FUSED, (k, w, canonical, mode))
        cuts = sorted({0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE, nw - 1, nw})
        parts, parts_sk = [], []
        for a, e in zip(cuts[:-1], cuts[1:]):
            o = torch.full((e - a + 1,), SENTINEL, dtype=torch.int32, device="cuda")
            s = torch.full((e - a + 1,), SENTINEL, dtype=torch.int32, device="cuda") if mode == 0 else None
            c = b.run_text_device(d, n, o, out_sk=s, win_begin=a, win_end=e)
            assert gpu.last_path() == sm.PATH_FUSED and int(o[c].item()) == SENTINEL
            parts.append(o[:c].cpu().numpy().view(np.uint32))
            if mode == 0:
                parts_sk.append(s[:c].cpu().numpy().view(np.uint32))
        # (a range's first window dedups against the window in front of the range: the parts join without repeats)
        assert np.array_equal(np.concatenate(parts), want), (k, w, canonical, mode)
        if mode == 0:
            assert np.array_equal(np.concatenate(parts_sk), wsk), (k, w, canonical, mode)


# ------------------------------------------------------------------ (c) dispatch limits

DISPATCH = [(1024, 128, "fused"), (1025, 5, "generic"), (1500, 11, "generic"), (1024, 129, "generic")]


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k0,w0,family", DISPATCH)
def test_dispatch_limits(sm, gpu, k0, w0, family, canonical):
    """The fused text kernel takes k <= 1024 and w <= 128, the generic text family everything beyond; results equal the
    checker on both sides.  Where the plan does not exist the neighbour on the same side of the limit stands in: open
    syncmers of w = 128 take w = 127, canonical windows with an even l take k - 1 at k = 1024 (1023 and w = 129 is
    generic by w alone) and k + 1 elsewhere (1501)."""
    import torch
    rng = np.random.default_rng(5500 + k0 + w0 + canonical)
    path = sm.PATH_FUSED if family == "fused" else sm.PATH_GENERIC
    for mode in (0, 1, 2):
        k, w = _range_plan(k0, w0, canonical, mode)
        assert (k <= 1024 and w <= 128) == (family == "fused")
        l = k + w - 1
        th = _hasher(sm, HASHERS[(mode + 2 * canonical + k0) % len(HASHERS)], canonical, seed=k0 + mode)
        b = _ctor(sm, mode, canonical)(k, w).hasher(th)
        for n in (l - 1, l, l + 1, 20_000):
            text = _text(TEXTS[(mode + n) % 2], n, rng)  # uniform / two symbols
            want, wsk = _want(text, k, w, th, canonical, mode)
            for phase in range(4):
                d, _keep = _dev_text(torch, text, phase)
                _run_and_compare(sm, gpu, torch, b, d, n, l, mode, want, wsk, path, (k, w, canonical, mode, n, phase))


# ------------------------------------------------------------------ (d) batches


def _sweep_starts(l, rng, s0):
    """1. lengths {0, 1, l-1, l, l+1, 2l, 8191, 8192, 8193, 20 000} permuted, with runs of empty records."""
    lens = [int(x) for x in rng.permutation([0, 1, l - 1, l, l + 1, 2 * l, 8191, 8192, 8193, 20_000])]
    lens[3:3] = [0] * 5
    lens += [0] * 3 + [l + 2]
    return np.concatenate([[s0], s0 + np.cumsum(lens)]).astype(np.uint64)


def _seam_starts(l, s0):
    """2. record boundaries (absolute text offsets) at -1, 0, +1 of a tile's first window and of a thread's first window,
    each group with records of at least 2 l bytes around it, and one boundary alone at each kind of place."""
    x = ((TILE + 1 + 2 * l + 40) // 32 + 1) * 32
    assert x % TILE != 0 and x + 1 + 2 * l < 2 * TILE
    y = ((2 * TILE + 2 * l) // 32 + 1) * 32
    starts = [s0, TILE - 1, TILE, TILE + 1, x - 1, x, x + 1, 2 * TILE, y + 1, y + 1 + 2 * l + 13]
    return np.array(starts, dtype=np.uint64)


def _dense_starts(l, rng, s0):
    """3. 3 000 records of 0-3 bytes between two records of 3 l bytes: more than kTextBnd = 2048 starts in one tile, the
    list read from global memory; none of the short records has a window."""
    lens = [3 * l] + [int(x) for x in rng.integers(0, 4, 3000)] + [3 * l]
    return np.concatenate([[s0], s0 + np.cumsum(lens)]).astype(np.uint64)


def _check_records(text, starts, pos, offs, idx, k, w, th, canonical, mode, cache, tag):
    """Every record's slice, every offset and the count against text_checker.run on the record alone."""
    n_rec = len(starts) - 1
    assert len(offs) == n_rec + 1 and offs[0] == 0 and offs[-1] == len(pos), tag
    kept = 0
    for r in range(n_rec):
        rec = text[int(starts[r]):int(starts[r + 1])]
        key = (int(starts[r]), int(starts[r + 1]))
        if key not in cache:
            cache[key] = _want(rec, k, w, th, canonical, mode)
        want, wsk = cache[key]
        assert offs[r + 1] - offs[r] == len(want), (tag, r, len(rec))
        assert np.array_equal(pos[offs[r]:offs[r + 1]], want), (tag, r, len(rec))
        if mode == 0:
            assert np.array_equal(idx[offs[r]:offs[r + 1]], wsk), (tag, r, len(rec))
        kept += len(want)
    return kept


def _batch_device(sm, gpu, torch, b, text, starts, mode, phase):
    n_chars = int(starts[-1])
    d, _keep = _dev_text(torch, text[:n_chars], phase)  # exactly n_chars readable bytes
    d_starts = torch.from_numpy(starts.view(np.int64)).cuda()
    out = torch.full((n_chars + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    sk = torch.full((n_chars + 8,), SENTINEL, dtype=torch.int32, device="cuda") if mode == 0 else None
    offs = torch.full((len(starts),), -1, dtype=torch.int64, device="cuda")
    cnt = sm.run_text_batch_device(b, d, d_starts, n_chars, out, offs, out_sk=sk)
    assert int(out[cnt].item()) == SENTINEL
    return (out[:cnt].cpu().numpy().view(np.uint32), [int(o) for o in offs.cpu().numpy()],
            sk[:cnt].cpu().numpy().view(np.uint32) if sk is not None else None)


BATCH_PLANS = [(k, w) for k in (65, 257, 1000, 1024) for w in (5, 37)]


@pytest.mark.parametrize("record_set", ["sweep", "seams", "dense"])
@pytest.mark.parametrize("k0,w", BATCH_PLANS)
def test_text_batches_long_k(sm, gpu, k0, w, record_set):
    """Forward windows at k, canonical windows at k (odd) or k - 1 (l must be odd); the mode follows the plan's place in
    the list, minimizers with super-k-mer indices.  Each record set with the first start at 0 and past 0 (the records
    keep their absolute places, so a seam stays on its tile or thread boundary)."""
    import torch
    pi = BATCH_PLANS.index((k0, w))
    sets = ["sweep", "seams", "dense"]
    kept = 0
    for canonical in (False, True):
        k = k0 - 1 if canonical and (k0 + w - 1) % 2 == 0 else k0
        l = k + w - 1
        mode = (pi + sets.index(record_set) + canonical) % 3
        rng = np.random.default_rng(5600 + 10 * pi + sets.index(record_set) + canonical)
        th = _hasher(sm, HASHERS[(pi + canonical) % len(HASHERS)], canonical, seed=pi)
        b = _ctor(sm, mode, canonical)(k, w).hasher(th)
        for s0 in (0, 13):
            srng = np.random.default_rng(5700 + pi)  # (the same records for both first starts)
            starts = {"sweep": lambda: _sweep_starts(l, srng, s0), "seams": lambda: _seam_starts(l, s0),
                      "dense": lambda: _dense_starts(l, srng, s0)}[record_set]()
            text = _text(TEXTS[(pi + canonical) % 2], int(starts[-1]), np.random.default_rng(5800 + pi))
            if record_set != "seams":
                text = np.concatenate([text[:s0][::-1], text[:len(text) - s0]])  # (the same records behind the prefix)
            cache = {}
            tag = (k, w, canonical, mode, record_set, s0)
            pos, offs, idx = _batch_device(sm, gpu, torch, b, text, starts, mode, phase=(pi + s0) % 16)
            assert gpu.last_path() == sm.PATH_FUSED, tag
            kept += _check_records(text, starts, pos, offs, idx, k, w, th, canonical, mode, cache, tag)
            if s0 == 0 and record_set == "sweep":  # the host entry point on the same records
                recs = [text[int(starts[r]):int(starts[r + 1])] for r in range(len(starts) - 1)]
                hp, ho, hi = sm.run_text_batch_host(b, recs, super_kmers=mode == 0)
                assert gpu.last_path() == sm.PATH_FUSED, tag
                assert np.array_equal(hp, pos) and ho == offs, tag
                if mode == 0:
                    assert np.array_equal(hi, idx), tag
    assert kept > 100


@pytest.mark.parametrize("canonical", [False, True])
def test_text_batch_generic_at_k_1025(sm, gpu, canonical):
    """k = 1025 over six records: one generic launch per record (MM_PATH_GENERIC), the same contract."""
    import torch
    k, w = 1025, 5
    l = k + w - 1
    rng = np.random.default_rng(5900 + canonical)
    th = _hasher(sm, "rot8", canonical, seed=3)
    lens = [l + 1, 0, l - 1, 3 * l + 7, l, 9000]
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    text = _text("uniform", int(starts[-1]), rng)
    for mode in (0, 1):
        b = _ctor(sm, mode, canonical)(k, w).hasher(th)
        pos, offs, idx = _batch_device(sm, gpu, torch, b, text, starts, mode, phase=1 + mode)
        assert gpu.last_path() == sm.PATH_GENERIC
        kept = _check_records(text, starts, pos, offs, idx, k, w, th, canonical, mode, {}, (canonical, mode))
        assert kept > 100
