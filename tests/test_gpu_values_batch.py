"""K-mer values of every sequence of a device batch in one launch (mm_values_u64_batch_device_async /
mm_values_u128_batch_device_async, mm_device_group_values_batch): every expectation is the oracle's values_u64 /
values_u128 per sequence on a host copy of that sequence's bytes, bit-exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT = -0x0123456789ABCDEF  # what the value buffers hold before a call
PAD = 64                    # zero bytes behind a host copy: what a position past the end reads


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _u64s(values):
    return (C.c_uint64 * max(len(values), 1))(*[int(v) for v in values])


def _call(sm, ws, ptrs, nbytes, bases, lens, ln, canonical, d_pos, offs, d_out, u128=False, n_seqs=None):
    """The raw entry point: ptrs = device addresses (int / None), the other arrays host lists (None = a NULL array)."""
    f = sm.lib().mm_values_u128_batch_device_async if u128 else sm.lib().mm_values_u64_batch_device_async
    n = len(offs) - 1 if n_seqs is None else n_seqs
    return f(ws.h if ws is not None else None, n,
             (C.c_void_p * max(len(ptrs), 1))(*ptrs) if ptrs is not None else None,
             _u64s(nbytes) if nbytes is not None else None, _u64s(bases) if bases is not None else None,
             _u64s(lens) if lens is not None else None, ln, int(canonical), _vp(d_pos),
             _u64s(offs) if offs is not None else None, _vp(d_out))


def _device_values(sm, ws, ptrs, nbytes, bases, lens, ln, canonical, d_pos, offs, u128=False, slack=9):
    """One launch into a sentinel-filled buffer that is `slack` values longer than the count; returns the values after
    checking that the slack kept the sentinel."""
    import torch
    per, tot = (2 if u128 else 1), int(offs[-1])
    out = torch.full((per * (tot + slack),), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    sm._check(_call(sm, ws, ptrs, nbytes, bases, lens, ln, canonical, d_pos, offs, out, u128))
    ws.sync()
    ws.check()
    got = out.cpu().numpy()
    assert np.all(got[per * tot:] == SENT), "values past the count were written"
    got = got[: per * tot].view(np.uint64)
    return got.reshape(-1, 2) if u128 else got


def _expected(oracle, hosts, bases, pos, offs, ln, canonical, u128):
    """The oracle per sequence: hosts[s] = sequence s's own bytes (zero-padded), bases[s] its first base in them."""
    f = oracle.values_u128 if u128 else oracle.values_u64
    parts = [f(hosts[s], ln, pos[offs[s]: offs[s + 1]], canonical, base_offset=int(bases[s]))
             for s in range(len(offs) - 1) if offs[s + 1] > offs[s]]
    if not parts:
        return np.zeros((0, 2) if u128 else (0,), dtype=np.uint64)
    return np.concatenate(parts)


def _padded(a):
    return np.concatenate([a, np.zeros(PAD, dtype=np.uint8)])


def _synthetic(rng, seq_lens, counts, ln):
    """Sequence-local positions with pos + ln inside the sequence, back to back, and their offsets"""
    offs = np.zeros(len(counts) + 1, dtype=np.int64)
    offs[1:] = np.cumsum(counts)
    pos = np.zeros(int(offs[-1]), dtype=np.uint32)
    for s in np.flatnonzero(np.asarray(counts) > 0):
        assert seq_lens[s] >= ln
        pos[offs[s]: offs[s + 1]] = np.sort(rng.integers(0, seq_lens[s] - ln + 1, counts[s]))
    return pos, offs


def _slices(sm, seq_lens, counts, seed):
    """Sequences back to back from base 5 of one generated buffer, each handed over as its own {pointer, bytes, base
    offset}; sequences without values carry a NULL pointer and 0 bytes."""
    starts = np.zeros(len(seq_lens) + 1, dtype=np.int64)
    starts[0] = 5
    starts[1:] = 5 + np.cumsum(seq_lens)
    d = sm.generate_device(int(starts[-1]) + 64, seed)
    host = d.cpu().numpy()
    ptrs, nbytes, bases, hosts = [], [], [], []
    for s, n in enumerate(seq_lens):
        b0, bo = int(starts[s]) // 4, int(starts[s]) % 4
        nb = (bo + int(n) + 3) // 4
        if counts[s] == 0:
            ptrs.append(None), nbytes.append(0), bases.append(bo), hosts.append(None)
        else:
            ptrs.append(d.data_ptr() + b0), nbytes.append(nb), bases.append(bo), hosts.append(_padded(host[b0: b0 + nb]))
    return d, ptrs, nbytes, bases, hosts


PLANS = [  # (k, w, canonical, mode, u128): the value length is k for minimizers, k + w - 1 for syncmers
    (21, 11, True, 0, False),
    (21, 11, False, 0, False),
    (15, 17, False, 1, False),   # closed syncmers: len 31
    (31, 33, True, 1, True),     # canonical closed syncmers: len 63
]


@pytest.mark.parametrize("plan", PLANS, ids=["k21w11c", "k21w11f", "sync31", "u128sync63"])
def test_end_to_end(sm, oracle, gpu, plan):
    """About 300 sequences - empty, just too short, exactly one window, up to 3 000 bases, two of 200 kbp - half of them
    separate allocations, half slices of one tensor at every byte alignment, in shuffled address order; base offsets cover
    every 2-bit and dword phase.  Positions from run_batch_device, values against the oracle per sequence."""
    import torch
    k, w, canonical, mode, u128 = plan
    b = sm.Builder(k, w, canonical, mode)
    ln, l = (k if mode == 0 else k + w - 1), k + w - 1
    rng = np.random.default_rng(31)
    lens = [0, ln - 1, l - 1, l, l + 1] * 6 + [int(x) for x in rng.integers(16, 3001, 268)] + [200_000, 200_000]
    n = len(lens)
    bases = [s % 32 for s in range(n)]
    nbytes = [(bases[s] + lens[s] + 3) // 4 for s in range(n)]
    hosts = [rng.integers(0, 256, nbytes[s], dtype=np.uint8) for s in range(n)]
    slack = 80  # (the walk's loads run a few dwords past a sequence's last base: garbage there, never part of a value)
    # odd sequences: slices of one tensor, sequence s at byte alignment (s // 2) % 4
    at, cursor = {}, 0
    for s in range(1, n, 2):
        cursor = (cursor + 3) // 4 * 4 + (s // 2) % 4
        at[s] = cursor
        cursor += nbytes[s] + slack
    big_host = rng.integers(0, 256, cursor + 16, dtype=np.uint8)
    for s, a in at.items():
        big_host[a: a + nbytes[s]] = hosts[s]
    big = torch.from_numpy(big_host).cuda()
    run_t = []
    for s in range(n):
        if s in at:
            run_t.append(big[at[s]: at[s] + nbytes[s] + slack])
        else:
            run_t.append(torch.from_numpy(np.concatenate([hosts[s], rng.integers(0, 256, slack, dtype=np.uint8)])).cuda())
    order = rng.permutation(n)  # the batch order: addresses neither sorted nor of one allocation
    lens, bases, nbytes = [lens[s] for s in order], [bases[s] for s in order], [nbytes[s] for s in order]
    hosts, run_t = [_padded(hosts[s]) for s in order], [run_t[s] for s in order]
    assert {t.data_ptr() % 4 for t in run_t} == {0, 1, 2, 3}
    d_pos = torch.zeros(sum(lens) // 2 + 4096, dtype=torch.int32, device="cuda")
    offs = sm.run_batch_device(b, run_t, lens, d_pos, base_offsets=bases)
    tot = int(offs[-1])
    assert tot > 1024
    pos = d_pos[:tot].cpu().numpy().view(np.uint32)
    want = _expected(oracle, hosts, bases, pos, offs, ln, canonical, u128)
    # the values call gets every sequence's OWN bytes and no more
    got = _device_values(sm, gpu, [t.data_ptr() for t in run_t], nbytes, bases, lens, ln, canonical, d_pos, offs, u128)
    assert np.array_equal(got, want), plan
    # the wrapper takes len and canonical from the builder
    out = sm.values_batch_device(b, [t[:nb] for t, nb in zip(run_t, nbytes)], lens, d_pos, offs, base_offsets=bases, u128=u128)
    gpu.sync()
    got2 = out.cpu().numpy().view(np.uint64)
    assert np.array_equal(got2.reshape(-1, 2) if u128 else got2, want), plan


def _lookup_layouts(stage, per_block):
    """name -> (sequence lengths, values per sequence) of the layouts that steer the lookup"""
    e = stage + 50
    return {
        "straddle": ([40000] * 3, [1500, 1500, 1500]),
        "ladder": ([64] * (3 * stage), [1] * (3 * stage)),
        "empty_runs": ([0] * e + [30000] + [0] * e + [30000] + [0] * e, [0] * e + [1500] + [0] * e + [1501] + [0] * e),
        "single": ([100], [1]),
        "one_workgroup": ([50000], [per_block]),
        "one_workgroup_and_one": ([50000], [per_block + 1]),
    }


def _paths(offs, stage, per_block):
    """Which lookup path every workgroup takes, from the offsets alone: the sequences of its first and last value span
    r_last - r_first + 2 offsets, staged when they fit."""
    offs = np.asarray(offs, dtype=np.int64)
    tot = int(offs[-1])
    first = np.arange(0, tot, per_block)
    last = np.minimum(first + per_block, tot) - 1
    r_first = np.searchsorted(offs, first, "right") - 1
    r_last = np.searchsorted(offs, last, "right") - 1
    return ["lds" if x <= stage else "global" for x in (r_last - r_first + 2)]


@pytest.mark.parametrize("u128", [False, True], ids=["u64", "u128"])
def test_lookup_paths(sm, oracle, gpu, u128):
    """Both lookup paths and their edges on chosen layouts; positions are drawn inside every sequence (the kernel takes any
    position).  Before anything is launched the test works out from its own offsets and the exported stage size that some
    workgroup takes each path."""
    import torch
    rng = np.random.default_rng(32)
    stage = sm.values_batch_lds_stage()
    per_block = 256 if u128 else 1024
    ln, canonical = (47, True) if u128 else (21, True)
    cases, taken = {}, {}
    for name, (seq_lens, counts) in _lookup_layouts(stage, per_block).items():
        pos, offs = _synthetic(rng, seq_lens, counts, ln)
        cases[name] = (seq_lens, counts, pos, offs)
        taken[name] = set(_paths(offs, stage, per_block))
    assert any("global" in p for p in taken.values()), "no workgroup's span exceeds the stage"
    assert any("lds" in p for p in taken.values()), "no workgroup's span fits the stage"
    assert taken["empty_runs"] == {"lds", "global"} and taken["single"] == {"lds"}
    if not u128:
        assert taken["ladder"] == {"global"}  # (1 024 sequences per workgroup; the u128 kernel's 256 fit the stage)
    for name, (seq_lens, counts, pos, offs) in cases.items():
        d, ptrs, nbytes, bases, hosts = _slices(sm, seq_lens, counts, 80)
        tot = int(offs[-1])
        want = _expected(oracle, hosts, bases, pos, offs, ln, canonical, u128)
        # positions one element off a 16-byte boundary, and on it
        for shift in (1, 0):
            buf = torch.zeros(tot + 16 + shift, dtype=torch.int32, device="cuda")
            assert buf.data_ptr() % 16 == 0
            d_pos = buf[shift:]
            d_pos[:tot] = torch.from_numpy(pos.view(np.int32)).cuda()
            got = _device_values(sm, gpu, ptrs, nbytes, bases, seq_lens, ln, canonical, d_pos, offs, u128)
            assert np.array_equal(got, want), (name, shift)


def test_sequences_without_values_are_not_touched(sm, oracle, gpu):
    """Sequences without values carry NULL pointers and 0 bytes - also ones that claim bases - among sequences with values."""
    import torch
    rng = np.random.default_rng(33)
    seq_lens = [int(x) for x in rng.integers(100, 5000, 60)]
    counts = [0 if s % 3 == 1 else int(x) for s, x in enumerate(rng.integers(1, 90, 60))]
    counts[0] = counts[-1] = 0
    for u128, ln in ((False, 32), (True, 64)):
        pos, offs = _synthetic(rng, seq_lens, counts, ln)
        d, ptrs, nbytes, bases, hosts = _slices(sm, seq_lens, counts, 81)
        assert ptrs[0] is None and nbytes[1] == 0
        d_pos = torch.from_numpy(np.concatenate([pos, np.zeros(8, dtype=np.uint32)]).view(np.int32)).cuda()
        want = _expected(oracle, hosts, bases, pos, offs, ln, True, u128)
        got = _device_values(sm, gpu, ptrs, nbytes, bases, seq_lens, ln, True, d_pos, offs, u128)
        assert np.array_equal(got, want), u128


@pytest.mark.parametrize("u128", [False, True], ids=["u64", "u128"])
def test_bounds_per_sequence(sm, oracle, gpu, u128):
    """A sequence is a slice from the middle of a tensor filled with 0xFF, n_bases = 4 * packed_bytes.  Positions that hang
    1 .. len - 1 bases over its end give the value of the slice's bytes zero-extended: the neighbour's bytes were not read.
    The same at the slice's start, at every byte shift."""
    import torch
    rng = np.random.default_rng(34)
    ln = 64 if u128 else 32
    for nb in (37, 3, 64):
        for shift in range(4):
            big = torch.full((4096,), 0xFF, dtype=torch.uint8, device="cuda")
            assert big.data_ptr() % 4 == 0
            own = rng.integers(0, 256, nb, dtype=np.uint8)
            a = 1000 + shift
            big[a: a + nb] = torch.from_numpy(own).cuda()
            n_bases = 4 * nb
            over = [n_bases - ln + j for j in range(1, ln) if n_bases - ln + j >= 0]   # hang j bases over the end
            pos = np.array(sorted(set(list(range(0, min(16, n_bases))) + over)), dtype=np.uint32)
            offs = [0, len(pos)]
            d_pos = torch.from_numpy(np.concatenate([pos, np.zeros(8, dtype=np.uint32)]).view(np.int32)).cuda()
            want = _expected(oracle, [_padded(own)], [0], pos, offs, ln, True, u128)
            got = _device_values(sm, gpu, [big.data_ptr() + a], [nb], [0], [n_bases], ln, True, d_pos, offs, u128)
            assert np.array_equal(got, want), (nb, shift)
            # with a base offset: the same bytes, the k-mers two bases further on
            want = _expected(oracle, [_padded(own)], [2], pos, offs, ln, False, u128)
            got = _device_values(sm, gpu, [big.data_ptr() + a], [nb], [2], [n_bases - 2], ln, False, d_pos, offs, u128)
            assert np.array_equal(got, want), (nb, shift, "base offset")


def test_staging_reuse_back_to_back(sm, oracle, gpu):
    """Three calls with different tables and buffers queued back to back on one workspace with no wait in between: every
    result equals the oracle (no call overwrote a staging area whose copy was still in flight)."""
    import torch
    rng = np.random.default_rng(35)
    jobs = []
    for i, n_seqs in enumerate((300, 70, 1100)):
        seq_lens = [int(x) for x in rng.integers(60, 2000, n_seqs)]
        counts = [int(x) for x in rng.integers(0, 40, n_seqs)]
        pos, offs = _synthetic(rng, seq_lens, counts, 21)
        d, ptrs, nbytes, bases, hosts = _slices(sm, seq_lens, counts, 90 + i)
        d_pos = torch.from_numpy(np.concatenate([pos, np.zeros(8, dtype=np.uint32)]).view(np.int32)).cuda()
        out = torch.full((int(offs[-1]) + 5,), SENT, dtype=torch.int64, device="cuda")
        jobs.append((d, ptrs, nbytes, bases, seq_lens, d_pos, offs, out, _expected(oracle, hosts, bases, pos, offs, 21, True, False)))
    torch.cuda.synchronize()
    for (d, ptrs, nbytes, bases, seq_lens, d_pos, offs, out, want) in jobs:
        sm._check(_call(sm, gpu, ptrs, nbytes, bases, seq_lens, 21, True, d_pos, offs, out))
    gpu.sync()
    gpu.check()
    for i, (d, ptrs, nbytes, bases, seq_lens, d_pos, offs, out, want) in enumerate(jobs):
        got = out.cpu().numpy()
        tot = int(offs[-1])
        assert np.all(got[tot:] == SENT), i
        assert np.array_equal(got[:tot].view(np.uint64), want), i


def test_error_codes(sm, gpu):
    """Every refusal comes before anything is touched: the value buffer keeps its sentinel."""
    import torch
    E = sm.ERR
    d = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    d_pos = torch.zeros(16, dtype=torch.int32, device="cuda")
    out = torch.full((32,), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ptrs, nbytes, bases, lens, offs = [d.data_ptr(), d.data_ptr() + 512], [512, 512], [0, 3], [2048, 2045], [0, 2, 4]
    for u128, too_long in ((False, 33), (True, 65)):
        def call(ws=gpu, ptrs=ptrs, nbytes=nbytes, bases=bases, lens=lens, ln=21, d_pos=d_pos, offs=offs, out=out, n_seqs=None):
            return _call(sm, ws, ptrs, nbytes, bases, lens, ln, 1, d_pos, offs, out, u128, n_seqs)
        assert call(ws=None) == E["NULL"]
        assert call(ws=None, ln=0) == E["NULL"]
        for ln in (0, too_long):
            assert call(ln=ln) == E["VALUE_LEN"]
        for missing in ("ptrs", "nbytes", "lens", "d_pos", "offs", "out"):
            assert call(**{missing: None}, n_seqs=2) == E["NULL"], missing
        assert call(ptrs=[d.data_ptr(), None]) == E["NULL"]          # a sequence with values and no buffer
        assert call(offs=[0, 3, 2]) == E["UNSORTED"]
        assert call(lens=[2049, 2045]) == E["CAPACITY"]              # 512 bytes hold 2 048 bases
        assert call(lens=[2048, 2046]) == E["CAPACITY"]              # ... 2 045 behind a base offset of 3
        assert call(n_seqs=1 << 32) == E["LEN_TOO_LARGE"]
        # nothing to do: no sequences, no values (then nothing else is looked at)
        assert call(n_seqs=0, ptrs=None, nbytes=None, lens=None, d_pos=None, offs=None, out=None) == 0
        assert call(offs=[0, 0, 0], ptrs=None, nbytes=None, lens=None, d_pos=None, out=None) == 0
        gpu.sync()
        assert bool((out == SENT).all()), u128
        # and the same arguments without a fault are accepted
        assert call(bases=None, lens=[2048, 2048], ln=too_long - 1) == 0
        assert call(ptrs=[None, d.data_ptr()], nbytes=[0, 512], offs=[0, 0, 4]) == 0
        gpu.sync()
        gpu.check()
        out.fill_(SENT)
        torch.cuda.synchronize()


def _group_check(sm, oracle, devices):
    import torch
    rng = np.random.default_rng(36)
    n = 40
    lens = [int(x) for x in rng.integers(0, 50_001, n)]
    lens[0], lens[1] = 0, 50_000
    bases = [1 + s % 7 for s in range(n)]
    hosts = [rng.integers(0, 256, (bases[s] + lens[s] + 3) // 4, dtype=np.uint8) for s in range(n)]
    g = sm.DeviceGroup(devices)
    g.upload_batch(hosts)
    # no finished batch run yet
    with pytest.raises(sm.MinimizerError) as e:
        g.values_batch(sm.canonical_minimizers(21, 11))
    assert e.value.code == sm.ERR["NULL"]
    for (k, w, canonical, mode, u128) in (PLANS[0], PLANS[3]):
        b = sm.Builder(k, w, canonical, mode)
        ln = k if mode == 0 else k + w - 1
        counts = g.run_batch_device(b, lens, bases)
        with pytest.raises(sm.MinimizerError) as e:  # (the run invalidated what an earlier values_batch left)
            g.batch_values(0)
        assert e.value.code == sm.ERR["NULL"]
        assert g.values_batch(b, u128=u128) == sum(counts)
        f = oracle.values_u128 if u128 else oracle.values_u64
        entries = set()
        for s in range(n):
            host = _padded(hosts[s])
            pos = oracle.run(host, lens[s], k, w, canonical=canonical, mode=mode, base_offset=bases[s])
            assert len(pos) == counts[s], s
            entry, vals = g.batch_values(s)
            entries.add(entry)
            assert vals.device.index == devices[entry]
            got = vals.cpu().numpy().view(np.uint64)
            want = f(host, ln, pos, canonical, base_offset=bases[s])
            assert np.array_equal(got.reshape(-1, 2) if u128 else got, want), (s, u128)
        assert entries == set(range(len(devices)))
    # a new upload invalidates the run and its values
    g.upload_batch(hosts[:3])
    with pytest.raises(sm.MinimizerError) as e:
        g.values_batch(sm.canonical_minimizers(21, 11))
    assert e.value.code == sm.ERR["NULL"]
    with pytest.raises(sm.MinimizerError) as e:
        g.batch_values(0)
    assert e.value.code == sm.ERR["NULL"]
    g.close()


def test_device_group(sm, oracle, gpu):
    """A group of [0, 0] with 40 resident sequences of 0 .. 50 kbp at non-zero base offsets: upload_batch,
    run_batch_device, values_batch; every sequence's values from batch_values equal the oracle, u64 and u128."""
    _group_check(sm, oracle, [0, 0])


def test_device_group_two_devices(sm, oracle, gpu):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    _group_check(sm, oracle, [0, 1])


def test_cxx_values_batch_example_runs(oracle, gpu):
    """DeviceGroup::values_batch / batch_values through the header-only C++ mirror: the example checks itself against
    Output::values_* per sequence and prints a checksum of all values, recomputed here with the oracle."""
    exe = os.path.join(os.path.dirname(__file__), "cxx", "values_batch_example")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe), "-f", "values_batch_example.mk"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    m = re.search(r"u64 (\d+) values checksum ([0-9a-f]{16}); u128 (\d+) values checksum ([0-9a-f]{16})", r.stdout)
    assert m, r.stdout
    # the example's sequences: bytes of one xorshift64 stream, sequence s = 500 + 977 s bases from base s % 5 (3 and 7 empty)
    x, mask = 0x9E3779B97F4A7C15, (1 << 64) - 1
    seqs = []
    for s in range(12):
        n, off = (0 if s in (3, 7) else 500 + 977 * s), s % 5
        data = np.zeros((off + n + 3) // 4 + 1, dtype=np.uint8)
        for i in range(len(data)):
            x ^= (x << 13) & mask
            x ^= x >> 7
            x ^= (x << 17) & mask
            data[i] = (x >> 32) & 0xFF
        seqs.append((_padded(data), off, n))
    for (k, w, u128, n_got, c_got) in ((21, 11, False, m.group(1), m.group(2)), (43, 9, True, m.group(3), m.group(4))):
        h, count = 0xCBF29CE484222325, 0
        for host, off, n in seqs:
            pos = oracle.run(host, n, k, w, canonical=True, base_offset=off)
            vals = (oracle.values_u128 if u128 else oracle.values_u64)(host, k, pos, True, base_offset=off)
            for v in vals.reshape(-1):
                h = ((h ^ int(v)) * 0x100000001B3) & mask
            count += len(pos)
        assert (count, f"{h:016x}") == (int(n_got), c_got), (k, w)
