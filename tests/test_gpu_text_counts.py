"""Text batch run and values with their two counts read on the DEVICE (mm_run_text_batch_counts_*,
mm_values_*_text_batch_counts_*, fasta_text_pipeline_device).  Expected values are the existing calls given the same counts
as host arguments (mm_run_text_batch_device, values_text_batch_device), on buffers filled the same way - so the comparison
is of whole buffers, bit for bit - and tests/text_checker.py per record.  Every output buffer is pre-filled with 0xA5 and has
slack behind it: nothing at or past the count, past `capacity`, or past offsets[n_records] may change."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import text_checker as tc

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL32 = int.from_bytes(bytes([FILL]) * 4, "little")
FILL64 = int.from_bytes(bytes([FILL]) * 8, "little")
TILE = 8192
SLACK = 64

# one plan of each kind: prebuilt-W instances (w = 5, 11) and run-time-w ones (w = 7, 2) both run
PLANS = {
    "fwd_min_sk_k7_w11": dict(ctor="minimizers", k=7, w=11, canonical=False, mode=0, sk=True),
    "canon_min_k21_w11": dict(ctor="canonical_minimizers", k=21, w=11, canonical=True, mode=0, sk=False),
    "fwd_closed_k5_w5": dict(ctor="closed_syncmers", k=5, w=5, canonical=False, mode=1, sk=False),
    "canon_open_k5_w7": dict(ctor="canonical_open_syncmers", k=5, w=7, canonical=True, mode=2, sk=False),
    "fwd_min_k3_w2": dict(ctor="minimizers", k=3, w=2, canonical=False, mode=0, sk=False),
}


def _plan(sm, name):
    p = PLANS[name]
    th = sm.TextMulHasher(canonical=p["canonical"])
    return getattr(sm, p["ctor"])(p["k"], p["w"]).hasher(th), th, p


def _filled(n, dtype):
    import torch
    return torch.full((n * np.dtype(dtype).itemsize,), FILL, dtype=torch.uint8, device="cuda")


class Case:
    """A text of max_chars bytes (random, non-zero; the first n_chars are the records), a starts table of max_records + 1
    entries (0xA5 past starts[n_records]) and the two counts, all on the device."""

    def __init__(self, text, starts, max_chars, max_records, counts=None, shift=0):
        import torch
        text = np.asarray(text, dtype=np.uint8)
        assert len(text) == max_chars
        self.text, self.starts = text, np.asarray(starts, dtype=np.uint64)
        self.n_rec = len(self.starts) - 1 if len(self.starts) else 0
        self.n_chars = int(self.starts[-1]) if len(self.starts) else 0
        self.max_chars, self.max_records = max_chars, max_records
        base = torch.from_numpy(np.concatenate([np.full(shift, 7, np.uint8), text])).cuda() if shift + max_chars else None
        self.d_text = base[shift:] if base is not None else None
        self._base = base
        tab = np.full(max_records + 1, FILL64, dtype=np.uint64)
        tab[: len(self.starts)] = self.starts
        self.d_starts = torch.from_numpy(tab.view(np.int64)).cuda()
        c = (self.n_chars, self.n_rec) if counts is None else counts
        self.d_counts = torch.from_numpy(np.array(c, dtype=np.uint64).view(np.int64)).cuda()
        self.true_counts = counts is None

    def records(self):
        return [self.text[int(self.starts[r]): int(self.starts[r + 1])] for r in range(self.n_rec)]


class Out:
    def __init__(self, case, cap, sk):
        import torch
        self.cap = cap
        self.pos_buf = _filled(cap + SLACK, np.uint32)
        self.sk_buf = _filled(cap + SLACK, np.uint32) if sk else None
        self.off_buf = _filled(case.max_records + 1 + SLACK, np.uint64)
        self.cnt_buf = _filled(1, np.uint64)
        self.pos = self.pos_buf.view(torch.int32)[:cap]
        self.sk = self.sk_buf.view(torch.int32)[:cap] if sk else None
        self.offs = self.off_buf.view(torch.int64)[: case.max_records + 1]
        self.count = self.cnt_buf.view(torch.int64)
        torch.cuda.synchronize()

    def host(self):
        import torch
        torch.cuda.synchronize()
        return (self.pos_buf.cpu().numpy().view(np.uint32), self.off_buf.cpu().numpy().view(np.uint64),
                self.sk_buf.cpu().numpy().view(np.uint32) if self.sk_buf is not None else None)


def run_counts(sm, gpu, b, case, cap=None, sk=False):
    """The asynchronous counts call and the one check; returns (count, positions buffer, offsets buffer, indices buffer,
    Out) - whole buffers, slack included."""
    cap = case.max_chars if cap is None else cap
    o = Out(case, cap, sk)
    sm.run_text_batch_counts_device(b, case.d_text, case.d_starts, case.d_counts, o.pos if cap else None, o.offs, o.sk if cap else None,
                                    max_chars=case.max_chars, d_count=o.count)
    gpu.check()
    pos, offs, idx = o.host()
    return int(o.count.item()), pos, offs, idx, o


def run_existing(sm, gpu, b, case, cap=None, sk=False):
    """mm_run_text_batch_device given the same counts as host arguments, on buffers filled the same way."""
    cap = case.max_chars if cap is None else cap
    o = Out(case, cap, sk)
    cnt = C.c_uint64()
    code = sm.lib().mm_run_text_batch_device(
        b.text_plan().h, gpu.h, C.c_void_p(case.d_text.data_ptr()) if case.d_text is not None else None, case.max_chars,
        case.n_rec, C.c_void_p(case.d_starts.data_ptr()), case.n_chars, C.c_void_p(o.pos.data_ptr()) if cap else None,
        C.c_void_p(o.sk.data_ptr()) if (sk and cap) else None, cap, C.c_void_p(o.offs.data_ptr()), C.byref(cnt))
    assert code in (0, sm.ERR["CAPACITY"]), code
    pos, offs, idx = o.host()
    return int(cnt.value), pos, offs, idx, o


def check_case(sm, gpu, name, case, oracle_records=True):
    """Counts call == existing call (whole buffers), fills intact behind the results, every record against text_checker."""
    b, th, p = _plan(sm, name)
    sk = p["sk"]
    cnt, pos, offs, idx, o = run_counts(sm, gpu, b, case, sk=sk)
    assert gpu.last_path() == sm.PATH_FUSED
    cnt0, pos0, offs0, idx0, _ = run_existing(sm, gpu, b, case, sk=sk)
    n_rec = case.n_rec
    assert cnt == cnt0, (name, cnt, cnt0)
    assert np.array_equal(pos, pos0) and np.array_equal(offs, offs0), name
    assert (pos[cnt:] == FILL32).all(), "a position at or past the count was written"
    assert (offs[n_rec + 1:] == FILL64).all(), "an offset past offsets[n_records] was written"
    assert offs[0] == 0 and offs[n_rec] == cnt
    if sk:
        assert np.array_equal(idx, idx0) and (idx[cnt:] == FILL32).all()
    if oracle_records:
        for r, rec in enumerate(case.records()):
            want = tc.run(rec, p["k"], p["w"], th, p["canonical"], p["mode"], super_kmers=sk)
            got = pos[int(offs[r]): int(offs[r + 1])]
            if sk:
                assert np.array_equal(got, want[0]) and np.array_equal(idx[int(offs[r]): int(offs[r + 1])], want[1]), (name, r)
            else:
                assert np.array_equal(got, want), (name, r)
    return cnt, pos, offs, o, b


def _text(rng, n, alphabet=None):
    if alphabet is None:
        return rng.integers(1, 256, n, dtype=np.uint8)  # (non-zero everywhere, also past n_chars)
    return alphabet[rng.integers(0, len(alphabet), n)]


def shape1(rng, l, alphabet=None):
    """Bound far above truth: 5 tiles of text, 100 characters in 3 records, 64 table entries."""
    return Case(_text(rng, 5 * TILE, alphabet), [0, 35, 70, 100], 5 * TILE, 64)


def shape2(rng, l, n, alphabet=None, shift=0):
    """Tile edges: n characters under a bound of 3 tiles; starts[0] > 0, an empty record, one shorter than l, one that
    starts in the last l - 1 bytes."""
    cuts = [c for c in [5, 5, 5 + l - 1, 3000, 8000, 8190, 8200, 12000] if c < n - 3]
    return Case(_text(rng, 3 * TILE, alphabet), cuts + [n - 3, n], 3 * TILE, 64, shift=shift)


def shape4(rng, alphabet=None):
    """3 000 records of 2-4 bytes: more than 2 048 record starts in one tile (the global-memory list)."""
    lens = rng.integers(2, 5, 3000)
    starts = np.concatenate([[0], np.cumsum(lens)])
    assert starts[2100] < TILE
    return Case(_text(rng, 3 * TILE, alphabet), starts, 3 * TILE, 4096)


@pytest.mark.parametrize("name", list(PLANS))
def test_bound_far_above_truth(sm, gpu, name):
    p = PLANS[name]
    check_case(sm, gpu, name, shape1(np.random.default_rng(1), p["k"] + p["w"] - 1))


@pytest.mark.parametrize("name", list(PLANS))
def test_tile_edges(sm, gpu, name):
    p = PLANS[name]
    l = p["k"] + p["w"] - 1
    rng = np.random.default_rng(2)
    for n in [8191, 8192, 8193, 16383, 16384]:
        case = shape2(rng, l, n)
        assert case.starts[0] > 0 and case.n_chars == n and n - int(case.starts[-2]) <= l - 1
        assert check_case(sm, gpu, name, case)[0] > 0


@pytest.mark.parametrize("name", list(PLANS))
def test_no_window_anywhere(sm, gpu, name):
    p = PLANS[name]
    l = p["k"] + p["w"] - 1
    rng = np.random.default_rng(3)
    for n_chars, n_rec in [(0, 0), (0, 5), (l - 1, 1), (50, 0)]:
        starts = [0] * (n_rec + 1) if n_chars == 0 else ([0, n_chars] if n_rec else [])
        case = Case(_text(rng, 2 * TILE), starts, 2 * TILE, 8, counts=(n_chars, n_rec))
        case.n_chars, case.n_rec, case.true_counts = n_chars, n_rec, True
        cnt, pos, offs, _, _ = check_case(sm, gpu, name, case, oracle_records=False)
        assert cnt == 0 and (offs[: n_rec + 1] == 0).all() and (pos == FILL32).all()
    # max_chars == 0: one tile is still launched, it writes offsets[0 .. n_records] and the count
    for n_rec in (0, 5):
        case = Case(np.zeros(0, np.uint8), [0] * (n_rec + 1), 0, 8, counts=(0, n_rec))
        case.n_chars, case.n_rec = 0, n_rec
        b, _, _ = _plan(sm, name)
        cnt, pos, offs, _, _ = run_counts(sm, gpu, b, case, cap=0)
        assert cnt == 0 and (offs[: n_rec + 1] == 0).all() and (offs[n_rec + 1:] == FILL64).all() and (pos == FILL32).all()


def test_more_record_starts_than_the_lds_list(sm, gpu):
    check_case(sm, gpu, "fwd_min_k3_w2", shape4(np.random.default_rng(4)))


@pytest.mark.parametrize("name", ["fwd_min_sk_k7_w11", "canon_open_k5_w7"])
def test_counts_beyond_the_bounds(sm, gpu, name):
    b, th, p = _plan(sm, name)
    rng = np.random.default_rng(5)
    good = shape2(rng, p["k"] + p["w"] - 1, 8193)
    for counts in [(good.n_chars, good.max_records + 1), (good.max_chars + 1, good.n_rec), (1 << 63, 1 << 63)]:
        bad = Case(good.text, good.starts, good.max_chars, good.max_records, counts=counts)
        o = Out(bad, bad.max_chars, p["sk"])
        vals = _filled(bad.max_chars, np.uint64)
        sm.run_text_batch_counts_device(b, bad.d_text, bad.d_starts, bad.d_counts, o.pos, o.offs, o.sk, d_count=o.count)
        import torch
        encoding = sm.TEXT_VALUES_DNA if p["canonical"] else sm.TEXT_VALUES_BYTES  # (BYTES has no canonical form)
        sm.values_text_batch_counts_device(b, bad.d_text, bad.d_starts, bad.d_counts, o.pos, o.offs, bad.max_chars,
                                           encoding, out=vals.view(torch.int64))
        with pytest.raises(sm.MinimizerError) as e:
            gpu.check()
        assert e.value.code == sm.ERR["CAPACITY"], e.value
        assert b"mm_run_text_batch_counts_device_async" in sm.lib().mm_last_error()
        pos, offs, idx = o.host()
        assert int(o.count.item()) == 0 and offs[0] == 0
        assert (offs[1:] == FILL64).all() and (pos == FILL32).all() and (idx is None or (idx == FILL32).all())
        assert bool((vals == FILL).all()), "the values call wrote something in the refused state"
        gpu.check()  # (the word was consumed)
        # the synchronous form: CAPACITY, the need 0 and the true counts from its one wait
        o2 = Out(bad, bad.max_chars, False)
        with pytest.raises(sm.MinimizerError) as e:
            sm.run_text_batch_counts_device(b, bad.d_text, bad.d_starts, bad.d_counts, o2.pos, o2.offs, wait=True)
        assert e.value.code == sm.ERR["CAPACITY"] and str(counts[0]) in str(e.value) and str(counts[1]) in str(e.value)
        out3 = (C.c_uint64 * 3)(9, 9, 9)
        code = sm.lib().mm_run_text_batch_counts_device(
            b.text_plan().h, gpu.h, C.c_void_p(bad.d_text.data_ptr()), bad.max_chars, bad.max_chars, bad.max_records,
            C.c_void_p(bad.d_starts.data_ptr()), C.c_void_p(bad.d_counts.data_ptr()), C.c_void_p(o2.pos.data_ptr()), None,
            bad.max_chars, C.c_void_p(o2.offs.data_ptr()), out3)
        assert code == sm.ERR["CAPACITY"] and list(out3) == [0, counts[0], counts[1]]
        gpu.check()
        # the next run on the same workspace is correct
        check_case(sm, gpu, name, good)


@pytest.mark.parametrize("name", ["fwd_min_sk_k7_w11", "canon_min_k21_w11", "fwd_closed_k5_w5"])
def test_capacity_below_the_need(sm, gpu, name):
    b, th, p = _plan(sm, name)
    case = shape2(np.random.default_rng(6), p["k"] + p["w"] - 1, 16383)
    need, pos_full, offs_full, idx_full, _ = run_counts(sm, gpu, b, case, sk=p["sk"])
    assert need > 100
    for cap in (need - 1, need // 2, 1):
        cnt, pos, offs, idx, _ = run_counts(sm, gpu, b, case, cap=cap, sk=p["sk"])
        assert cnt == need, "*d_count is the need"
        assert np.array_equal(pos[:cap], pos_full[:cap]) and (pos[cap:] == FILL32).all()
        if p["sk"]:
            assert np.array_equal(idx[:cap], idx_full[:cap]) and (idx[cap:] == FILL32).all()
        assert np.array_equal(offs, offs_full)
        cnt0, pos0, offs0, _, _ = run_existing(sm, gpu, b, case, cap=cap, sk=p["sk"])
        assert cnt0 == need and np.array_equal(pos, pos0) and np.array_equal(offs, offs0)
    # count only, and the synchronous form's three words
    cnt, pos, offs, _, _ = run_counts(sm, gpu, b, case, cap=0)
    assert cnt == need and (pos == FILL32).all() and np.array_equal(offs, offs_full)
    o = Out(case, need - 1, False)
    with pytest.raises(sm.MinimizerError) as e:
        sm.run_text_batch_counts_device(b, case.d_text, case.d_starts, case.d_counts, o.pos, o.offs, wait=True)
    assert e.value.code == sm.ERR["CAPACITY"] and str(need) in str(e.value)
    o = Out(case, need, False)
    assert sm.run_text_batch_counts_device(b, case.d_text, case.d_starts, case.d_counts, o.pos, o.offs,
                                           wait=True) == (need, case.n_chars, case.n_rec)
    assert np.array_equal(o.host()[0][:need], pos_full[:need])


# ------------------------------------------------------------------ values

DNA = np.frombuffer(b"ACGT", dtype=np.uint8)


def _expect_values(text, starts, pos, offs, n_rec, encoding, length, canonical, u128):
    """Straight from the definition (include/simd_minimizers_amd.h): BYTES sum text[p + j] << 8j; DNA code (c >> 1) & 3,
    fwd = sum code << 2j, rc = sum (code ^ 2) reversed, min of the two when canonical.  Python integers, then {lo, hi}."""
    out = []
    for r in range(n_rec):
        for i in range(int(offs[r]), int(offs[r + 1])):
            q = int(starts[r]) + int(pos[i])
            s = [int(c) for c in text[q: q + length]]
            if encoding == 0:
                v = sum(c << (8 * j) for j, c in enumerate(s))
            else:
                codes = [(c >> 1) & 3 for c in s]
                v = sum(c << (2 * j) for j, c in enumerate(codes))
                if canonical:
                    v = min(v, sum((c ^ 2) << (2 * j) for j, c in enumerate(reversed(codes))))
            out += [v & (2**64 - 1), v >> 64] if u128 else [v]
    return np.array(out, dtype=np.uint64)


VALUE_PLANS = [("fwd_min_sk_k7_w11", 0, None), ("canon_min_k21_w11", 1, DNA), ("fwd_min_k3_w2", 0, None)]


@pytest.mark.parametrize("u128", [False, True])
@pytest.mark.parametrize("name,encoding,alphabet", VALUE_PLANS)
@pytest.mark.parametrize("shape", ["bound_above", "tile_edges", "many_starts"])
def test_values(sm, gpu, shape, name, encoding, alphabet, u128):
    import torch
    b, th, p = _plan(sm, name)
    l = p["k"] + p["w"] - 1
    rng = np.random.default_rng(7)
    cases = {"bound_above": lambda: [shape1(rng, l, alphabet)],
             "tile_edges": lambda: [shape2(rng, l, n, alphabet) for n in (8192, 16383)],
             "many_starts": lambda: [shape4(rng, alphabet)]}[shape]()
    per = 2 if u128 else 1
    for case in cases:
        o = Out(case, case.max_chars, False)
        got = _filled(per * (case.max_chars + SLACK), np.uint64)
        sm.run_text_batch_counts_device(b, case.d_text, case.d_starts, case.d_counts, o.pos, o.offs, d_count=o.count)
        sm.values_text_batch_counts_device(b, case.d_text, case.d_starts, case.d_counts, o.pos, o.offs, case.max_chars,
                                           encoding, u128=u128, out=got.view(torch.int64))
        gpu.check()  # (the one wait: run and values were queued back to back)
        cnt = int(o.count.item())
        pos, offs, _ = o.host()
        want = _filled(per * (case.max_chars + SLACK), np.uint64)
        sm.values_text_batch_device(b, case.d_text, case.d_starts[: case.n_rec + 1], case.n_chars, o.pos,
                                    o.offs[: case.n_rec + 1], case.max_chars, encoding, u128=u128, out=want.view(torch.int64))
        gpu.check()
        got, want = got.cpu().numpy().view(np.uint64), want.cpu().numpy().view(np.uint64)
        assert np.array_equal(got, want), (shape, name)
        assert (got[per * cnt:] == FILL64).all(), "a value at or past the count was written"
        exp = _expect_values(case.text, case.starts, pos, offs, case.n_rec, encoding, b.text_plan().value_len(),
                             p["canonical"], u128)
        assert len(exp) == per * cnt and np.array_equal(got[: per * cnt], exp), (shape, name)
        if shape == "many_starts" and name == "fwd_min_k3_w2":
            assert cnt > 0 and case.n_rec > sm.values_text_lds_stage()  # (a workgroup's values span more records than its stage)


# ------------------------------------------------------------------ pipeline

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)


def _protein_fasta(rng, n_rec=200):
    parts = [b"junk in front of the first header\nMORE\n"]
    for i in range(n_rec):
        m = 0 if i == 17 else int(rng.integers(1, 700))
        nl = b"\r\n" if 40 <= i < 60 else b"\n"  # (one CRLF stretch)
        s = AA[rng.integers(0, 20, m)].tobytes()
        parts.append(b">sp|Q%05d|NAME_%d protein" % (i, i) + nl + nl.join(s[q:q + 60] for q in range(0, m, 60)) + (nl if m else b""))
    return b"".join(parts)


def test_pipeline_file_to_values_on_one_stream(sm, oracle, gpu):
    import torch
    text = _protein_fasta(np.random.default_rng(8))
    recs = oracle.fasta_records(text)
    assert len(recs) == 200 and any(len(s) == 0 for _, _, s in recs)
    k, w = 7, 11
    th = sm.TextMulHasher(canonical=False)
    b = sm.minimizers(k, w).hasher(th)
    for u128 in (False, True):
        pipe = sm.fasta_text_pipeline_device(b, text, 256, encoding=sm.TEXT_VALUES_BYTES, u128=u128)
        got, cnt, pos, offs, vals = pipe.finish()
        assert gpu.last_path() == sm.PATH_FUSED
        # today's route: synchronous loader, synchronous run, values
        ref = sm.fasta_text_device(text, max_records=256)
        out = torch.full((max(ref.n_chars, 1),), -1, dtype=torch.int32, device="cuda")
        o2 = torch.full((len(ref) + 1,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        cnt2 = sm.run_fasta_text_device(b, ref, out, o2)
        v2 = sm.values_text_batch_device(b, ref.seq, ref.starts, ref.n_chars, out, o2, cnt2, sm.TEXT_VALUES_BYTES, u128=u128)
        gpu.check()
        assert len(got) == len(ref) == 200 and got.n_chars == ref.n_chars and cnt == cnt2
        assert torch.equal(got.seq, ref.seq) and torch.equal(got.starts, ref.starts)
        assert np.array_equal(got.text_pos, ref.text_pos)
        assert torch.equal(pos, out[:cnt]) and torch.equal(offs, o2) and torch.equal(vals, v2)
        # the oracle's reader and the checker, per record
        p, o = pos.cpu().numpy().view(np.uint32), offs.cpu().numpy()
        for r, (_, hdr, s) in enumerate(recs):
            assert np.array_equal(p[o[r]:o[r + 1]], tc.run(s, k, w, th)), r
            assert got.header(text, r) == hdr
        st = got.starts.cpu().numpy()
        exp = _expect_values(np.frombuffer(b"".join(s for _, _, s in recs), dtype=np.uint8), st, p, o, 200, 0, k, False, u128)
        assert np.array_equal(vals.cpu().numpy().view(np.uint64), exp)
    # a table too small for the file's records: the one check says so
    pipe = sm.fasta_text_pipeline_device(b, text, 100, encoding=sm.TEXT_VALUES_BYTES)
    with pytest.raises(sm.MinimizerError) as e:
        pipe.finish()
    assert e.value.code == sm.ERR["CAPACITY"]
    assert int(pipe.count.item()) == 0 and int(pipe.offsets[0].item()) == 0 and not bool(pipe.values.any())
    gpu.check()
    # the synchronous counts call on the loader's output: positions and both counts from one wait
    pipe = sm.fasta_text_pipeline_device(b, text, 256)
    got, cnt, pos, offs, vals = pipe.finish()
    assert vals is None
    out = torch.full((pipe.seq.numel(),), -1, dtype=torch.int32, device="cuda")
    o3 = torch.full((257,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    res = sm.run_text_batch_counts_device(b, pipe.seq, pipe.starts, pipe.counts, out, o3, wait=True)
    assert res == (cnt, got.n_chars, 200)
    assert torch.equal(out[:cnt], pos) and torch.equal(o3[:201], offs) and bool((o3[201:] == -1).all())


# ------------------------------------------------------------------ other behaviour

def test_plans_the_fused_text_kernel_does_not_take(sm, gpu):
    case = shape1(np.random.default_rng(9), 31)
    o = Out(case, case.max_chars, False)
    b = sm.minimizers(21, 11)
    gpu.force_generic(True)
    try:
        for wait in (False, True):
            with pytest.raises(sm.MinimizerError) as e:
                sm.run_text_batch_counts_device(b, case.d_text, case.d_starts, case.d_counts, o.pos, o.offs, wait=wait)
            assert e.value.code == sm.ERR["BAD_MODE"] and "mm_run_text_batch_device" in str(e.value)
    finally:
        gpu.force_generic(False)
    for wait in (False, True):
        with pytest.raises(sm.MinimizerError) as e:
            sm.run_text_batch_counts_device(sm.minimizers(21, 129), case.d_text, case.d_starts, case.d_counts, o.pos, o.offs,
                                            wait=wait)
        assert e.value.code == sm.ERR["BAD_MODE"] and "mm_run_text_batch_device" in str(e.value)
    gpu.check()  # (nothing was queued, nothing raised)
    pos, offs, _ = o.host()
    assert (pos == FILL32).all() and (offs == FILL64).all()


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_unaligned_text(sm, gpu, shift):
    rng = np.random.default_rng(10 + shift)
    for name in ("canon_min_k21_w11", "fwd_min_k3_w2"):
        p = PLANS[name]
        case = shape2(rng, p["k"] + p["w"] - 1, 16384, shift=shift)
        assert case.d_text.data_ptr() % 4 == shift
        check_case(sm, gpu, name, case)


def test_first_counts_run_after_prepare_loads_nothing(sm, gpu):
    b, th, p = _plan(sm, "canon_open_k5_w7")
    rep = b.prepare(text=True)
    assert rep["unavailable"] == 0 and rep["compiled"] == 0 and rep["kernels"] >= 3, rep
    before = sm.jit_stats()
    check_case(sm, gpu, "canon_open_k5_w7", shape1(np.random.default_rng(11), 11))
    after = sm.jit_stats()
    for key in ("compiled", "from_disk", "failed"):
        assert after[key] == before[key], (before, after)
    assert b.prepare(text=True) == rep


def test_cxx_text_counts_example(gpu, tmp_path):
    """The C mirror: file bytes -> loader -> counts run -> values through the C ABI, one check at the end
    (tests/cxx/text_counts_example.cpp)."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    exe = str(tmp_path / "text_counts_example")
    libdir = os.path.join(root, "simd-minimizers_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(root, "include"), "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", "-o", exe, os.path.join(here, "cxx", "text_counts_example.cpp"),
                    "-L" + libdir, "-lsimd_minimizers_amd", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
