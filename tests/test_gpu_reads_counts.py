"""Packed reads run with its two counts read on the DEVICE (mm_run_packed_reads_counts_*, fastx_pipeline_device): a FASTQ /
FASTA packer, the counts run and the reads values queue on one stream, one wait.  The texts are built from known reads, so
the records are known without a parser.  Every result is compared with the CPU oracle per read AND with
mm_run_packed_reads_device given the true counts as host arguments.  Workspaces run at one block per lane
(mm_workspace_set_blocks_per_lane), so a lane holds w windows and small reads already span lanes and tiles.  Every output
buffer is pre-filled with 0xA5 and has slack behind it: nothing behind the count or past offsets[max_records] may change,
and the starts table holds 0xA5 behind starts[n_records] - no address or length may come from there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL32 = int.from_bytes(bytes([FILL]) * 4, "little")
FILL64 = int.from_bytes(bytes([FILL]) * 8, "little")
SLACK = 64

# prebuilt reads-mode window sizes only: nothing compiles
FLAVOURS = {
    "fwd_min_k21_w11": dict(ctor="minimizers", k=21, w=11, canonical=False, mode=0, sk=False),
    "canon_min_k21_w11": dict(ctor="canonical_minimizers", k=21, w=11, canonical=True, mode=0, sk=False),
    "canon_min_k5_w5": dict(ctor="canonical_minimizers", k=5, w=5, canonical=True, mode=0, sk=False),
    "fwd_min_sk_k21_w11": dict(ctor="minimizers", k=21, w=11, canonical=False, mode=0, sk=True),
    "canon_closed_k15_w17": dict(ctor="canonical_closed_syncmers", k=15, w=17, canonical=True, mode=1, sk=False),
    "fwd_open_k15_w11": dict(ctor="open_syncmers", k=15, w=11, canonical=False, mode=2, sk=False),
}


@pytest.fixture(scope="module")
def ws1(sm, gpu):
    """A workspace of its own at one block per lane."""
    ws = sm.Workspace(0)
    ws.set_blocks_per_lane(1)
    yield ws
    ws.close()


def _builder(sm, ws, name):
    p = FLAVOURS[name]
    return getattr(sm, p["ctor"])(p["k"], p["w"]).workspace(ws), p


def _reads(rng, lengths, alphabet=b"ACGT"):
    return [rng.choice(list(alphabet), size=int(n)).astype(np.uint8).tobytes() for n in lengths]


def _mixed_lengths(rng, l, n=300, long_read=10000, empty_ends=False):
    """0, 1, l - 1, l, l + 1, a few hundred, one read of about 10 kbp (more than three tiles at one block per lane)."""
    edge = [0, 1, l - 1, l, l + 1]
    lens = [edge[i % len(edge)] if i % 3 == 0 else int(rng.integers(l, 400)) for i in range(n)]
    lens[n // 2] = long_read
    if empty_ends:
        lens[0] = lens[-1] = 0
    else:
        lens[0], lens[-1] = 150, l
    return lens


def _text(reads, fmt):
    out = bytearray()
    for i, s in enumerate(reads):
        if fmt == "fastq":
            out += b"@r%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n"
        else:
            out += b">r%d\n" % i + s + (b"\n" if s else b"")
    return bytes(out)


def _expected(oracle, reads, p, amb=False):
    """(per-read positions, per-read indices or None, offsets) from the oracle."""
    pos, idx, offs = [], [], [0]
    for s in reads:
        if amb:
            pk, am = oracle.pack_ascii_n(s)
            got = oracle.run_skip_ambiguous(pk, am, len(s), p["k"], p["w"], canonical=True, mode=p["mode"])
        else:
            pk = oracle.pack_ascii(s) if s else np.zeros(1, dtype=np.uint8)
            got = oracle.run(pk, len(s), p["k"], p["w"], canonical=p["canonical"], mode=p["mode"], super_kmers=p["sk"])
        if p["sk"]:
            pos.append(got[0])
            idx.append(got[1])
        else:
            pos.append(got)
        offs.append(offs[-1] + len(pos[-1]))
    cat = np.concatenate(pos).astype(np.uint32) if pos else np.zeros(0, np.uint32)
    cat_idx = np.concatenate(idx).astype(np.uint32) if p["sk"] and idx else None
    return cat, cat_idx, np.array(offs, dtype=np.uint64)


def _filled(n, dtype):
    import torch
    return torch.full((n * np.dtype(dtype).itemsize,), FILL, dtype=torch.uint8, device="cuda")


class Packed:
    """Text on the device and what an asynchronous packer leaves: packed bases, (ambiguity bits,) starts, counts."""

    def __init__(self, sm, ws, text, fmt, max_records, with_amb=False):
        import torch
        n = len(text)
        self.n_text = n
        self.max_records = max_records
        self.d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda() if n else None
        self.packed = _filled((n // 4 + 8 + 3) // 4 * 4 + 64, np.uint8)
        self.amb = _filled((n // 8 + 8 + 3) // 4 * 4 + 64, np.uint8) if with_amb else None
        self.starts = _filled(max_records + 1, np.uint64).view(torch.int64)
        self.counts = torch.zeros(2, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        L = sm.lib()
        head = (ws.h, C.c_void_p(self.d_text.data_ptr()) if n else None, n, C.c_void_p(self.packed.data_ptr()),
                self.packed.numel() // 4 * 4)
        tail = (C.c_void_p(self.starts.data_ptr()), None, max_records, C.c_void_p(self.counts.data_ptr()))
        if with_amb:
            f = L.mm_fastq_pack_n_device_async if fmt == "fastq" else L.mm_fasta_pack_n_device_async
            code = f(*head, C.c_void_p(self.amb.data_ptr()), self.amb.numel() // 4 * 4, *tail)
        else:
            f = L.mm_fastq_pack_device_async if fmt == "fastq" else L.mm_fasta_pack_device_async
            code = f(*head, *tail)
        assert code == 0, code


class Out:
    def __init__(self, cap, max_records, sk):
        import torch
        self.cap = cap
        self.pos_buf = _filled(cap + SLACK, np.uint32)
        self.sk_buf = _filled(cap + SLACK, np.uint32) if sk else None
        self.off_buf = _filled(max_records + 1 + SLACK, np.uint64)
        self.cnt_buf = _filled(1, np.uint64)
        self.pos = self.pos_buf.view(torch.int32)[:cap]
        self.sk = self.sk_buf.view(torch.int32)[:cap] if sk else None
        self.offs = self.off_buf.view(torch.int64)[: max_records + 1]
        self.count = self.cnt_buf.view(torch.int64)
        torch.cuda.synchronize()

    def host(self):
        import torch
        torch.cuda.synchronize()
        return (self.pos_buf.cpu().numpy().view(np.uint32), self.off_buf.cpu().numpy().view(np.uint64),
                self.sk_buf.cpu().numpy().view(np.uint32) if self.sk_buf is not None else None)


def counts_run(sm, ws, b, pk, sk=False, max_bases=None, max_records=None, cap=None):
    """Packer output -> the asynchronous counts run, nothing waited for in between; returns the Out (unchecked)."""
    max_records = pk.max_records if max_records is None else max_records
    max_bases = pk.n_text if max_bases is None else max_bases
    o = Out(max(pk.n_text, 1) if cap is None else cap, max_records, sk)
    sm.run_packed_reads_counts_device(b, pk.packed, pk.starts, pk.counts, o.pos, o.offs, o.sk, max_bases=max_bases,
                                      max_records=max_records, amb=pk.amb, sync=False, d_count=o.count)
    return o


def existing_run(sm, ws, b, pk, n, total_bases, sk=False):
    """mm_run_packed_reads_device (or its skip-ambiguous form) given the true counts as host arguments, on buffers filled
    the same way."""
    o = Out(max(pk.n_text, 1), pk.max_records, sk)
    cnt = C.c_uint64()
    vp = C.c_void_p
    if pk.amb is not None:
        code = sm.lib().mm_run_packed_reads_skip_ambiguous_device(
            b.plan().h, ws.h, vp(pk.packed.data_ptr()), pk.packed.numel(), 0, vp(pk.amb.data_ptr()), pk.amb.numel(), 0, n,
            vp(pk.starts.data_ptr()), total_bases, 0xFFFFFFFF, vp(o.pos.data_ptr()), o.cap, vp(o.offs.data_ptr()), C.byref(cnt))
    else:
        code = sm.lib().mm_run_packed_reads_device(
            b.plan().h, ws.h, vp(pk.packed.data_ptr()), pk.packed.numel(), 0, n, vp(pk.starts.data_ptr()), total_bases,
            0xFFFFFFFF, vp(o.pos.data_ptr()), vp(o.sk.data_ptr()) if sk else None, o.cap, vp(o.offs.data_ptr()), C.byref(cnt))
    assert code == 0, code
    return int(cnt.value), o


def check_case(sm, oracle, ws, name, reads, fmt, max_records, tight=False, want=None, with_amb=False):
    """One text through packer + counts run: against the oracle per read, against the existing call on the true counts,
    the filled tail, the count, and the fill bytes behind everything."""
    b, p = _builder(sm, ws, name)
    n = len(reads)
    total_bases = sum(len(s) for s in reads)
    text = _text(reads, fmt)
    pk = Packed(sm, ws, text, fmt, max_records, with_amb)
    o = counts_run(sm, ws, b, pk, sk=p["sk"], max_bases=total_bases if tight else None)
    ws.check()
    assert ws.last_lane_table()
    pos, offs, idx = o.host()
    assert [int(x) for x in pk.counts.cpu().numpy()] == [total_bases, n], "the text does not hold the reads it was built from"
    want_pos, want_idx, want_offs = want if want is not None else _expected(oracle, reads, p, with_amb)
    total = int(want_offs[-1])
    assert int(o.count.item()) == total
    assert np.array_equal(offs[: n + 1], want_offs), name
    assert (offs[n: max_records + 1] == total).all(), "the offsets' tail is not filled with the total"
    assert (offs[max_records + 1:] == FILL64).all(), "an offset past offsets[max_records] was written"
    assert np.array_equal(pos[:total], want_pos), name
    assert (pos[total:] == FILL32).all(), "a position at or past the count was written"
    if p["sk"]:
        assert np.array_equal(idx[:total], want_idx) and (idx[total:] == FILL32).all()
    cnt0, o0 = existing_run(sm, ws, b, pk, n, total_bases, sk=p["sk"])
    pos0, offs0, idx0 = o0.host()
    assert cnt0 == total and np.array_equal(pos, pos0) and np.array_equal(offs[: n + 1], offs0[: n + 1]), name
    if p["sk"]:
        assert np.array_equal(idx, idx0)
    return pk, o


# ------------------------------------------------------------------------------------------------------- flavours
@pytest.mark.parametrize("name", sorted(FLAVOURS))
def test_flavours_fastq_and_fasta_loose_and_tight(sm, oracle, ws1, name):
    p = FLAVOURS[name]
    l = p["k"] + p["w"] - 1
    rng = np.random.default_rng(sum(name.encode()))
    for empty_ends in (True, False):
        reads = _reads(rng, _mixed_lengths(rng, l, empty_ends=empty_ends))
        want = _expected(oracle, reads, p)
        n = len(reads)
        # loose bounds as a real caller has them, and tight ones (= the counts); FASTQ and FASTA
        check_case(sm, oracle, ws1, name, reads, "fastq", 2 * n + 7, tight=False, want=want)
        check_case(sm, oracle, ws1, name, reads, "fasta", n, tight=True, want=want)
        check_case(sm, oracle, ws1, name, reads, "fasta" if empty_ends else "fastq", 2 * n + 7, tight=empty_ends, want=want)


# ------------------------------------------------------------------------------------------------------- scan paths
def test_both_scan_paths(sm, oracle, ws1):
    """max_records <= 2048 takes two table kernels (every other test); above it four: few real records in a large table,
    and a real count past one block of 2048 reads."""
    name = "canon_min_k21_w11"
    rng = np.random.default_rng(11)
    few = _reads(rng, [int(x) for x in rng.integers(0, 600, size=100)])
    check_case(sm, oracle, ws1, name, few, "fastq", 3000)
    many = _reads(rng, [int(x) for x in rng.integers(28, 52, size=2100)])
    want = _expected(oracle, many, FLAVOURS[name])
    check_case(sm, oracle, ws1, name, many, "fastq", 5000, want=want)
    check_case(sm, oracle, ws1, name, many, "fasta", 2100, tight=True, want=want)


# ------------------------------------------------------------------------------------------------------- empties
@pytest.mark.parametrize("name", ["fwd_min_sk_k21_w11", "canon_closed_k15_w17"])
def test_empties_write_count_zero_and_every_offset_zero(sm, oracle, ws1, name):
    b, p = _builder(sm, ws1, name)
    l = p["k"] + p["w"] - 1
    rng = np.random.default_rng(5)
    short = _reads(rng, [0, 1, l - 1, 5, l - 1, 0, 2])
    for text, fmt, n in [(b"junk without a record\n\n", "fasta", 0), (b"", "fasta", 0), (b"", "fastq", 0),
                         (_text(short, "fastq"), "fastq", len(short)), (_text(short, "fasta"), "fasta", len(short))]:
        for max_records in (0, 9) if n == 0 else (n, 2 * n + 7):
            pk = Packed(sm, ws1, text, fmt, max_records)
            o = counts_run(sm, ws1, b, pk, sk=p["sk"])
            ws1.check()
            pos, offs, idx = o.host()
            assert int(pk.counts[1].item()) == n
            assert int(o.count.item()) == 0
            assert (offs[: max_records + 1] == 0).all() and (offs[max_records + 1:] == FILL64).all()
            assert (pos == FILL32).all() and (idx is None or (idx == FILL32).all())


# ------------------------------------------------------------------------------------------------------- refused
def test_counts_beyond_a_bound_are_refused_and_the_workspace_goes_on(sm, oracle, ws1):
    name = "canon_min_k21_w11"
    b, p = _builder(sm, ws1, name)
    rng = np.random.default_rng(3)
    reads = _reads(rng, [int(x) for x in rng.integers(40, 300, size=60)])
    total_bases = sum(len(s) for s in reads)
    text = _text(reads, "fastq")
    E = sm.ERR
    # (a) the packer's table is too small: it counts 60 records, tabulates 50; (b) the run's max_bases is below the bases
    for max_records, max_bases in ((50, None), (80, total_bases - 1)):
        pk = Packed(sm, ws1, text, "fastq", max_records)
        o = counts_run(sm, ws1, b, pk, max_bases=max_bases)
        with pytest.raises(sm.MinimizerError) as e:
            ws1.check()
        assert e.value.code == E["CAPACITY"]
        assert b"mm_run_packed_reads_counts_device" in sm.lib().mm_last_error()
        pos, offs, _ = o.host()
        assert int(o.count.item()) == 0
        assert (offs[: max_records + 1] == 0).all() and (offs[max_records + 1:] == FILL64).all()
        assert (pos == FILL32).all(), "d_out_pos was touched by a refused run"
        ws1.check()  # (reported once)
        # the synchronous form returns the true counts
        o2 = Out(len(text), max_records, False)
        out3 = (C.c_uint64 * 3)(9, 9, 9)
        vp = C.c_void_p
        code = sm.lib().mm_run_packed_reads_counts_device(
            b.plan().h, ws1.h, vp(pk.packed.data_ptr()), pk.packed.numel(), 0, len(text) if max_bases is None else max_bases,
            max_records, vp(pk.starts.data_ptr()), vp(pk.counts.data_ptr()), vp(o2.pos.data_ptr()), None, o2.cap,
            vp(o2.offs.data_ptr()), out3)
        assert code == E["CAPACITY"] and list(out3) == [0, total_bases, len(reads)]
        pos2, offs2, _ = o2.host()
        assert (offs2[: max_records + 1] == 0).all() and (pos2 == FILL32).all()
        ws1.check()  # (a synchronous run's error is not news for the check)
        # the same workspace then runs a good batch
        check_case(sm, oracle, ws1, name, reads, "fastq", 80)


# ------------------------------------------------------------------------------------------------------- no stale state
def test_big_small_big_on_one_workspace(sm, oracle, ws1):
    name = "fwd_min_k21_w11"
    p = FLAVOURS[name]
    rng = np.random.default_rng(17)
    big = _reads(rng, _mixed_lengths(rng, 31, n=400, long_read=12000))
    small = _reads(rng, [33, 0, 31, 90])
    want_big, want_small = _expected(oracle, big, p), _expected(oracle, small, p)
    check_case(sm, oracle, ws1, name, big, "fastq", 3000, want=want_big)
    check_case(sm, oracle, ws1, name, small, "fastq", 5, want=want_small)
    check_case(sm, oracle, ws1, name, small, "fasta", 4, tight=True, want=want_small)
    check_case(sm, oracle, ws1, name, big, "fasta", 407, want=want_big)


# ------------------------------------------------------------------------------------------------------- skip-ambiguous
@pytest.mark.parametrize("name", ["canon_min_k21_w11", "canon_closed_k15_w17"])
def test_skip_ambiguous_form(sm, oracle, ws1, name):
    p = FLAVOURS[name]
    l, w = p["k"] + p["w"] - 1, p["w"]
    rng = np.random.default_rng(23)
    reads = [bytearray(s) for s in _reads(rng, _mixed_lengths(rng, l, n=200, long_read=6000))]
    for i, s in enumerate(reads):
        if not len(s):
            continue
        kind = i % 5
        if kind == 0:
            s[0] = ord("N")                                  # a record's first base
        elif kind == 1:
            s[-1] = ord("n")                                 # ... its last
        elif kind == 2 and len(s) > l + w:
            s[l + w - 2: l + w + 1] = b"NNN"                 # across the seam of the first two lanes (w windows each)
        elif kind == 3 and len(s) > 3 * w + l:
            for q in range(w - 1, len(s) - 1, 7 * w):        # every seventh lane seam
                s[q] = ord("N")
    reads[100] = bytearray(b"N" * 77)
    reads = [bytes(s) for s in reads]
    for fmt, max_records in (("fastq", 2 * len(reads) + 7), ("fasta", len(reads))):
        check_case(sm, oracle, ws1, name, reads, fmt, max_records, with_amb=True)


def test_skip_ambiguous_form_wants_a_canonical_plan(sm, ws1):
    b, _ = _builder(sm, ws1, "fwd_min_k21_w11")
    pk = Packed(sm, ws1, b"@a\nACGTN\n+\nIIIII\n", "fastq", 4, with_amb=True)
    o = Out(16, 4, False)
    with pytest.raises(sm.MinimizerError) as e:
        sm.run_packed_reads_counts_device(b, pk.packed, pk.starts, pk.counts, o.pos, o.offs, amb=pk.amb, max_bases=16)
    assert e.value.code == sm.ERR["HASHER_NOT_CANONICAL"]


# ------------------------------------------------------------------------------------------------------- composition
@pytest.mark.parametrize("fmt,u128", [("fastq", False), ("fasta", True)])
def test_pipeline_packer_run_values_one_check(sm, oracle, ws1, fmt, u128):
    """packer -> counts run -> mm_values_*_reads_device_async with n_reads = max_records, one check: the existing values
    kernel follows a counts run as it is (the offsets' tail is filled, the starts behind n_records are never read)."""
    name = "canon_min_k21_w11" if not u128 else "canon_closed_k15_w17"
    b, p = _builder(sm, ws1, name)
    ln = p["k"] if p["mode"] == 0 else p["k"] + p["w"] - 1
    rng = np.random.default_rng(29)
    reads = _reads(rng, _mixed_lengths(rng, p["k"] + p["w"] - 1, n=150, long_read=5000, empty_ends=True))
    pipe = sm.fastx_pipeline_device(b, _text(reads, fmt), 2 * len(reads) + 7, fmt, values=True, u128=u128)
    recs, cnt, pos, offs, vals = pipe.finish()
    assert recs.lengths() == [len(s) for s in reads]
    want_pos, _, want_offs = _expected(oracle, reads, p)
    assert cnt == int(want_offs[-1])
    assert np.array_equal(offs.cpu().numpy().view(np.uint64), want_offs)
    assert np.array_equal(pos.cpu().numpy().view(np.uint32), want_pos)
    assert (pipe.offsets.cpu().numpy()[len(reads):] == cnt).all()
    got = vals.cpu().numpy().view(np.uint64)
    want = []
    for r, s in enumerate(reads):
        rp = want_pos[int(want_offs[r]): int(want_offs[r + 1])]
        if len(rp):
            v = oracle.values_u128(oracle.pack_ascii(s), ln, rp, True) if u128 else oracle.values_u64(oracle.pack_ascii(s), ln, rp, True)
            want.append(np.asarray(v, dtype=np.uint64).reshape(-1))
    want = np.concatenate(want) if want else np.zeros(0, np.uint64)
    assert np.array_equal(got, want)
    assert not pipe.values.cpu().numpy()[len(want):].any(), "a value at or past the count was written"


def test_pipeline_reports_a_table_that_was_too_small(sm, ws1):
    b, _ = _builder(sm, ws1, "canon_min_k21_w11")
    rng = np.random.default_rng(31)
    pipe = sm.fastx_pipeline_device(b, _text(_reads(rng, [50] * 12), "fastq"), 8, "fastq", values=True)
    with pytest.raises(sm.MinimizerError) as e:
        pipe.finish()
    assert e.value.code == sm.ERR["CAPACITY"] and "max_records was 8" in str(e.value)
    assert not pipe.values.cpu().numpy().any() and int(pipe.count.item()) == 0


# ------------------------------------------------------------------------------------------------------- refusals
def test_plans_without_a_lane_table_are_refused_before_anything_is_queued(sm, gpu):
    ws = sm.Workspace(0)
    try:
        rng = np.random.default_rng(37)
        text = _text(_reads(rng, [200] * 5), "fastq")
        for name_or_w, generic in (("canon_min_k21_w11", True), (129, False)):
            if generic:
                b, _ = _builder(sm, ws, name_or_w)
            else:
                b = sm.minimizers(21, name_or_w).workspace(ws)
            ws.force_generic(generic)
            pk = Packed(sm, ws, text, "fastq", 9)
            o = Out(len(text), 9, False)
            for sync in (False, True):
                with pytest.raises(sm.MinimizerError) as e:
                    sm.run_packed_reads_counts_device(b, pk.packed, pk.starts, pk.counts, o.pos, o.offs, max_bases=len(text),
                                                      sync=sync, d_count=None if sync else o.count)
                assert e.value.code == sm.ERR["BAD_MODE"] and "mm_run_packed_reads_device" in str(e.value)
            ws.check()
            pos, offs, _ = o.host()
            assert (pos == FILL32).all() and (offs == FILL64).all()
            assert int(o.cnt_buf.cpu().numpy().view(np.uint64)[0]) == FILL64
            ws.force_generic(False)
    finally:
        ws.close()


def test_prepare_reads_leaves_nothing_to_load_at_the_first_counts_run(sm, oracle, gpu):
    ws = sm.Workspace(0)
    try:
        ws.set_blocks_per_lane(1)
        name = "canon_closed_k15_w17"
        b, p = _builder(sm, ws, name)
        b.prepare(ws, sequence=False, reads=True)
        before = sm.jit_stats()
        rng = np.random.default_rng(41)
        check_case(sm, oracle, ws, name, _reads(rng, [0, 31, 500, 40, 2000]), "fastq", 17)
        after = sm.jit_stats()
        assert (after["compiled"], after["from_disk"], after["failed"]) == (before["compiled"], before["from_disk"],
                                                                            before["failed"]), (before, after)
    finally:
        ws.close()


# ------------------------------------------------------------------------------------------------------- C example
def test_c_example_runs(sm, gpu, tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    libdir = os.path.join(root, "simd-minimizers_amd")
    exe = str(tmp_path / "reads_counts_example")
    subprocess.run(["g++", "-std=c++17", "-O2", "-x", "c++", "-I" + os.path.join(root, "include"), "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", "-o", exe, os.path.join(here, "cxx", "reads_counts_example.cpp"),
                    "-L" + libdir, "-lsimd_minimizers_amd", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
