"""Queued asynchronous runs on a caller's NON-BLOCKING stream, bit-exact against the CPU oracle.

Every other GPU test binds its workspace to a stream that is ordered against the legacy default stream (the private
blocking stream of ``mm_workspace_create(..., NULL)`` or torch's current stream) and waits on the host after almost every
asynchronous call.  There, a kernel, a ``hipMemsetAsync`` or a copy that the library put on the wrong stream would still run
in order, and state that is only right because of stream order - the epoch-tagged status words, ``total[0..2]``, the window
ambiguity bits, the lane tables, the ring of text tables, the staging areas of the batch values - is never shared by
runs of different families that are all still queued.  Here it is: ``tests/stream_queue.py`` describes the scheme (own
``torch.cuda.Stream()``, inputs uploaded inside the queue over 0xA5, outputs over -7 with slack, a delay kernel in front).

Pass A: a fresh workspace and no delay (scratch grows - ``hipFree`` - in the middle of the queue, kernels load at first use).
Pass B: the same workspace, warm, behind a delay kernel of about 50 ms; for queues made only of calls the header documents
as not waiting, the host must get through the whole queue while the delay kernel still runs (``Queue.end(no_wait=True)``).
Each in the listed order and in two seeded permutations that keep the data dependencies.

The reads calls of Q1 are in the no-wait set: ``mm_run_reads_device_async`` with 2 000 reads of 150 bases takes the
one-lane-per-read launch, ``mm_run_packed_reads_device_async`` with a 40 kbp read the lane table; neither copies starts or
lengths to the host (only the per-read fallback - no reads-mode kernel for the plan - does, and waits for them)."""
import ctypes as C
import types

import numpy as np
import pytest

import stream_queue as sq
import text_checker as tc
from stream_queue import check_exact, check_positions, vp
from test_gpu_reads_counts import _expected as reads_expected
from test_gpu_reads_counts import _reads as random_reads
from test_gpu_reads_counts import _text as fastx_text
from test_gpu_text import _random_text_hasher
from test_gpu_text_counts import _expect_values as text_values_expected
from test_gpu_text_counts import _protein_fasta
from test_gpu_values_batch import _expected as batch_values_expected
from test_gpu_values_batch import _padded, _synthetic

pytestmark = pytest.mark.gpu

ORDERS = {"listed": None, "perm1": 101, "perm2": 202}
U64 = C.c_uint64
_REF = {}


def passes(q, order_seed, no_wait, expect=None, calls=None):
    """Pass A (fresh workspace, no delay) and pass B (warm, behind the delay) of one order."""
    order = q.order(order_seed, calls)
    q.run(order)
    q.finish(expect, calls, "pass A (fresh, no delay): ")
    q.run(order, delay=True, no_wait=no_wait)
    q.finish(expect, calls, "pass B (warm, delayed): ")


# ------------------------------------------------------------------------------------------------------- Q1: packed DNA
N_A, N_B, N_C, N_E, N_G = 3_000, 1_500_013, 250_007, 40_000, 200_000
RANGE_D = (70_001, 201_003)  # both ends inside tiles of every geometry (no multiple of 256 lanes x w windows)
READS_I = (2_000, 150)
LENS_J = [0, 20, 150, 5_000, 40_000]


def q1_ref(oracle):
    if "q1" in _REF:
        return _REF["q1"]
    r = types.SimpleNamespace()
    r.data = oracle.gen_packed(41, N_B + 64)
    r.a = oracle.run(r.data, N_A, 21, 11, canonical=True)
    r.b = oracle.run(r.data, N_B, 21, 11, canonical=True)
    r.c, r.c_sk = oracle.run(r.data, N_C, 21, 11, canonical=False, base_offset=3, super_kmers=True)
    # (d): the per-window stream of the range and the closed-syncmer rule on it, as _range_expect of test_gpu_round4.py
    # builds a range's minimizers (syncmers have no seam rule, src/syncmers.rs:166-169)
    k, w = 15, 17
    a, e = RANGE_D
    per_window = oracle.window_positions(r.data, N_C, k, w, oracle.default_hasher(True), True)
    idx = np.arange(a, e, dtype=np.uint32)
    sub = per_window[a:e]
    r.d = idx[(sub == idx) | (sub == idx + np.uint32(w - 1))]
    whole = oracle.run(r.data, N_C, k, w, canonical=True, mode=1)
    assert np.array_equal(r.d, whole[(whole >= a) & (whole < e)]) and e < N_C - (k + w - 1) + 1
    r.e = oracle.run(r.data, N_E, 5, 129, canonical=False)
    r.f = oracle.run(r.data, N_C, 31, 51, canonical=True)
    rng = np.random.default_rng(43)
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, N_G + 8)].copy()
    g[rng.integers(0, N_G, N_G // 200)] = ord("N")
    g[123_457: 123_457 + 300] = ord("N")
    r.g_packed, r.g_amb = oracle.pack_ascii_n(g.tobytes())
    r.g = oracle.run_skip_ambiguous(r.g_packed, r.g_amb, N_G, 21, 11)
    n_reads, rl = READS_I
    per_read = [oracle.run(r.data, rl, 21, 11, canonical=True, base_offset=rl * i) for i in range(n_reads)]
    r.i = np.concatenate(per_read)
    r.i_offs = np.concatenate([[0], np.cumsum([len(p) for p in per_read])]).astype(np.uint64)
    r.j_starts = np.concatenate([[0], np.cumsum(LENS_J)]).astype(np.uint64)
    per_read = [oracle.run(r.data, m, 21, 11, canonical=True, base_offset=int(s)) for m, s in zip(LENS_J, r.j_starts)]
    r.j = np.concatenate(per_read)
    r.j_offs = np.concatenate([[0], np.cumsum([len(p) for p in per_read])]).astype(np.uint64)
    assert len(per_read[0]) == 0 and len(per_read[1]) == 0 and len(per_read[2]) > 0
    r.k64 = oracle.values_u64(r.data, 21, r.b, True)
    r.k128 = oracle.values_u128(r.data, 31, r.d, True).reshape(-1)
    _REF["q1"] = r
    return r


def builders(sm):
    if "builders" not in _REF:
        b = dict(canon=sm.canonical_minimizers(21, 11), fwd=sm.minimizers(21, 11), sync=sm.canonical_closed_syncmers(15, 17),
                 long_w=sm.minimizers(5, 129), w51=sm.canonical_minimizers(31, 51))
        for x in b.values():
            x.plan()
        assert b["sync"].plan().value_len() == 31
        _REF["builders"] = b
    return _REF["builders"]


Q1_NEEDS = dict(a=("al",), b=("al",), c=("sh",), d=("al",), e=("al",), f=("al",), g=("g_packed", "g_amb"), h=("al",), i=("al",),
                j=("al", "j_starts"), k=("al",), l=("al",), m=("al",))


def q1_inputs(q, ref, which):
    make = dict(al=lambda: q.input(ref.data), sh=lambda: q.input(ref.data, shift=1), g_packed=lambda: q.input(ref.g_packed),
                g_amb=lambda: q.input(ref.g_amb), j_starts=lambda: q.input(ref.j_starts, index=True))
    names = [n for n in make if any(n in Q1_NEEDS[c] for c in which)]
    return {n: make[n]() for n in names}


def add_q1(q, sm, ref, which, ins=None, tag=""):
    """The packed-DNA calls that the letters of ``which`` name, on ``q``: (a) canonical k=21 w=11 on 3 000 bases, (b) the same
    on 1.5 Mbp, (c) forward with super-k-mer indices, base offset 3, pointer shifted one byte, (d) canonical closed syncmers
    over a window range, (e) w = 129 (generic family), (f) canonical k=31 w=51, (g) skip-ambiguous, (h) plan (a) on (b)'s data
    with capacity 1 000, (i) strided reads, (j) packed reads of mixed lengths (lane table), (k) values of (b) and (d),
    (l) an empty run, (m) (a) again.  ``ins``: the inputs of another queue to share (that
    queue uploads them; this one is ordered behind the uploads by an event)."""
    L, ws = sm.lib(), q.ws
    if ins is None:
        ins = q1_inputs(q, ref, which)
        for n, i in ins.items():
            q.upload("up_" + n, i)
    else:
        for n in ins:
            q.add("up_" + n, lambda: None)
    B = {n: b.workspace(ws) for n, b in builders(sm).items()}
    up = lambda c: tuple("up_" + n for n in Q1_NEEDS[c])  # noqa: E731

    def run(c, b, inp, n, want, cap=None, want_sk=None, name=None, **kw):
        name = tag + (name or c)
        l = b.k + b.w - 1
        cap = max(1, n - l + 1) if cap is None else cap
        out, cnt = q.output(cap), q.output(1, np.int64)
        sk = q.output(cap) if want_sk is not None else None

        def verify():
            check_positions(name, out, cnt, want, cap)
            if sk is not None:
                check_exact(name, sk, want_sk[:cap], "super-k-mer indices")

        q.add(name, lambda: b.run_device(inp.d, n, out.d, out_sk=sk.d if sk else None, sync=False, d_count=cnt.d, **kw),
              up(c), verify)
        return out, cnt

    outs = {}
    for c in which:
        if c == "a":
            outs[c] = run(c, B["canon"], ins["al"], N_A, ref.a)
        elif c == "b":
            outs[c] = run(c, B["canon"], ins["al"], N_B, ref.b)
        elif c == "c":
            run(c, B["fwd"], ins["sh"], N_C, ref.c, want_sk=ref.c_sk, base_offset=3)
        elif c == "d":
            outs[c] = run(c, B["sync"], ins["al"], N_C, ref.d, win_begin=RANGE_D[0], win_end=RANGE_D[1])
        elif c == "e":
            run(c, B["long_w"], ins["al"], N_E, ref.e)
        elif c == "f":
            run(c, B["w51"], ins["al"], N_C, ref.f)
        elif c == "g":
            out, cnt = q.output(N_G), q.output(1, np.int64)
            q.add(tag + "g", lambda out=out, cnt=cnt: B["canon"].run_skip_ambiguous_device(
                ins["g_packed"].d, ins["g_amb"].d, N_G, out.d, sync=False, d_count=cnt.d), up(c),
                lambda out=out, cnt=cnt: check_positions(tag + "g", out, cnt, ref.g))
        elif c == "h":
            run(c, B["canon"], ins["al"], N_B, ref.b, cap=1000)
        elif c == "i":
            n_i, len_i = READS_I
            out, cnt, offs = q.output(n_i * (len_i - 30)), q.output(1, np.int64), q.output(n_i + 1, np.int64)

            def verify_i(out=out, cnt=cnt, offs=offs):
                check_positions(tag + "i", out, cnt, ref.i)
                check_exact(tag + "i", offs, ref.i_offs, "offsets")

            q.add(tag + "i", lambda out=out, cnt=cnt, offs=offs: sm.run_reads_device(
                B["canon"], ins["al"].d, n_i, len_i, len_i, out.d, offs.d, d_count=cnt.d, sync=False), up(c), verify_i)
        elif c == "j":
            n_j, total_j = len(LENS_J), int(ref.j_starts[-1])
            out, cnt, offs = q.output(total_j), q.output(1, np.int64), q.output(n_j + 1, np.int64)

            def issue_j(out=out, cnt=cnt, offs=offs):
                sm._check(L.mm_run_packed_reads_device_async(
                    B["canon"].plan().h, ws.h, vp(ins["al"].d), ins["al"].d.numel(), 0, n_j, vp(ins["j_starts"].d), total_j,
                    max(LENS_J), vp(out.d), None, out.n, vp(offs.d), vp(cnt.d)))
                assert ws.last_lane_table(), "a 40 kbp read did not take the lane-table launch"

            def verify_j(out=out, cnt=cnt, offs=offs):
                check_positions(tag + "j", out, cnt, ref.j)
                check_exact(tag + "j", offs, ref.j_offs, "offsets")

            q.add(tag + "j", issue_j, up(c), verify_j)
        elif c == "k":
            # u64 values of (b)'s positions with the count read on the device: mm_values_u64_device_async takes n_pos from
            # the host, its reads form reads the true count from d_out_offsets[n_reads] - here ONE read from base 0, whose
            # offsets {0, count} the queue builds from (b)'s count word on the stream
            (out_b, cnt_b), (out_d, _) = outs["b"], outs["d"]
            offs2, v64 = q.output(2, np.int64, fill=0), q.output(out_b.n, np.int64)
            v128 = q.output(2 * len(ref.d), np.int64)

            def issue_k64():
                offs2.d[1:2].copy_(cnt_b.d[0:1], non_blocking=True)
                sm._check(L.mm_values_u64_reads_device_async(ws.h, vp(ins["al"].d), ins["al"].d.numel(), 0, 1, None, 0, 21, 1,
                                                             vp(out_b.d), vp(offs2.d), out_b.n, vp(v64.d)))

            q.add(tag + "k_u64", issue_k64, (tag + "b",), lambda: check_exact(tag + "k_u64", v64, ref.k64))
            # u128 values of (d)'s window indices (len = k + w - 1 = 31); n_pos is a host argument: the oracle's count
            q.add(tag + "k_u128", lambda: sm._check(L.mm_values_u128_device_async(
                ws.h, vp(ins["al"].d), ins["al"].d.numel(), 0, N_C, 31, 1, vp(out_d.d), len(ref.d), vp(v128.d))),
                (tag + "d",), lambda: check_exact(tag + "k_u128", v128, ref.k128))
        elif c == "l":
            run(c, B["canon"], ins["al"], 30, ref.a[:0])  # n = l - 1: no window, count 0, nothing written
        elif c == "m":
            run(c, B["canon"], ins["al"], N_A, ref.a, name="m")
    return ins


@pytest.mark.parametrize("order", list(ORDERS))
def test_q1_packed_dna_one_workspace(sm, oracle, gpu, order):
    """(a) .. (m) on one workspace: small behind big, the fused family behind the generic one (untagged status words, a
    cleared total), window ranges, skip-ambiguous bits uploaded in the queue, a capacity below the count, reads in both
    layouts, values that read a count word on the stream, an empty run.  No host wait anywhere in the queue."""
    q = sq.Queue(sm)
    add_q1(q, sm, q1_ref(oracle), "abcdefghijklm")
    passes(q, ORDERS[order], no_wait=True)
    q.close()


def test_q1_with_tile_ids_from_the_ticket(sm, oracle, gpu, monkeypatch):
    """The whole queue once more with MM_FORCE_TICKET=1: every fused launch clears and uses the workspace's one ticket."""
    monkeypatch.setenv("MM_FORCE_TICKET", "1")
    q = sq.Queue(sm)
    add_q1(q, sm, q1_ref(oracle), "abcdefghijklm")
    passes(q, None, no_wait=True)
    q.close()


@pytest.mark.parametrize("delay", [False, True], ids=["fresh", "delayed"])
def test_q1_synchronous_call_behind_unchecked_asynchronous_ones(sm, oracle, gpu, delay):
    """(a) .. (f) queued, then the synchronous run of plan (c) on the same workspace (it lets the queue drain before it
    reuses the result words), then the check: all seven results."""
    ref = q1_ref(oracle)
    q = sq.Queue(sm)
    ins = add_q1(q, sm, ref, "abcdef")
    out, sk = q.output(N_C - 30), q.output(N_C - 30)
    b = builders(sm)["fwd"].workspace(q.ws)
    for with_delay in ([False, True] if delay else [False]):
        q.run(q.order(), delay=with_delay)
        c = b.run_device(ins["sh"].d, N_C, out.d, out_sk=sk.d, base_offset=3)
        q.finish()
        assert c == len(ref.c)
        check_exact("sync c", out, ref.c, "positions")
        check_exact("sync c", sk, ref.c_sk, "super-k-mer indices")
    q.close()


# ------------------------------------------------------------------------------------------------------- Q4: two workspaces
def test_q4_two_workspaces_two_streams(sm, oracle, gpu):
    """Two Q1 queues on two workspaces and two non-blocking streams, issued alternately from one thread in different
    permutations; the inputs are shared (uploaded on the first stream, the second waits for an event), the outputs are
    not; each stream has its own delay kernel."""
    import torch
    ref = q1_ref(oracle)
    which = "abcdefghijklm"
    q1, q2 = sq.Queue(sm), sq.Queue(sm)
    ins = add_q1(q1, sm, ref, which)
    add_q1(q2, sm, ref, which, ins=ins)
    uploads = [c for c in q1.calls if c.name.startswith("up_")]
    work1 = [c for c in q1.calls if not c.name.startswith("up_")]
    work2 = [c for c in q2.calls if not c.name.startswith("up_")]
    for delay, (s1, s2) in ((False, (None, 7)), (True, (11, 12)), (True, (13, None))):
        q1.begin(delay)
        q2.begin(delay)
        for c in uploads:
            q1.issue(c)
        ev = torch.cuda.Event()
        ev.record(q1.s)
        q2.s.wait_event(ev)
        o1, o2 = q1.order(s1, work1), q2.order(s2, work2)
        for c1, c2 in zip(o1, o2):
            q1.issue(c1)
            q2.issue(c2)
        q1.end(no_wait=delay)
        q2.end(no_wait=delay)
        q1.finish()
        q2.finish()
    q2.close()
    q1.close()


# ------------------------------------------------------------------------------------------------------- pipelines (Q2, Q5)
def add_reads_pipeline(q, sm, oracle, tag, reads, fmt, plan, with_amb, max_records, refused=False, values=True):
    """FASTA / FASTQ text -> packer -> counts run (-> u64 values) as three calls of the queue.  ``refused``: max_records is
    below the text's records, so the run writes count 0 and offsets of 0, no position, and the check says MM_ERR_CAPACITY."""
    L, ws = sm.lib(), q.ws
    text = fastx_text(reads, fmt)
    n = len(text)
    b = getattr(sm, plan["ctor"])(plan["k"], plan["w"]).workspace(ws)
    b.plan()
    t_in = q.input(np.frombuffer(text, dtype=np.uint8))
    packed = q.output((n // 4 + 8 + 3) // 4 * 4 + 64, np.uint8)
    amb = q.output((n // 8 + 8 + 3) // 4 * 4 + 64, np.uint8) if with_amb else None
    starts, counts = q.output(max_records + 1, np.int64, fill=0), q.output(2, np.int64, fill=0)
    pos, offs, cnt = q.output(n), q.output(max_records + 1, np.int64), q.output(1, np.int64)
    vals = q.output(n, np.int64) if values else None
    want_pos, want_sk, want_offs = reads_expected(oracle, reads, plan, with_amb)
    sk = q.output(n) if plan["sk"] else None
    total_bases, n_rec = sum(len(s) for s in reads), len(reads)
    ln = plan["k"] if plan["mode"] == 0 else plan["k"] + plan["w"] - 1
    want_vals = [oracle.values_u64(oracle.pack_ascii(s), ln, want_pos[int(want_offs[r]): int(want_offs[r + 1])], plan["canonical"])
                 for r, s in enumerate(reads) if want_offs[r + 1] > want_offs[r]]
    want_vals = np.concatenate(want_vals) if want_vals else np.zeros(0, np.uint64)
    codes = np.concatenate([np.frombuffer(s, dtype=np.uint8) for s in reads] + [np.zeros(0, np.uint8)])
    want_packed = oracle.pack_ascii(codes.tobytes())[: total_bases // 4]
    up = codes & 0xDF
    want_amb = np.packbits(~((up == 65) | (up == 67) | (up == 71) | (up == 84)), bitorder="little")[: total_bases // 8]

    def issue_pack():
        head = (ws.h, vp(t_in.d), n, vp(packed.d), packed.n)
        tail = (vp(starts.d), None, max_records, vp(counts.d))
        if with_amb:
            f = L.mm_fastq_pack_n_device_async if fmt == "fastq" else L.mm_fasta_pack_n_device_async
            sm._check(f(*head, vp(amb.d), amb.n, *tail))
        else:
            f = L.mm_fastq_pack_device_async if fmt == "fastq" else L.mm_fasta_pack_device_async
            sm._check(f(*head, *tail))

    def verify_pack():
        assert [int(x) for x in counts.host()[:2]] == [total_bases, n_rec], (tag, "packer counts")
        m = n_rec + 1 if n_rec <= max_records else max_records  # (records past max_records are counted, not tabulated)
        want_starts = np.concatenate([[0], np.cumsum([len(s) for s in reads])]).astype(np.uint64)
        assert np.array_equal(starts.host()[:m].view(np.uint64), want_starts[:m]), (tag, "record starts")
        assert (starts.host()[max_records + 1:] == 0).all() and (counts.host()[2:] == 0).all(), (tag, "packer tables overrun")
        assert np.array_equal(packed.host()[: len(want_packed)].view(np.uint8), want_packed), (tag, "packed bases")
        assert (packed.host()[packed.n:] == -7).all(), (tag, "written past the packed capacity")
        if with_amb:
            assert np.array_equal(amb.host()[: len(want_amb)].view(np.uint8), want_amb), (tag, "ambiguity bits")
            assert (amb.host()[amb.n:] == -7).all(), (tag, "written past the ambiguity capacity")

    q.upload(tag + "up_text", t_in)
    q.add(tag + "pack", issue_pack, (tag + "up_text",), verify_pack)

    def issue_run():
        sm.run_packed_reads_counts_device(b, packed.d, starts.d, counts.d, pos.d, offs.d, sk.d if sk else None, max_bases=n,
                                          max_records=max_records, amb=amb.d if with_amb else None, sync=False, d_count=cnt.d)
        assert ws.last_lane_table()

    def verify_run():
        if refused:
            check_positions(tag + "run", pos, cnt, want_pos[:0])
            check_exact(tag + "run", offs, np.zeros(max_records + 1, np.uint64), "offsets of a refused run")
            if sk is not None:
                check_exact(tag + "run", sk, want_sk[:0], "indices of a refused run")
            return
        total = len(want_pos)
        check_positions(tag + "run", pos, cnt, want_pos)
        tail = np.full(max_records + 1 - n_rec, total, dtype=np.uint64)
        check_exact(tag + "run", offs, np.concatenate([want_offs[:n_rec], tail]), "offsets and their filled tail")
        if sk is not None:
            check_exact(tag + "run", sk, want_sk, "super-k-mer indices")

    q.add(tag + "run", issue_run, (tag + "pack",), verify_run)
    if values:
        q.add(tag + "values", lambda: sm.values_reads_device(b, packed.d, max_records, pos.d, offs.d, read_starts=starts.d,
                                                             n_pos_max=pos.n, out=vals.d),
              (tag + "run",), lambda: check_exact(tag + "values", vals, want_vals[:0] if refused else want_vals))


PLAN_CANON = dict(ctor="canonical_minimizers", k=21, w=11, canonical=True, mode=0, sk=False)
PLAN_FWD_SK = dict(ctor="minimizers", k=21, w=11, canonical=False, mode=0, sk=True)
PLAN_SYNC = dict(ctor="canonical_closed_syncmers", k=15, w=17, canonical=True, mode=1, sk=False)


def mixed_reads(rng, n, long_read, with_n):
    """Reads of 0 .. 400 bases (empty ones, some below a window) and one long one; ``with_n``: a few N in every third."""
    lens = [0 if i % 17 == 0 else int(rng.integers(1, 400)) for i in range(n)]
    lens[n // 2] = long_read
    reads = [bytearray(s) for s in random_reads(rng, lens)]
    if with_n:
        for i, s in enumerate(reads):
            if i % 3 == 0 and len(s):
                for p in rng.integers(0, len(s), 1 + len(s) // 150):
                    s[int(p)] = ord("N")
    return [bytes(s) for s in reads]


def add_ascii_packers(q, sm, oracle):
    """mm_pack_ascii_device_async and mm_pack_ascii_n_device_async on about 200 kB each (the 16- and 32-base fast paths
    and their tails: the length is no multiple of 8)."""
    L, ws = sm.lib(), q.ws
    rng = np.random.default_rng(61)
    n = 200_003
    a1 = np.frombuffer(b"ACGTacgt", dtype=np.uint8)[rng.integers(0, 8, n)]
    a2 = np.frombuffer(b"ACGTacgtNnRY", dtype=np.uint8)[rng.integers(0, 12, n)]
    i1, i2 = q.input(a1), q.input(a2)
    p1, p2, m2 = q.output((n + 3) // 4, np.uint8), q.output((n + 3) // 4, np.uint8), q.output((n + 7) // 8, np.uint8)
    w1 = oracle.pack_ascii(a1.tobytes())[: (n + 3) // 4]
    w2, wm = oracle.pack_ascii_n(a2.tobytes())
    q.upload("up_ascii", i1)
    q.upload("up_ascii_n", i2)
    q.add("pack_ascii", lambda: sm._check(L.mm_pack_ascii_device_async(ws.h, vp(i1.d), n, vp(p1.d))), ("up_ascii",),
          lambda: check_exact("pack_ascii", p1, w1, "packed bases"))

    def verify_n():
        check_exact("pack_ascii_n", p2, w2[: (n + 3) // 4], "packed bases")
        check_exact("pack_ascii_n", m2, wm[: (n + 7) // 8], "ambiguity bits")

    q.add("pack_ascii_n", lambda: sm._check(L.mm_pack_ascii_n_device_async(ws.h, vp(i2.d), n, vp(p2.d), vp(m2.d))),
          ("up_ascii_n",), verify_n)


def add_text_pipeline(q, sm, oracle):
    """Protein FASTA -> mm_fasta_text_device_async -> mm_run_text_batch_counts_device_async ->
    mm_values_u64_text_batch_counts_device_async."""
    L, ws = sm.lib(), q.ws
    text = _protein_fasta(np.random.default_rng(8), n_rec=580)
    recs = oracle.fasta_records(text)
    n, n_rec, max_records = len(text), len(recs), 640
    assert 150_000 < n < 260_000 and any(len(s) == 0 for _, _, s in recs)
    k, w = 7, 11
    th = sm.TextMulHasher(canonical=False)
    b = sm.minimizers(k, w).hasher(th).workspace(ws)
    b.text_plan()
    t_in = q.input(np.frombuffer(text, dtype=np.uint8))
    seq, rec_pos = q.output(n, np.uint8), q.output(max_records, np.int64)
    starts, counts = q.output(max_records + 1, np.int64, fill=0), q.output(2, np.int64, fill=0)
    pos, offs, cnt, vals = q.output(n), q.output(max_records + 1, np.int64), q.output(1, np.int64), q.output(n, np.int64)
    chars = np.frombuffer(b"".join(s for _, _, s in recs), dtype=np.uint8)
    want_starts = np.concatenate([[0], np.cumsum([len(s) for _, _, s in recs])]).astype(np.uint64)
    per_rec = [tc.run(s, k, w, th) for _, _, s in recs]
    want_pos = np.concatenate(per_rec).astype(np.uint32)
    want_offs = np.concatenate([[0], np.cumsum([len(p) for p in per_rec])]).astype(np.uint64)
    want_vals = text_values_expected(chars, want_starts, want_pos, want_offs, n_rec, 0, k, False, False)

    def verify_load():
        assert [int(x) for x in counts.host()[:2]] == [len(chars), n_rec]
        assert (counts.host()[2:] == 0).all() and (starts.host()[n_rec + 1:] == 0).all()
        assert np.array_equal(starts.host()[: n_rec + 1].view(np.uint64), want_starts)
        check_exact("fasta_text", seq, chars, "sequence bytes")
        check_exact("fasta_text", rec_pos, np.array([p for p, _, _ in recs], dtype=np.uint64), "header offsets")

    q.upload("up_protein", t_in)
    q.add("fasta_text", lambda: sm._check(L.mm_fasta_text_device_async(
        ws.h, vp(t_in.d), n, vp(seq.d), n, vp(starts.d), vp(rec_pos.d), max_records, vp(counts.d))), ("up_protein",), verify_load)

    def verify_run():
        check_positions("text_run", pos, cnt, want_pos)
        check_exact("text_run", offs, want_offs, "offsets (none past [n_records] is written)")

    q.add("text_run", lambda: sm.run_text_batch_counts_device(b, seq.d, starts.d, counts.d, pos.d, offs.d, max_chars=n,
                                                              d_count=cnt.d), ("fasta_text",), verify_run)
    q.add("text_values", lambda: sm.values_text_batch_counts_device(b, seq.d, starts.d, counts.d, pos.d, offs.d, pos.n,
                                                                    sm.TEXT_VALUES_BYTES, out=vals.d, max_chars=n),
          ("text_run",), lambda: check_exact("text_values", vals, want_vals))


def add_batch_values(q, sm, oracle):
    """mm_values_u64_batch_device_async three times with three different tables: the third comes back to the first of the
    two page-locked staging areas (and waits for its upload, which the header's "staged through page-locked memory" covers)."""
    L, ws = sm.lib(), q.ws
    rng = np.random.default_rng(35)
    prev = ()
    for j, n_seqs in enumerate((300, 70, 1100)):
        seq_lens = [int(x) for x in rng.integers(60, 2000, n_seqs)]
        counts = [int(x) for x in rng.integers(0, 40, n_seqs)]
        pos, offs = _synthetic(rng, seq_lens, counts, 21)
        begins = np.concatenate([[5], 5 + np.cumsum(seq_lens)])
        host = oracle.gen_packed(90 + j, int(begins[-1]) + 64)
        d_in, p_in = q.input(host), q.input(np.concatenate([pos, np.zeros(8, np.uint32)]), index=True)
        out = q.output(int(offs[-1]), np.int64)
        ptrs, nbytes, bases, hosts = [], [], [], []
        for s, m in enumerate(seq_lens):
            b0, bo = int(begins[s]) // 4, int(begins[s]) % 4
            nb = (bo + m + 3) // 4
            has = counts[s] > 0
            ptrs.append(d_in.d.data_ptr() + b0 if has else None), nbytes.append(nb if has else 0), bases.append(bo)
            hosts.append(_padded(host[b0: b0 + nb]) if has else None)
        want = batch_values_expected(oracle, hosts, bases, pos, offs, 21, True, False)
        args = ((C.c_void_p * n_seqs)(*ptrs), (U64 * n_seqs)(*nbytes), (U64 * n_seqs)(*bases), (U64 * n_seqs)(*seq_lens),
                (U64 * (n_seqs + 1))(*[int(o) for o in offs]))
        q.upload(f"up_batch{j}", d_in)
        q.upload(f"up_batch_pos{j}", p_in)
        # (the three calls stay in this order: which staging area a call takes depends on it)
        q.add(f"batch_values{j}", lambda a=args, n_seqs=n_seqs, p_in=p_in, out=out: sm._check(L.mm_values_u64_batch_device_async(
            ws.h, n_seqs, a[0], a[1], a[2], a[3], 21, 1, vp(p_in.d), a[4], vp(out.d))),
            (f"up_batch{j}", f"up_batch_pos{j}") + prev, lambda j=j, out=out, want=want: check_exact(f"batch_values{j}", out, want))
        prev = (f"batch_values{j}",)


@pytest.mark.parametrize("order", list(ORDERS))
def test_q2_loaders_and_pipelines_between_runs(sm, oracle, gpu, order):
    """The ASCII packers, FASTQ with N -> skip-ambiguous counts run -> values, Q1 (c), protein FASTA -> text counts run ->
    values, Q1 (g), three batch-values calls, Q1 (a): one stream, one check, every result what the call gives alone."""
    ref = q1_ref(oracle)
    q = sq.Queue(sm)
    add_ascii_packers(q, sm, oracle)
    add_reads_pipeline(q, sm, oracle, "fastq_n_", mixed_reads(np.random.default_rng(62), 330, 40_000, True), "fastq", PLAN_CANON,
                       True, 700)
    add_q1(q, sm, ref, "c")
    add_text_pipeline(q, sm, oracle)
    add_q1(q, sm, ref, "g")
    add_batch_values(q, sm, oracle)
    add_q1(q, sm, ref, "a")
    passes(q, ORDERS[order], no_wait=False)  # (the third batch-values call waits for its staging area)
    q.close()


@pytest.mark.parametrize("order", list(ORDERS))
def test_q5_a_refused_run_between_two_pipelines(sm, oracle, gpu, order):
    """Three packer -> counts run -> values pipelines back to back; the second one's max_records is below the packer's count.
    The check returns MM_ERR_CAPACITY once and MM_OK after it, the refused run wrote count 0, offsets of 0 and no position,
    and its neighbours in flight are bit for bit right.  All nine calls are documented as not waiting."""
    rng = np.random.default_rng(63)
    q = sq.Queue(sm)
    add_reads_pipeline(q, sm, oracle, "p1_", mixed_reads(rng, 200, 12_000, False), "fastq", PLAN_FWD_SK, False, 260)
    add_reads_pipeline(q, sm, oracle, "p2_", mixed_reads(rng, 60, 3_000, False), "fastq", PLAN_CANON, False, 50, refused=True)
    add_reads_pipeline(q, sm, oracle, "p3_", mixed_reads(rng, 150, 9_000, True), "fasta", PLAN_SYNC, True, 150)
    passes(q, ORDERS[order], no_wait=True, expect=sm.ERR["CAPACITY"])
    assert b"mm_run_packed_reads_counts_device" in sm.lib().mm_last_error()
    q.close()


# ------------------------------------------------------------------------------------------------------- Q3: byte text
N_TEXT = 20_000  # three tiles of 8 192 windows


def text_tables(sm, n):
    """``n`` distinct hashers: forward ones over all 256 bytes (k = 7) alternating with canonical 4-symbol ones for code
    bytes (k = 21), all w = 11."""
    out = []
    for i in range(n):
        if i % 2 == 0:
            out.append((_random_text_hasher(sm, 500 + i, False), False, 7))
        else:
            rng = np.random.default_rng(500 + i)
            f4, r4 = rng.integers(0, 1 << 32, 4, dtype=np.uint64), rng.integers(0, 1 << 32, 4, dtype=np.uint64)
            th = sm.TextHasher.from_tables([f4[c & 3] for c in range(256)], [r4[c & 3] for c in range(256)], rot=7, canonical=True)
            out.append((th, True, 21))
    return out


def add_text_runs(q, sm, tables, repeats):
    ws = q.ws
    rng = np.random.default_rng(71)
    texts = {False: tc.english_like(N_TEXT, 72), True: rng.integers(0, 4, N_TEXT, dtype=np.uint8)}
    ins = {c: q.input(t) for c, t in texts.items()}
    q.upload("up_english", ins[False])
    q.upload("up_codes", ins[True])
    plans = []
    for th, canonical, k in tables:
        b = (sm.canonical_minimizers if canonical else sm.minimizers)(k, 11).hasher(th).workspace(ws)
        b.text_plan()
        plans.append((b, canonical, tc.run(texts[canonical], k, 11, th, canonical, 0)))
    for rep in range(repeats):
        for t, (b, canonical, want) in enumerate(plans):
            name = f"text{t}_{rep}"
            out, cnt = q.output(N_TEXT), q.output(1, np.int64)
            q.add(name, lambda b=b, c=canonical, out=out, cnt=cnt: b.run_text_device(ins[c].d, N_TEXT, out.d, sync=False, d_count=cnt.d),
                  ("up_codes" if canonical else "up_english",),
                  lambda name=name, out=out, cnt=cnt, want=want: check_positions(name, out, cnt, want))


@pytest.mark.parametrize("order", list(ORDERS))
def test_q3_text_tables_within_the_ring(sm, gpu, order):
    """7 distinct table sets, three runs each, interleaved: no table needs a slot of the eight-slot ring twice, so no call
    waits."""
    q = sq.Queue(sm)
    add_text_runs(q, sm, text_tables(sm, 7), 3)
    passes(q, ORDERS[order], no_wait=True)
    assert q.ws.last_path() == sm.PATH_FUSED
    q.close()


@pytest.mark.parametrize("order", list(ORDERS))
def test_q3_text_tables_wrap_the_ring(sm, gpu, order):
    """20 distinct table sets, one run each: the ninth upload reuses the first page-locked slot while - under the delay -
    the first upload is still queued.  The header documents that wait, so there is no no-wait assertion; every output
    must be the checker's for its OWN table."""
    q = sq.Queue(sm)
    add_text_runs(q, sm, text_tables(sm, 20), 1)
    passes(q, ORDERS[order], no_wait=False)
    q.close()
