"""The first call: prebuilt reads-mode kernels for closed syncmers, open syncmers and minimizers + super-k-mers,
mm_plan_prepare (Builder.prepare) and the run-time compiler's locking and counters.

The reference's Builder::run (src/lib.rs:378) is compiled code with no first-call cost; these tests pin down how far
this engine restores that: which flavours never compile, that prepare moves a compile out of the first run, and that a
kernel already loaded is never waited for behind another thread's compile.

Scenarios that need an empty run-time-compile cache and an untouched process run this file as a child process
(``python test_gpu_prepare.py <scenario>``), each under its own time limit; a child prints one JSON line.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NEW_FLAVOUR_WINDOWS = [5, 7, 11, 15, 17, 19, 21, 31]
FLAVOURS = ("super_kmers", "closed", "open")


def _fused_threads(sm):
    """Lanes per workgroup of the fused kernel (kFusedThreads), from the library's launch planner: windows per block of
    a tile are kFusedThreads x w."""
    out = (C.c_uint64 * 7)()
    nw = (C.c_uint64 * 1)(1000)
    w = 11
    assert sm.lib().mm_debug_launch_plan(w, 0, 0, 0, nw, out, None, None, None, 0, None) == 0
    assert out[6] % w == 0 and out[6] // w >= 64
    return int(out[6] // w)


def _n_reads(sm):
    """More than two workgroups of lanes and a partial one: 700 reads with 256 lanes per workgroup."""
    t = _fused_threads(sm)
    return 2 * t + t * 47 // 64


def _builder(sm, k, w, canonical, flavour):
    if flavour == "super_kmers":
        return (sm.canonical_minimizers if canonical else sm.minimizers)(k, w).super_kmers([])
    if flavour == "closed":
        return (sm.canonical_closed_syncmers if canonical else sm.closed_syncmers)(k, w)
    if flavour == "open":
        return (sm.canonical_open_syncmers if canonical else sm.open_syncmers)(k, w)
    return (sm.canonical_minimizers if canonical else sm.minimizers)(k, w)


def _oracle_mode(oracle, flavour):
    return {"closed": oracle.CLOSED_SYNCMERS, "open": oracle.OPEN_SYNCMERS}.get(flavour, oracle.MINIMIZERS)


def _expect_reads(oracle, h, starts, lens, k, w, canonical, flavour):
    """Per read: (positions, super-k-mer indices or None) of the oracle on that read alone."""
    sk = flavour == "super_kmers"
    out = []
    for s, m in zip(starts, lens):
        r = oracle.run(h, int(m), k, w, canonical=canonical, base_offset=int(s), mode=_oracle_mode(oracle, flavour),
                       super_kmers=sk)
        out.append(r if sk else (r, None))
    return out


def _compare_reads(tag, want, pos, sk, offs):
    assert len(offs) == len(want) + 1 and offs[0] == 0, tag
    for r, (wp, ws_) in enumerate(want):
        a, e = int(offs[r]), int(offs[r + 1])
        assert np.array_equal(pos[a:e], wp), f"{tag}: read {r} positions"
        if ws_ is not None:
            assert np.array_equal(sk[a:e], ws_), f"{tag}: read {r} super-k-mer indices"
    assert int(offs[-1]) == sum(len(wp) for wp, _ in want), tag


def _run_fixed_stride(sm, torch, b, d, n_reads, rl, with_sk):
    cap = n_reads * rl
    pos = torch.zeros(cap, dtype=torch.int32, device=d.device)
    sk = torch.zeros(cap, dtype=torch.int32, device=d.device) if with_sk else None
    offs = torch.zeros(n_reads + 1, dtype=torch.int64, device=d.device)
    cnt = sm.run_reads_device(b, d, n_reads, rl, rl, pos, offs, out_sk=sk)
    return (pos[:cnt].cpu().numpy().view(np.uint32), sk[:cnt].cpu().numpy().view(np.uint32) if with_sk else None,
            offs.cpu().numpy())


def _run_packed(sm, torch, b, d, starts, with_sk):
    total = int(starts[-1])
    rec = sm.FastaRecords(d, np.asarray(starts, dtype=np.uint64), np.zeros(len(starts) - 1, dtype=np.uint64))
    pos = torch.zeros(total + 64, dtype=torch.int32, device=d.device)
    sk = torch.zeros(total + 64, dtype=torch.int32, device=d.device) if with_sk else None
    offs = torch.zeros(len(starts), dtype=torch.int64, device=d.device)
    cnt = sm.run_packed_reads_device(b, rec, pos, offs, out_sk=sk)
    return (pos[:cnt].cpu().numpy().view(np.uint32), sk[:cnt].cpu().numpy().view(np.uint32) if with_sk else None,
            offs.cpu().numpy())


def _mixed_lengths(l, n_reads):
    """n_reads reads: l - 1 (no window), l, l + 1 and 150 in turn, and three reads of 4 000 bp for the lane table."""
    cyc = [l - 1, l, l + 1, 150]
    lens = [cyc[i % 4] for i in range(n_reads)]
    for i in (101, n_reads // 2, n_reads - 1):
        lens[i] = 4000
    return lens


# ------------------------------------------------------------------ 1. the new instances against the oracle
@pytest.mark.gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("w", NEW_FLAVOUR_WINDOWS)
def test_new_reads_instances_match_oracle(sm, oracle, gpu, w, canonical, flavour):
    import torch
    k = 21 if (not canonical or (21 + w - 1) % 2 == 1) else 20
    l = k + w - 1
    N_READS = _n_reads(sm)
    assert N_READS > 2 * _fused_threads(sm) and N_READS % _fused_threads(sm) != 0
    before = sm.jit_stats()
    b = _builder(sm, k, w, canonical, flavour)
    with_sk = flavour == "super_kmers"
    assert w in sm.prebuilt_flavour_window_sizes(canonical, True, b.mode, with_sk)

    # fixed stride, equal lengths: one lane per read
    rl = 150
    h = oracle.gen_packed(9000 + w, N_READS * rl)
    d = torch.from_numpy(h).cuda()
    starts = [r * rl for r in range(N_READS)]
    want = _expect_reads(oracle, h, starts, [rl] * N_READS, k, w, canonical, flavour)
    pos, sk, offs = _run_fixed_stride(sm, torch, b, d, N_READS, rl, with_sk)
    assert b._ws().last_path() == sm.PATH_FUSED
    _compare_reads(f"fixed stride w={w} canonical={canonical} {flavour}", want, pos, sk, offs)

    # packed starts, mixed lengths: the 4 000 bp reads do not fit a lane each, so the lane table is taken
    lens = _mixed_lengths(l, N_READS)
    st = np.zeros(N_READS + 1, dtype=np.int64)
    st[1:] = np.cumsum(lens)
    h = oracle.gen_packed(9100 + w, int(st[-1]))
    d = torch.from_numpy(h).cuda()
    want = _expect_reads(oracle, h, st[:-1], lens, k, w, canonical, flavour)
    pos, sk, offs = _run_packed(sm, torch, b, d, st, with_sk)
    assert sm.lib().mm_workspace_last_lane_table(b._ws().h) == 1, "the mixed reads did not take the lane table"
    _compare_reads(f"packed w={w} canonical={canonical} {flavour}", want, pos, sk, offs)

    after = sm.jit_stats()
    assert (after["compiled"] + after["from_disk"]) - (before["compiled"] + before["from_disk"]) == 0, (before, after)


# ------------------------------------------------------------------ children
def _child_env(cache):
    env = {k: v for k, v in os.environ.items() if k != "MM_ENV_DYNAMIC" and not k.startswith("MM_")}
    env["MM_JIT_CACHE_DIR"] = str(cache)
    if os.environ.get("MM_LIB_PATH"):
        env["MM_LIB_PATH"] = os.environ["MM_LIB_PATH"]
    return env


def _child(args, env, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True,
                       timeout=timeout)
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    s = json.loads(lines[-1])
    print(json.dumps(s))
    return s


def _hsaco(d):
    return {f: os.stat(os.path.join(d, f)).st_mtime_ns for f in os.listdir(d) if f.endswith(".hsaco")}


def _cache(tmp_path):
    cache = tmp_path / "jit"
    cache.mkdir(mode=0o700)
    return cache


# ------------------------------------------------------------------ 2. the new flavours compile nothing
@pytest.mark.gpu
def test_new_flavours_compile_nothing_in_a_fresh_process(sm, gpu, tmp_path):
    """Reads + super-k-mers at k=21 w=11 and reads closed syncmers at k=15 w=17, fresh process, empty cache: both equal
    the oracle, nothing was compiled and the cache stays empty.  (Before these flavours were prebuilt both compiled.)"""
    cache = _cache(tmp_path)
    s = _child(["new_flavours"], _child_env(cache), 600)
    assert s["ok"], s
    assert s["jit_stats"]["compiled"] == 0 and s["jit_stats"]["from_disk"] == 0, s
    assert _hsaco(str(cache)) == {}, "a prebuilt flavour was compiled at run time"


# ------------------------------------------------------------------ 3. prepare moves the compile
@pytest.mark.gpu
def test_prepare_moves_the_compile(sm, gpu, tmp_path):
    cache = _cache(tmp_path)
    env = _child_env(cache)
    s1 = _child(["prepare_then_run", "37"], env, 900)
    assert s1["report"]["compiled"] == 1 and s1["report"]["unavailable"] == 0 and s1["report"]["kernels"] == 1, s1
    assert s1["hsaco_after_prepare"] == 1, s1
    assert s1["ok"] and s1["compiled_after_run"] == s1["compiled_after_prepare"] == 1, s1
    first = _hsaco(str(cache))
    assert len(first) == 1
    s2 = _child(["prepare_then_run", "37"], env, 600)
    assert s2["report"]["compiled"] == 0 and s2["report"]["from_disk"] == 1 and s2["report"]["unavailable"] == 0, s2
    assert s2["ok"] and s2["compiled_after_run"] == 0, s2
    assert _hsaco(str(cache)) == first


# ------------------------------------------------------------------ 4. prebuilt plans
@pytest.mark.gpu
def test_prepare_of_prebuilt_plan_compiles_nothing(sm, gpu):
    b = sm.canonical_minimizers(21, 11)
    before = sm.jit_stats()
    r1 = b.prepare(sequence=True, reads=True, super_kmers=True)
    r2 = b.prepare(sequence=True, reads=True, super_kmers=True)
    assert r1 == r2, (r1, r2)
    assert r1["compiled"] == r1["from_disk"] == r1["unavailable"] == 0 and r1["kernels"] >= 4, r1
    after = sm.jit_stats()
    assert after["compiled"] == before["compiled"] and after["from_disk"] == before["from_disk"]
    # super_kmers=None: as the builder was configured
    assert sm.canonical_minimizers(21, 11).super_kmers([]).prepare(reads=True) == r1
    assert sm.canonical_minimizers(21, 11).prepare(reads=True)["kernels"] < r1["kernels"]


# ------------------------------------------------------------------ 5. contract edges
@pytest.mark.gpu
def test_prepare_contract_edges(sm, oracle, gpu):
    import torch
    L = sm.lib()
    E = sm.ERR
    ws = gpu
    rep = sm.PrepareReport(9, 9, 9, 9)
    sync = sm.canonical_closed_syncmers(15, 17)
    assert L.mm_plan_prepare(sync.plan().h, ws.h, sm.PREPARE_SEQUENCE | sm.PREPARE_SUPERKMERS, C.byref(rep)) == E["BAD_MODE"]
    assert L.mm_plan_prepare(sync.plan().h, ws.h, sm.PREPARE_SEQUENCE | sm.PREPARE_READS, C.byref(rep)) == 0
    assert rep.unavailable == 0 and rep.compiled == 0 and rep.from_disk == 0 and rep.kernels >= 2
    b = sm.canonical_minimizers(21, 11)
    assert L.mm_plan_prepare(None, ws.h, 1, C.byref(rep)) == E["NULL"]
    assert L.mm_plan_prepare(b.plan().h, None, 1, C.byref(rep)) == E["NULL"]
    assert L.mm_plan_prepare(b.plan().h, ws.h, 1, None) == 0  # (the report is optional)
    rep = sm.PrepareReport(9, 9, 9, 9)
    assert L.mm_plan_prepare(b.plan().h, ws.h, 0, C.byref(rep)) == 0
    assert (rep.kernels, rep.compiled, rep.from_disk, rep.unavailable) == (0, 0, 0, 0)
    # a text plan: nothing to compile
    rt = sm.minimizers(21, 11).prepare(text=True)
    assert rt["compiled"] == rt["from_disk"] == rt["unavailable"] == 0 and rt["kernels"] >= 1, rt
    assert sm.minimizers(21, 200).prepare(text=True)["unavailable"] == 0  # (the generic family's text kernels)

    # run-time compiler switched off: the kernel cannot be had, prepare says so and the run takes the generic family
    k, w, n = 21, 37, 10_000
    assert w not in sm.prebuilt_window_sizes(False)
    h = oracle.gen_packed(4242, n)
    want = oracle.run(h, n, k, w, canonical=False)
    d = torch.from_numpy(h).cuda()
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    old = os.environ.get("MM_JIT")
    os.environ["MM_JIT"] = "0"
    try:
        b37 = sm.minimizers(k, w)
        r = b37.prepare()
        assert r["unavailable"] == 1 and r["compiled"] == 0 and r["from_disk"] == 0, r
        assert L.mm_last_error(), "mm_last_error() should carry the reason"
        cnt = b37.run_device(d, n, out)
        assert b37._ws().last_path() == sm.PATH_GENERIC
        assert np.array_equal(out[:cnt].cpu().numpy().view(np.uint32), want)
    finally:
        if old is None:
            del os.environ["MM_JIT"]
        else:
            os.environ["MM_JIT"] = old


@pytest.mark.gpu
def test_prepare_on_second_device_keeps_current_device(sm, gpu):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device")
    torch.cuda.set_device(0)
    ws1 = sm.Workspace(1)
    r = sm.canonical_minimizers(21, 11).prepare(ws=ws1, sequence=True, reads=True, super_kmers=True)
    assert r["unavailable"] == 0 and r["kernels"] >= 4
    assert torch.cuda.current_device() == 0


# ------------------------------------------------------------------ 6. a hit does not wait behind a compile
@pytest.mark.gpu
def test_hit_does_not_wait_behind_a_compile(sm, gpu, tmp_path):
    """Thread A prepares forward w=39 cold (T_A); thread B, started 0.2 s later, keeps running the loaded w=37 plan.
    With one lock around the whole compile B's first call waits about T_A - 0.2 s; now its slowest call is below T_A / 2.
    Both are measured in the same run.  A compile under 1 s proves nothing either way: the test then skips.  One
    forward kernel compiles in about 0.8 s on an MI355X host, so A prepares the plan's sequence and reads kernels with
    their super-k-mer twins - four cold compiles of forward w=39, one after the other inside the one call."""
    cache = _cache(tmp_path)
    s = _child(["hit_during_compile"], _child_env(cache), 900)
    assert s["ok"], s
    print(f"T_A = {s['t_a']:.3f} s, slowest w=37 call = {s['slowest']:.4f} s over {s['calls']} calls")
    if s["t_a"] < 1.0:
        pytest.skip(f"the cold compile took only T_A = {s['t_a']:.3f} s: too short to tell a wait from a run")
    assert s["calls"] >= 1
    assert s["slowest"] < s["t_a"] / 2, s


# ------------------------------------------------------------------ 7. two cold keys from two threads
@pytest.mark.gpu
def test_two_cold_keys_from_two_threads(sm, gpu, tmp_path):
    cache = _cache(tmp_path)
    s = _child(["two_cold_keys"], _child_env(cache), 900)
    assert s["ok"], s
    assert s["reports"]["43"]["compiled"] == 1 and s["reports"]["45"]["compiled"] == 1, s
    assert s["reports"]["43"]["unavailable"] == 0 and s["reports"]["45"]["unavailable"] == 0, s
    assert len(_hsaco(str(cache))) == 2
    assert s["jit_stats"]["compiled"] == 2 and s["jit_stats"]["failed"] == 0, s


# ------------------------------------------------------------------ the child process
def _child_main(argv):
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch

    import mm_oracle as oracle
    import simd_minimizers_amd as sm

    cache = os.environ["MM_JIT_CACHE_DIR"]
    n = 10_000

    def seq_case(w, seed):
        h = oracle.gen_packed(seed, n)
        return dict(b=sm.minimizers(21, w), h=h, d=torch.from_numpy(h).cuda(), want=oracle.run(h, n, 21, w, canonical=False),
                    out=torch.zeros(n, dtype=torch.int32, device="cuda"))

    def run_seq(c, ws=None):
        b = c["b"].workspace(ws) if ws is not None else c["b"]
        cnt = b.run_device(c["d"], n, c["out"])
        return bool(np.array_equal(c["out"][:cnt].cpu().numpy().view(np.uint32), c["want"]))

    scenario = argv[0]
    res = {"scenario": scenario}
    if scenario == "new_flavours":
        ok = True
        for k, w, canonical, flavour in ((21, 11, True, "super_kmers"), (15, 17, True, "closed")):
            n_reads, rl = 300, 150
            h = oracle.gen_packed(70 + w, n_reads * rl)
            d = torch.from_numpy(h).cuda()
            b = _builder(sm, k, w, canonical, flavour)
            want = _expect_reads(oracle, h, [r * rl for r in range(n_reads)], [rl] * n_reads, k, w, canonical, flavour)
            pos, sk, offs = _run_fixed_stride(sm, torch, b, d, n_reads, rl, flavour == "super_kmers")
            _compare_reads(f"{flavour} k={k} w={w}", want, pos, sk, offs)
            ok = ok and b._ws().last_path() == sm.PATH_FUSED
        res.update(ok=ok, jit_stats=sm.jit_stats())
    elif scenario == "prepare_then_run":
        c = seq_case(int(argv[1]), 11)
        res["report"] = c["b"].prepare(sequence=True)
        res["hsaco_after_prepare"] = len(_hsaco(cache))
        res["compiled_after_prepare"] = sm.jit_stats()["compiled"]
        ok = run_seq(c) and c["b"]._ws().last_path() == sm.PATH_FUSED
        res.update(ok=ok, compiled_after_run=sm.jit_stats()["compiled"], jit_stats=sm.jit_stats())
    elif scenario == "hit_during_compile":
        hot, cold = seq_case(37, 21), seq_case(39, 22)
        ws_a, ws_b = sm.Workspace(0), sm.Workspace(0)
        r0 = hot["b"].prepare(ws=ws_b)
        ok = r0["unavailable"] == 0 and run_seq(hot, ws_b)  # (loaded, and every buffer of the workspace grown)
        started = threading.Event()
        out = {}

        def a():
            started.set()
            t0 = time.perf_counter()
            out["report"] = cold["b"].prepare(ws=ws_a, sequence=True, reads=True, super_kmers=True)
            out["t_a"] = time.perf_counter() - t0

        ta = threading.Thread(target=a)
        ta.start()
        started.wait()
        time.sleep(0.2)
        slowest, calls, good = 0.0, 0, True
        while ta.is_alive():
            t0 = time.perf_counter()
            good = run_seq(hot, ws_b) and good
            slowest = max(slowest, time.perf_counter() - t0)
            calls += 1
        ta.join()
        ok = ok and good and out["report"]["compiled"] == 4 and run_seq(cold, ws_a)
        res.update(ok=ok, t_a=out["t_a"], slowest=slowest, calls=calls, jit_stats=sm.jit_stats())
    elif scenario == "two_cold_keys":
        cases = {43: seq_case(43, 31), 45: seq_case(45, 32)}
        wss = {w: sm.Workspace(0) for w in cases}
        reports = {}
        barrier = threading.Barrier(2)

        def body(w):
            barrier.wait()
            reports[str(w)] = cases[w]["b"].prepare(ws=wss[w])

        ts = [threading.Thread(target=body, args=(w,)) for w in cases]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        ok = all(run_seq(cases[w], wss[w]) for w in cases)
        res.update(ok=ok, reports=reports, jit_stats=sm.jit_stats())
    else:
        raise SystemExit(f"unknown scenario {scenario}")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(_child_main(sys.argv[1:]))
