"""Many host threads against the engine (one workspace per host thread / stream; plans are immutable
and shareable): every result is compared with the CPU oracle, and a thread's current device must be what it was.

The workload itself is tests/thread_workload.py; these tests run it in-process, in fresh processes with the product's
environment cache and an empty run-time-compile cache, and add the narrower contracts: many workspaces on one thread
with asynchronous runs, the per-thread default workspace of the Python package, a workspace handed between threads,
per-thread error text, device groups from two threads, several devices and the C++ mirror.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import thread_workload

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
K, W = 21, 11


def _threads(fn, n):
    """fn(i) in n threads released at a barrier; their results in order (re-raises the first failure)."""
    barrier = threading.Barrier(n)
    out, errs = [None] * n, []

    def body(i):
        try:
            barrier.wait()
            out[i] = fn(i)
        except BaseException as e:
            errs.append(e)
            barrier.abort()

    ts = [threading.Thread(target=body, args=(i,)) for i in range(n)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errs:
        raise errs[0]
    return out


def _assert_summary(s):
    assert not s["failures"], s["failures"]
    assert s["device_unchanged"], "a thread's current device changed"
    assert s["ok"], s
    for name, st in s["jobs"].items():
        assert st["calls"] > 0, name


@pytest.mark.gpu
def test_threads_own_workspaces_mixed_jobs(sm, oracle, gpu):
    s = thread_workload.run_workload(n_threads=8, rounds=3)
    print(json.dumps(s))
    _assert_summary(s)
    assert set(s["jobs"]) == set(thread_workload.JOBS)


def _child(args, env, timeout):
    r = subprocess.run([sys.executable, os.path.join(HERE, "thread_workload.py")] + args, env=env, capture_output=True,
                       text=True, timeout=timeout)
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    s = json.loads(lines[-1])
    _assert_summary(s)
    return s


def _hsaco(d):
    return {f: os.stat(os.path.join(d, f)).st_mtime_ns for f in os.listdir(d) if f.endswith(".hsaco")}


@pytest.mark.gpu
def test_threads_fresh_process_product_env(sm, gpu, tmp_path):
    """The product's environment cache (mm_env.h; MM_ENV_DYNAMIC unset) and first compiles of the run-time-compiled
    kernels from 8 threads at once into an empty cache; then a second process loads them from disk, compiling nothing."""
    cache = tmp_path / "jit"
    cache.mkdir(mode=0o700)
    env = {k: v for k, v in os.environ.items() if k != "MM_ENV_DYNAMIC" and not k.startswith("MM_")}
    env["MM_JIT_CACHE_DIR"] = str(cache)
    if os.environ.get("MM_LIB_PATH"):
        env["MM_LIB_PATH"] = os.environ["MM_LIB_PATH"]
    s1 = _child(["--threads", "8", "--rounds", "1"], env, 900)
    print(json.dumps(s1))
    first = _hsaco(str(cache))
    assert len(first) >= 2, f"the run-time-compiled flavours left {sorted(first)} in the cache"
    jit = ",".join(thread_workload.JIT_JOBS)
    s2 = _child(["--threads", "8", "--rounds", "1", "--jobs", jit], env, 600)
    print(json.dumps(s2))
    assert _hsaco(str(cache)) == first, "the second process compiled kernels again instead of loading them"
    assert set(s2["jobs"]) == set(thread_workload.JIT_JOBS)


@pytest.mark.gpu
def test_async_many_workspaces_one_thread(sm, oracle, gpu):
    """Four workspaces on one thread, each with its own stream: asynchronous sequence, reads and byte-text batch runs
    round-robin with no sync in between, then sync + check each.  A check that reports MM_ERR_ORDER is followed as
    the header says: that workspace's runs since the last check are repeated, then compared."""
    import torch
    L = sm.lib()
    n_ws = 4
    wss = [sm.Workspace(0) for _ in range(n_ws)]
    b = sm.canonical_minimizers(K, W)
    bt = sm.minimizers(K, W)
    plan, tplan = b.plan(), bt.text_plan()
    th = sm.TextMulHasher(K, canonical=False)
    rng = np.random.default_rng(77)
    runs = []  # per workspace: list of (issue(), check())
    for i in range(n_ws):
        todo = []
        # sequence
        n = 3_000_000 + 1_000_003 * i
        h = oracle.gen_packed(500 + i, n)
        d = torch.from_numpy(h).cuda()
        out = torch.zeros(n // 3 + 64, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        todo.append((lambda ws, d=d, n=n, out=out, cnt=cnt: L.mm_run_device_async(
            plan.h, ws.h, C.c_void_p(d.data_ptr()), d.numel(), 0, n, 0, sm.U64_MAX, C.c_void_p(out.data_ptr()), None,
            out.numel(), C.c_void_p(cnt.data_ptr())),
            lambda out=out, cnt=cnt, h=h, n=n: np.array_equal(out[:int(cnt.item())].cpu().numpy().view(np.uint32),
                                                              oracle.run(h, n, K, W, canonical=True))))
        # reads
        n_reads, rl = 3000 + 500 * i, 150
        hr = oracle.gen_packed(600 + i, n_reads * rl)
        dr = torch.from_numpy(hr).cuda()
        rout = torch.zeros(n_reads * rl // 2, dtype=torch.int32, device="cuda")
        roffs = torch.zeros(n_reads + 1, dtype=torch.int64, device="cuda")
        rcnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        todo.append((lambda ws, dr=dr, n_reads=n_reads, rout=rout, roffs=roffs, rcnt=rcnt: L.mm_run_reads_device_async(
            plan.h, ws.h, C.c_void_p(dr.data_ptr()), dr.numel(), 0, n_reads, rl, rl, None, C.c_void_p(rout.data_ptr()),
            rout.numel(), C.c_void_p(roffs.data_ptr()), C.c_void_p(rcnt.data_ptr())),
            lambda rout=rout, rcnt=rcnt, hr=hr, n_reads=n_reads: np.array_equal(
                rout[:int(rcnt.item())].cpu().numpy().view(np.uint32),
                np.concatenate([oracle.run(hr, rl, K, W, canonical=True, base_offset=r * rl) for r in range(n_reads)]))))
        # byte-text batch
        lens = [int(x) for x in rng.integers(0, 300, 2000 + 100 * i)]
        text = rng.integers(0, 256, sum(lens), dtype=np.uint8)
        st = np.zeros(len(lens) + 1, dtype=np.int64)
        st[1:] = np.cumsum(lens)
        dt, dst = torch.from_numpy(text).cuda(), torch.from_numpy(st).cuda()
        tout = torch.zeros(int(st[-1]) + 8, dtype=torch.int32, device="cuda")
        toffs = torch.zeros(len(lens) + 1, dtype=torch.int64, device="cuda")
        tcnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        todo.append((lambda ws, dt=dt, dst=dst, n_rec=len(lens), tout=tout, toffs=toffs, tcnt=tcnt, nc=int(st[-1]):
                     L.mm_run_text_batch_device_async(
                         tplan.h, ws.h, C.c_void_p(dt.data_ptr()), dt.numel(), n_rec, C.c_void_p(dst.data_ptr()), nc,
                         C.c_void_p(tout.data_ptr()), None, tout.numel(), C.c_void_p(toffs.data_ptr()),
                         C.c_void_p(tcnt.data_ptr())),
                     lambda tout=tout, tcnt=tcnt, toffs=toffs, text=text, st=st: (
                         lambda wp_wo: np.array_equal(tout[:int(tcnt.item())].cpu().numpy().view(np.uint32), wp_wo[0])
                         and list(toffs.cpu().numpy()) == wp_wo[1])(
                         thread_workload._text_batch_expect(text, st, K, W, th))))
        runs.append(todo)
    torch.cuda.synchronize()
    for j in range(3):  # round-robin over the workspaces, no sync in between
        for i in range(n_ws):
            sm._check(runs[i][j][0](wss[i]))
    redone = 0
    for i in range(n_ws):
        wss[i].sync()
        try:
            wss[i].check()
        except sm.MinimizerError as e:
            assert e.code == sm.ERR["ORDER"], e
            redone += 1
            for issue, _ in runs[i]:
                sm._check(issue(wss[i]))
            wss[i].sync()
            wss[i].check()
    for i in range(n_ws):
        for j, (_, ok) in enumerate(runs[i]):
            assert ok(), (i, ["sequence", "reads", "text batch"][j])
    print(f"async runs on {n_ws} workspaces: {redone} repeated after MM_ERR_ORDER, "
          f"{sum(ws.ticket_mode() for ws in wss)} in ticket mode")
    for ws in wss:
        ws.close()


@pytest.mark.gpu
def test_default_workspace_is_per_thread(sm, oracle, gpu):
    """The free functions and Builder.run without a workspace use the calling thread's default workspace: one per
    thread, never another thread's."""
    import text_checker
    hasher = sm.TextMulHasher(K, canonical=False)
    inputs = []
    for t in range(8):
        n = 400_000 + 7919 * t
        h = oracle.gen_packed(700 + t, n)
        text = np.random.default_rng(t).integers(0, 256, 300_000 + 13 * t, dtype=np.uint8).tobytes()
        inputs.append((h, n, text, oracle.run(h, n, K, W, canonical=True), oracle.run(h, n, K, W),
                       text_checker.run(text, K, W, hasher, canonical=False)))
    bt = sm.minimizers(K, W)
    bt.text_plan()

    def body(t):
        h, n, text, *_ = inputs[t]
        ws = sm.default_workspace(0)
        got = []
        for _ in range(3):
            got.append((sm.canonical_minimizer_positions(sm.PackedSeq(h, 0, n), K, W),
                        sm.minimizer_positions(sm.PackedSeq(h, 0, n), K, W), bt.run_once(text)))
        assert sm.default_workspace(0) is ws
        return ws, got

    res = _threads(body, 8)
    for t, (ws, got) in enumerate(res):
        _, _, _, wc, wf, wt = inputs[t]
        for c, f, x in got:
            assert np.array_equal(np.asarray(c, np.uint32), wc), t
            assert np.array_equal(np.asarray(f, np.uint32), wf), t
            assert np.array_equal(np.asarray(x, np.uint32), wt), t
    wss = [ws for ws, _ in res]
    assert len({id(ws) for ws in wss}) == 8 and all(ws is not gpu for ws in wss)


@pytest.mark.gpu
def test_workspace_passed_between_threads(sm, oracle, gpu):
    """One workspace, made in the main thread, used by worker threads one after another (a join between them)."""
    import torch
    ws = sm.Workspace(0)
    b = sm.canonical_minimizers(K, W).workspace(ws)
    for t in range(6):
        n = 2_000_000 + 100_003 * t
        h = oracle.gen_packed(800 + t, n)
        d = torch.from_numpy(h).cuda()
        out = torch.zeros(n // 3 + 64, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        box = []
        th = threading.Thread(target=lambda: box.append((b.run_device(d, n, out), b._run_arrays(sm.PackedSeq(h, 0, n))[0])))
        th.start()
        th.join()
        assert box, "the worker failed"
        cnt, host = box[0]
        want = oracle.run(h, n, K, W, canonical=True)
        assert np.array_equal(out[:cnt].cpu().numpy().view(np.uint32), want), t
        assert np.array_equal(host, want), t
    ws.close()


@pytest.mark.gpu
def test_last_error_is_per_thread(sm, oracle, gpu):
    """mm_last_error() is per thread: thread A provokes host-side errors that launch nothing (a device group run with
    no resident sequence); thread B, running valid calls meanwhile, never reads A's text."""
    import torch
    L = sm.lib()
    b = sm.canonical_minimizers(K, W)
    plan = b.plan()
    stop = threading.Event()
    seen_a, seen_b = [0, set()], []  # (calls, distinct texts) of A

    def thread_a():
        g = sm.DeviceGroup([0])
        counts, total = (C.c_uint64 * 1)(), C.c_uint64()
        try:
            while not stop.is_set():
                assert L.mm_run_sharded_device(plan.h, g.h, 0, 100_000, 0, counts, C.byref(total)) == sm.ERR["NULL"]
                seen_a[0] += 1
                seen_a[1].add(L.mm_last_error().decode())
        finally:
            g.close()

    n = 500_000
    h = oracle.gen_packed(900, n)
    d = torch.from_numpy(h).cuda()
    out = torch.zeros(n // 3 + 64, dtype=torch.int32, device="cuda")
    want = oracle.run(h, n, K, W, canonical=True)
    torch.cuda.synchronize()

    def thread_b():
        ws = sm.Workspace(0)
        bb = b.workspace(ws)
        try:
            for _ in range(200):
                cnt = bb.run_device(d, n, out)
                seen_b.append((L.mm_last_error().decode(), cnt))
        finally:
            stop.set()
            ws.close()

    ta, tb = threading.Thread(target=thread_a), threading.Thread(target=thread_b)
    ta.start()
    tb.start()
    tb.join()
    ta.join()
    assert seen_a[0] > 0 and len(seen_a[1]) == 1 and "no resident sequence" in seen_a[1].pop(), seen_a
    assert len(seen_b) == 200
    assert not any("resident" in x for x, _ in seen_b), [x for x, _ in seen_b if x][:3]
    assert np.array_equal(out[:seen_b[-1][1]].cpu().numpy().view(np.uint32), want)


@pytest.mark.gpu
def test_device_groups_from_two_threads(sm, oracle, gpu):
    """Two threads, each with its own DeviceGroup([0, 0, 0]), run g.run and g.run_batch at the same time (the library
    runs a host thread per entry inside each call)."""
    b = sm.canonical_minimizers(K, W)
    b.plan()
    inputs = []
    for t in range(2):
        n = 4_000_003 + 999_999 * t
        h = oracle.gen_packed(1000 + t, n)
        lens = [300_000 + t, 7, 0, 1_000_001, 250_000 + 17 * t]
        seqs = [oracle.gen_packed(1100 + 10 * t + i, m + 3) for i, m in enumerate(lens)]
        inputs.append((h, n, seqs, lens, oracle.run(h, n, K, W, canonical=True),
                       [oracle.run(s, m, K, W, canonical=True) for s, m in zip(seqs, lens)]))

    def body(t):
        h, n, seqs, lens, _, _ = inputs[t]
        g = sm.DeviceGroup([0, 0, 0])
        try:
            return [(g.run(b, h, n)[0], g.run_batch(b, seqs, lens)) for _ in range(3)]
        finally:
            g.close()

    for t, res in enumerate(_threads(body, 2)):
        _, _, _, _, want, want_b = inputs[t]
        for pos, (bp, _, o) in res:
            assert np.array_equal(pos, want), t
            for i, wb in enumerate(want_b):
                assert np.array_equal(bp[o[i]:o[i + 1]], wb), (t, i)


@pytest.mark.gpu
def test_threads_on_distinct_devices(sm, gpu):
    import torch
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("one GPU: threads on distinct devices need two or more")
    s = thread_workload.run_workload(n_threads=8, rounds=1, devices=list(range(n)))
    print(json.dumps(s))
    _assert_summary(s)


@pytest.mark.gpu
def test_cxx_threads_thread_default(sm, oracle, gpu, tmp_path):
    """The C++ mirror: 8 std::threads share one Builder and each uses Workspace::thread_default()
    (tests/cxx/threads_example.cpp); its outputs are compared with the oracle here."""
    import text_checker
    exe = str(tmp_path / "threads_example")
    libdir = os.path.join(ROOT, "simd-minimizers_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(HERE, "cxx", "threads_example.cpp"), "-L" + libdir, "-lsimd_minimizers_amd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    n_threads = 8
    rng = np.random.default_rng(99)
    hasher = sm.TextMulHasher(K, canonical=True)
    want = []
    for t in range(n_threads):
        n = 1_000_000 + 31_337 * t
        h = oracle.gen_packed(1200 + t, n)
        m = 500_000 + 1000 * t
        a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, m)].copy()
        a[rng.integers(0, m, m // 200)] = ord("N")
        packed, amb = oracle.pack_ascii_n(a.tobytes())
        text = rng.integers(0, 256, 200_000 + 17 * t, dtype=np.uint8)
        d = str(tmp_path)
        h.tofile(f"{d}/in_{t}_packed.bin")
        packed.tofile(f"{d}/in_{t}_nseq.bin")
        amb.tofile(f"{d}/in_{t}_amb.bin")
        text.tofile(f"{d}/in_{t}_text.bin")
        with open(f"{d}/in_{t}_len.txt", "w") as f:
            f.write(f"{n} {m}\n")
        want.append((oracle.run(h, n, K, W, canonical=True), oracle.run_skip_ambiguous(packed, amb, m, K, W),
                     text_checker.run(text, K, W, hasher, canonical=True)))
    r = subprocess.run([exe, str(tmp_path), str(n_threads)], capture_output=True, text=True, timeout=600)
    if r.returncode == 77:
        pytest.skip("no GPU visible to the C++ example")
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    for t, (w_run, w_skip, w_text) in enumerate(want):
        for kind, w_ in (("run", w_run), ("skip", w_skip), ("text", w_text)):
            got = np.fromfile(f"{tmp_path}/out_{t}_{kind}.bin", dtype=np.uint32)
            assert np.array_equal(got, w_), (t, kind, len(got), len(w_))
