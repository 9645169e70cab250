"""A threaded workload over the engine's entry points, compared with the CPU oracle (tests/test_gpu_threads.py,
tests/test_sanitizers.py).  Importable (``run_workload``) and a script that prints one JSON summary line:

    python tests/thread_workload.py [--threads 8] [--rounds 3] [--lib path/to/libsimd_minimizers_amd*.so] [--jobs a,b]

Every worker thread has its own ``Workspace`` and its own inputs (seeds and lengths depend on thread and round, so a
result that landed in another thread's buffers cannot pass); the ``Builder``s and their plans are made once in the main
thread and shared.  The main thread does all torch and oracle work before the workers start; the workers only call
the engine, and the main thread compares after ``join``.  Rounds start at a barrier, so first uses overlap; in round 0
the kernels compiled at run time (JIT) come first in every thread.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

K, W = 21, 11
ORACLE_THREADS = 16
JOBS = ("fused", "fused_sk", "host_small", "host_pipelined", "batch_lane_table", "reads_sk", "skip_ambiguous",
        "text_single", "text_batch", "values_u64", "fastq_reads", "jit_fwd_w37", "jit_reads_sk")
JIT_JOBS = ("jit_fwd_w37", "jit_reads_sk")


class Job:
    """One call (or group of calls) of a worker: ``run(ws)`` in the worker, ``check(result)`` in the main thread after
    the join; ``check`` returns the number of positions it compared and raises AssertionError on a difference."""

    def __init__(self, name, run, check, calls=1):
        self.name, self.run, self.check, self.calls = name, run, check, calls


def _eq(got, want, what):
    got = np.asarray(got, dtype=np.uint32)
    want = np.asarray(want, dtype=np.uint32)
    if len(got) != len(want) or not np.array_equal(got, want):
        bad = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
        raise AssertionError(f"{what}: {len(got)} vs {len(want)} positions, first difference at {bad}")
    return len(want)


def _text_batch_expect(text, starts, k, w, hasher):
    """Per-record minimizer positions of records back to back, from the definition (tests/text_checker.py): windows of
    the whole text, kept when they lie inside one record, record-local, deduplicated within the record."""
    import text_checker
    l = k + w - 1
    p = text_checker.window_positions(text, k, w, hasher, False).astype(np.int64)
    i = np.arange(len(p), dtype=np.int64)
    rec = np.searchsorted(starts, i, side="right") - 1
    ok = i + l <= starts[rec + 1]
    out, offs = [], [0]
    for r in range(len(starts) - 1):
        sel = p[ok & (rec == r)] - starts[r]
        if len(sel):
            keep = np.ones(len(sel), dtype=bool)
            keep[1:] = sel[1:] != sel[:-1]
            sel = sel[keep]
        out.append(sel)
        offs.append(offs[-1] + len(sel))
    return (np.concatenate(out) if out else np.zeros(0, np.int64)).astype(np.uint32), offs


class Workload:
    def __init__(self, sm, oracle, torch, devices, jobs):
        self.sm, self.oracle, self.torch = sm, oracle, torch
        self.devices, self.jobs = list(devices), tuple(jobs)
        self.pool = ThreadPoolExecutor(max_workers=ORACLE_THREADS)  # (oracle calls release the GIL)
        rng = np.random.default_rng(12345)
        self.b_canon = sm.canonical_minimizers(K, W)
        self.b_canon_sk = sm.canonical_minimizers(K, W).super_kmers([])
        self.b_fwd = sm.minimizers(K, W)
        self.text_hashers = [sm.TextMulHasher(K, canonical=False),
                             sm.TextHasher.from_tables(rng.integers(0, 1 << 32, 256, dtype=np.uint64),
                                                       rng.integers(0, 1 << 32, 256, dtype=np.uint64), 7, False)]
        self.b_text = [sm.minimizers(K, W).hasher(h) for h in self.text_hashers]
        self.w37 = next(w for w in (37, 35, 39, 43, 45) if w not in sm.prebuilt_window_sizes(False))
        self.b_w37 = sm.minimizers(K, self.w37)
        pre = set(sm.prebuilt_window_sizes(False, reads=True))
        self.w_reads = next(w for w in (23, 27, 29, 31, 35, 37, 45, 61) if w not in pre)
        self.b_reads_jit = sm.minimizers(K, self.w_reads).super_kmers([])
        for b in (self.b_canon, self.b_canon_sk, self.b_fwd, self.b_w37, self.b_reads_jit):
            b.plan()  # (made here, shared by every worker)
        for b in self.b_text:
            b.text_plan()

    # ---------------------------------------------------------------- inputs + expectations (main thread)
    def _dev(self, t):
        return self.devices[t % len(self.devices)]

    def _gen(self, seed, n):
        return self.oracle.gen_packed(seed, n)

    def make_jobs(self, t, r):
        torch, oracle, sm = self.torch, self.oracle, self.sm
        dev = f"cuda:{self._dev(t)}"
        rng = np.random.default_rng(1_000_003 * (t + 1) + 7919 * r)
        seed = lambda j: 100_000 * t + 1000 * r + j  # noqa: E731
        jobs = []
        want = lambda f, *a, **kw: self.pool.submit(f, *a, **kw)  # noqa: E731

        if "fused" in self.jobs:
            n = int(rng.integers(8_000_000, 24_000_000))
            h = self._gen(seed(1), n)
            d = torch.from_numpy(h).to(dev)
            out = torch.zeros(n // 3 + 64, dtype=torch.int32, device=dev)
            f = want(oracle.run_threads, h, n, K, W, canonical=True, threads=ORACLE_THREADS)
            jobs.append(Job("fused", lambda ws, d=d, n=n, out=out: self.b_canon.workspace(ws).run_device(d, n, out),
                            lambda cnt, out=out, f=f: _eq(out[:cnt].cpu().numpy().view(np.uint32), f.result(), "fused")))
        if "fused_sk" in self.jobs:
            n = int(rng.integers(4_000_000, 8_000_000))
            h = self._gen(seed(2), n)
            d = torch.from_numpy(h).to(dev)
            out = torch.zeros(n // 3 + 64, dtype=torch.int32, device=dev)
            sk = torch.zeros_like(out)
            f = want(oracle.run_threads, h, n, K, W, canonical=True, super_kmers=True, threads=ORACLE_THREADS)

            def check(cnt, out=out, sk=sk, f=f):
                wp, ws_ = f.result()
                _eq(sk[:cnt].cpu().numpy().view(np.uint32), ws_, "fused_sk indices")
                return _eq(out[:cnt].cpu().numpy().view(np.uint32), wp, "fused_sk")
            jobs.append(Job("fused_sk", lambda ws, d=d, n=n, out=out, sk=sk:
                            self.b_canon_sk.workspace(ws).run_device(d, n, out, out_sk=sk), check))
        if "host_small" in self.jobs:
            lens = [int(x) for x in rng.integers(1000, 5001, 200)]
            hs = [self._gen(seed(3) * 1000 + i, m) for i, m in enumerate(lens)]
            fs = [want(oracle.run, h, m, K, W, canonical=True) for h, m in zip(hs, lens)]

            def run(ws, hs=hs, lens=lens):
                b = self.b_canon.workspace(ws)
                return [b._run_arrays(sm.PackedSeq(h, 0, m))[0].copy() for h, m in zip(hs, lens)]
            jobs.append(Job("host_small", run,
                            lambda got, fs=fs: (len(got) == len(fs) or _eq([], [0], "host_small calls")) and
                            sum(_eq(g, f.result(), "host_small") for g, f in zip(got, fs)), calls=200))
        if "host_pipelined" in self.jobs and t < 2:
            n = 52_000_000 + int(rng.integers(0, 1000))
            h = self._gen(seed(4), n)
            f = want(oracle.run_threads, h, n, K, W, canonical=True, threads=ORACLE_THREADS)
            jobs.append(Job("host_pipelined", lambda ws, h=h, n=n:
                            self.b_canon.workspace(ws)._run_arrays(sm.PackedSeq(h, 0, n))[0].copy(),
                            lambda got, f=f: _eq(got, f.result(), "host_pipelined")))
        if "batch_lane_table" in self.jobs:
            lens = [int(x) for x in rng.integers(0, 10_001, 2000)]
            st = np.zeros(len(lens) + 1, dtype=np.int64)
            st[1:] = np.cumsum(lens)
            h = self._gen(seed(5), int(st[-1]) + 4)
            d = torch.from_numpy(h).to(dev)
            seqs = [d[int(s) // 4:] for s in st[:-1]]
            boffs = [int(s) % 4 for s in st[:-1]]
            out = torch.zeros(int(st[-1]) // 3 + 64, dtype=torch.int32, device=dev)

            def expect(h=h, st=st, lens=lens):
                return [oracle.run(h, m, K, W, canonical=True, base_offset=int(s)) for s, m in zip(st[:-1], lens)]
            f = want(expect)

            def run(ws, seqs=seqs, lens=lens, boffs=boffs, out=out):
                b = self.b_canon.workspace(ws)
                offs = sm.run_batch_device(b, seqs, lens, out, base_offsets=boffs)
                return offs, ws.last_lane_table()

            def check(res, out=out, f=f):
                offs, lane_table = res
                assert lane_table, "the batch in one allocation did not take the lane table"
                got = out[:offs[-1]].cpu().numpy().view(np.uint32)
                return sum(_eq(got[offs[i]:offs[i + 1]], e, f"batch contig {i}") for i, e in enumerate(f.result()))
            jobs.append(Job("batch_lane_table", run, check))
        if "reads_sk" in self.jobs:
            jobs.append(self._reads_job(t, r, dev, seed(6), 10_000, 150, self.b_canon_sk, True, "reads_sk"))
        if "skip_ambiguous" in self.jobs:
            n = int(rng.integers(1_000_000, 2_000_001))
            a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
            for s0 in rng.integers(0, n, 40):  # runs of N
                a[s0: s0 + int(rng.integers(1, 300))] = ord("N")
            a[rng.integers(0, n, n // 500)] = ord("n")
            packed, amb = oracle.pack_ascii_n(a.tobytes())
            nseq = sm.PackedNSeq(sm.PackedSeq(packed, 0, n), amb, 0)
            f = want(oracle.run_skip_ambiguous, packed, amb, n, K, W)
            jobs.append(Job("skip_ambiguous", lambda ws, nseq=nseq:
                            self.b_canon.workspace(ws).run_skip_ambiguous_windows_once(nseq),
                            lambda got, f=f: _eq(got, f.result(), "skip_ambiguous")))
        if "text_single" in self.jobs:
            import text_checker
            n = 1_000_000 + int(rng.integers(0, 5000))
            text = (text_checker.english_like(n, seed(7)) if (t + r) % 2 else
                    rng.integers(0, 256, n, dtype=np.uint8)).tobytes()
            hi = (t + r) % 2  # the two hashers alternate between threads and rounds
            f = want(text_checker.run, text, K, W, self.text_hashers[hi], canonical=False)
            jobs.append(Job("text_single", lambda ws, text=text, hi=hi: self.b_text[hi].workspace(ws)._run_arrays(text)[0],
                            lambda got, f=f: _eq(got, f.result(), "text_single")))
        if "text_batch" in self.jobs:
            lens = [int(x) for x in rng.integers(0, 200, 10_000)]
            lens[int(rng.integers(0, len(lens)))] = 50_000  # one record spans several tiles
            text = rng.integers(0, 256, sum(lens), dtype=np.uint8)
            st = np.zeros(len(lens) + 1, dtype=np.int64)
            st[1:] = np.cumsum(lens)
            recs = [text[st[i]:st[i + 1]] for i in range(len(lens))]
            f = want(_text_batch_expect, text, st, K, W, self.text_hashers[0])

            def check(res, f=f):
                pos, offs, _ = res
                wp, wo = f.result()
                assert offs == wo, "text_batch offsets"
                return _eq(pos, wp, "text_batch")
            jobs.append(Job("text_batch", lambda ws, recs=recs: sm.run_text_batch_host(self.b_text[0].workspace(ws), recs),
                            check))
        if "values_u64" in self.jobs:
            n = 8_000_000 + int(rng.integers(0, 1000))
            h = self._gen(seed(8), n)
            pos = np.sort(rng.integers(0, n - K + 1, 4_000_000)).astype(np.uint32)
            canon = bool((t + r) % 2)
            f = want(oracle.values_u64, h, K, pos, canon)

            def run(ws, h=h, n=n, pos=pos, canon=canon):
                vals = np.zeros(len(pos), dtype=np.uint64)
                sm._check(sm.lib().mm_values_u64_host(ws.h, h.ctypes.data_as(C.POINTER(C.c_uint8)), 0, n, K, int(canon),
                                                      pos.ctypes.data_as(C.POINTER(C.c_uint32)), len(pos),
                                                      vals.ctypes.data_as(C.POINTER(C.c_uint64))))
                return vals

            def check(vals, f=f):
                want_ = f.result()
                if not np.array_equal(vals, want_):
                    raise AssertionError(f"values_u64: first difference at {int(np.argmax(vals != want_))}")
                return len(want_)
            jobs.append(Job("values_u64", run, check))
        if "fastq_reads" in self.jobs:
            jobs.append(self._fastq_job(t, r, dev, rng, seed(9)))
        if "jit_fwd_w37" in self.jobs:
            n = 1_000_000 + int(rng.integers(0, 1000))
            h = self._gen(seed(10), n)
            d = torch.from_numpy(h).to(dev)
            out = torch.zeros(n // 3 + 64, dtype=torch.int32, device=dev)
            f = want(oracle.run, h, n, K, self.w37)
            jobs.append(Job("jit_fwd_w37", lambda ws, d=d, n=n, out=out: self.b_w37.workspace(ws).run_device(d, n, out),
                            lambda cnt, out=out, f=f: _eq(out[:cnt].cpu().numpy().view(np.uint32), f.result(),
                                                          "jit_fwd_w37")))
        if "jit_reads_sk" in self.jobs:
            jobs.append(self._reads_job(t, r, dev, seed(11), 3000, 150, self.b_reads_jit, False, "jit_reads_sk"))
        return jobs

    def _reads_job(self, t, r, dev, sd, n_reads, rl, builder, canonical, name):
        torch, oracle, sm = self.torch, self.oracle, self.sm
        h = self._gen(sd, n_reads * rl)
        d = torch.from_numpy(h).to(dev)
        out = torch.zeros(n_reads * rl // 2, dtype=torch.int32, device=dev)
        sk = torch.zeros_like(out)
        offs = torch.zeros(n_reads + 1, dtype=torch.int64, device=dev)

        def expect():
            res = [oracle.run(h, rl, builder.k, builder.w, canonical=canonical, base_offset=i * rl, super_kmers=True)
                   for i in range(n_reads)]
            return np.concatenate([p for p, _ in res]), np.concatenate([s for _, s in res]), [len(p) for p, _ in res]
        f = self.pool.submit(expect)

        def run(ws):
            return sm.run_reads_device(builder.workspace(ws), d, n_reads, rl, rl, out, offs, out_sk=sk)

        def check(cnt):
            wp, wsk, lens = f.result()
            o = offs.cpu().numpy()
            assert np.array_equal(np.diff(o), lens), f"{name}: per-read counts"
            _eq(sk[:cnt].cpu().numpy().view(np.uint32), wsk, f"{name} indices")
            return _eq(out[:cnt].cpu().numpy().view(np.uint32), wp, name)
        return Job(name, run, check)

    def _fastq_job(self, t, r, dev, rng, sd):
        torch, oracle, sm = self.torch, self.oracle, self.sm
        parts, size, i = [], 0, 0
        g = np.random.default_rng(sd)
        while size < 1_000_000:
            m = int(g.integers(60, 400))
            s = np.frombuffer(b"ACGT", dtype=np.uint8)[g.integers(0, 4, m)].tobytes()
            rec = b"@t%dr%dn%d\n" % (t, r, i) + s + b"\n+\n" + b"I" * m + b"\n"
            parts.append(rec)
            size += len(rec)
            i += 1
        text = b"".join(parts)
        d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
        out = torch.zeros(len(text) // 2, dtype=torch.int32, device=dev)
        offs = torch.zeros(i + 1, dtype=torch.int64, device=dev)
        device = self._dev(t)

        def expect():
            res = []
            for _, _, s in oracle.fastq_records(text):
                res.append(oracle.run(oracle.pack_ascii(s), len(s), K, W, canonical=True))
            return np.concatenate(res), [len(p) for p in res]
        f = self.pool.submit(expect)

        def run(ws):
            rec = sm.fasta_pack_device(d_text, max_records=i + 16, device=device)
            return len(rec), sm.run_packed_reads_device(self.b_canon.workspace(ws), rec, out, offs)

        def check(res):
            n_rec, cnt = res
            wp, lens = f.result()
            assert n_rec == len(lens) == i, f"fastq_reads: {n_rec} records, {len(lens)} expected"
            assert np.array_equal(np.diff(offs.cpu().numpy()), lens), "fastq_reads: per-read counts"
            return _eq(out[:cnt].cpu().numpy().view(np.uint32), wp, "fastq_reads")
        return Job("fastq_reads", run, check)


def run_workload(n_threads=8, rounds=3, devices=None, jobs=JOBS):
    """Runs the workload; returns the summary dict ("ok", "failures", per-job "calls" / "positions", "wall_s",
    "ticket_mode_workspaces", "device_unchanged")."""
    import torch

    import mm_oracle as oracle
    import simd_minimizers_amd as sm

    devices = list(devices) if devices is not None else [0]
    wl = Workload(sm, oracle, torch, devices, jobs)
    t0 = time.time()
    plans = [[None] * rounds for _ in range(n_threads)]
    for t in range(n_threads):
        for r in range(rounds):
            js = wl.make_jobs(t, r)
            order = np.random.default_rng(31 * t + r).permutation(len(js))
            js = [js[i] for i in order]
            if r == 0:  # (first uses of the run-time-compiled kernels overlap in every thread)
                js = [j for j in js if j.name in JIT_JOBS] + [j for j in js if j.name not in JIT_JOBS]
            plans[t][r] = js
    for d in devices:
        torch.cuda.synchronize(d)
    t_prep = time.time() - t0
    workspaces = [sm.Workspace(devices[t % len(devices)]) for t in range(n_threads)]
    results = [[None] * rounds for _ in range(n_threads)]
    errors, dev_same = [], [None] * n_threads
    barrier = threading.Barrier(n_threads)

    def worker(t):
        try:
            before = torch.cuda.current_device()
            for r in range(rounds):
                barrier.wait()
                results[t][r] = [job.run(workspaces[t]) for job in plans[t][r]]
            dev_same[t] = torch.cuda.current_device() == before
        except BaseException as e:  # (reported by the main thread)
            errors.append(f"thread {t}: {type(e).__name__}: {e}")
            barrier.abort()

    t1 = time.time()
    threads = [threading.Thread(target=worker, args=(t,)) for t in range(n_threads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    t_run = time.time() - t1
    stats = {}
    failures = list(errors)
    if not errors:
        for t in range(n_threads):
            for r in range(rounds):
                for job, res in zip(plans[t][r], results[t][r]):
                    s = stats.setdefault(job.name, {"calls": 0, "positions": 0})
                    try:
                        s["positions"] += int(job.check(res))
                        s["calls"] += job.calls
                    except AssertionError as e:
                        failures.append(f"thread {t} round {r}: {e}")
    ticket = sum(ws.ticket_mode() for ws in workspaces)
    for ws in workspaces:
        ws.close()
    wl.pool.shutdown()
    return {"ok": not failures and all(dev_same), "failures": failures[:20], "threads": n_threads, "rounds": rounds,
            "devices": devices, "jobs": stats, "prep_s": round(t_prep, 2), "wall_s": round(t_run, 2),
            "ticket_mode_workspaces": ticket, "device_unchanged": all(x is True for x in dev_same)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lib", help="the engine library to load (MM_LIB_PATH), e.g. the host-sanitized build")
    ap.add_argument("--jobs", help="comma-separated subset of: " + ",".join(JOBS))
    ap.add_argument("--devices", help="comma-separated device ids (thread t works on devices[t % n]); default 0")
    a = ap.parse_args(argv)
    if a.lib:
        os.environ["MM_LIB_PATH"] = a.lib  # (before the package is imported: it reads it once)
    jobs = tuple(a.jobs.split(",")) if a.jobs else JOBS
    unknown = set(jobs) - set(JOBS)
    if unknown:
        ap.error(f"unknown jobs {sorted(unknown)}")
    devices = [int(x) for x in a.devices.split(",")] if a.devices else None
    summary = run_workload(a.threads, a.rounds, devices, jobs)
    print(json.dumps(summary), flush=True)
    return 0 if summary["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
