"""K-mer values of every sequence of a device batch in one launch on one MI355X: values per second of
mm_values_u64_batch_device_async.

Two shapes, both generated on the device (mm_generate_device_async) as one buffer whose sequences are handed over one by
one ({pointer, bytes, base offset} each), positions from mm_run_batch_device:

  BATCH10K   20 000 sequences x 10 kbp, canonical minimizers k=21 w=11
  C4         the 24 CHM13-like contigs, canonical minimizers k=31 w=51

Per shape, in the same process, on the same positions:

  batch       (a) mm_values_u64_batch_device_async over all sequences' positions: one launch (the call stages the tables
              and queues their upload as well; all of it is inside the timed step)
  loop        (b) mm_values_u64_device_async once per sequence (asynchronous calls, one synchronize at the end): the only
              way before the batch call existed
  single      (c) mm_values_u64_device_async on the SAME NUMBER of positions of ONE sequence of the batch's size: the
              yardstick - the single-sequence kernel, which has no lookup and no per-sequence descriptors
  and where (a)'s time goes: the host's share of the call (building and staging the tables, wall clock), and the device's
  share alone (the tables' upload + the kernel), timed by events behind queued work that hides the host's share

bench.py's protocol: a 200 ms untimed ramp of the step, warm-up steps, then the median of timed steps.  (a) and (c) are
bracketed by HIP events on the workspace stream; (b) is host-bound (one launch per sequence) and timed by the wall clock
around the loop and its synchronize.  Nothing is gated: the ratios are reported.

  python tools/gpu_values_batch_bench.py [--steps 7] [--warmup 3] [--shapes BATCH10K,C4] [--out profiles/values_batch_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="BATCH10K,C4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import simd_minimizers_amd as sm
    from simd_minimizers_amd import sharding

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ws = sm.Workspace(0, stream.cuda_stream)
    L = sm.lib()
    ramp_ms = float(os.environ.get("MM_BENCH_RAMP_MS", "200"))

    def vp(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def timed_events(step, before=None):
        """median milliseconds of `step` (asynchronous on the workspace stream), by HIP events; `before` is queued ahead of
        the first event of every timed step (work that keeps the device busy while the host prepares `step`)"""
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < ramp_ms:
            step()
            ws.sync()
        for _ in range(args.warmup):
            step()
        ws.sync()
        ms = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if before is not None:
                before()
            e0.record(stream)
            step()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ws.check()
        return statistics.median(ms), ms

    def timed_call(step):
        """median milliseconds the host spends inside `step` (the call returns with its work queued)"""
        ms = []
        for _ in range(args.steps):
            ws.sync()
            t0 = time.perf_counter()
            step()
            ms.append((time.perf_counter() - t0) * 1e3)
        ws.sync()
        return statistics.median(ms), ms

    def timed_wall(step):
        """median milliseconds of `step` + synchronize, by the wall clock (host-bound steps)"""
        for _ in range(max(1, args.warmup)):
            step()
            ws.sync()
        ms = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            step()
            ws.sync()
            ms.append((time.perf_counter() - t0) * 1e3)
        ws.check()
        return statistics.median(ms), ms

    def measure(label, lens, k, w, seed):
        n_seqs, n = len(lens), sum(lens)
        b = sm.canonical_minimizers(k, w).workspace(ws)
        d = torch.zeros((n + 3) // 4 + 64, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        sm._check(L.mm_generate_device_async(ws.h, seed, 0, n, vp(d)))
        ws.sync()
        starts = [0]
        for m in lens:
            starts.append(starts[-1] + m)
        ptrs = (C.c_void_p * n_seqs)(*[d.data_ptr() + starts[s] // 4 for s in range(n_seqs)])
        bases = (C.c_uint64 * n_seqs)(*[starts[s] % 4 for s in range(n_seqs)])
        n_bases = (C.c_uint64 * n_seqs)(*lens)
        # what the run may read (the walk's loads run past a sequence's last base) and a sequence's own bytes
        run_bytes = (C.c_uint64 * n_seqs)(*[d.numel() - starts[s] // 4 for s in range(n_seqs)])
        own_bytes = (C.c_uint64 * n_seqs)(*[(starts[s] % 4 + lens[s] + 3) // 4 for s in range(n_seqs)])
        d_pos = torch.empty(int(n * 2.3 / (w + 1)) + 4096, dtype=torch.int32, device=dev)
        offs = (C.c_uint64 * (n_seqs + 1))()
        torch.cuda.synchronize(dev)
        sm._check(L.mm_run_batch_device(b.plan().h, ws.h, n_seqs, ptrs, run_bytes, bases, n_bases, vp(d_pos), None,
                                        d_pos.numel(), offs))
        count = int(offs[n_seqs])
        vals = torch.empty(count + 16, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)

        def batch_step():
            sm._check(L.mm_values_u64_batch_device_async(ws.h, n_seqs, ptrs, own_bytes, bases, n_bases, k, 1, vp(d_pos), offs,
                                                         vp(vals)))
        batch_ms, batch_all = timed_events(batch_step)

        ptr_pos, ptr_val = d_pos.data_ptr(), vals.data_ptr()
        calls = [(C.c_void_p(ptrs[s]), int(run_bytes[s]), int(bases[s]), int(lens[s]), C.c_void_p(ptr_pos + 4 * int(offs[s])),
                  int(offs[s + 1] - offs[s]), C.c_void_p(ptr_val + 8 * int(offs[s]))) for s in range(n_seqs)]

        def loop_step():
            for p, nb, bo, m, pp, cnt, pv in calls:
                if cnt:
                    sm._check(L.mm_values_u64_device_async(ws.h, p, nb, bo, m, k, 1, pp, cnt, pv))
        loop_ms, loop_all = timed_wall(loop_step)

        # (c) the same number of positions of ONE sequence of the same size
        one_pos = torch.empty(d_pos.numel(), dtype=torch.int32, device=dev)
        c = min(b.run_device(d, n, one_pos), count)

        def single_step():
            sm._check(L.mm_values_u64_device_async(ws.h, vp(d), d.numel(), 0, n, k, 1, vp(one_pos), c, vp(vals)))
        single_ms, single_all = timed_events(single_step)

        # where (a)'s time goes: the host's share of the call (it builds and stages the tables before anything is queued,
        # the device idles meanwhile), and the device's share alone - the tables' upload and the kernel - timed behind
        # enough queued work that the host's share overlaps it
        host_ms, host_all = timed_call(batch_step)
        busy = max(2, int(4 * host_ms / single_ms) + 1)

        def keep_busy():
            for _ in range(busy):
                single_step()
        device_ms, device_all = timed_events(batch_step, before=keep_busy)

        a_rate, b_rate, c_rate = count / batch_ms / 1e6, count / loop_ms / 1e6, c / single_ms / 1e6
        row = {
            "shape": label, "sequences": n_seqs, "bases": n, "k": k, "w": w, "values": count,
            "batch_ms": batch_ms, "batch_ms_all": batch_all, "batch_Gvalues_per_s": a_rate,
            "loop_ms": loop_ms, "loop_ms_all": loop_all, "loop_Gvalues_per_s": b_rate,
            "loop_us_per_call": loop_ms * 1e3 / n_seqs,
            "single_values": c, "single_ms": single_ms, "single_ms_all": single_all, "single_Gvalues_per_s": c_rate,
            "batch_over_loop": a_rate / b_rate, "batch_over_single": a_rate / c_rate,
            "batch_host_ms": host_ms, "batch_host_ms_all": host_all,
            "batch_device_ms": device_ms, "batch_device_ms_all": device_all,
            "batch_device_Gvalues_per_s": count / device_ms / 1e6,
            "batch_device_over_single": (count / device_ms) / (c / single_ms),
            # what the batch kernel moves: the sequence, 4 (position) + 8 (value) per value, 8 + 32 per sequence
            "batch_alg_bytes": (n + 3) // 4 + 12 * count + 40 * n_seqs,
        }
        row["batch_alg_GBps"] = row["batch_alg_bytes"] / batch_ms / 1e6
        print(json.dumps(row), flush=True)
        return row

    rows = []
    for shape in args.shapes.split(","):
        if shape == "BATCH10K":
            rows.append(measure("BATCH10K: 20 000 sequences x 10 kbp", [10_000] * 20_000, 21, 11, 9))
        elif shape == "C4":
            rows.append(measure("C4: 24 CHM13-like contigs", list(sharding.CHM13_CONTIG_LENGTHS), 31, 51, 100))
        else:
            raise SystemExit(f"unknown shape {shape}")
        torch.cuda.empty_cache()
    result = {"tool": "gpu_values_batch_bench", "canonical": True, "steps": args.steps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    ws.close()


if __name__ == "__main__":
    main()
