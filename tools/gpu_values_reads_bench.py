"""K-mer values of every read in one launch on one MI355X: values per second of mm_values_u64_reads_device_async.

Two batches, both generated on the device (mm_generate_device_async), canonical minimizers k=21 w=11:

  short   8 M reads x 150 bases, fixed stride        positions from mm_run_reads_device
  long    200 k reads, lengths log-uniform 1-50 kbp  positions from mm_run_packed_reads_device (reads back to back)

Per batch, in the same process:

  reads       mm_values_u64_reads_device_async over all reads' positions (one launch; the true count read on the device)
  single      (a) mm_values_u64_device_async on the SAME NUMBER of positions of ONE sequence of the batch's size: the
              yardstick - the existing values kernel, which has no read lookup and no per-read starts
  loop        (b) a per-read loop: mm_values_u64_device_async once per read over the first 10 000 reads (asynchronous
              calls, one synchronize at the end), scaled to values per second of those reads

bench.py's protocol: a 200 ms untimed ramp of the step, warm-up steps, then the median of timed steps, each bracketed by
HIP events on the workspace stream.  Nothing is gated: `reads_over_single` is reported.

  python tools/gpu_values_reads_bench.py [--steps 7] [--warmup 3] [--reads 8000000] [--long-reads 200000]
                                         [--out profiles/values_reads_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, W = 21, 11
LOOP_READS = 10_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reads", type=int, default=8_000_000)
    ap.add_argument("--long-reads", type=int, default=200_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import simd_minimizers_amd as sm

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ws = sm.Workspace(0, stream.cuda_stream)
    L = sm.lib()
    ramp_ms = float(os.environ.get("MM_BENCH_RAMP_MS", "200"))
    b = sm.canonical_minimizers(K, W).workspace(ws)

    def vp(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def generate(n, seed):
        t = torch.zeros((n + 3) // 4 + 64, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        sm._check(L.mm_generate_device_async(ws.h, seed, 0, n, vp(t)))
        ws.sync()
        return t

    def timed(step):
        """median milliseconds of `step` (asynchronous on the workspace stream)"""
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
            e0.record(stream)
            step()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ws.check()
        return statistics.median(ms), ms

    def measure(label, d, n_bases, n_reads, d_starts, stride, d_pos, d_offs, count, host_starts, host_offs):
        vals = torch.empty(count + 16, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)

        def reads_step():
            sm._check(L.mm_values_u64_reads_device_async(ws.h, vp(d), d.numel(), 0, n_reads, vp(d_starts), stride, K, 1,
                                                         vp(d_pos), vp(d_offs), count, vp(vals)))
        reads_ms, reads_all = timed(reads_step)

        # (a) the same number of positions of ONE sequence of the same size
        one_pos = torch.empty(int(n_bases * 0.2) + 4096, dtype=torch.int32, device=dev)
        c1 = b.run_device(d, n_bases, one_pos)
        c = min(c1, count)

        def single_step():
            sm._check(L.mm_values_u64_device_async(ws.h, vp(d), d.numel(), 0, n_bases, K, 1, vp(one_pos), c, vp(vals)))
        single_ms, single_all = timed(single_step)
        del one_pos

        # (b) one call per read over the first LOOP_READS reads
        m = min(LOOP_READS, n_reads)
        ptr_pos, ptr_val = d_pos.data_ptr(), vals.data_ptr()
        calls = [(int(host_starts[r]), int(host_starts[r + 1] - host_starts[r]) if d_starts is not None else stride,
                  int(host_offs[r]), int(host_offs[r + 1] - host_offs[r])) for r in range(m)]
        loop_values = int(host_offs[m] - host_offs[0])

        def loop_step():
            for start, ln, off, cnt in calls:
                if cnt:
                    sm._check(L.mm_values_u64_device_async(ws.h, vp(d), d.numel(), start, ln, K, 1, C.c_void_p(ptr_pos + 4 * off),
                                                           cnt, C.c_void_p(ptr_val + 8 * off)))
        for _ in range(2):  # (warm-up)
            loop_step()
            ws.sync()
        t1 = time.perf_counter()
        loop_step()
        ws.sync()
        loop_s = time.perf_counter() - t1
        row = {
            "batch": label, "reads": n_reads, "bases": n_bases, "values": count,
            "reads_ms": reads_ms, "reads_ms_all": reads_all, "reads_Gvalues_per_s": count / reads_ms / 1e6,
            "single_values": c, "single_ms": single_ms, "single_ms_all": single_all,
            "single_Gvalues_per_s": c / single_ms / 1e6,
            "reads_over_single": (count / reads_ms) / (c / single_ms),
            "loop_reads": m, "loop_values": loop_values, "loop_s": loop_s, "loop_us_per_call": loop_s / max(1, m) * 1e6,
            "loop_Gvalues_per_s": loop_values / loop_s / 1e9,
            # what the reads kernel moves per value beyond the sequence: 4 (position) + 8 (value), plus 8 per read (offset)
            # and 8 per read with starts
            "reads_alg_bytes": (n_bases + 3) // 4 + 12 * count + (16 if d_starts is not None else 8) * (n_reads + 1),
        }
        row["reads_alg_GBps"] = row["reads_alg_bytes"] / reads_ms / 1e6
        print(json.dumps(row), flush=True)
        return row

    rows = []
    # short: fixed-stride reads
    n_reads, rl = args.reads, 150
    n = n_reads * rl
    d = generate(n, 4)
    d_pos = torch.empty(int(n * 0.2) + 4096, dtype=torch.int32, device=dev)
    d_offs = torch.zeros(n_reads + 1, dtype=torch.int64, device=dev)
    count = sm.run_reads_device(b, d, n_reads, rl, rl, d_pos, d_offs)
    m = min(LOOP_READS, n_reads)
    host_offs = d_offs[: m + 1].cpu().numpy()
    host_starts = [r * rl for r in range(m + 1)]
    rows.append(measure(f"{n_reads} reads x {rl} bases, fixed stride", d, n, n_reads, None, rl, d_pos, d_offs, count,
                        host_starts, host_offs))
    del d, d_pos, d_offs
    torch.cuda.empty_cache()

    # long: log-uniform 1-50 kbp, packed back to back
    g = torch.Generator(device=dev)
    g.manual_seed(6)
    u = torch.rand(args.long_reads, device=dev, generator=g, dtype=torch.float64)
    lens = torch.exp(math.log(1000.0) + u * (math.log(50_000.0) - math.log(1000.0))).to(torch.int64)
    n_reads = int(lens.numel())
    starts = torch.zeros(n_reads + 1, dtype=torch.int64, device=dev)
    starts[1:] = torch.cumsum(lens, 0)
    n = int(starts[-1].item())
    mx = int(lens.max().item())
    d = generate(n, 7)
    d_pos = torch.empty(int(n * 0.2) + 4096, dtype=torch.int32, device=dev)
    d_offs = torch.zeros(n_reads + 1, dtype=torch.int64, device=dev)
    cnt = C.c_uint64()
    sm._check(L.mm_run_packed_reads_device(b.plan().h, ws.h, vp(d), d.numel(), 0, n_reads, vp(starts), n, mx, vp(d_pos), None,
                                           d_pos.numel(), vp(d_offs), C.byref(cnt)))
    m = min(LOOP_READS, n_reads)
    rows.append(measure(f"{n_reads} reads, lengths log-uniform 1-50 kbp, packed back to back", d, n, n_reads, starts, 0, d_pos,
                        d_offs, int(cnt.value), starts[: m + 1].cpu().numpy(), d_offs[: m + 1].cpu().numpy()))
    result = {"tool": "gpu_values_reads_bench", "k": K, "w": W, "canonical": True, "steps": args.steps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    ws.close()


if __name__ == "__main__":
    main()
