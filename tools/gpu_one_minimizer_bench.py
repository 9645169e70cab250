"""One minimizer per record on one MI355X: mm_one_minimizer_reads_device_async / mm_one_minimizer_text_batch_device_async
against the closest existing kernels on the same buffers, and against the traffic bound.

Forward NtHasher, k = 21, inputs resident in HBM, both read workloads taken from simd_minimizers_amd/workloads.py:

  READS       8 M reads x 150 bp, fixed stride
  LONGREADS   200 000 reads, lengths log-uniform 1-50 kbp, packed back to back

Per workload:
  (a) the new call
  (b) mm_run_reads_device / mm_run_packed_reads_device, forward minimizers k=21 w=11, on the same buffers: it reads the same
      bytes and does more work per base
  (c) the traffic bound: packed bytes + 8 n_reads (starts; fixed stride: none) + 4 n_reads (out) + the key array's traffic
      (8 n_reads written by the fill, 8 n_reads read by the finish kernel; the atomics' traffic is not counted) at the HBM
      peak bench.py's roofline uses
and (d) on 1 M protein-like records (20 letters, lengths log-normal around 300), the text form with TextMulHasher k=7
against mm_run_text_batch_device forward k=7 w=11.

bench.py's protocol: a 200 ms untimed ramp of the step, 3 warm-up steps, then the median of 7 timed steps, each bracketed
by HIP events on the workspace's stream.  Nothing is gated: a/b, a/c and d's ratio are reported as ratios of RATES
(a_over_b = b's time / a's time: below 1 means the new call is slower than the minimizer run; a_over_c: the fraction of the
traffic bound's rate it reaches; d_ratio: the text form's rate over the text batch run's).

  python tools/gpu_one_minimizer_bench.py [--steps 7] [--warmup 3] [--out profiles/one_minimizer_bench.json]
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

K, W, TEXT_K = 21, 11, 7
HBM_PEAK_GBPS = 8000.0  # (bench.py's roofline)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--only", default=None, help="READS, LONGREADS or TEXT: one row (for a profiler run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import simd_minimizers_amd as sm
    from simd_minimizers_amd import workloads

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ws = sm.Workspace(0, stream.cuda_stream)
    L = sm.lib()
    ramp_ms = float(os.environ.get("MM_BENCH_RAMP_MS", "200"))
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def timed(step):
        """median milliseconds of `step` (asynchronous on the workspace stream)"""
        with torch.cuda.stream(stream):
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

    rows = []
    nt = sm.NtHasher(K, False)
    fwd = sm.minimizers(K, W).workspace(ws)
    for name in ("READS", "LONGREADS"):
        if args.only and args.only != name:
            continue
        with torch.cuda.stream(stream):
            c = workloads.component(name, ws, dev)
        ws.sync()
        n = c["units"]
        if name == "READS":
            d, out, _, offs, cnt = c["keep"]
            n_reads, stride, starts, mx = 8_000_000, 150, None, 150
        else:
            d, out, offs, cnt, starts = c["keep"]
            n_reads, stride = c["reads"], 0
            mx = int((starts[1:] - starts[:-1]).max().item())
        pos = torch.empty(n_reads + 16, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)

        def one_step():
            sm._check(L.mm_one_minimizer_reads_device_async(ws.h, C.byref(nt), K, vp(d), d.numel(), 0, n_reads, vp(starts),
                                                            stride, stride, vp(pos)))

        def run_step():
            if starts is None:
                sm.run_reads_device(fwd, d, n_reads, stride, stride, out, offs, d_count=cnt, sync=False)
            else:
                sm._check(L.mm_run_packed_reads_device_async(fwd.plan().h, ws.h, vp(d), d.numel(), 0, n_reads, vp(starts), n, mx,
                                                             vp(out), None, out.numel(), vp(offs), vp(cnt)))
        a_ms, a_all = timed(one_step)
        b_ms, b_all = timed(run_step)
        traffic = (n + 3) // 4 + (8 * (n_reads + 1) if starts is not None else 0) + 4 * n_reads + 16 * n_reads
        c_ms = traffic / (HBM_PEAK_GBPS * 1e9) * 1e3
        row = {"workload": name, "what": c["what"].split(",")[0], "reads": n_reads, "bases": n,
               "a_one_minimizer_ms": a_ms, "a_ms_all": a_all, "a_Gbases_per_s": n / a_ms / 1e6,
               "b_minimizer_run_ms": b_ms, "b_ms_all": b_all, "b_what": f"forward minimizers k={K} w={W}, same buffers",
               "c_traffic_bytes": traffic, "c_bound_ms": c_ms, "a_GBps": traffic / a_ms / 1e6,
               "a_over_b": b_ms / a_ms, "a_over_c": c_ms / a_ms}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del c, d, out, offs, cnt, starts, pos
        torch.cuda.empty_cache()

    if not args.only or args.only == "TEXT":
        g = torch.Generator(device=dev)
        g.manual_seed(12)
        lens = torch.exp(5.7 + 0.6 * torch.randn(args.records, device=dev, generator=g, dtype=torch.float64)).to(torch.int64) + 1
        starts = torch.zeros(args.records + 1, dtype=torch.int64, device=dev)
        starts[1:] = torch.cumsum(lens, 0)
        n = int(starts[-1].item())
        letters = torch.tensor(list(b"ACDEFGHIKLMNPQRSTVWY"), dtype=torch.uint8, device=dev)
        text = letters[torch.randint(0, 20, (n,), device=dev, generator=g)]
        th = sm.TextMulHasher(TEXT_K, False)
        tb = sm.minimizers(TEXT_K, W).workspace(ws)
        pos = torch.empty(args.records + 16, dtype=torch.int32, device=dev)
        out = torch.empty(int(n * 0.25) + 4096, dtype=torch.int32, device=dev)
        offs = torch.zeros(args.records + 1, dtype=torch.int64, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)

        def text_step():
            sm._check(L.mm_one_minimizer_text_batch_device_async(ws.h, C.byref(th), TEXT_K, vp(text), n, args.records, vp(starts),
                                                                 vp(pos)))

        def text_run_step():
            sm._check(L.mm_run_text_batch_device_async(tb.text_plan().h, ws.h, vp(text), n, args.records, vp(starts), n, vp(out),
                                                       None, out.numel(), vp(offs), vp(cnt)))
        a_ms, a_all = timed(text_step)
        b_ms, b_all = timed(text_run_step)
        row = {"workload": "TEXT", "what": f"{args.records} protein-like records, {n} bytes", "records": args.records, "bytes": n,
               "d_one_minimizer_ms": a_ms, "d_ms_all": a_all, "d_GB_per_s": n / a_ms / 1e6,
               "d_text_batch_run_ms": b_ms, "d_run_ms_all": b_all,
               "d_run_what": f"mm_run_text_batch_device forward k={TEXT_K} w={W}", "d_ratio": b_ms / a_ms}
        print(json.dumps(row), flush=True)
        rows.append(row)

    result = {"tool": "gpu_one_minimizer_bench", "k": K, "w": W, "text_k": TEXT_K, "hasher": "forward NtHasher / TextMulHasher",
              "tile": sm.one_minimizer_tile(), "steps": args.steps, "warmup": args.warmup, "hbm_peak_GBps": HBM_PEAK_GBPS,
              "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    ws.close()


if __name__ == "__main__":
    main()
