"""Many records of byte text in one call (mm_run_text_batch_device) on one MI355X, against the single-text ceiling and a
per-record loop.

The workload is protein-like: about 1 M records whose lengths come from a seeded log-normal (median 300, clipped to
30 .. 35 000), bytes drawn from the 20 amino-acid letters, about 350 Mchar in all, generated on the device.  bench.py's
protocol: a 200 ms untimed ramp of the step, warm-up steps, then the median of timed steps, each bracketed by HIP events
on the workspace stream around the WHOLE call (the tile pre-kernel, the memsets and the walk).  Rows: forward and
canonical k=21 w=11 (comparable with tools/gpu_text_bench.py), a protein-typical forward k=7 w=11, closed syncmers
k=21 w=11.  Every row reports the batch call's Gchar/s, the single-text fused rate on the same characters
(mm_run_text_device over the concatenation, the ceiling) and their ratio, and a per-record loop of synchronous
mm_run_text_device calls over 10 000 of the records, as us per record (wall clock).

  python tools/gpu_text_batch_bench.py [--records 1000000] [--steps 5] [--warmup 3] [--loop 10000] [--out FILE]
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

ROWS = [  # (name, k, w, canonical, mode)
    ("minimizers", 21, 11, False, 0),
    ("canonical minimizers", 21, 11, True, 0),
    ("minimizers", 7, 11, False, 0),
    ("closed syncmers", 21, 11, False, 1),
]
MEDIAN, SIGMA, MIN_LEN, MAX_LEN = 300.0, 0.555, 30, 35_000  # (mean about 350: about 350 Mchar per 10^6 records)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop", type=int, default=10_000, help="records in the per-record loop")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", type=int, default=None, help="one row, by index")
    args = ap.parse_args()

    import torch

    import simd_minimizers_amd as sm

    dev = torch.device("cuda:0")
    ws = sm.default_workspace(0)
    L = sm.lib()
    g = torch.Generator(device=dev).manual_seed(args.seed)
    z = torch.randn(args.records, generator=g, device=dev, dtype=torch.float64)
    lens = torch.exp(math.log(MEDIAN) + SIGMA * z).round().clamp_(MIN_LEN, MAX_LEN).to(torch.int64)
    starts = torch.zeros(args.records + 1, dtype=torch.int64, device=dev)
    starts[1:] = torch.cumsum(lens, 0)
    n = int(starts[-1].item())
    aa = torch.tensor(list(b"ACDEFGHIKLMNPQRSTVWY"), dtype=torch.uint8, device=dev)
    text = aa[torch.randint(0, 20, (n,), generator=g, device=dev)]
    out = torch.empty(n, dtype=torch.int32, device=dev)
    offs = torch.empty(args.records + 1, dtype=torch.int64, device=dev)
    one = torch.empty(MAX_LEN, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ramp_ms = float(os.environ.get("MM_BENCH_RAMP_MS", "200"))
    starts_h = starts.cpu().numpy()
    rows = []
    for i, (name, k, w, canonical, mode) in enumerate(ROWS):
        if args.only is not None and args.only != i:
            continue
        ctor = {(0, False): sm.minimizers, (0, True): sm.canonical_minimizers,
                (1, False): sm.closed_syncmers}[(mode, canonical)]
        b = ctor(k, w).workspace(ws)
        plan = b.text_plan()

        def batch_step():
            r = L.mm_run_text_batch_device_async(plan.h, ws.h, C.c_void_p(text.data_ptr()), n, args.records,
                                                 C.c_void_p(starts.data_ptr()), n, C.c_void_p(out.data_ptr()), None, n,
                                                 C.c_void_p(offs.data_ptr()), None)
            if r:
                raise sm.MinimizerError(r, "mm_run_text_batch_device_async")

        def single_step():
            b.run_text_device(text, n, out, sync=False)

        def timed(step, steps):
            t0 = time.perf_counter()
            while (time.perf_counter() - t0) * 1e3 < ramp_ms:
                step()
                torch.cuda.synchronize(dev)
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize(dev)
            ws.check()
            ms = []
            for _ in range(steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step()
                e1.record()
                torch.cuda.synchronize(dev)
                ms.append(e0.elapsed_time(e1))
            ws.check()
            return ms

        ms_batch = timed(batch_step, args.steps)
        count = sm.run_text_batch_device(b, text, starts, n, out, offs)
        path = ws.last_path()
        ms_single = timed(single_step, args.steps)
        single_count = b.run_text_device(text, n, out)
        # the per-record loop: synchronous single-text calls, wall clock
        n_loop = min(args.loop, args.records)
        t0 = time.perf_counter()
        loop_chars = 0
        for r in range(n_loop):
            a, e = int(starts_h[r]), int(starts_h[r + 1])
            b.run_text_device(text[a:e], e - a, one)
            loop_chars += e - a
        loop_s = time.perf_counter() - t0
        med_b, med_s = statistics.median(ms_batch), statistics.median(ms_single)
        row = {"row": name, "k": k, "w": w, "canonical": canonical, "records": args.records, "n_chars": n,
               "outputs": int(count), "single_text_outputs": int(single_count),
               "path": {sm.PATH_GENERIC: "generic", sm.PATH_FUSED: "fused"}.get(path, str(path)),
               "batch_ms": round(med_b, 3), "batch_ms_all": [round(x, 3) for x in ms_batch],
               "batch_gchar_per_s": round(n / (med_b * 1e-3) / 1e9, 2),
               "single_text_ms": round(med_s, 3), "single_text_gchar_per_s": round(n / (med_s * 1e-3) / 1e9, 2),
               "batch_over_single_text": round(med_s / med_b, 3),
               "loop_records": n_loop, "loop_us_per_record": round(loop_s / n_loop * 1e6, 2),
               "loop_gchar_per_s": round(loop_chars / loop_s / 1e9, 4),
               "batch_us_per_record": round(med_b * 1e3 / args.records, 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {"tool": "gpu_text_batch_bench", "device": torch.cuda.get_device_name(dev), "ramp_ms": ramp_ms,
              "warmup": args.warmup, "steps": args.steps, "seed": args.seed,
              "lengths": {"lognormal_median": MEDIAN, "sigma": SIGMA, "clip": [MIN_LEN, MAX_LEN]}, "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
