"""File -> records -> positions -> values on ONE stream (mm_run_text_batch_counts_*, mm_values_*_text_batch_counts_*) on one
MI355X: what taking the counts from the device costs the batch run, and what the removed host waits are worth.

Rows
  a  the counts run against the existing run, tools/gpu_text_batch_bench.py's input (about 1 M protein-like records, about
     350 Mchar, generated on the device), forward and canonical k=21 w=11, device time between HIP events on the
     workspace's stream:
       existing        mm_run_text_batch_device_async of this library
       existing_again  the same call once more: the A/A spread of the process
       parent          the same call of another build of the library (--parent-lib: the parent commit's), if given
       counts          mm_run_text_batch_counts_device_async with max_chars = n_chars
       counts_125      the same with max_chars = 1.25 n_chars (a quarter of the grid leaves at once)
     The variants run INTERLEAVED round by round in one process, so clock and cache state are shared.
  b  file in HBM -> positions -> values (forward k=7 w=11, MM_TEXT_VALUES_BYTES), whole-route wall-clock (perf_counter):
       today     mm_fasta_text_device (waits), mm_run_text_batch_device (waits), mm_values_u64_text_batch_device_async,
                 mm_workspace_check
       pipeline  mm_fasta_text_device_async, mm_run_text_batch_counts_device_async,
                 mm_values_u64_text_batch_counts_device_async, mm_workspace_check: one wait
     on tools/gpu_fasta_text_bench.py's 1 GiB protein FASTA, and on 1 000 files of about 1 MiB processed one after the
     other (copies of one file at 1 000 places of a buffer, outputs reused) - the case the calls exist for.

Protocol (the README's text benches): a 200 ms untimed ramp of each step, warm-up steps, then the median of the timed
steps.  "Not slower" = within the larger of 3 % (the box-to-box spread the README states) and the A/A spread measured here
between two repeats of the same call; the verdicts are recorded, nothing is gated on.

  python tools/gpu_text_pipeline_bench.py [--records 1000000] [--n 1073741824] [--files 1000] [--file-bytes 1048576]
         [--steps 7] [--warmup 3] [--parent-lib PATH] [--rows ab] [--out profiles/text_pipeline_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import datetime
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEDIAN, SIGMA, MIN_LEN, MAX_LEN = 300.0, 0.555, 30, 35_000  # (tools/gpu_text_batch_bench.py's lengths)
MARGIN = 0.03


def spread(a, b):
    return abs(a - b) / min(a, b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--n", type=int, default=1 << 30)
    ap.add_argument("--files", type=int, default=1000)
    ap.add_argument("--file-bytes", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="another build of the library (the parent commit's) for row a")
    ap.add_argument("--rows", default="ab")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import simd_minimizers_amd as sm
    from tools.gpu_fasta_text_bench import make_text

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ws = sm.Workspace(0, stream.cuda_stream)
    L = sm.lib()
    vp = C.c_void_p
    ramp_ms = float(os.environ.get("MM_BENCH_RAMP_MS", "200"))
    result = {"tool": "gpu_text_pipeline_bench", "device": torch.cuda.get_device_name(dev),
              "date": datetime.date.today().isoformat(), "ramp_ms": ramp_ms, "warmup": args.warmup, "steps": args.steps,
              "margin": MARGIN, "rows": {}}

    def ramp_and_warm(step, wait):
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < ramp_ms:
            step()
            wait()
        for _ in range(args.warmup):
            step()
        wait()

    def device_ms(step):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        step()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    # ------------------------------------------------------------------ row a
    if "a" in args.rows:
        g = torch.Generator(device=dev).manual_seed(1)
        z = torch.randn(args.records, generator=g, device=dev, dtype=torch.float64)
        lens = torch.exp(math.log(MEDIAN) + SIGMA * z).round().clamp_(MIN_LEN, MAX_LEN).to(torch.int64)
        starts = torch.zeros(args.records + 1, dtype=torch.int64, device=dev)
        starts[1:] = torch.cumsum(lens, 0)
        n = int(starts[-1].item())
        n125 = n + n // 4
        aa = torch.tensor(list(b"ACDEFGHIKLMNPQRSTVWY"), dtype=torch.uint8, device=dev)
        text = aa[torch.randint(0, 20, (n125,), generator=g, device=dev)]  # (the bound's bytes exist: max_chars <= text_bytes)
        out = torch.empty(n125, dtype=torch.int32, device=dev)
        offs = torch.empty(args.records + 1, dtype=torch.int64, device=dev)
        counts = torch.tensor([n, args.records], dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        parent = None
        if args.parent_lib:
            P = C.CDLL(os.path.abspath(args.parent_lib))
            P.mm_workspace_create.argtypes = [C.POINTER(vp), C.c_int, vp]
            P.mm_plan_create_text.argtypes = [C.POINTER(vp), C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(sm.TextHasher)]
            P.mm_text_mul_hasher.argtypes = [C.POINTER(sm.TextHasher), C.c_int]
            P.mm_run_text_batch_device_async.argtypes = L.mm_run_text_batch_device_async.argtypes
            P.mm_workspace_check.argtypes = [vp]
            pws = vp()
            assert P.mm_workspace_create(C.byref(pws), 0, vp(stream.cuda_stream)) == 0
            parent = (P, pws)
        rows_a = []
        for canonical in (False, True):
            b = (sm.canonical_minimizers if canonical else sm.minimizers)(21, 11).workspace(ws)
            plan = b.text_plan()
            tp, sp, op, fp, cp = (vp(t.data_ptr()) for t in (text, starts, out, offs, counts))

            def existing(lib=L, p=plan.h, w=ws.h):
                r = lib.mm_run_text_batch_device_async(p, w, tp, n125, args.records, sp, n, op, None, n125, fp, None)
                assert r == 0, r

            def counts_call(max_chars):
                r = L.mm_run_text_batch_counts_device_async(plan.h, ws.h, tp, n125, max_chars, args.records, sp, cp, op, None,
                                                            n125, fp, None)
                assert r == 0, r

            variants = {"existing": existing, "existing_again": existing, "counts": lambda: counts_call(n),
                        "counts_125": lambda: counts_call(n125)}
            if parent:
                P, pws = parent
                th = sm.TextHasher()
                assert P.mm_text_mul_hasher(C.byref(th), int(canonical)) == 0
                pplan = vp()
                assert P.mm_plan_create_text(C.byref(pplan), 21, 11, int(canonical), 0, C.byref(th)) == 0
                variants["parent"] = lambda: existing(P, pplan, pws)
            for step in variants.values():
                ramp_and_warm(step, stream.synchronize)
            ws.check()
            ms = {name: [] for name in variants}
            for _ in range(args.steps):
                for name, step in variants.items():
                    ms[name].append(device_ms(step))
            ws.check()
            if parent:
                assert parent[0].mm_workspace_check(parent[1]) == 0
            med = {name: statistics.median(v) for name, v in ms.items()}
            aa_spread = spread(med["existing"], med["existing_again"])
            tol = max(MARGIN, aa_spread)
            base = min(med["existing"], med["existing_again"])
            row = {"canonical": canonical, "k": 21, "w": 11, "records": args.records, "n_chars": n,
                   "ms": {k: round(v, 4) for k, v in med.items()}, "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                   "gchar_per_s": {k: round(n / (v * 1e-3) / 1e9, 2) for k, v in med.items()},
                   "aa_spread": round(aa_spread, 4), "tolerance": round(tol, 4),
                   "counts_not_slower_than_existing": med["counts"] <= base * (1 + tol),
                   "counts_125_not_slower_than_existing": med["counts_125"] <= base * (1 + tol)}
            if parent:
                row["existing_not_slower_than_parent"] = base <= med["parent"] * (1 + tol)
            rows_a.append(row)
            print(json.dumps({"a": row}), flush=True)
        result["rows"]["a"] = rows_a
        del text, out, offs, starts

    # ------------------------------------------------------------------ row b
    if "b" in args.rows:
        K, W = 7, 11
        b = sm.minimizers(K, W).hasher(sm.TextMulHasher(canonical=False)).workspace(ws)
        plan = b.text_plan()
        host_counts = (C.c_uint64 * 2)()
        cnt = C.c_uint64()

        def routes(files, max_rec, seq, starts, counts, pos, offs, vals):
            """(today, pipeline): each processes every file of `files` (device tensors) one after the other"""
            sq, st, ct, po, of, va = (vp(t.data_ptr()) for t in (seq, starts, counts, pos, offs, vals))
            cap = pos.numel()

            def today():
                for f in files:
                    m = f.numel()
                    sm._check(L.mm_fasta_text_device(ws.h, vp(f.data_ptr()), m, sq, m, st, None, max_rec, ct, host_counts))
                    nc, nr = int(host_counts[0]), int(host_counts[1])
                    sm._check(L.mm_run_text_batch_device(plan.h, ws.h, sq, nc, nr, st, nc, po, None, cap, of, C.byref(cnt)))
                    sm._check(L.mm_values_u64_text_batch_device_async(ws.h, sq, nc, nr, st, nc, sm.TEXT_VALUES_BYTES, K, 0, po, of,
                                                                      int(cnt.value), va))
                    ws.check()

            def pipeline():
                for f in files:
                    m = f.numel()
                    sm._check(L.mm_fasta_text_device_async(ws.h, vp(f.data_ptr()), m, sq, m, st, None, max_rec, ct))
                    sm._check(L.mm_run_text_batch_counts_device_async(plan.h, ws.h, sq, m, m, max_rec, st, ct, po, None, cap, of,
                                                                      None))
                    sm._check(L.mm_values_u64_text_batch_counts_device_async(ws.h, sq, m, m, max_rec, st, ct,
                                                                             sm.TEXT_VALUES_BYTES, K, 0, po, of, cap, va))
                    ws.check()

            return today, pipeline

        def wall_rows(label, files, max_rec, total_bytes):
            m = max(f.numel() for f in files)
            seq = torch.empty(m, dtype=torch.uint8, device=dev)
            starts = torch.zeros(max_rec + 1, dtype=torch.int64, device=dev)
            counts = torch.zeros(2, dtype=torch.int64, device=dev)
            pos = torch.empty(m // 2, dtype=torch.int32, device=dev)
            offs = torch.zeros(max_rec + 1, dtype=torch.int64, device=dev)
            vals = torch.empty(m // 2, dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)
            today, pipeline = routes(files, max_rec, seq, starts, counts, pos, offs, vals)
            variants = {"today": today, "today_again": today, "pipeline": pipeline}
            with torch.cuda.stream(stream):
                for step in variants.values():
                    ramp_and_warm(step, stream.synchronize)
                ms = {name: [] for name in variants}
                for _ in range(args.steps):
                    for name, step in variants.items():
                        t0 = time.perf_counter()
                        step()
                        ms[name].append((time.perf_counter() - t0) * 1e3)
            # the same answer on both routes (the last file's)
            today()
            a = (pos[: int(cnt.value)].clone(), offs[: int(host_counts[1]) + 1].clone(), vals[: int(cnt.value)].clone())
            pos.fill_(0), offs.fill_(0), vals.fill_(0)
            pipeline()
            same = all(torch.equal(x, y) for x, y in zip(a, (pos[: a[0].numel()], offs[: a[1].numel()], vals[: a[2].numel()])))
            med = {name: statistics.median(v) for name, v in ms.items()}
            aa_spread = spread(med["today"], med["today_again"])
            tol = max(MARGIN, aa_spread)
            base = min(med["today"], med["today_again"])
            row = {"input": label, "files": len(files), "text_bytes": total_bytes, "k": K, "w": W, "positions_last_file": a[0].numel(),
                   "same_result": bool(same), "ms": {k: round(v, 3) for k, v in med.items()},
                   "ms_all": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                   "text_GBps": {k: round(total_bytes / (v * 1e-3) / 1e9, 3) for k, v in med.items()},
                   "aa_spread": round(aa_spread, 4), "tolerance": round(tol, 4),
                   "today_over_pipeline": round(base / med["pipeline"], 3),
                   "pipeline_not_slower": med["pipeline"] <= base * (1 + tol)}
            print(json.dumps({"b": row}), flush=True)
            return row

        rows_b = []
        text, n_rec = make_text(torch, dev, args.n)
        rows_b.append(wall_rows("one protein FASTA", [text], n_rec, int(text.numel())))
        del text
        small, small_rec = make_text(torch, dev, args.file_bytes)
        m = int(small.numel())
        many = small.repeat(args.files)
        files = [many[i * m: (i + 1) * m] for i in range(args.files)]
        rows_b.append(wall_rows(f"{args.files} files of {m} bytes, one after the other", files, small_rec, m * args.files))
        result["rows"]["b"] = rows_b

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
