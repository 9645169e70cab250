"""FASTQ -> packed reads -> positions -> values on ONE stream (mm_run_packed_reads_counts_*) on one MI355X: what taking the
counts from the device costs the reads run, what always taking the lane table costs short reads, and what the removed host
waits are worth.

Rows
  a  the counts run against the existing call on the same reads, canonical minimizers k=21 w=11, device time between HIP
     events on the workspace's stream.  Shapes: LONGREADS (200 k reads, lengths log-uniform in 1 .. 50 kbp) and 8 M x 150 bp.
       existing        mm_run_packed_reads_device_async with MM_LANE_TABLE=1
       existing_again  the same call once more: the A/A spread of the process
       counts_tight    mm_run_packed_reads_counts_device_async with bounds = the counts
       counts_loose    the same with bounds as a real caller has them: max_bases = the bytes of the reads' FASTQ text
                       (2 x bases + 6 per read), max_records = 2 x the reads
     The variants run INTERLEAVED round by round in one process, so clock and cache state are shared.
  b  8 M x 150 bp only: the same against the existing call under its default policy (one lane per read) - what always
     taking the table costs short reads.
  c  FASTQ in HBM -> positions -> values (150 bp reads), whole-route wall-clock (perf_counter):
       today     mm_fasta_pack_device (waits, counts to the host), mm_run_packed_reads_device (waits),
                 mm_values_u64_reads_device_async, mm_workspace_check
       pipeline  mm_fastq_pack_device_async, mm_run_packed_reads_counts_device_async,
                 mm_values_u64_reads_device_async (n_reads = max_records), mm_workspace_check: one wait
     on one FASTQ of about 1 GiB, and on 1 000 files of about 1 MiB processed one after the other.

Protocol (the README's benches): a 200 ms untimed ramp of each step, warm-up steps, then the median of the timed steps.
"Not slower" = within the larger of 3 % (the box-to-box spread the README states) and the A/A spread measured here between
two repeats of the same call; the verdicts are recorded, nothing is gated on.

  python tools/gpu_reads_pipeline_bench.py [--n 1073741824] [--files 1000] [--file-bytes 1048576] [--steps 7] [--warmup 3]
         [--rows abc] [--out profiles/reads_pipeline_bench.json]
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

MARGIN = 0.03
K, W, READ = 21, 11, 150
REC = 2 * READ + 6  # bytes of a FASTQ record of READ bases with a one-byte name


def spread(a, b):
    return abs(a - b) / min(a, b)


def make_fastq(torch, dev, n_bytes, seed=3):
    """About n_bytes of FASTQ on the device: records "@\\n<150 bases>\\n+\\n<150 x I>\\n"; returns (text, records)."""
    n = max(1, n_bytes // REC)
    g = torch.Generator(device=dev).manual_seed(seed)
    t = torch.full((n, REC), ord("I"), dtype=torch.uint8, device=dev)
    t[:, 0] = ord("@")
    t[:, 1] = t[:, READ + 2] = t[:, READ + 4] = t[:, REC - 1] = ord("\n")
    t[:, READ + 3] = ord("+")
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    t[:, 2: READ + 2] = acgt[torch.randint(0, 4, (n, READ), generator=g, device=dev)]
    return t.reshape(-1), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 30)
    ap.add_argument("--files", type=int, default=1000)
    ap.add_argument("--file-bytes", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="abc")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    os.environ["MM_ENV_DYNAMIC"] = "1"  # (row a / b flip MM_LANE_TABLE between calls of one process)
    import torch

    import simd_minimizers_amd as sm

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ws = sm.Workspace(0, stream.cuda_stream)
    L = sm.lib()
    vp = C.c_void_p
    ramp_ms = float(os.environ.get("MM_BENCH_RAMP_MS", "200"))
    result = {"tool": "gpu_reads_pipeline_bench", "device": torch.cuda.get_device_name(dev),
              "date": datetime.date.today().isoformat(), "ramp_ms": ramp_ms, "warmup": args.warmup, "steps": args.steps,
              "margin": MARGIN, "rows": {}}
    b = sm.canonical_minimizers(K, W).workspace(ws)
    plan = b.plan()
    b.prepare(ws, sequence=False, reads=True)

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

    # ------------------------------------------------------------------ rows a, b
    if "a" in args.rows or "b" in args.rows:
        rows_a, rows_b = [], []
        for shape in ("LONGREADS", "8M x 150 bp"):
            g = torch.Generator(device=dev).manual_seed(6)
            if shape == "LONGREADS":
                u = torch.rand(200_000, device=dev, generator=g, dtype=torch.float64)
                lens = torch.exp(math.log(1000.0) + u * (math.log(50_000.0) - math.log(1000.0))).to(torch.int64)
            else:
                lens = torch.full((8_000_000,), READ, dtype=torch.int64, device=dev)
            n_reads = int(lens.numel())
            loose_reads = 2 * n_reads
            starts = torch.zeros(loose_reads + 1, dtype=torch.int64, device=dev)
            starts[1: n_reads + 1] = torch.cumsum(lens, 0)
            n = int(starts[n_reads].item())
            mx = int(lens.max().item())
            loose_bases = 2 * n + 6 * n_reads
            del lens
            d = sm.generate_device((loose_bases + 3) // 4 * 4 + 256, 7)  # (the bound's bytes exist)
            out = torch.empty(int(n * 0.19) + 4096, dtype=torch.int32, device=dev)
            offs = torch.zeros(loose_reads + 1, dtype=torch.int64, device=dev)
            counts = torch.tensor([n, n_reads], dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)
            dp, sp, op, fp, cp = (vp(t.data_ptr()) for t in (d, starts, out, offs, counts))

            def existing(policy):
                if policy is None:
                    os.environ.pop("MM_LANE_TABLE", None)
                else:
                    os.environ["MM_LANE_TABLE"] = policy
                r = L.mm_run_packed_reads_device_async(plan.h, ws.h, dp, d.numel(), 0, n_reads, sp, n, mx, op, None, out.numel(),
                                                       fp, None)
                os.environ.pop("MM_LANE_TABLE", None)
                assert r == 0, r

            def counts_call(max_bases, max_records):
                r = L.mm_run_packed_reads_counts_device_async(plan.h, ws.h, dp, d.numel(), 0, max_bases, max_records, sp, cp, op,
                                                              None, out.numel(), fp, None)
                assert r == 0, r

            variants = {"existing": lambda: existing("1"), "existing_again": lambda: existing("1"),
                        "counts_tight": lambda: counts_call(n, n_reads),
                        "counts_loose": lambda: counts_call(loose_bases, loose_reads)}
            if shape != "LONGREADS" and "b" in args.rows:
                variants["existing_default_policy"] = lambda: existing(None)
            for step in variants.values():
                ramp_and_warm(step, stream.synchronize)
            ws.check()
            ms = {name: [] for name in variants}
            for _ in range(args.steps):
                for name, step in variants.items():
                    ms[name].append(device_ms(step))
            ws.check()
            med = {name: statistics.median(v) for name, v in ms.items()}
            aa_spread = spread(med["existing"], med["existing_again"])
            tol = max(MARGIN, aa_spread)
            base = min(med["existing"], med["existing_again"])
            row = {"shape": shape, "k": K, "w": W, "reads": n_reads, "bases": n,
                   "ms": {k: round(v, 4) for k, v in med.items()}, "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                   "gbases_per_s": {k: round(n / (v * 1e-3) / 1e9, 1) for k, v in med.items()},
                   "aa_spread": round(aa_spread, 4), "tolerance": round(tol, 4),
                   "tight_over_existing": round(med["counts_tight"] / base, 4),
                   "loose_over_existing": round(med["counts_loose"] / base, 4),
                   "tight_not_slower_than_existing": med["counts_tight"] <= base * (1 + tol)}
            print(json.dumps({"a": row}), flush=True)
            rows_a.append(row)
            if "existing_default_policy" in med:
                rb = {"shape": shape, "ms_default_policy": round(med["existing_default_policy"], 4),
                      "ms_counts_tight": round(med["counts_tight"], 4),
                      "counts_over_default_policy": round(med["counts_tight"] / med["existing_default_policy"], 4)}
                print(json.dumps({"b": rb}), flush=True)
                rows_b.append(rb)
            del d, out, offs, starts
        result["rows"]["a"] = rows_a
        if rows_b:
            result["rows"]["b"] = rows_b

    # ------------------------------------------------------------------ row c
    if "c" in args.rows:
        host_counts = (C.c_uint64 * 2)()
        cnt = C.c_uint64()

        def wall_rows(label, files, max_rec, total_bytes):
            m = max(f.numel() for f in files)
            cap_bytes = (m // 4 + 8 + 3) // 4 * 4
            packed = torch.empty(cap_bytes + 64, dtype=torch.uint8, device=dev)
            starts = torch.zeros(max_rec + 1, dtype=torch.int64, device=dev)
            counts = torch.zeros(2, dtype=torch.int64, device=dev)
            pos = torch.empty(m // 8 + 4096, dtype=torch.int32, device=dev)
            offs = torch.zeros(max_rec + 1, dtype=torch.int64, device=dev)
            vals = torch.empty(pos.numel(), dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)
            pk, st, ct, po, of, va = (vp(t.data_ptr()) for t in (packed, starts, counts, pos, offs, vals))
            cap = pos.numel()

            def today():
                for f in files:
                    sm._check(L.mm_fasta_pack_device(ws.h, vp(f.data_ptr()), f.numel(), pk, cap_bytes, st, None, max_rec, ct,
                                                     host_counts))
                    nb, nr = int(host_counts[0]), int(host_counts[1])
                    sm._check(L.mm_run_packed_reads_device(plan.h, ws.h, pk, cap_bytes, 0, nr, st, nb, READ, po, None, cap, of,
                                                           C.byref(cnt)))
                    sm._check(L.mm_values_u64_reads_device_async(ws.h, pk, cap_bytes, 0, nr, st, 0, K, 1, po, of, int(cnt.value),
                                                                 va))
                    ws.check()

            def pipeline():
                for f in files:
                    m_f = f.numel()
                    sm._check(L.mm_fastq_pack_device_async(ws.h, vp(f.data_ptr()), m_f, pk, cap_bytes, st, None, max_rec, ct))
                    sm._check(L.mm_run_packed_reads_counts_device_async(plan.h, ws.h, pk, cap_bytes, 0, m_f, max_rec, st, ct, po,
                                                                        None, cap, of, None))
                    sm._check(L.mm_values_u64_reads_device_async(ws.h, pk, cap_bytes, 0, max_rec, st, 0, K, 1, po, of, cap, va))
                    ws.check()

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
            c, nr = int(cnt.value), int(host_counts[1])
            a = (pos[:c].clone(), offs[: nr + 1].clone(), vals[:c].clone())
            pos.fill_(0), offs.fill_(0), vals.fill_(0)
            torch.cuda.synchronize(dev)
            pipeline()
            same = all(torch.equal(x, y) for x, y in zip(a, (pos[:c], offs[: nr + 1], vals[:c])))
            med = {name: statistics.median(v) for name, v in ms.items()}
            aa_spread = spread(med["today"], med["today_again"])
            tol = max(MARGIN, aa_spread)
            base = min(med["today"], med["today_again"])
            row = {"input": label, "files": len(files), "text_bytes": total_bytes, "k": K, "w": W, "positions_last_file": c,
                   "same_result": bool(same), "ms": {k: round(v, 3) for k, v in med.items()},
                   "ms_all": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                   "text_GBps": {k: round(total_bytes / (v * 1e-3) / 1e9, 3) for k, v in med.items()},
                   "aa_spread": round(aa_spread, 4), "tolerance": round(tol, 4),
                   "today_over_pipeline": round(base / med["pipeline"], 3),
                   "pipeline_not_slower": med["pipeline"] <= base * (1 + tol)}
            print(json.dumps({"c": row}), flush=True)
            return row

        rows_c = []
        text, n_rec = make_fastq(torch, dev, args.n)
        rows_c.append(wall_rows("one FASTQ of 150 bp reads", [text], n_rec + n_rec // 4, int(text.numel())))
        del text
        small, small_rec = make_fastq(torch, dev, args.file_bytes)
        m = int(small.numel())
        many = small.repeat(args.files)
        files = [many[i * m: (i + 1) * m] for i in range(args.files)]
        rows_c.append(wall_rows(f"{args.files} files of {m} bytes, one after the other", files, small_rec + small_rec // 4,
                                m * args.files))
        result["rows"]["c"] = rows_c

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
