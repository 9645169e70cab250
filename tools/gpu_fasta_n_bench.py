"""FASTA with N on one MI355X: what the ambiguity bits cost the packer, and what skipping costs the run.

One process, one FASTA text per N share - 1 GiB of 60-base lines, built on the device the way
tests/test_gpu_fasta.py::test_fasta_large_against_ascii_pack builds its text (random ACGT, a '\\n' after every 60 bases,
24 records at even distances) - at 0 %, 0.1 % (single bases) and 5 % N (runs of 500).  Per text:

  pack        mm_fasta_pack_device_async      (the plain packer: its code object is the parent commit's)
  pack_n      mm_fasta_pack_n_device_async    (the same plus one ambiguity bit per base: 1.5 x the output bytes)
  run         mm_run_packed_reads_device                 canonical minimizers k=21 w=11 over the packed records
  run_skip    mm_run_packed_reads_skip_ambiguous_device  the same with Builder::run_skip_ambiguous_windows per record

bench.py's protocol: a 200 ms untimed ramp of the step, warm-up steps, then the median of timed steps, each bracketed by
HIP events on the workspace stream (the packers are several launches: one event pair around the call).  Rates are text
bytes per second for the packers (and their algorithmic bytes - text read twice, codes and bits written - against the
8 TB/s HBM peak) and bases per second for the runs.  `pack_n_over_pack` is reported, not gated on; the plain packer's
rate is what a run of this tool on the parent commit (rows pack / run only: --plain-only) is compared with.

  python tools/gpu_fasta_n_bench.py [--n 1073741824] [--steps 5] [--warmup 3] [--out profiles/fasta_n_bench.json] [--plain-only]
                                    [--parent parent_plain_only.json]
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

HBM_PEAK_GBPS = 8000.0
WIDTH, N_REC, K, W = 60, 24, 21, 11
SHARES = [("0", 0.0, 1), ("0.1", 0.001, 1), ("5", 0.05, 500)]  # (label in %, share of the bases, run length)


def make_text(torch, dev, n, share, run):
    g = torch.Generator(device=dev).manual_seed(5)
    t = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (n,), device=dev, generator=g)]
    if share > 0:
        # runs of `run` text bytes starting at random multiples of `run` (line ends inside a run are restored below)
        slots = (n + run - 1) // run
        hit = torch.rand(slots, device=dev, generator=g) < share
        t[hit.repeat_interleave(run)[:n]] = ord("N")
        del hit
    i = torch.arange(n, device=dev)
    t[i % (WIDTH + 1) == WIDTH] = 10
    del i
    for r in range(N_REC):
        p = (n // N_REC) * r + (r * 7919) % 50
        hdr = b">record %d\n" % r
        if p:
            t[p - 1] = 10
        t[p: p + len(hdr)] = torch.tensor(list(hdr), dtype=torch.uint8, device=dev)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="JSON of a --plain-only run of the parent commit on the same box: the plain packer is compared with it")
    ap.add_argument("--plain-only", action="store_true", help="the rows a library without the N entry points has (the parent commit)")
    args = ap.parse_args()

    import numpy as np
    import torch

    import simd_minimizers_amd as sm

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ws = sm.Workspace(0, stream.cuda_stream)
    L = sm.lib()
    n = args.n
    ramp_ms = float(os.environ.get("MM_BENCH_RAMP_MS", "200"))
    packed = torch.empty((n // 4 + 8 + 3) // 4 * 4 + 64, dtype=torch.uint8, device=dev)
    amb = torch.empty((n // 8 + 8 + 3) // 4 * 4 + 64, dtype=torch.uint8, device=dev)
    rec_base = torch.zeros(N_REC + 1, dtype=torch.int64, device=dev)
    rec_pos = torch.zeros(N_REC, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    out = torch.empty(n // 4, dtype=torch.int32, device=dev)
    offs = torch.zeros(N_REC + 1, dtype=torch.int64, device=dev)
    vp = C.c_void_p

    def measure(step):
        """ramp, warm-up, median of the timed steps (ms), each between two events on the workspace stream"""
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < ramp_ms:
            step()
            stream.synchronize()
        for _ in range(args.warmup):
            step()
        stream.synchronize()
        ws.check()
        ms = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            step()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ws.check()
        return statistics.median(ms), [round(x, 4) for x in ms]

    rows = []
    for label, share, run in SHARES:
        text = make_text(torch, dev, n, share, run)
        torch.cuda.synchronize(dev)
        tp = vp(text.data_ptr())

        def pack():
            sm._check(L.mm_fasta_pack_device_async(ws.h, tp, n, vp(packed.data_ptr()), packed.numel() // 4 * 4,
                                                   vp(rec_base.data_ptr()), vp(rec_pos.data_ptr()), N_REC, vp(counts.data_ptr())))

        def pack_n():
            sm._check(L.mm_fasta_pack_n_device_async(ws.h, tp, n, vp(packed.data_ptr()), packed.numel() // 4 * 4,
                                                     vp(amb.data_ptr()), amb.numel() // 4 * 4, vp(rec_base.data_ptr()),
                                                     vp(rec_pos.data_ptr()), N_REC, vp(counts.data_ptr())))

        row = {"n_percent": label, "n_run": run, "text_bytes": n}
        med, all_ms = measure(pack)
        stream.synchronize()
        bases, recs = (int(x) for x in counts.cpu().numpy())
        row.update(bases=bases, records=recs)

        def pack_row(med, all_ms, out_bytes):
            alg = 2 * n + out_bytes  # (two passes read the text, the second writes the output)
            return {"ms": round(med, 4), "ms_all": all_ms, "text_GBps": round(n / (med * 1e-3) / 1e9, 1),
                    "hbm_frac": round(alg / (med * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)}

        row["pack"] = pack_row(med, all_ms, bases / 4)
        if not args.plain_only:
            med_n, all_n = measure(pack_n)
            stream.synchronize()
            row["pack_n"] = pack_row(med_n, all_n, bases / 4 + bases / 8)
            row["pack_n_over_pack"] = round(med_n / med, 3)
            row["ambiguous_bases"] = int(torch.count_nonzero(text == ord("N")).item())
        else:
            pack()
            stream.synchronize()
        del text
        records = sm.FastaRecords(packed, rec_base.cpu().numpy().astype(np.uint64), rec_pos.cpu().numpy().astype(np.uint64))
        if not args.plain_only:
            records.amb = amb
        b = sm.canonical_minimizers(K, W).workspace(ws)
        with torch.cuda.stream(stream):
            cnt = {}

            def run_plain():
                cnt["run"] = sm.run_packed_reads_device(b, records, out, offs)

            def run_skip():
                cnt["run_skip"] = sm.run_packed_reads_skip_ambiguous_device(b, records, out, offs)

            for name, step in (("run", run_plain),) + ((("run_skip", run_skip),) if not args.plain_only else ()):
                med, all_ms = measure(step)
                row[name] = {"ms": round(med, 4), "ms_all": all_ms, "Gbases_per_s": round(bases / (med * 1e-3) / 1e9, 1),
                             "positions": cnt[name], "lane_table": bool(ws.last_lane_table())}
            if not args.plain_only:
                row["run_skip_over_run"] = round(row["run_skip"]["ms"] / row["run"]["ms"], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {"tool": "gpu_fasta_n_bench", "device": torch.cuda.get_device_name(dev), "k": K, "w": W, "line_width": WIDTH,
              "ramp_ms": ramp_ms, "warmup": args.warmup, "steps": args.steps, "hbm_peak_gbps": HBM_PEAK_GBPS,
              "note": "run / run_skip are synchronous calls timed with events around the call: wall-clock per call (upload of the "
                      "read starts, launches, copy-back of the count), not kernel time",
              "rows": rows}
    if args.parent:
        # the plain packer's code object is meant to be the parent's: its rate has to agree within the box-to-box spread
        with open(args.parent) as f:
            parent = {r["n_percent"]: r for r in json.load(f)["rows"]}
        ratios = {r["n_percent"]: round(r["pack"]["ms"] / parent[r["n_percent"]]["pack"]["ms"], 4) for r in rows}
        result["plain_pack_vs_parent"] = {"parent_ms": {k: v["pack"]["ms"] for k, v in parent.items()}, "ms_over_parent_ms": ratios,
                                          "agrees_within_3_percent": all(abs(x - 1) <= 0.03 for x in ratios.values())}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
