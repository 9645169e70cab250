"""Byte text (``&[u8]``) throughput on one MI355X: the text entry point (mm_run_text_device) on 1 Gchar resident in HBM.

bench.py's protocol: inputs generated on the device, a 200 ms untimed ramp of the step, warm-up steps, then the median of
timed steps, each bracketed by HIP events on the workspace stream (mm_workspace_enable_timing).  Rows: forward and
canonical k=21 w=11, k=31 w=5, k=19 w=19, closed syncmers k=21 w=11; each on random ASCII DNA (NtHasher's tables over
ASCII, mm_text_hasher_from_dna) and on uniform random bytes (the default text MulHasher).  Every row reports Gchar/s, the
per-launch time, the kernel family that ran (and the generic text family's figure for contrast), and the HBM fraction of the algorithmic bytes (1 B per character read +
4 B per output written) against the 8 TB/s peak.  Next to the matching rows: the reference's published single-core
figure (bench/results.json of rust-seq/simd-minimizers, median over its repeats, ns per character, n = 10^8).

  python tools/gpu_text_bench.py [--n 1073741824] [--steps 5] [--warmup 3] [--out FILE] [--only ascii-dna:0]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0

# reference, single core (bench/results.json, experiment "external", n = 10^8): ns per character
REFERENCE_NS_PER_CHAR = {
    ("ascii-dna", False, 21, 11): 1.836, ("ascii-dna", True, 21, 11): 2.421,
    ("ascii-dna", False, 31, 5): 1.924, ("ascii-dna", False, 19, 19): 1.907,
    ("bytes", False, 21, 11): 2.062, ("bytes", True, 21, 11): 2.633,
    ("bytes", False, 31, 5): 2.111, ("bytes", False, 19, 19): 2.014,
}
REFERENCE_ROW_NAME = {"ascii-dna": "ascii-dna simd-minimizers", "bytes": "ascii mul simd-minimizers"}

ROWS = [  # (name, k, w, canonical, mode)
    ("minimizers", 21, 11, False, 0),
    ("canonical minimizers", 21, 11, True, 0),
    ("minimizers", 31, 5, False, 0),
    ("minimizers", 19, 19, False, 0),
    ("closed syncmers", 21, 11, False, 1),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one row, TEXT:INDEX (e.g. ascii-dna:0 = forward k=21 w=11 on ASCII DNA)")
    args = ap.parse_args()

    import torch

    import simd_minimizers_amd as sm

    dev = torch.device("cuda:0")
    ws = sm.default_workspace(0)
    n = args.n
    g = torch.Generator(device=dev).manual_seed(1)
    inputs = {
        "ascii-dna": torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[
            torch.randint(0, 4, (n,), dtype=torch.uint8, device=dev, generator=g).long()],
        "bytes": torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev, generator=g),
    }
    out = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ramp_ms = float(os.environ.get("MM_BENCH_RAMP_MS", "200"))
    rows = []
    for text_kind, text in inputs.items():
        for i, (name, k, w, canonical, mode) in enumerate(ROWS):
            if args.only and args.only != f"{text_kind}:{i}":
                continue
            ctor = {(0, False): sm.minimizers, (0, True): sm.canonical_minimizers,
                    (1, False): sm.closed_syncmers, (1, True): sm.canonical_closed_syncmers}[(mode, canonical)]
            th = (sm.TextHasher.from_dna(sm.NtHasher(canonical=canonical)) if text_kind == "ascii-dna"
                  else sm.TextMulHasher(canonical=canonical))
            b = ctor(k, w).hasher(th).workspace(ws)

            def step():
                b.run_text_device(text, n, out, sync=False)

            t0 = time.perf_counter()
            while (time.perf_counter() - t0) * 1e3 < ramp_ms:
                step()
                torch.cuda.synchronize(dev)
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize(dev)
            ws.check()
            count = b.run_text_device(text, n, out)
            path = ws.last_path()

            def timed(steps):
                ms = []
                ws.enable_timing(True)
                ws.kernel_time(True)
                for _ in range(steps):
                    step()
                    torch.cuda.synchronize(dev)
                    t, launches = ws.kernel_time(True)
                    ms.append(t / max(1, launches))
                ws.enable_timing(False)
                ws.check()
                return ms

            ms = timed(args.steps)
            med = statistics.median(ms)
            # the generic text family on the same row, for contrast (mm_workspace_force_generic)
            ws.force_generic(True)
            try:
                step()
                torch.cuda.synchronize(dev)
                gen = statistics.median(timed(3))
            finally:
                ws.force_generic(False)
            alg_bytes = n + 4 * count
            row = {"text": text_kind, "row": name, "k": k, "w": w, "canonical": canonical, "n": n,
                   "outputs": int(count), "path": {sm.PATH_GENERIC: "generic", sm.PATH_FUSED: "fused"}.get(path, str(path)),
                   "ms_per_launch": round(med, 3), "ms_all": [round(x, 3) for x in ms],
                   "gchar_per_s": round(n / (med * 1e-3) / 1e9, 2),
                   "hbm_frac": round(alg_bytes / (med * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                   "generic_ms_per_launch": round(gen, 3), "generic_gchar_per_s": round(n / (gen * 1e-3) / 1e9, 2),
                   "fused_over_generic": round(gen / med, 1)}
            ref = REFERENCE_NS_PER_CHAR.get((text_kind, canonical, k, w)) if mode == 0 else None
            if ref is not None:
                row["reference_single_core"] = {
                    "row": REFERENCE_ROW_NAME[text_kind].replace("simd", "canonical simd") if canonical
                    else REFERENCE_ROW_NAME[text_kind], "ns_per_char": ref,
                    "gchar_per_s": round(1.0 / ref, 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    result = {"tool": "gpu_text_bench", "device": torch.cuda.get_device_name(dev), "ramp_ms": ramp_ms,
              "warmup": args.warmup, "steps": args.steps, "hbm_peak_gbps": HBM_PEAK_GBPS, "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
