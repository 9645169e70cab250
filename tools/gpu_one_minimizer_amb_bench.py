"""One minimizer per read that skips ambiguous bases on one MI355X: mm_one_minimizer_reads_skip_ambiguous_device_async
against the plain call on the same bytes in the same session.

Forward NtHasher, k = 21, inputs resident in HBM, both read workloads taken from simd_minimizers_amd/workloads.py, with
about 0.5 % of the bases marked ambiguous (independent bits, one byte of bits per 8 bases, bit 0 = base 0):

  READS       8 M reads x 150 bp, fixed stride
  LONGREADS   200 000 reads, lengths log-uniform 1-50 kbp, packed back to back

Per workload:
  (a) the skip-ambiguous call
  (b) the plain call, mm_one_minimizer_reads_device_async, on the same packed bytes
a_over_b = b's time / a's time, a ratio of RATES: below 1 means the skip-ambiguous call is slower.  By traffic the new form
reads 3/8 byte per base against 1/4; the plain kernel is far from its traffic bound, so near 1 is expected.  Nothing is
gated.

tools/gpu_one_minimizer_bench.py's protocol: a 200 ms untimed ramp of the step, 3 warm-up steps, then the median of 7
timed steps, each bracketed by HIP events on the workspace's stream.

  python tools/gpu_one_minimizer_amb_bench.py [--steps 7] [--warmup 3] [--out profiles/one_minimizer_amb_bench.json]
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

K = 21
N_DENSITY = 0.005


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="READS or LONGREADS: one row (for a profiler run)")
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
    for name in ("READS", "LONGREADS"):
        if args.only and args.only != name:
            continue
        with torch.cuda.stream(stream):
            c = workloads.component(name, ws, dev)
        ws.sync()
        n = c["units"]
        if name == "READS":
            d = c["keep"][0]
            n_reads, stride, starts = 8_000_000, 150, None
        else:
            d, starts = c["keep"][0], c["keep"][4]
            n_reads, stride = c["reads"], 0
        # the bits: a byte holds a set bit with probability 8 * density, and then exactly one (close enough to independent
        # bits at this density, and made without a tensor of one byte per base)
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        n_bytes = (n + 7) // 8 + 8
        hit = torch.rand(n_bytes, device=dev, generator=g) < 8 * N_DENSITY
        which = torch.randint(0, 8, (n_bytes,), device=dev, generator=g, dtype=torch.int32)
        amb = (hit.to(torch.int32) << which).to(torch.uint8)
        set_bits = int(hit.sum().item())
        del hit, which
        pos_a = torch.empty(n_reads + 16, dtype=torch.int32, device=dev)
        pos_b = torch.empty(n_reads + 16, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)

        def amb_step():
            sm._check(L.mm_one_minimizer_reads_skip_ambiguous_device_async(ws.h, C.byref(nt), K, vp(d), d.numel(), 0, vp(amb),
                                                                           amb.numel(), 0, n_reads, vp(starts), stride, stride,
                                                                           vp(pos_a)))

        def plain_step():
            sm._check(L.mm_one_minimizer_reads_device_async(ws.h, C.byref(nt), K, vp(d), d.numel(), 0, n_reads, vp(starts),
                                                            stride, stride, vp(pos_b)))
        a_ms, a_all = timed(amb_step)
        b_ms, b_all = timed(plain_step)
        ws.sync()
        moved = int((pos_a[:n_reads] != pos_b[:n_reads]).sum().item())
        none = int((pos_a[:n_reads] == -1).sum().item())
        row = {"workload": name, "what": c["what"].split(",")[0], "reads": n_reads, "bases": n, "ambiguous_bases": set_bits,
               "a_skip_ambiguous_ms": a_ms, "a_ms_all": a_all, "a_Gbases_per_s": n / a_ms / 1e6,
               "b_plain_ms": b_ms, "b_ms_all": b_all, "b_Gbases_per_s": n / b_ms / 1e6, "a_over_b": b_ms / a_ms,
               "reads_whose_answer_differs": moved, "reads_without_a_clean_kmer": none}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del c, d, starts, amb, pos_a, pos_b
        torch.cuda.empty_cache()

    result = {"tool": "gpu_one_minimizer_amb_bench", "k": K, "hasher": "forward NtHasher", "n_density": N_DENSITY,
              "tile": sm.one_minimizer_tile(), "steps": args.steps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    ws.close()


if __name__ == "__main__":
    main()
