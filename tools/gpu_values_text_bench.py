"""K-mer values of byte text on one MI355X: values per second of mm_values_u64_text_device_async and
mm_values_u64_text_batch_device_async, against what a caller had before them.

ASCII DNA, one text of --chars characters (default 2^30), positions from the text run at k=21 w=11 (canonical,
mm_text_hasher_from_dna), u64, canonical:

  (a) text    mm_values_u64_text_device_async, MM_TEXT_VALUES_DNA: the values straight from the characters
  (b) pack    what a caller did before: mm_pack_ascii_device_async over the whole text, then mm_values_u64_device_async on
              the packed copy; both parts timed, their sum reported
  (c) packed  mm_values_u64_device_async alone on an already packed copy: the yardstick for the gather's extra loads
              (9 dwords per value against 3)

Protein-like records (tools/gpu_text_batch_bench.py's: --records of them, default 10^6, log-normal lengths, 20 letters),
positions from the text batch run at k=7 w=11 (forward), MM_TEXT_VALUES_BYTES, len 7, u64:

  (d) batch   mm_values_u64_text_batch_device_async: every record in one launch
  (e) single  mm_values_u64_text_device_async on the same number of positions of the whole text as ONE text: the kernel
              without the record lookup
  (f) loop    mm_values_u64_text_device_async once per record over --loop records (default 2000), scaled to all records
              (host-bound: wall clock)

bench.py's protocol: a 200 ms untimed ramp of the step, warm-up steps, then the median of timed steps, bracketed by HIP
events on the workspace stream.  Nothing is gated: the ratios are reported.

  python tools/gpu_values_text_bench.py [--steps 7] [--warmup 3] [--chars N] [--records N] [--loop N] [--out FILE]
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

MEDIAN, SIGMA, MIN_LEN, MAX_LEN = 300.0, 0.555, 30, 35_000  # (tools/gpu_text_batch_bench.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chars", type=int, default=1 << 30)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--loop", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=1)
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
    g = torch.Generator(device=dev).manual_seed(args.seed)

    def vp(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def timed_events(step):
        """median milliseconds of `step` (asynchronous on the workspace stream), by HIP events"""
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

    def dna_row():
        n, k, w = args.chars, 21, 11
        letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
        text = torch.empty(n, dtype=torch.uint8, device=dev)
        piece = 1 << 26  # (generated in pieces: the index tensor of torch.randint is 8 bytes per character)
        for at in range(0, n, piece):
            m = min(piece, n - at)
            text[at:at + m] = letters[torch.randint(0, 4, (m,), generator=g, device=dev)]
        b = sm.canonical_minimizers(k, w).hasher(sm.TextHasher.from_dna(sm.NtHasher(canonical=True))).workspace(ws)
        d_pos = torch.empty(int(n * 2.3 / (w + 1)) + 4096, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        count = int(b.run_text_device(text, n, d_pos))
        vals = torch.empty(count + 16, dtype=torch.int64, device=dev)
        packed = torch.zeros((n + 3) // 4 + 64, dtype=torch.uint8, device=dev)
        check = torch.empty(count + 16, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)

        def text_step():
            sm._check(L.mm_values_u64_text_device_async(ws.h, vp(text), n, n, sm.TEXT_VALUES_DNA, k, 1, vp(d_pos), count, vp(vals)))

        def pack_step():
            sm._check(L.mm_pack_ascii_device_async(ws.h, vp(text), n, vp(packed)))

        def packed_step():
            sm._check(L.mm_values_u64_device_async(ws.h, vp(packed), packed.numel(), 0, n, k, 1, vp(d_pos), count, vp(check)))

        a_ms, a_all = timed_events(text_step)
        p_ms, p_all = timed_events(pack_step)
        c_ms, c_all = timed_events(packed_step)
        ws.sync()
        if not torch.equal(vals[:count], check[:count]):
            raise SystemExit("values of the text differ from the values of its packed copy")
        rate = lambda ms: count / ms / 1e6
        row = {"row": "ASCII DNA, one text", "chars": n, "k": k, "w": w, "canonical": True, "values": count,
               "a_text_ms": a_ms, "a_text_ms_all": a_all, "a_text_Gvalues_per_s": rate(a_ms),
               "b_pack_ms": p_ms, "b_pack_ms_all": p_all, "b_pack_then_values_ms": p_ms + c_ms,
               "b_pack_then_values_Gvalues_per_s": rate(p_ms + c_ms),
               "c_packed_ms": c_ms, "c_packed_ms_all": c_all, "c_packed_Gvalues_per_s": rate(c_ms),
               "a_over_b": (p_ms + c_ms) / a_ms, "a_over_c": c_ms / a_ms}
        print(json.dumps(row), flush=True)
        return row

    def protein_row():
        n_rec, k, w = args.records, 7, 11
        z = torch.randn(n_rec, generator=g, device=dev, dtype=torch.float64)
        lens = torch.exp(math.log(MEDIAN) + SIGMA * z).round().clamp_(MIN_LEN, MAX_LEN).to(torch.int64)
        starts = torch.zeros(n_rec + 1, dtype=torch.int64, device=dev)
        starts[1:] = torch.cumsum(lens, 0)
        n = int(starts[-1].item())
        aa = torch.tensor(list(b"ACDEFGHIKLMNPQRSTVWY"), dtype=torch.uint8, device=dev)
        text = aa[torch.randint(0, 20, (n,), generator=g, device=dev)]
        b = sm.minimizers(k, w).workspace(ws)
        d_pos = torch.empty(n, dtype=torch.int32, device=dev)
        offs = torch.empty(n_rec + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        count = sm.run_text_batch_device(b, text, starts, n, d_pos, offs)
        vals = torch.empty(count + 16, dtype=torch.int64, device=dev)
        one_pos = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        c = min(int(b.run_text_device(text, n, one_pos)), count)
        enc = sm.TEXT_VALUES_BYTES

        def batch_step():
            sm._check(L.mm_values_u64_text_batch_device_async(ws.h, vp(text), n, n_rec, vp(starts), n, enc, k, 0, vp(d_pos),
                                                              vp(offs), count, vp(vals)))

        def single_step():
            sm._check(L.mm_values_u64_text_device_async(ws.h, vp(text), n, n, enc, k, 0, vp(one_pos), c, vp(vals)))

        d_ms, d_all = timed_events(batch_step)
        e_ms, e_all = timed_events(single_step)
        n_loop = min(args.loop, n_rec)
        starts_h, offs_h = starts[:n_loop + 1].cpu().tolist(), offs[:n_loop + 1].cpu().tolist()
        p_text, p_pos, p_val = text.data_ptr(), d_pos.data_ptr(), vals.data_ptr()
        calls = [(C.c_void_p(p_text + starts_h[r]), starts_h[r + 1] - starts_h[r], C.c_void_p(p_pos + 4 * offs_h[r]),
                  offs_h[r + 1] - offs_h[r], C.c_void_p(p_val + 8 * offs_h[r])) for r in range(n_loop)]

        def loop_step():
            for pt, m, pp, cnt, pv in calls:
                if cnt:
                    sm._check(L.mm_values_u64_text_device_async(ws.h, pt, m, m, enc, k, 0, pp, cnt, pv))
        f_ms, f_all = timed_wall(loop_step)
        f_scaled = f_ms * n_rec / n_loop
        row = {"row": "protein-like records", "records": n_rec, "chars": n, "k": k, "w": w, "len": k, "values": count,
               "d_batch_ms": d_ms, "d_batch_ms_all": d_all, "d_batch_Gvalues_per_s": count / d_ms / 1e6,
               "e_single_values": c, "e_single_ms": e_ms, "e_single_ms_all": e_all, "e_single_Gvalues_per_s": c / e_ms / 1e6,
               "f_loop_records": n_loop, "f_loop_ms": f_ms, "f_loop_ms_all": f_all, "f_loop_us_per_record": f_ms * 1e3 / n_loop,
               "f_loop_scaled_ms": f_scaled, "f_loop_Gvalues_per_s": count / f_scaled / 1e6,
               "d_over_e": (count / d_ms) / (c / e_ms), "d_over_f": f_scaled / d_ms}
        print(json.dumps(row), flush=True)
        return row

    rows = [dna_row()]
    torch.cuda.empty_cache()
    rows.append(protein_row())
    result = {"tool": "gpu_values_text_bench", "steps": args.steps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
              "lds_stage": sm.values_text_lds_stage(), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    ws.close()


if __name__ == "__main__":
    main()
