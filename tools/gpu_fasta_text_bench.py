"""Protein FASTA -> records of byte text on one MI355X: the loader against the packer, and file -> minimizers against a
host parser.

One process, one text: about 1 GiB of protein-like FASTA generated on the device - 20 letters, 60-character lines,
records of 300..400 characters behind a 22-byte header line.  Rows:

  a  mm_fasta_text_device_async   the new call: text read twice, the sequence bytes written once (about 3 n bytes)
  b  mm_fasta_pack_device_async   the 2-bit packer on the same text: the same two read passes, a quarter of the output
                                  (about 2.25 n bytes) - the yardstick, its kernels are the parent commit's
  c  file in HBM -> mm_fasta_text_device -> mm_run_text_batch_device (forward k=7 w=11) -> positions on the device
  d  what a caller did before: the same bytes parsed on the host with numpy, then run_text_batch_host

Protocol (bench.py's): a 200 ms untimed ramp of the step, warm-up steps, then the median of the timed steps, each
bracketed by HIP events on the workspace's stream (a and b are several launches: one event pair around the call; c is two
synchronous calls: events around both, which is wall-clock).  Row d runs on the host and is timed with perf_counter.
Rates are text bytes per second.  `a_over_b` and `c_over_d` are ratios of RATES (a's text GB/s over b's; by traffic about
0.75 is expected for a/b).  Nothing is gated on.

  python tools/gpu_fasta_text_bench.py [--n 1073741824] [--steps 7] [--warmup 3] [--host-steps 7] [--out profiles/fasta_text_bench.json]
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
WIDTH, HDR, K, W = 60, 22, 7, 11
LETTERS = b"ACDEFGHIKLMNPQRSTVWY"


def make_text(torch, dev, n):
    """About n bytes of FASTA, whole records only, built slab by slab: record r holds 300 + (r * 7919) % 101 characters."""
    n_rec = n // 415 + 2
    r = torch.arange(n_rec, device=dev, dtype=torch.int64)
    lens = 300 + (r * 7919) % 101
    size = HDR + lens + (lens + WIDTH - 1) // WIDTH          # header line, characters, one '\n' per line
    begin = torch.cumsum(size, 0) - size
    n_rec = int((begin + size <= n).sum().item())
    total = int((begin[n_rec - 1] + size[n_rec - 1]).item())
    begin, size = begin[:n_rec].contiguous(), size[:n_rec]
    g = torch.Generator(device=dev).manual_seed(5)
    letters = torch.tensor(list(LETTERS), dtype=torch.uint8, device=dev)
    t = torch.empty(total, dtype=torch.uint8, device=dev)
    slab = 1 << 25
    for s0 in range(0, total, slab):
        m = min(slab, total - s0)
        i = torch.arange(s0, s0 + m, device=dev, dtype=torch.int64)
        rec = torch.searchsorted(begin, i, right=True) - 1
        off = i - begin[rec]
        q = off - HDR
        x = letters[torch.randint(0, len(LETTERS), (m,), device=dev, generator=g)]
        x[(q >= 0) & ((q % (WIDTH + 1) == WIDTH) | (off == size[rec] - 1))] = 10
        x[(off > 0) & (off < HDR - 1)] = ord("h")
        x[off == HDR - 1] = 10
        x[off == 0] = ord(">")
        t[s0: s0 + m] = x
        del i, rec, off, q, x
    return t, n_rec


def host_parse(np, a):
    """FASTA records of a host byte array with numpy: (sequence bytes back to back, starts).  The reader's rules, line by
    line: header lines start with '>', '\\n' and '\\r' are dropped, bytes in front of the first header are ignored."""
    n = len(a)
    nl = np.flatnonzero(a == 10)
    ls = np.concatenate([np.zeros(1, dtype=np.int64), nl + 1])
    ls = ls[ls < n]
    le = np.concatenate([nl, np.full(1, n, dtype=np.int64)])[: len(ls)]
    hdr = a[ls] == 62
    first = int(np.argmax(hdr)) if hdr.any() else len(ls)
    keep = (a != 10) & (a != 13)
    delta = np.zeros(n + 1, dtype=np.int8)
    delta[ls[hdr]] += 1
    delta[le[hdr]] -= 1
    keep &= np.cumsum(delta[:n], dtype=np.int8) == 0
    if first < len(ls):
        keep[: ls[first]] = False
    else:
        keep[:] = False
    kept = np.add.reduceat(keep, ls, dtype=np.int64) if len(ls) else np.zeros(0, dtype=np.int64)
    before = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(kept)])
    starts = np.concatenate([before[:-1][hdr], before[-1:]]).astype(np.uint64)
    return a[keep], starts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import simd_minimizers_amd as sm

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ws = sm.Workspace(0, stream.cuda_stream)
    L = sm.lib()
    vp = C.c_void_p
    ramp_ms = float(os.environ.get("MM_BENCH_RAMP_MS", "200"))
    text, n_rec = make_text(torch, dev, args.n)
    n = int(text.numel())
    seq = torch.empty(n, dtype=torch.uint8, device=dev)
    packed = torch.empty((n // 4 + 8 + 3) // 4 * 4 + 64, dtype=torch.uint8, device=dev)
    starts = torch.zeros(n_rec + 1, dtype=torch.int64, device=dev)
    rec_pos = torch.zeros(n_rec, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    out_pos = torch.empty(n // 2, dtype=torch.int32, device=dev)
    offs = torch.zeros(n_rec + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    tp = vp(text.data_ptr())

    def measure(step):
        """ramp, warm-up, median of the timed steps (ms), each between two events on the workspace's stream"""
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

    def row(med, all_ms, alg_bytes=None, **more):
        r = {"ms": round(med, 4), "ms_all": all_ms, "text_GBps": round(n / (med * 1e-3) / 1e9, 2)}
        if alg_bytes is not None:
            r["hbm_frac"] = round(alg_bytes / (med * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)
        r.update(more)
        return r

    def text_call():
        sm._check(L.mm_fasta_text_device_async(ws.h, tp, n, vp(seq.data_ptr()), n, vp(starts.data_ptr()), vp(rec_pos.data_ptr()),
                                               n_rec, vp(counts.data_ptr())))

    def pack_call():
        sm._check(L.mm_fasta_pack_device_async(ws.h, tp, n, vp(packed.data_ptr()), packed.numel() // 4 * 4, vp(starts.data_ptr()),
                                               vp(rec_pos.data_ptr()), n_rec, vp(counts.data_ptr())))

    result = {"tool": "gpu_fasta_text_bench", "device": torch.cuda.get_device_name(dev), "text_bytes": n, "records": n_rec,
              "line_width": WIDTH, "k": K, "w": W, "ramp_ms": ramp_ms, "warmup": args.warmup, "steps": args.steps,
              "host_steps": args.host_steps, "hbm_peak_gbps": HBM_PEAK_GBPS, "rows": {}}
    rows = result["rows"]

    med, all_ms = measure(pack_call)
    stream.synchronize()
    bases = int(counts[0].item())
    rows["b"] = row(med, all_ms, 2 * n + bases / 4, what="mm_fasta_pack_device_async")
    print(json.dumps({"b": rows["b"]}), flush=True)

    med, all_ms = measure(text_call)
    stream.synchronize()
    chars, recs = (int(x) for x in counts.cpu().numpy())
    assert chars == bases and recs == n_rec, (chars, bases, recs, n_rec)
    rows["a"] = row(med, all_ms, 2 * n + chars, what="mm_fasta_text_device_async")
    result["characters"] = chars
    result["a_over_b"] = round(rows["a"]["text_GBps"] / rows["b"]["text_GBps"], 3)
    print(json.dumps({"a": rows["a"], "a_over_b": result["a_over_b"]}), flush=True)

    b = sm.minimizers(K, W).hasher(sm.TextMulHasher(canonical=False)).workspace(ws)
    plan = b.text_plan()
    host_counts = (C.c_uint64 * 2)()
    cnt = C.c_uint64()

    def end_to_end():
        sm._check(L.mm_fasta_text_device(ws.h, tp, n, vp(seq.data_ptr()), n, vp(starts.data_ptr()), vp(rec_pos.data_ptr()), n_rec,
                                         vp(counts.data_ptr()), host_counts))
        sm._check(L.mm_run_text_batch_device(plan.h, ws.h, vp(seq.data_ptr()), int(host_counts[0]), int(host_counts[1]),
                                             vp(starts.data_ptr()), int(host_counts[0]), vp(out_pos.data_ptr()), None,
                                             out_pos.numel(), vp(offs.data_ptr()), C.byref(cnt)))

    with torch.cuda.stream(stream):
        med, all_ms = measure(end_to_end)
    positions = int(cnt.value)
    rows["c"] = row(med, all_ms, what="mm_fasta_text_device + mm_run_text_batch_device (synchronous calls: wall-clock)",
                    positions=positions, path_fused=ws.last_path() == sm.PATH_FUSED)
    print(json.dumps({"c": rows["c"]}), flush=True)

    host_text = text.cpu().numpy()
    torch.cuda.synchronize(dev)

    def host_route():
        hs, hstarts = host_parse(np, host_text)
        n_r = len(hstarts) - 1
        pos = np.empty(max(1, len(hs)), dtype=np.uint32)
        ho = np.zeros(n_r + 1, dtype=np.uint64)
        c = C.c_uint64()
        sm._check(L.mm_run_text_batch_host(plan.h, ws.h, hs.ctypes.data_as(C.POINTER(C.c_uint8)), n_r,
                                           hstarts.ctypes.data_as(C.POINTER(C.c_uint64)), pos.ctypes.data_as(C.POINTER(C.c_uint32)),
                                           None, len(pos), ho.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(c)))
        return len(hs), n_r, int(c.value)

    got = host_route()  # (warm-up, and the same answer as the device route)
    assert got == (chars, n_rec, positions), (got, chars, n_rec, positions)
    ms = []
    for _ in range(args.host_steps):
        t0 = time.perf_counter()
        host_route()
        ms.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(ms)
    rows["d"] = row(med, [round(x, 1) for x in ms], what="numpy parser on the host + mm_run_text_batch_host (perf_counter)")
    result["c_over_d"] = round(rows["c"]["text_GBps"] / rows["d"]["text_GBps"], 1)
    print(json.dumps({"d": rows["d"], "c_over_d": result["c_over_d"]}), flush=True)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
