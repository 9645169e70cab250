"""A FASTQ larger than 2^32 bytes streamed through one MI355X in chunks (mm_fastx_stream_*): how close the stream comes to
the host link, and what keeping several chunks in flight buys over the serial route.

Input: a synthetic FASTQ block of 150 bp reads, 64 MiB in page-locked memory, fed again and again until more than 4.5 GiB
have gone through (the blocks end on a record, so the repeated text is one long valid FASTQ; its absolute offsets pass 2^32).
Plan: canonical minimizers k=21 w=11.

Rows
  a  stream throughput, text GB/s wall-clock from the first feed to the last batch: positions only, and positions + u64
     values; swept over chunk_bytes 4 / 16 / 64 / 256 MiB and slots 2 / 3 / 4.  Every batch is drained (its arrays are
     not copied: a consumer reads them in place).
  b  the link's bound for the same bytes up and down: mm_link_probe's rates (up alone, down alone, the sum while both
     directions are busy) applied to the bytes one block moves - text up; record tables, offsets, positions (and values)
     down: time = max(up / rate_up, down / rate_down, (up + down) / rate_both).
  c  the serial route on one block, times the number of blocks: upload, fastx_pipeline_device(...).finish(), downloads of
     the filled parts - each step waits for the one before.
a / b says how close the stream is to the link, a / c what the overlap buys.

--one-minimizer adds MM_FASTX_ONE_MINIMIZER to every stream of row a (one minimizer per read delivered with each batch),
--skip-ambiguous MM_FASTX_SKIP_AMBIGUOUS (the N packer, skipped windows and, with the flag above, clean k-mers only); rows b
and c are the plain ones either way.

Protocol: an untimed ramp of 200 ms of each measured step, warm-up steps, then the median of the timed steps.

  python tools/gpu_fastx_stream_bench.py [--total 4831838208] [--block 67108864] [--steps 3] [--warmup 1]
         [--chunks 4,16,64,256] [--slots 2,3,4] [--one-minimizer] [--skip-ambiguous] [--out profiles/fastx_stream_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import datetime
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, W, READ = 21, 11, 150
REC = 2 * READ + 6  # bytes of a FASTQ record of READ bases with a one-byte name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total", type=int, default=int(4.5 * (1 << 30)) + 1)
    ap.add_argument("--block", type=int, default=64 << 20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chunks", default="4,16,64,256")
    ap.add_argument("--slots", default="2,3,4")
    ap.add_argument("--one-minimizer", action="store_true")
    ap.add_argument("--skip-ambiguous", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import simd_minimizers_amd as sm

    dev = torch.device("cuda:0")
    L = sm.lib()
    ramp_ms = float(os.environ.get("MM_BENCH_RAMP_MS", "200"))
    n_rec = args.block // REC
    block_bytes = n_rec * REC
    n_blocks = -(-args.total // block_bytes)
    total = n_blocks * block_bytes

    # the block, page-locked
    block, _block_owner = sm.pinned_array(block_bytes, np.uint8)
    rng = np.random.default_rng(3)
    rec = block.reshape(n_rec, REC)
    rec[:] = ord("I")
    rec[:, 0] = ord("@")
    rec[:, 1] = rec[:, READ + 2] = rec[:, READ + 4] = rec[:, REC - 1] = ord("\n")
    rec[:, READ + 3] = ord("+")
    rec[:, 2:READ + 2] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n_rec, READ))]
    block_ptr = block.ctypes.data

    b = sm.canonical_minimizers(K, W)
    result = {"tool": "gpu_fastx_stream_bench", "device": torch.cuda.get_device_name(dev),
              "date": datetime.date.today().isoformat(), "ramp_ms": ramp_ms, "warmup": args.warmup, "steps": args.steps,
              "k": K, "w": W, "read": READ, "block_bytes": block_bytes, "blocks": n_blocks, "text_bytes": total, "rows": {}}

    def median_of(step, steps=args.steps, warmup=args.warmup):
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < ramp_ms:
            step(ramp=True)
        for _ in range(warmup):
            step()
        out = []
        for _ in range(steps):
            out.append(step())
        return statistics.median(out), out

    # ------------------------------------------------------------------ row a
    batch = sm._FastxBatchC()
    took = C.c_uint64()

    options = {}
    if args.one_minimizer:
        options["one_minimizer"] = True
    if args.skip_ambiguous:
        options["skip_ambiguous"] = True
    result["one_minimizer"], result["skip_ambiguous"] = args.one_minimizer, args.skip_ambiguous

    def stream_pass(chunk, slots, values, blocks):
        """One stream over `blocks` blocks; returns (seconds, records, positions, last text_end)."""
        st = sm.FastxStream(b, chunk, 2 * chunk // REC + 16, fmt="fastq", values=values, max_positions=chunk // 4 + 4096,
                            slots=slots, **options)
        records = positions = end = 0
        t0 = time.perf_counter()
        for _ in range(blocks):
            done = 0
            while done < block_bytes:
                sm._check(L.mm_fastx_stream_feed(st.h, block_ptr + done, block_bytes - done, C.byref(took)))
                done += took.value
                if done < block_bytes:
                    r = L.mm_fastx_stream_next(st.h, C.byref(batch))
                    if r == 0:
                        records += batch.n_records
                        positions += batch.n_positions
                    elif r != sm.FASTX_NEED_INPUT:
                        st._raise(r)
        st.finish()
        while True:
            r = L.mm_fastx_stream_next(st.h, C.byref(batch))
            if r == sm.FASTX_END:
                break
            if r:
                st._raise(r)
            records += batch.n_records
            positions += batch.n_positions
            end = batch.text_end
        dt = time.perf_counter() - t0
        st.close()
        return dt, records, positions, end

    rows_a = []
    positions_per_block = None
    for values in (None, "u64"):
        for chunk_mib in [int(x) for x in args.chunks.split(",")]:
            for slots in [int(x) for x in args.slots.split(",")]:
                chunk = chunk_mib << 20
                seen = {}

                def step(ramp=False):
                    dt, records, positions, end = stream_pass(chunk, slots, values, 2 if ramp else n_blocks)
                    if not ramp:
                        seen.update(records=records, positions=positions, end=end)
                    return dt

                med, every = median_of(step)
                assert seen["records"] == n_rec * n_blocks and seen["end"] == total, seen
                positions_per_block = seen["positions"] // n_blocks
                row = {"values": values or "none", "chunk_MiB": chunk_mib, "slots": slots, "s": round(med, 4),
                       "s_all": [round(x, 4) for x in every], "text_GBps": round(total / med / 1e9, 3),
                       "records": seen["records"], "positions": seen["positions"], "text_end": seen["end"]}
                print(json.dumps({"a": row}), flush=True)
                rows_a.append(row)
    result["rows"]["a"] = rows_a

    # ------------------------------------------------------------------ row b
    ws = sm.Workspace(0)
    probe_out, _probe_owner = sm.pinned_array(block_bytes, np.uint8)
    rates = (C.c_double * 3)()
    sm._check(L.mm_link_probe(ws.h, block_ptr, probe_out.ctypes.data, block_bytes, rates))
    sm._check(L.mm_link_probe(ws.h, block_ptr, probe_out.ctypes.data, block_bytes, rates))
    up_rate, down_rate, both_rate = (float(x) for x in rates)
    rows_b = []
    for values in (None, "u64"):
        up = block_bytes
        down = n_rec * 24 + 16 + positions_per_block * (4 + (8 if values else 0))
        t = max(up / up_rate, down / down_rate, (up + down) / both_rate) / 1e9
        rows_b.append({"values": values or "none", "bytes_up": up, "bytes_down": down, "link_GBps": [round(x, 2) for x in rates],
                       "s_per_block": round(t, 6), "text_GBps": round(block_bytes / t / 1e9, 3)})
        print(json.dumps({"b": rows_b[-1]}), flush=True)
    result["rows"]["b"] = rows_b

    # ------------------------------------------------------------------ row c
    rows_c = []
    bw = b.workspace(ws)
    d_text = torch.empty(block_bytes, dtype=torch.uint8, device=dev)
    h_pos, _o1 = sm.pinned_array(block_bytes // 4, np.uint32)
    h_vals, _o2 = sm.pinned_array(block_bytes // 4, np.uint64)
    h_tab, _o3 = sm.pinned_array(3 * (n_rec + 1), np.uint64)
    t_block = torch.from_numpy(block)  # (views of the page-locked arrays: torch copies straight between them and the device)
    t_pos, t_vals, t_tab = torch.from_numpy(h_pos.view(np.int32)), torch.from_numpy(h_vals.view(np.int64)), torch.from_numpy(h_tab.view(np.int64))
    for values in (None, "u64"):
        def serial(ramp=False):
            t0 = time.perf_counter()
            d_text.copy_(t_block)
            torch.cuda.synchronize(dev)
            pipe = sm.fastx_pipeline_device(bw, d_text, n_rec + 16, "fastq", values=bool(values))
            recs, cnt, pos, offs, vals = pipe.finish()  # (the record tables come to the host here)
            t_tab[: len(recs) + 1].copy_(offs)
            if cnt:
                t_pos[:cnt].copy_(pos)
                if vals is not None:
                    t_vals[:cnt].copy_(vals)
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0

        med, every = median_of(serial, steps=max(args.steps, 5), warmup=max(args.warmup, 2))
        rows_c.append({"values": values or "none", "s_per_block": round(med, 5), "s_all": [round(x, 5) for x in every],
                       "s_total": round(med * n_blocks, 4), "text_GBps": round(block_bytes / med / 1e9, 3)})
        print(json.dumps({"c": rows_c[-1]}), flush=True)
    result["rows"]["c"] = rows_c

    # ------------------------------------------------------------------ figures
    figures = []
    for i, values in enumerate(("none", "u64")):
        best = max((r for r in rows_a if r["values"] == values), key=lambda r: r["text_GBps"])
        figures.append({"values": values, "best": {k: best[k] for k in ("chunk_MiB", "slots", "text_GBps")},
                        "stream_over_link": round(best["text_GBps"] / rows_b[i]["text_GBps"], 3),
                        "stream_over_serial": round(best["text_GBps"] / rows_c[i]["text_GBps"], 3)})
    result["figures"] = figures
    print(json.dumps({"figures": figures}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
