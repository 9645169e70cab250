"""What verifying the CRC32 of BGZF blocks costs on one MI355X: the verify kernel beside the inflate kernel, the stream fed
with compressed blocks with and without MM_FASTX_BGZF_CRC, and the plain stream's default cell against the parent commit's
library.  Input as tools/gpu_bgzf_bench.py makes it: one tile of 64 MiB of synthetic FASTQ (150 bp reads) compressed
block-wise (65 280 bytes of text per block) with Python's zlib, levels 6 and 1, repeated until --total bytes of text.

Rows
  a  the verify kernel alone on resident text (the inflate's output), with the trailers' CRC32s to compare with: GB/s of
     text for 1, 4 and 17 tiles per launch (1 029, 4 116 and 17 493 blocks) - HIP events on the workspace's stream around
     the one launch, 200 ms ramp, median of 7.
  b  the inflate launch on the same blocks, timed the same way.  a / b is the flag's cost per chunk on the device.
  c  the stream with feed_bgzf from page-locked compressed bytes, with and without the flag, 64 MiB and 256 MiB chunks,
     3 slots, positions and positions + u64 values; flag and no flag ALTERNATE --rounds times (wall clock, median of
     --steps per round).  The ratio flag / no flag is given per round and over the rounds' medians; `spread` is the
     largest ratio between two rounds of the SAME setting, the session's noise the ratio has to be read against.
  d  tools/gpu_fastx_stream_bench.py --chunks 64 --slots 3 --steps 5 (the plain stream's default cell) as child processes,
     this change's library and --parent-lib (the parent commit's, loaded through MM_LIB_PATH) alternating --cell-rounds times.
Every row in one session.

  python tools/gpu_bgzf_crc_bench.py [--total 1073741824] [--tile 67108864] [--steps 3] [--rounds 2] [--levels 6,1]
         [--chunks 64,256] [--parent-lib path/to/libsimd_minimizers_amd.so] [--cell-rounds 2] [--out profiles/bgzf_crc_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import datetime
import json
import os
import statistics
import struct
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, W, READ = 21, 11, 150
REC = 2 * READ + 6
BLOCK_TEXT = 65280


def bgzf_block(raw: bytes, level: int) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9)
    payload = c.compress(raw) + c.flush()
    head = struct.pack("<4BI2BH2sHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, b"BC", 2, 18 + len(payload) + 8 - 1)
    return head + payload + struct.pack("<II", zlib.crc32(raw) & 0xffffffff, len(raw))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total", type=int, default=1 << 30)
    ap.add_argument("--tile", type=int, default=64 << 20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--chunks", default="64,256")
    ap.add_argument("--slots", type=int, default=3)
    ap.add_argument("--levels", default="6,1")
    ap.add_argument("--kernel-tiles", default="1,4,17")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--cell-rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import simd_minimizers_amd as sm

    dev = torch.device("cuda:0")
    L = sm.lib()
    ramp_ms = float(os.environ.get("MM_BENCH_RAMP_MS", "200"))
    n_rec = args.tile // REC
    tile_bytes = n_rec * REC
    n_tiles = max(1, -(-args.total // tile_bytes))
    total = n_tiles * tile_bytes

    text = np.empty(tile_bytes, np.uint8)
    rng = np.random.default_rng(3)
    rec = text.reshape(n_rec, REC)
    rec[:] = ord("I")
    rec[:, 0] = ord("@")
    rec[:, 1] = rec[:, READ + 2] = rec[:, READ + 4] = rec[:, REC - 1] = ord("\n")
    rec[:, READ + 3] = ord("+")
    rec[:, 2:READ + 2] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n_rec, READ))]
    raw = text.tobytes()

    b = sm.canonical_minimizers(K, W)
    stream = torch.cuda.Stream(dev)  # (the workspace runs on this stream, so torch's events time its launches)
    ws = sm.Workspace(0, stream=stream.cuda_stream)
    result = {"tool": "gpu_bgzf_crc_bench", "device": torch.cuda.get_device_name(dev), "date": datetime.date.today().isoformat(),
              "ramp_ms": ramp_ms, "warmup": args.warmup, "steps": args.steps, "rounds": args.rounds, "k": K, "w": W, "read": READ,
              "tile_text_bytes": tile_bytes, "tiles": n_tiles, "text_bytes": total, "block_text_bytes": BLOCK_TEXT,
              "slots": args.slots, "levels": {}}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)

    def ramp(step):
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < ramp_ms:
            step()

    batch = sm._FastxBatchC()
    took = C.c_uint64()

    def stream_pass(ptr, size, tiles, values, chunk, crc):
        st = sm.FastxStream(b, chunk, 2 * chunk // REC + 16, fmt="fastq", values=values, max_positions=chunk // 4 + 4096,
                            slots=args.slots, bgzf_crc=crc)
        records = positions = end = 0
        t0 = time.perf_counter()
        for _ in range(tiles):
            done = 0
            while done < size:
                r = L.mm_fastx_stream_feed_bgzf(st.h, ptr + done, size - done, C.byref(took))
                if r:
                    st._raise(r)
                done += took.value
                if done < size:
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
        assert tiles != n_tiles or (records == n_rec * n_tiles and end == total), (records, end)
        return dt

    for level in [int(x) for x in args.levels.split(",")]:
        blocks = [bgzf_block(raw[i:i + BLOCK_TEXT], level) for i in range(0, tile_bytes, BLOCK_TEXT)]
        data = b"".join(blocks)
        comp, _comp_owner = sm.pinned_array(len(data), np.uint8)
        comp[:] = np.frombuffer(data, np.uint8)
        scan = sm.bgzf_scan(comp, crc=True)
        assert scan["consumed"] == len(data) and scan["out_bytes"] == tile_bytes
        out = {"compressed_tile_bytes": len(data), "ratio": round(tile_bytes / len(data), 3), "blocks_per_tile": len(blocks)}

        # ---- rows a and b: one launch each between two events on the workspace's stream
        rows = []
        d_tile = torch.from_numpy(comp).to(dev)
        for tiles in [int(x) for x in args.kernel_tiles.split(",")]:
            d_comp = d_tile.repeat(tiles)
            table = np.tile(scan["blocks"], tiles)
            for t in range(tiles):
                part = table[t * len(blocks):(t + 1) * len(blocks)]
                part["comp_off"] += t * len(data)
                part["out_off"] += t * tile_bytes
            d_blocks = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
            d_expect = torch.from_numpy(np.tile(scan["crc"], tiles).view(np.int32).copy()).to(dev)
            d_out = torch.empty(tiles * tile_bytes, dtype=torch.uint8, device=dev)
            d_status = torch.zeros(len(table), dtype=torch.int32, device=dev)
            d_crc = torch.zeros(len(table), dtype=torch.int32, device=dev)

            torch.cuda.synchronize(dev)  # (the buffers were made on torch's stream, the launches go to the workspace's)

            def inflate():
                sm._check(L.mm_bgzf_inflate_device_async(ws.h, sm._ptr(d_comp), d_comp.numel(), sm._ptr(d_blocks), len(table),
                                                         sm._ptr(d_out), d_out.numel(), sm._ptr(d_status)))

            def verify():
                sm._check(L.mm_bgzf_crc32_device_async(ws.h, sm._ptr(d_out), d_out.numel(), sm._ptr(d_blocks), len(table),
                                                       sm._ptr(d_expect), sm._ptr(d_crc), sm._ptr(d_status)))

            def timed(launch):
                """milliseconds of one launch, between two events on the workspace's stream"""
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch()
                e1.record(stream)
                e1.synchronize()
                ws.check()
                return e0.elapsed_time(e1)

            row = {"text_MiB": tiles * tile_bytes >> 20, "blocks_per_launch": len(table),
                   "timed": "HIP events on the workspace's stream"}
            for name, launch in (("b_inflate", inflate), ("a_verify", verify)):
                ramp(lambda: timed(launch))
                every = [timed(launch) for _ in range(7)]
                med = statistics.median(every)
                row[name] = {"ms": round(med, 4), "ms_all": [round(x, 4) for x in every],
                             "text_GBps": round(tiles * tile_bytes / (med * 1e-3) / 1e9, 2)}
            assert not bool(d_status.any())
            assert np.array_equal(d_crc.cpu().numpy().view(np.uint32), np.tile(scan["crc"], tiles))
            row["a_over_b"] = round(row["a_verify"]["ms"] / row["b_inflate"]["ms"], 4)
            rows.append(row)
            print(json.dumps({"level": level, "ab": row}), flush=True)
            del d_comp, d_blocks, d_expect, d_out, d_status, d_crc
        out["a_b"] = rows
        del d_tile

        # ---- row c
        rows_c = []
        for chunk_mib in [int(x) for x in args.chunks.split(",")]:
            for values in (None, "u64"):
                chunk = chunk_mib << 20
                runs = {False: [], True: []}
                for rnd in range(args.rounds):
                    for crc in (False, True):
                        ramp(lambda: stream_pass(comp.ctypes.data, len(data), min(2, n_tiles), values, chunk, crc))
                        for _ in range(args.warmup):
                            stream_pass(comp.ctypes.data, len(data), n_tiles, values, chunk, crc)
                        every = [stream_pass(comp.ctypes.data, len(data), n_tiles, values, chunk, crc) for _ in range(args.steps)]
                        runs[crc].append({"round": rnd + 1, "s": round(statistics.median(every), 4), "s_all": [round(x, 4) for x in every]})
                med = {crc: statistics.median(r["s"] for r in runs[crc]) for crc in runs}
                spread = max(max(r["s"] for r in runs[crc]) / min(r["s"] for r in runs[crc]) for crc in runs)
                row = {"chunk_MiB": chunk_mib, "values": values or "none", "no_flag": runs[False], "flag": runs[True],
                       "text_GBps_no_flag": round(total / med[False] / 1e9, 3), "text_GBps_flag": round(total / med[True] / 1e9, 3),
                       "flag_over_no_flag_s": round(med[True] / med[False], 4),
                       "flag_over_no_flag_s_per_round": [round(f["s"] / n["s"], 4) for f, n in zip(runs[True], runs[False])],
                       "spread": round(spread, 4)}
                rows_c.append(row)
                print(json.dumps({"level": level, "c": row}), flush=True)
        out["c"] = rows_c
        result["levels"][str(level)] = out
        save()

    # ---- row d
    if args.parent_lib:
        cell = {"change": [], "parent": []}
        for rnd in range(args.cell_rounds):
            for who in ("parent", "change"):
                env = dict(os.environ)
                if who == "parent":
                    env["MM_LIB_PATH"] = os.path.abspath(args.parent_lib)
                else:
                    env.pop("MM_LIB_PATH", None)
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gpu_fastx_stream_bench.py"), "--chunks", "64", "--slots", "3",
                                    "--steps", "5"], env=env, capture_output=True, text=True, timeout=600)
                if r.returncode:
                    print(r.stdout[-2000:], r.stderr[-2000:], flush=True)
                    raise SystemExit("row d: the stream benchmark failed with the %s library" % who)
                for line in r.stdout.splitlines():
                    if line.startswith('{"a"'):
                        a = json.loads(line)["a"]
                        cell[who].append({"round": rnd + 1, "values": a["values"], "s": a["s"], "s_all": a["s_all"], "text_GBps": a["text_GBps"]})
                print(json.dumps({"d": who, "round": rnd + 1, "rows": cell[who][-2:]}), flush=True)
        figures = []
        for values in ("none", "u64"):
            s = {who: [x["s"] for x in cell[who] if x["values"] == values] for who in cell}
            figures.append({"values": values, "change_over_parent_s": round(statistics.median(s["change"]) / statistics.median(s["parent"]), 4),
                            "spread": round(max(max(v) / min(v) for v in s.values()), 4)})
        result["d"] = {"tool": "gpu_fastx_stream_bench --chunks 64 --slots 3 --steps 5",
                       "protocol": "child processes, parent commit's library and this change's alternating (parent, change, ...), %d rounds" % args.cell_rounds,
                       "cells": cell, "figures": figures}
        print(json.dumps({"d": figures}), flush=True)
    save()


if __name__ == "__main__":
    main()
