"""BGZF-compressed FASTQ through one MI355X: the inflate kernel alone, the stream fed with compressed blocks
(mm_fastx_stream_feed_bgzf), the stream fed with the inflated text (the existing capability, the baseline) and what a
caller did before: zlib on one host thread in front of the stream.

Input: a synthetic FASTQ of 150 bp reads.  Python's zlib is slow, so ONE tile of 64 MiB of text is compressed block-wise
(65 280 bytes of text per BGZF block, as bgzip cuts them) and the tile is repeated until --total bytes of text have gone
through; the tile ends on a record, so the repeated text is one valid FASTQ.  Random bases and a constant quality line: the
compression ratio is that of this text, not of a sequencer's.  Levels 6 and 1.

Rows
  a  the inflate kernel alone, compressed bytes and block table resident in HBM: GB/s of inflated text (host clock around
     the launch and mm_workspace_check, milliseconds against tens of microseconds of launch cost),
     compression ratio, blocks per launch - for 64 MiB, 256 MiB and the whole --total of text per launch (one wavefront per
     block: a launch of 1 000 blocks cannot fill 256 CUs).
  b  the stream with feed_bgzf from page-locked compressed bytes: GB/s of inflated text, positions and positions + u64.
  c  the stream with feed on the inflated text (page-locked), same chunk size and slots.
  d  zlib.decompress block by block on one host thread: GB/s of text alone, and in front of c (serial: t_d + t_c).
Figures: a as it stands, b / c, b / (d in front of c).
Plan: canonical minimizers k=21 w=11.  Protocol: an untimed ramp of 200 ms of each measured step, one warm-up, then the
median of the timed steps; every row in one session.

  python tools/gpu_bgzf_bench.py [--total 1073741824] [--tile 67108864] [--steps 3] [--warmup 1] [--chunk-mib 64]
         [--slots 3] [--levels 6,1] [--out profiles/bgzf_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import datetime
import json
import os
import statistics
import struct
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
    ap.add_argument("--chunk-mib", type=int, default=64)
    ap.add_argument("--slots", type=int, default=3)
    ap.add_argument("--levels", default="6,1")
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
    chunk = args.chunk_mib << 20

    text, _text_owner = sm.pinned_array(tile_bytes, np.uint8)
    rng = np.random.default_rng(3)
    rec = text.reshape(n_rec, REC)
    rec[:] = ord("I")
    rec[:, 0] = ord("@")
    rec[:, 1] = rec[:, READ + 2] = rec[:, READ + 4] = rec[:, REC - 1] = ord("\n")
    rec[:, READ + 3] = ord("+")
    rec[:, 2:READ + 2] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n_rec, READ))]
    raw = text.tobytes()

    b = sm.canonical_minimizers(K, W)
    ws = sm.Workspace(0)
    result = {"tool": "gpu_bgzf_bench", "device": torch.cuda.get_device_name(dev), "date": datetime.date.today().isoformat(),
              "ramp_ms": ramp_ms, "warmup": args.warmup, "steps": args.steps, "k": K, "w": W, "read": READ,
              "tile_text_bytes": tile_bytes, "tiles": n_tiles, "text_bytes": total, "block_text_bytes": BLOCK_TEXT,
              "chunk_MiB": args.chunk_mib, "slots": args.slots,
              "note": "one tile of text compressed with Python's zlib and repeated; random bases, constant quality line",
              "levels": {}}

    def median_of(step, steps=args.steps, warmup=args.warmup):
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < ramp_ms:
            step(ramp=True)
        for _ in range(warmup):
            step()
        out = [step() for _ in range(steps)]
        return statistics.median(out), out

    batch = sm._FastxBatchC()
    took = C.c_uint64()

    def stream_pass(ptr, size, tiles, values, bgzf):
        st = sm.FastxStream(b, chunk, 2 * chunk // REC + 16, fmt="fastq", values=values, max_positions=chunk // 4 + 4096,
                            slots=args.slots)
        feed = L.mm_fastx_stream_feed_bgzf if bgzf else L.mm_fastx_stream_feed
        records = positions = end = 0
        t0 = time.perf_counter()
        for _ in range(tiles):
            done = 0
            while done < size:
                r = feed(st.h, ptr + done, size - done, C.byref(took))
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
        return dt, records, positions, end

    def stream_row(ptr, size, values, bgzf):
        seen = {}

        def step(ramp=False):
            dt, records, positions, end = stream_pass(ptr, size, min(2, n_tiles) if ramp else n_tiles, values, bgzf)
            if not ramp:
                seen.update(records=records, positions=positions, end=end)
            return dt

        med, every = median_of(step)
        assert seen["records"] == n_rec * n_tiles and seen["end"] == total, seen
        return {"values": values or "none", "s": round(med, 4), "s_all": [round(x, 4) for x in every],
                "text_GBps": round(total / med / 1e9, 3), "records": seen["records"], "positions": seen["positions"]}

    # ---- row c: the text itself (once: it does not depend on the level)
    rows_c = [stream_row(text.ctypes.data, tile_bytes, values, False) for values in (None, "u64")]
    for r in rows_c:
        print(json.dumps({"c": r}), flush=True)
    result["rows_c"] = rows_c

    for level in [int(x) for x in args.levels.split(",")]:
        t0 = time.perf_counter()
        blocks = [bgzf_block(raw[i:i + BLOCK_TEXT], level) for i in range(0, tile_bytes, BLOCK_TEXT)]
        t_comp = time.perf_counter() - t0
        data = b"".join(blocks)
        comp, _comp_owner = sm.pinned_array(len(data), np.uint8)
        comp[:] = np.frombuffer(data, np.uint8)
        scan = sm.bgzf_scan(comp)
        assert scan["consumed"] == len(data) and scan["out_bytes"] == tile_bytes
        out = {"compressed_tile_bytes": len(data), "ratio": round(tile_bytes / len(data), 3), "blocks_per_tile": len(blocks),
               "host_compress_s": round(t_comp, 2)}

        # ---- row a
        rows_a = []
        d_tile = torch.from_numpy(comp).to(dev)
        for tiles in sorted({1, min(4, n_tiles), n_tiles}):
            d_comp = d_tile.repeat(tiles)
            table = np.tile(scan["blocks"], tiles)
            for t in range(tiles):
                part = table[t * len(blocks):(t + 1) * len(blocks)]
                part["comp_off"] += t * len(data)
                part["out_off"] += t * tile_bytes
            d_blocks = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
            d_out = torch.empty(tiles * tile_bytes, dtype=torch.uint8, device=dev)
            d_status = torch.zeros(len(table), dtype=torch.int32, device=dev)

            def kernel(ramp=False):
                ws.sync()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                sm.bgzf_inflate_device(d_comp, d_blocks, d_out, d_status, ws=ws)
                ws.check()
                return time.perf_counter() - t0

            med, every = median_of(kernel, steps=max(args.steps, 5))
            assert not bool(d_status.any())
            assert d_out[:tile_bytes].cpu().numpy().tobytes() == raw
            assert bool((d_out[-tile_bytes:] == d_out[:tile_bytes]).all())
            rows_a.append({"text_MiB": tiles * tile_bytes >> 20, "blocks_per_launch": len(table), "s": round(med, 6),
                           "s_all": [round(x, 6) for x in every], "text_GBps": round(tiles * tile_bytes / med / 1e9, 3),
                           "timed": "host clock around launch + mm_workspace_check"})
            print(json.dumps({"level": level, "a": rows_a[-1]}), flush=True)
            del d_comp, d_blocks, d_out, d_status
        out["a"] = rows_a

        # ---- row b
        rows_b = [stream_row(comp.ctypes.data, len(data), values, True) for values in (None, "u64")]
        for r in rows_b:
            print(json.dumps({"level": level, "b": r}), flush=True)
        out["b"] = rows_b

        # ---- row d
        def host_inflate(ramp=False):
            t0 = time.perf_counter()
            n = 0
            for blk in (blocks[:64] if ramp else blocks):
                n += len(zlib.decompress(blk, 31))
            return time.perf_counter() - t0

        med, every = median_of(host_inflate, warmup=0)
        d_rate = tile_bytes / med / 1e9
        out["d"] = {"s_per_tile": round(med, 4), "s_all": [round(x, 4) for x in every], "text_GBps": round(d_rate, 3),
                    "in_front_of_c_text_GBps": [round(total / (med * n_tiles + c["s"]) / 1e9, 3) for c in rows_c]}
        print(json.dumps({"level": level, "d": out["d"]}), flush=True)
        out["figures"] = [{"values": c["values"], "b_over_c": round(bb["text_GBps"] / c["text_GBps"], 3),
                           "b_over_d_in_front_of_c": round(bb["text_GBps"] / dc, 3)}
                          for bb, c, dc in zip(rows_b, rows_c, out["d"]["in_front_of_c_text_GBps"])]
        print(json.dumps({"level": level, "figures": out["figures"]}), flush=True)
        result["levels"][str(level)] = out
        del d_tile

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
