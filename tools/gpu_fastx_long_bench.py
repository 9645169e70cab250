"""A genome-like FASTA larger than 2^32 bytes streamed through one MI355X with MM_FASTX_LONG_RECORDS: what splitting
records costs against the stream as it was, and how close both come to the host link.

Input: a synthetic block of 24 chromosome-like records (lengths in the proportions of a 24-chromosome genome, lines of 60,
runs of N at both ends and in the middle of every record), about 256 MiB in page-locked memory, fed again and again until
more than 4.5 GiB have gone through (the block ends on a line end, so the repeated text is one long valid FASTA).
Plan: canonical minimizers k=21 w=11; the stream's defaults, 3 slots and chunks of 64 MiB.

Rows
  a  the flagged stream (long_records=True), text GB/s wall-clock from the first feed to the last batch: positions only,
     positions + u64 values, and positions with skip_ambiguous.  Every batch is drained in place.
  b  the yardstick, the stream without the flag on a text it takes: the same bases as records of 10 kbp (lines of 60), the
     same three forms.
  c  the link's bound for row a's bytes: mm_link_probe's rates applied to what one block moves up (text) and down (tables,
     positions, values), as tools/gpu_fastx_stream_bench.py does.
a / b says what the split rule, the seam epilogue and the pieces cost; a / c how close the flagged stream is to the link.

Protocol (tools/gpu_fastx_stream_bench.py's): an untimed ramp of 200 ms, warm-up steps, then the median of the timed steps.

  python tools/gpu_fastx_long_bench.py [--total 4831838209] [--block-bases 268435456] [--steps 3] [--warmup 1]
         [--chunk 64] [--slots 3] [--out profiles/fastx_long_bench.json]
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

K, W, LINE, SHORT = 21, 11, 60, 10000
# (the lengths of the 24 chromosomes of a human assembly, in Mbp, as proportions)
PROPORTIONS = [248, 242, 198, 190, 182, 171, 159, 145, 138, 134, 135, 133, 114, 107, 102, 90, 83, 80, 59, 64, 47, 51, 156, 57]


def fold(np, bases, header):
    """header line + the bases in lines of LINE, every line ended: a uint8 array."""
    full = len(bases) // LINE
    lines = np.empty((full, LINE + 1), dtype=np.uint8)
    lines[:, :LINE] = bases[:full * LINE].reshape(full, LINE)
    lines[:, LINE] = 10
    rest = bases[full * LINE:]
    parts = [np.frombuffer(header + b"\n", dtype=np.uint8), lines.reshape(-1)]
    if len(rest):
        parts += [rest, np.frombuffer(b"\n", dtype=np.uint8)]
    return np.concatenate(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total", type=int, default=int(4.5 * (1 << 30)) + 1)
    ap.add_argument("--block-bases", type=int, default=256 << 20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=64, help="MiB")
    ap.add_argument("--slots", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import simd_minimizers_amd as sm

    dev = torch.device("cuda:0")
    L = sm.lib()
    ramp_ms = float(os.environ.get("MM_BENCH_RAMP_MS", "200"))
    chunk = args.chunk << 20

    # ---- the bases, once; the two texts made of them
    rng = np.random.default_rng(5)
    n_bases = args.block_bases // SHORT * SHORT
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n_bases, dtype=np.uint8)]
    lens = [int(n_bases * p / sum(PROPORTIONS)) for p in PROPORTIONS]
    lens[0] += n_bases - sum(lens)
    at = 0
    for n in lens:  # telomere-like runs of 10 kb at both ends, a centromere-like run of 1 % of the record in its middle
        bases[at:at + 10000] = ord("N")
        bases[at + n - 10000:at + n] = ord("N")
        bases[at + n // 2:at + n // 2 + n // 100] = ord("N")
        at += n
    parts, at = [], 0
    for i, n in enumerate(lens):
        parts.append(fold(np, bases[at:at + n], b">chr%d a chromosome-like record" % (i + 1)))
        at += n
    long_len = sum(len(x) for x in parts)
    long_block, _o1 = sm.pinned_array(long_len, np.uint8)
    np.concatenate(parts, out=long_block)
    del parts
    n_short = n_bases // SHORT
    short_rec = len(fold(np, bases[:SHORT], b">r"))
    short_block, _o2 = sm.pinned_array(n_short * short_rec, np.uint8)
    full = SHORT // LINE
    view = short_block.reshape(n_short, short_rec)
    view[:, 0], view[:, 1], view[:, 2] = ord(">"), ord("r"), 10
    body = view[:, 3:3 + full * (LINE + 1)].reshape(n_short, full, LINE + 1)
    src = bases.reshape(n_short, SHORT)
    body[:, :, :LINE] = src[:, :full * LINE].reshape(n_short, full, LINE)
    body[:, :, LINE] = 10
    view[:, 3 + full * (LINE + 1):short_rec - 1] = src[:, full * LINE:]
    view[:, short_rec - 1] = 10

    b = sm.canonical_minimizers(K, W)
    result = {"tool": "gpu_fastx_long_bench", "device": torch.cuda.get_device_name(dev), "date": datetime.date.today().isoformat(),
              "ramp_ms": ramp_ms, "warmup": args.warmup, "steps": args.steps, "k": K, "w": W, "chunk_MiB": args.chunk,
              "slots": args.slots, "block_bases": n_bases, "records_per_block": len(lens), "rows": {}}

    def median_of(step, steps=args.steps, warmup=args.warmup):
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < ramp_ms:
            step(ramp=True)
        for _ in range(warmup):
            step()
        out = [step() for _ in range(steps)]
        return statistics.median(out), out

    batch = sm._FastxBatchC()
    pieces = sm._FastxPiecesC()
    took = C.c_uint64()

    def stream_pass(block, max_records, blocks, long_records, values, skip):
        """One stream over `blocks` blocks; returns (seconds, records, pieces, positions, last text_end)."""
        st = sm.FastxStream(b, chunk, max_records, fmt="fasta", values=values, skip_ambiguous=skip, max_positions=chunk // 2,
                            slots=args.slots, long_records=long_records)
        ptr, n = block.ctypes.data, block.size
        seen = [0, 0, 0, 0]

        def take():
            seen[0] += batch.n_records
            seen[2] += batch.n_positions
            seen[3] = batch.text_end
            if long_records:
                sm._check(L.mm_fastx_stream_pieces(st.h, C.byref(pieces)))
                seen[0] -= pieces.first_continues
                seen[1] += pieces.first_continues

        t0 = time.perf_counter()
        for _ in range(blocks):
            done = 0
            while done < n:
                sm._check(L.mm_fastx_stream_feed(st.h, ptr + done, n - done, C.byref(took)))
                done += took.value
                if done < n:
                    r = L.mm_fastx_stream_next(st.h, C.byref(batch))
                    if r == 0:
                        take()
                    elif r != sm.FASTX_NEED_INPUT:
                        st._raise(r)
        st.finish()
        while True:
            r = L.mm_fastx_stream_next(st.h, C.byref(batch))
            if r == sm.FASTX_END:
                break
            if r:
                st._raise(r)
            take()
        dt = time.perf_counter() - t0
        st.close()
        return (dt, *seen)

    forms = (("none", None, False), ("u64", "u64", False), ("skip_ambiguous", None, True))
    rows = {"a": [], "b": []}
    for key, block, per_block, max_records, flag in (("a", long_block, len(lens), 64, True),
                                                      ("b", short_block, n_short, 2 * chunk // short_rec + 16, False)):
        n_blocks = -(-args.total // block.size)
        total = n_blocks * block.size
        for name, values, skip in forms:
            seen = {}

            def step(ramp=False):
                dt, records, n_pieces, positions, end = stream_pass(block, max_records, 1 if ramp else n_blocks, flag, values, skip)
                if not ramp:
                    seen.update(records=records, pieces=n_pieces, positions=positions, end=end)
                return dt

            med, every = median_of(step)
            assert seen["records"] == per_block * n_blocks and seen["end"] == total, seen
            row = {"form": name, "long_records": flag, "s": round(med, 4), "s_all": [round(x, 4) for x in every],
                   "text_bytes": total, "text_GBps": round(total / med / 1e9, 3), "records": seen["records"],
                   "continuing_pieces": seen["pieces"], "positions": seen["positions"], "blocks": n_blocks}
            print(json.dumps({key: row}), flush=True)
            rows[key].append(row)
    result["rows"].update(rows)

    # ---- row c: the link's bound for the flagged stream's bytes
    ws = sm.Workspace(0)
    probe_n = 64 << 20
    probe_out, _o3 = sm.pinned_array(probe_n, np.uint8)
    rates = (C.c_double * 3)()
    for _ in range(2):
        sm._check(L.mm_link_probe(ws.h, long_block.ctypes.data, probe_out.ctypes.data, probe_n, rates))
    up_rate, down_rate, both_rate = (float(x) for x in rates)
    rows_c = []
    for row in rows["a"]:
        up = row["text_bytes"]
        down = row["positions"] * (4 + (8 if row["form"] == "u64" else 0)) + (row["records"] + row["continuing_pieces"]) * 40
        t = max(up / up_rate, down / down_rate, (up + down) / both_rate) / 1e9
        rows_c.append({"form": row["form"], "bytes_up": up, "bytes_down": down, "link_GBps": [round(x, 2) for x in rates],
                       "s": round(t, 4), "text_GBps": round(up / t / 1e9, 3)})
        print(json.dumps({"c": rows_c[-1]}), flush=True)
    result["rows"]["c"] = rows_c

    figures = [{"form": a["form"], "flagged_GBps": a["text_GBps"], "yardstick_GBps": y["text_GBps"], "link_GBps": c["text_GBps"],
                "a_over_b": round(a["text_GBps"] / y["text_GBps"], 3), "a_over_c": round(a["text_GBps"] / c["text_GBps"], 3)}
               for a, y, c in zip(rows["a"], rows["b"], rows_c)]
    result["figures"] = figures
    print(json.dumps({"figures": figures}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
