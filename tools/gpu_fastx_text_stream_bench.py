"""A protein-like FASTA larger than 2^32 bytes streamed through one MI355X in chunks (mm_fastx_text_stream_create), and
the one-minimizer counts call against the host-n call.  The protocol of tools/gpu_fastx_stream_bench.py: an untimed ramp
of 200 ms of each measured step, 1 warm-up, the median of 3, wall-clock.

Input: a block of protein-like records (20 letters, 60-character lines, lengths 50 .. 700) of about 64 MiB in page-locked
memory, fed again and again until more than 4.5 GiB have gone through.  Plan: forward minimizers k=7 w=11 on byte text.

Rows
  a    stream text GB/s at the default 3 slots / 64 MiB: positions only, positions + u64 values (BYTES), positions + one
       minimizer per record
  b    mm_link_probe's bound for the same bytes up and down
  c    the serial route on one block: upload, fasta_text_pipeline_device(...).finish(), downloads
  d    the DNA stream's default cell (150-bp FASTQ, canonical k=21 w=11, 64 MiB, 3 slots), taken in the same session as the
       yardstick
  one  the one-minimizer calls on 1 M protein-like records (the input and the timing of tools/gpu_one_minimizer_bench.py
       row d: events on a torch stream the workspace is built on, median of 7): the host-n call, held against the committed
       profiles/one_minimizer_bench.json within +-3 %, and the counts call
Figures: a/b, a/c, a/d, counts / host-n.  Every row runs in a child process of its own under a time limit; after a row
that fails or runs out of time nothing more is started on the device: the rows taken so far are written, the rest are
marked "not measured".

  python tools/gpu_fastx_text_stream_bench.py [--out profiles/fastx_text_stream_bench.json] [--rows a,b,c,d,one]
"""
from __future__ import annotations

import argparse
import ctypes as C
import datetime
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, W = 7, 11
LIMITS = {"a": 240, "b": 60, "c": 90, "d": 120, "one": 90}  # seconds per row


def protein_block(np, target_bytes, seed=3):
    """(page-locked uint8 block, owner, records, characters): whole records only, so the repeated text is one valid FASTA."""
    import simd_minimizers_amd as sm
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    parts, size, n_rec, chars = [], 0, 0, 0
    while size < target_bytes - 1024:
        m = int(rng.integers(50, 701))
        s = letters[rng.integers(0, 20, m)].tobytes()
        rec = b">sp|P%07d|NAME\n" % n_rec + b"".join(s[q:q + 60] + b"\n" for q in range(0, m, 60))
        parts.append(rec)
        size += len(rec)
        n_rec += 1
        chars += m
    text = b"".join(parts)
    block, owner = sm.pinned_array(len(text), np.uint8)
    block[:] = np.frombuffer(text, dtype=np.uint8)
    return block, owner, n_rec, chars


def median_of(step, steps, warmup, ramp_ms):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ramp_ms:
        step(ramp=True)
    for _ in range(warmup):
        step()
    out = [step() for _ in range(steps)]
    return statistics.median(out), out


def stream_pass(sm, L, st, block_ptr, block_bytes, blocks):
    batch, took = sm._FastxBatchC(), C.c_uint64()
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


def row(name, args):
    import numpy as np
    import torch

    import simd_minimizers_amd as sm

    dev = torch.device("cuda:0")
    L = sm.lib()
    ramp_ms = float(os.environ.get("MM_BENCH_RAMP_MS", "200"))
    out = {"device": torch.cuda.get_device_name(dev)}
    if name in ("a", "b", "c"):
        block, _owner, n_rec, chars = protein_block(np, args.block)
        block_bytes = block.size
        n_blocks = -(-args.total // block_bytes)
        total = n_blocks * block_bytes
        out.update(block_bytes=block_bytes, blocks=n_blocks, text_bytes=total, records_per_block=n_rec, chars_per_block=chars)
        b = sm.minimizers(K, W).hasher(sm.TextMulHasher(canonical=False))
    if name == "a":
        chunk = 64 << 20
        cells = []
        for label, opt in (("positions", {}), ("positions+u64", {"values": "u64"}), ("positions+one_minimizer", {"one_minimizer": True})):
            seen = {}

            def step(ramp=False):
                st = sm.FastxTextStream(b, chunk, 2 * chunk // 64 + 16, fmt="fasta", max_positions=chunk // 2 + 4096, **opt)
                dt, records, positions, end = stream_pass(sm, L, st, block.ctypes.data, block_bytes, 2 if ramp else n_blocks)
                if not ramp:
                    seen.update(records=records, positions=positions, end=end)
                return dt

            med, every = median_of(step, args.steps, args.warmup, ramp_ms)
            assert seen["records"] == n_rec * n_blocks and seen["end"] == total, seen
            cells.append({"what": label, "chunk_MiB": 64, "slots": 3, "s": round(med, 4), "s_all": [round(x, 4) for x in every],
                          "text_GBps": round(total / med / 1e9, 3), **seen})
        out["cells"] = cells
    elif name == "b":
        ws = sm.Workspace(0)
        probe_out, _po = sm.pinned_array(block_bytes, np.uint8)
        rates = (C.c_double * 3)()
        for _ in range(2):
            sm._check(L.mm_link_probe(ws.h, block.ctypes.data, probe_out.ctypes.data, block_bytes, rates))
        up_rate, down_rate, both_rate = (float(x) for x in rates)
        st = sm.FastxTextStream(b, 64 << 20, 2 * (64 << 20) // 64 + 16, fmt="fasta")
        _, _, positions, _ = stream_pass(sm, L, st, block.ctypes.data, block_bytes, 1)
        cells = []
        for label, extra in (("positions", 0), ("positions+u64", 8 * positions), ("positions+one_minimizer", 4 * n_rec)):
            up, down = block_bytes, n_rec * 24 + 16 + 4 * positions + extra
            t = max(up / up_rate, down / down_rate, (up + down) / both_rate) / 1e9
            cells.append({"what": label, "bytes_up": up, "bytes_down": down, "text_GBps": round(block_bytes / t / 1e9, 3)})
        out.update(link_GBps=[round(x, 2) for x in rates], cells=cells)
    elif name == "c":
        ws = sm.Workspace(0)
        bw = b.workspace(ws)
        d_text = torch.empty(block_bytes, dtype=torch.uint8, device=dev)
        h_pos, _o1 = sm.pinned_array(block_bytes, np.uint32)
        h_vals, _o2 = sm.pinned_array(block_bytes, np.uint64)
        h_tab, _o3 = sm.pinned_array(n_rec + 17, np.uint64)
        t_block = torch.from_numpy(block)
        t_pos, t_vals, t_tab = (torch.from_numpy(h_pos.view(np.int32)), torch.from_numpy(h_vals.view(np.int64)),
                                torch.from_numpy(h_tab.view(np.int64)))
        cells = []
        for label, enc in (("positions", None), ("positions+u64", sm.TEXT_VALUES_BYTES)):
            def serial(ramp=False):
                t0 = time.perf_counter()
                d_text.copy_(t_block)
                torch.cuda.synchronize(dev)
                recs, cnt, pos, offs, vals = sm.fasta_text_pipeline_device(bw, d_text, n_rec + 16, encoding=enc).finish()
                t_tab[: len(recs) + 1].copy_(offs)
                if cnt:
                    t_pos[:cnt].copy_(pos)
                    if vals is not None:
                        t_vals[:cnt].copy_(vals)
                torch.cuda.synchronize(dev)
                return time.perf_counter() - t0

            med, every = median_of(serial, max(args.steps, 5), max(args.warmup, 2), ramp_ms)
            cells.append({"what": label, "s_per_block": round(med, 5), "s_all": [round(x, 5) for x in every],
                          "text_GBps": round(block_bytes / med / 1e9, 3)})
        out["cells"] = cells
    elif name == "d":
        read, rec_bytes = 150, 306
        n_rec = args.block // rec_bytes
        block_bytes = n_rec * rec_bytes
        n_blocks = -(-args.total // block_bytes)
        block, _owner = sm.pinned_array(block_bytes, np.uint8)
        rng = np.random.default_rng(3)
        rec = block.reshape(n_rec, rec_bytes)
        rec[:] = ord("I")
        rec[:, 0] = ord("@")
        rec[:, 1] = rec[:, read + 2] = rec[:, read + 4] = rec[:, rec_bytes - 1] = ord("\n")
        rec[:, read + 3] = ord("+")
        rec[:, 2:read + 2] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n_rec, read))]
        bd = sm.canonical_minimizers(21, 11)
        chunk = 64 << 20
        cells = []
        for label, values in (("positions", None), ("positions+u64", "u64")):
            def step(ramp=False):
                st = sm.FastxStream(bd, chunk, 2 * chunk // rec_bytes + 16, fmt="fastq", values=values,
                                    max_positions=chunk // 4 + 4096, slots=3)
                return stream_pass(sm, L, st, block.ctypes.data, block_bytes, 2 if ramp else n_blocks)[0]

            med, every = median_of(step, args.steps, args.warmup, ramp_ms)
            cells.append({"what": label, "s": round(med, 4), "s_all": [round(x, 4) for x in every],
                          "text_GBps": round(n_blocks * block_bytes / med / 1e9, 3)})
        out.update(cells=cells, text_bytes=n_blocks * block_bytes)
    elif name == "one":
        # the input and the timing of tools/gpu_one_minimizer_bench.py row (d): a torch stream, the workspace built on it,
        # events recorded on it; the committed figure of that row is read and compared with
        stream = torch.cuda.Stream(dev)
        ws = sm.Workspace(0, stream.cuda_stream)
        n_rec = 1_000_000
        g = torch.Generator(device=dev)
        g.manual_seed(12)
        lens = torch.exp(5.7 + 0.6 * torch.randn(n_rec, device=dev, generator=g, dtype=torch.float64)).to(torch.int64) + 1
        starts = torch.zeros(n_rec + 1, dtype=torch.int64, device=dev)
        starts[1:] = torch.cumsum(lens, 0)
        n = int(starts[-1].item())
        letters = torch.tensor(list(b"ACDEFGHIKLMNPQRSTVWY"), dtype=torch.uint8, device=dev)
        text = letters[torch.randint(0, 20, (n,), device=dev, generator=g)]
        counts = torch.tensor([n, n_rec], dtype=torch.int64, device=dev)
        th = sm.TextMulHasher(K, False)
        pos = torch.empty(n_rec + 16, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        vp = lambda t: C.c_void_p(t.data_ptr())

        def timed(step, steps=7, warmup=3):
            with torch.cuda.stream(stream):
                t0 = time.perf_counter()
                while (time.perf_counter() - t0) * 1e3 < ramp_ms:
                    step()
                    ws.sync()
                for _ in range(warmup):
                    step()
                ws.sync()
                ms = []
                for _ in range(steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    step()
                    e1.record(stream)
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                ws.check()
            return statistics.median(ms), ms

        def host_n_step():
            sm._check(L.mm_one_minimizer_text_batch_device_async(ws.h, C.byref(th), K, vp(text), n, n_rec, vp(starts), vp(pos)))

        def counts_step():
            sm._check(L.mm_one_minimizer_text_batch_counts_device_async(ws.h, C.byref(th), K, vp(text), n, n, n_rec, vp(starts),
                                                                        vp(counts), vp(pos)))

        host_ms, host_all = timed(host_n_step)
        counts_ms, counts_all = timed(counts_step)
        out.update(records=n_rec, text_bytes=n, timing="events on the workspace's stream, median of 7, 3 warm-up",
                   host_n_ms=host_ms, host_n_all_ms=host_all, counts_ms=counts_ms, counts_all_ms=counts_all,
                   counts_over_host_n=counts_ms / host_ms)
        with open(os.path.join(ROOT, "profiles", "one_minimizer_bench.json")) as f:
            committed = [r for r in json.load(f)["rows"] if r.get("workload") == "TEXT"][0]
        out.update(committed_host_n_ms=committed["d_one_minimizer_ms"], committed_bytes=committed["bytes"],
                   host_n_over_committed=host_ms / committed["d_one_minimizer_ms"],
                   within_3_percent=bool(abs(host_ms / committed["d_one_minimizer_ms"] - 1.0) <= 0.03))
        ws.close()
    print("ROW " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total", type=int, default=int(4.5 * (1 << 30)) + 1)
    ap.add_argument("--block", type=int, default=64 << 20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", default="a,b,c,d,one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastx_text_stream_bench.json"))
    ap.add_argument("--row", default=None, help="(internal) run one row in this process")
    args = ap.parse_args()
    if args.row:
        row(args.row, args)
        return
    result = {"tool": "gpu_fastx_text_stream_bench", "date": datetime.date.today().isoformat(), "k": K, "w": W,
              "protocol": "200 ms ramp, 1 warm-up, median of 3, wall-clock; one child process per row under a time limit",
              "rows": {}}
    names = args.rows.split(",")
    for i, name in enumerate(names):
        cmd = [sys.executable, os.path.abspath(__file__), "--row", name, "--total", str(args.total), "--block", str(args.block),
               "--steps", str(args.steps), "--warmup", str(args.warmup)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[name])
            lines = [x for x in r.stdout.splitlines() if x.startswith("ROW ")]
            result["rows"][name] = json.loads(lines[-1][4:]) if r.returncode == 0 and lines else \
                {"not_measured": f"exit status {r.returncode}", "stderr": r.stderr[-600:]}
        except subprocess.TimeoutExpired:
            result["rows"][name] = {"not_measured": f"ran past its limit of {LIMITS[name]} s"}
        print(json.dumps({name: result["rows"][name]}), flush=True)
        if "not_measured" in result["rows"][name]:
            # a row that failed or ran out of time may have faulted or hung the device: nothing more is started on it
            for later in names[i + 1:]:
                result["rows"][later] = {"not_measured": f"not started: row {name} did not finish"}
            break
    rows = result["rows"]
    figures = {}
    try:
        for i, cell in enumerate(rows["a"]["cells"]):
            f = {}
            if "cells" in rows.get("b", {}):
                f["a_over_b"] = round(cell["text_GBps"] / rows["b"]["cells"][i]["text_GBps"], 3)
            if "cells" in rows.get("c", {}) and i < len(rows["c"]["cells"]):
                f["a_over_c"] = round(cell["text_GBps"] / rows["c"]["cells"][i]["text_GBps"], 3)
            if "cells" in rows.get("d", {}):
                f["a_over_d"] = round(cell["text_GBps"] / rows["d"]["cells"][min(i, 1)]["text_GBps"], 3)
            figures[cell["what"]] = f
    except (KeyError, TypeError):
        pass
    result["figures"] = figures
    print(json.dumps({"figures": figures}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
