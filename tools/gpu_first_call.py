"""First-call cost per flavour: wall ms of the first and of the fifth call of a fresh process with an EMPTY run-time
compile cache, and the run-time compiler's counters (mm_jit_stats).

    python tools/gpu_first_call.py [--root TREE] [--label NAME] [--out FILE.json]

Every row runs in a child process of its own (this file with --row) under `timeout`, with MM_JIT_CACHE_DIR pointing at a
new empty 0700 directory; the script stops at the first child that fails.  --root selects the built tree whose package
is measured (default: this one), so that the same script measures an older commit; rows that need an interface the tree
lacks (prepare) are skipped there.  The result is one JSON object {label, rows}; with --out it is merged into that file
under its label (profiles/first_call.json).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = ["sequence_canonical_k21_w11", "reads_minimizers_w11", "reads_super_kmers_w11", "reads_closed_syncmers_k15_w17",
        "sequence_forward_w37", "sequence_forward_w37_prepared"]
ROW_TIMEOUT_S = 240


def row_main(root, row):
    for p in (root, os.path.join(root, "oracle")):
        sys.path.insert(0, p)
    import numpy as np
    import torch

    import mm_oracle as oracle
    import simd_minimizers_amd as sm

    torch.zeros(1, device="cuda")  # (the device context is not what is measured)
    torch.cuda.synchronize()
    res = {"row": row}
    stats = (lambda: sm.jit_stats()) if hasattr(sm, "jit_stats") else (lambda: None)

    def timed(call, calls=5):
        ms = []
        for _ in range(calls):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    if row.startswith("sequence"):
        n = 100_000
        k, w, canonical = (21, 11, True) if "canonical" in row else (21, 37, False)
        b = sm.canonical_minimizers(k, w) if canonical else sm.minimizers(k, w)
        h = oracle.gen_packed(1, n)
        d = torch.from_numpy(h).cuda()
        out = torch.zeros(n, dtype=torch.int32, device="cuda")
        if row.endswith("_prepared"):
            if not hasattr(b, "prepare"):
                res["skipped"] = "this tree has no prepare"
                print(json.dumps(res))
                return 0
            t0 = time.perf_counter()
            res["prepare_report"] = b.prepare(sequence=True)
            res["prepare_ms"] = (time.perf_counter() - t0) * 1e3
        cnt = [0]

        def call():
            cnt[0] = b.run_device(d, n, out)
        ms = timed(call)
        ok = np.array_equal(out[:cnt[0]].cpu().numpy().view(np.uint32), oracle.run(h, n, k, w, canonical=canonical))
    else:
        n_reads, rl = 10_000, 150
        if "closed" in row:
            k, w, b, mode, sk = 15, 17, sm.canonical_closed_syncmers(15, 17), oracle.CLOSED_SYNCMERS, False
        else:
            sk = "super_kmers" in row
            k, w, mode = 21, 11, oracle.MINIMIZERS
            b = sm.canonical_minimizers(k, w).super_kmers([]) if sk else sm.canonical_minimizers(k, w)
        h = oracle.gen_packed(2, n_reads * rl)
        d = torch.from_numpy(h).cuda()
        pos = torch.zeros(n_reads * rl, dtype=torch.int32, device="cuda")
        osk = torch.zeros_like(pos) if sk else None
        offs = torch.zeros(n_reads + 1, dtype=torch.int64, device="cuda")
        cnt = [0]

        def call():
            cnt[0] = sm.run_reads_device(b, d, n_reads, rl, rl, pos, offs, out_sk=osk)
        ms = timed(call)
        want = [oracle.run(h, rl, k, w, canonical=True, base_offset=r * rl, mode=mode, super_kmers=sk)
                for r in range(0, n_reads, 97)]
        o = offs.cpu().numpy()
        got = pos[:cnt[0]].cpu().numpy().view(np.uint32)
        ok = all(np.array_equal(got[o[r]:o[r + 1]], (wr[0] if sk else wr)) for r, wr in zip(range(0, n_reads, 97), want))
    res.update(first_ms=ms[0], fifth_ms=ms[4], all_ms=ms, jit_stats=stats(), ok=bool(ok),
               hsaco=len([f for f in os.listdir(os.environ["MM_JIT_CACHE_DIR"]) if f.endswith(".hsaco")]))
    print(json.dumps(res))
    return 0 if ok else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--label", default="this")
    ap.add_argument("--out")
    ap.add_argument("--row")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    if a.row:
        return row_main(root, a.row)
    rows = []
    for row in ROWS:
        with tempfile.TemporaryDirectory() as tmp:
            cache = os.path.join(tmp, "jit")
            os.mkdir(cache, 0o700)
            env = {k: v for k, v in os.environ.items() if not k.startswith("MM_")}
            env["MM_JIT_CACHE_DIR"] = cache
            r = subprocess.run(["timeout", "-k", "10", str(ROW_TIMEOUT_S), sys.executable, os.path.abspath(__file__),
                                "--root", root, "--row", row], env=env, capture_output=True, text=True)
            lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
            if r.returncode != 0 or not lines:
                print(f"row {row} failed with status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", file=sys.stderr)
                return r.returncode or 1
            rows.append(json.loads(lines[-1]))
            print(lines[-1], flush=True)
    result = {"label": a.label, "rows": rows}
    if a.out:
        merged = {}
        if os.path.exists(a.out):
            merged = json.load(open(a.out))
        merged[a.label] = rows
        with open(a.out, "w") as f:
            json.dump(merged, f, indent=1)
            f.write("\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
