"""The number of timed launches (mm_workspace_kernel_time's `launches`) of one tiny call of every path of the host file
that owns a timed-launch site, with the call's result against the oracle (tests/text_checker.py for byte text).  The
timed launch is shared plumbing: a site that loses its event pair, or pushes one twice, shows up here.

Shapes of tests/test_gpu_abi_codes.py: k = 5, w = 3; 64 bases; 3 reads of 20 bases back to back; three 40-base sequences
sliced from one tensor; a 40-byte text in records of 10, 15 and 15 bytes."""
import os

import numpy as np
import pytest

import text_checker as tc

pytestmark = pytest.mark.gpu

K, W = 5, 3
TEXT = b"the quick brown fox jumps over the lazy!"
TSTARTS = [0, 10, 25, 40]

# (launches, lane-table launch) per path, as the library reported them BEFORE the timed launches were folded into one
# helper: measured by running paths() below on the parent commit of that change (MI355X), not derived from the code.
# (The per-record loop of a generic text batch reports 0: its launches, one per record, are not timed.)
PARENT = {
    "sequence fused": (1, False),
    "sequence generic": (1, False),
    "reads one lane per read": (1, False),
    "reads lane table": (1, True),
    "batch tiles": (1, False),
    "batch lane table": (1, True),
    "text single": (1, False),
    "text batch fused": (1, False),
    "text batch generic": (0, False),
    "text batch counts": (1, False),
    "packed reads counts": (1, True),
}


class _Switches:
    """MM_LANE_TABLE and mm_workspace_force_generic for one call (conftest.py makes the library re-read switches)."""

    def __init__(self, ws, lane_table=None, generic=False):
        self.ws, self.lane_table, self.generic = ws, lane_table, generic

    def __enter__(self):
        self.old = os.environ.get("MM_LANE_TABLE")
        if self.lane_table is None:
            os.environ.pop("MM_LANE_TABLE", None)
        else:
            os.environ["MM_LANE_TABLE"] = self.lane_table
        self.ws.force_generic(self.generic)

    def __exit__(self, *a):
        self.ws.force_generic(False)
        if self.old is None:
            os.environ.pop("MM_LANE_TABLE", None)
        else:
            os.environ["MM_LANE_TABLE"] = self.old


def paths(sm, oracle, ws):
    """Yields (path, launches, lane-table launch) after checking the call's result."""
    import torch
    b = sm.canonical_minimizers(K, W).workspace(ws)
    d = sm.generate_device(128, 21)
    host = np.concatenate([d.cpu().numpy(), np.zeros(16, dtype=np.uint8)])
    out = torch.zeros(256, dtype=torch.int32, device="cuda")
    offs = torch.zeros(4, dtype=torch.int64, device="cuda")

    def timed(call, **switches):
        out.fill_(-1)
        offs.fill_(-1)
        with _Switches(ws, **switches):
            ws.kernel_time(True)
            got = call()
            _, launches = ws.kernel_time(True)
        return got, launches, bool(ws.last_lane_table())

    def flat(n):
        return out[:n].cpu().numpy().view(np.uint32)

    # ---- one sequence
    want = oracle.run(host, 64, K, W, canonical=True)
    for name, generic in (("sequence fused", False), ("sequence generic", True)):
        cnt, launches, _ = timed(lambda: b.run_device(d, 64, out), generic=generic)
        assert ws.last_path() == (sm.PATH_GENERIC if generic else sm.PATH_FUSED), name
        assert cnt == len(want) and np.array_equal(flat(cnt), want), name
        yield name, launches, False

    # ---- 3 reads of 20 bases, back to back
    def check_reads(name, total, ho, starts, ln):
        assert ho[0] == 0 and ho[-1] == total, name
        for r, s0 in enumerate(starts):
            w_r = oracle.run(host[s0 // 4:], ln, K, W, canonical=True, base_offset=s0 % 4)
            assert np.array_equal(flat(total)[ho[r]:ho[r + 1]], w_r), (name, r)

    for name, table in (("reads one lane per read", "0"), ("reads lane table", "1")):
        total, launches, lt = timed(lambda: sm.run_reads_device(b, d, 3, 20, 20, out, offs), lane_table=table)
        check_reads(name, total, offs.cpu().numpy(), [0, 20, 40], 20)
        yield name, launches, lt

    # ---- three 40-base sequences sliced from one tensor
    seqs = [d[0:], d[10:], d[20:]]
    for name, table in (("batch tiles", "0"), ("batch lane table", "1")):
        ho, launches, lt = timed(lambda: sm.run_batch_device(b, seqs, [40, 40, 40], out), lane_table=table)
        check_reads(name, ho[-1], ho, [0, 40, 80], 40)
        yield name, launches, lt

    # ---- packed reads with the counts on the device
    d_starts = torch.tensor([0, 20, 40, 60], dtype=torch.int64, device="cuda")
    d_counts = torch.tensor([60, 3], dtype=torch.int64, device="cuda")
    got, launches, lt = timed(lambda: sm.run_packed_reads_counts_device(b, d, d_starts, d_counts, out, offs, max_bases=60))
    assert got[1:] == (60, 3)
    check_reads("packed reads counts", got[0], offs.cpu().numpy(), [0, 20, 40], 20)
    yield "packed reads counts", launches, lt

    # ---- byte text
    th = sm.TextMulHasher(canonical=False)
    tb = sm.minimizers(K, W).hasher(th).workspace(ws)
    text = np.frombuffer(TEXT, dtype=np.uint8)
    d_text = torch.from_numpy(text.copy()).cuda()
    want = tc.run(text, K, W, th, False, 0)
    cnt, launches, _ = timed(lambda: tb.run_text_device(d_text, 40, out))
    assert cnt == len(want) and np.array_equal(flat(cnt), want)
    yield "text single", launches, False

    d_tstarts = torch.tensor(TSTARTS, dtype=torch.int64, device="cuda")
    d_tcounts = torch.tensor([40, 3], dtype=torch.int64, device="cuda")

    def check_records(name, total):
        ho = offs.cpu().numpy()
        assert ho[0] == 0 and ho[-1] == total, name
        for r in range(3):
            w_r = tc.run(text[TSTARTS[r]:TSTARTS[r + 1]], K, W, th, False, 0)
            assert np.array_equal(flat(total)[ho[r]:ho[r + 1]], w_r), (name, r)

    for name, generic in (("text batch fused", False), ("text batch generic", True)):
        total, launches, _ = timed(lambda: sm.run_text_batch_device(tb, d_text, d_tstarts, 40, out, offs), generic=generic)
        check_records(name, total)
        yield name, launches, False
    got, launches, _ = timed(lambda: sm.run_text_batch_counts_device(tb, d_text, d_tstarts, d_tcounts, out, offs, wait=True))
    assert got[1:] == (40, 3)
    check_records("text batch counts", got[0])
    yield "text batch counts", launches, False


def test_launches_per_path(sm, oracle, gpu):
    ws = sm.Workspace(0)
    ws.enable_timing(True)
    got = {}
    try:
        for name, launches, lane_table in paths(sm, oracle, ws):
            print(name, launches, lane_table)
            got[name] = (launches, lane_table)
    finally:
        ws.enable_timing(False)
        ws.force_generic(False)
        ws.close()
    assert got == PARENT
