"""Queues of asynchronous calls on a caller's own NON-BLOCKING stream, shared by tests/test_gpu_stream_order.py.

The scheme: a ``Queue`` owns ``torch.cuda.Stream()`` - non-blocking, not the default stream - and a workspace bound to it
(``mm_workspace_create(..., hip_stream)``).  Data inputs (``Input``) are device buffers filled with 0xA5 that receive their
real content from page-locked host memory by a copy queued on that stream AS PART OF the queue; inputs a kernel uses as
an index (starts, lengths, counts, offsets) are filled with zeros instead, so that a read that comes too early gives a
wrong answer and never a wild address.  Outputs (``Output``) are filled with -7 and carry 8 elements of slack.  A delay
kernel (``torch.cuda._sleep``) in front of the queue keeps the device busy while the host enqueues everything: anything
the library puts on another stream, or reads on the host before its upload ran, meets the fill bytes.  Nothing on this
stream is ordered against the legacy default stream, which is what every other GPU test relies on without saying so."""
from __future__ import annotations

import ctypes as C

import numpy as np

FILL = 0xA5
SLACK = 8
TARGET_MS, CAP_MS = 50.0, 250.0
PROBE_CYCLES = 2_000_000


def vp(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else None


def _torch_dtype(dtype):
    import torch
    return {"uint8": torch.uint8, "int8": torch.int8, "int32": torch.int32, "uint32": torch.int32, "int64": torch.int64,
            "uint64": torch.int64}[np.dtype(dtype).name]


class Input:
    """A device buffer and its content in page-locked host memory.  ``reset`` fills the device bytes with 0xA5 (zeros for
    an ``index`` input), ``upload`` queues the copy on the current stream.  ``shift``: the device view starts that many bytes
    into its allocation (a pointer that is not 4-byte aligned)."""

    def __init__(self, host, index=False, shift=0):
        import torch
        host = np.ascontiguousarray(host)
        assert shift == 0 or host.dtype == np.uint8
        raw = host.view(np.uint8).reshape(-1)
        self.host = host
        self.index = index
        self.h = torch.from_numpy(raw.copy()).pin_memory()
        self.base = torch.empty(shift + raw.size, dtype=torch.uint8, device="cuda")
        self.bytes = self.base[shift:]
        self.d = self.bytes if host.dtype == np.uint8 else self.bytes.view(_torch_dtype(host.dtype))

    def reset(self):
        self.base.fill_(0 if self.index else FILL)

    def upload(self):
        self.bytes.copy_(self.h, non_blocking=True)


class Output:
    """``n`` elements for a call to write and ``SLACK`` more that it must not touch, all -7 before the queue starts
    (``fill``: another start value, for a word the queue itself builds on the stream)."""

    def __init__(self, n, dtype=np.int32, fill=-7):
        import torch
        self.n, self.fill = int(n), fill
        self.buf = torch.empty(self.n + SLACK, dtype=_torch_dtype(np.int8 if np.dtype(dtype) == np.uint8 else dtype),
                               device="cuda")
        self.d = self.buf[: self.n]

    def reset(self):
        self.buf.fill_(self.fill)

    def host(self):
        return self.buf.cpu().numpy()


class Call:
    def __init__(self, name, issue, after=(), verify=None):
        self.name, self.issue, self.after, self.verify = name, issue, tuple(after), verify


_CYCLES = None


def delay_cycles():
    """``torch.cuda._sleep`` cycles for about TARGET_MS on this device, measured once per session with two events on a
    non-blocking stream; never more than CAP_MS."""
    global _CYCLES
    if _CYCLES is None:
        import torch
        s = torch.cuda.Stream()

        def timed(cycles):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record(s)
                torch.cuda._sleep(cycles)
                e1.record(s)
            e1.synchronize()
            return e0.elapsed_time(e1)

        timed(1000)  # (loads the kernel)
        ms = max(timed(PROBE_CYCLES), 1e-3)
        cycles = max(1, int(PROBE_CYCLES * TARGET_MS / ms))
        got = timed(cycles)
        if got > CAP_MS:
            cycles = max(1, int(cycles * CAP_MS / got))
            got = timed(cycles)
        assert got <= 1.2 * CAP_MS, f"the delay kernel takes {got:.1f} ms for {cycles} cycles"
        print(f"stream_queue: {PROBE_CYCLES} sleep cycles took {ms:.3f} ms; delay = {cycles} cycles = {got:.1f} ms")
        _CYCLES = cycles
    return _CYCLES


class Queue:
    """Calls on one non-blocking stream and one workspace.  ``add`` registers a call (``after``: names of the calls whose
    results or uploads it reads), ``order(seed)`` gives the listed order or a seeded permutation that keeps those
    dependencies, ``begin`` / ``issue`` / ``end`` enqueue with no host wait in between, ``finish`` is the one
    ``Workspace.check`` and the comparison of every call's results."""

    def __init__(self, sm):
        import torch
        self.sm = sm
        self.s = torch.cuda.Stream()
        self.ws = sm.Workspace(0, self.s.cuda_stream)
        self.inputs, self.outputs, self.calls = [], [], []
        self.after_delay = None
        self.first_seen_done = None

    def close(self):
        self.s.synchronize()
        self.ws.close()

    def input(self, host, index=False, shift=0):
        i = Input(host, index, shift)
        self.inputs.append(i)
        return i

    def output(self, n, dtype=np.int32, fill=-7):
        o = Output(n, dtype, fill)
        self.outputs.append(o)
        return o

    def add(self, name, issue, after=(), verify=None):
        assert all(any(c.name == a for c in self.calls) for a in after), (name, after)
        self.calls.append(Call(name, issue, after, verify))

    def upload(self, name, inp):
        self.add(name, inp.upload)

    def order(self, seed=None, calls=None):
        calls = list(self.calls if calls is None else calls)
        if seed is None:
            return calls
        rng = np.random.default_rng(seed)
        names = {c.name for c in calls}
        done, out = set(), []
        while calls:
            ready = [c for c in calls if all(a in done or a not in names for a in c.after)]
            c = ready[int(rng.integers(0, len(ready)))]
            calls.remove(c)
            done.add(c.name)
            out.append(c)
        return out

    def begin(self, delay=False):
        """Fills every buffer, waits for the fills, then queues the delay kernel and the event behind it."""
        import torch
        with torch.cuda.stream(self.s):
            for b in self.inputs + self.outputs:
                b.reset()
        self.s.synchronize()
        self.after_delay = self.first_seen_done = None
        if delay:
            with torch.cuda.stream(self.s):
                torch.cuda._sleep(delay_cycles())
                self.after_delay = torch.cuda.Event()
                self.after_delay.record(self.s)

    def issue(self, call):
        import torch
        with torch.cuda.stream(self.s):
            call.issue()
        if self.after_delay is not None and self.first_seen_done is None and self.after_delay.query():
            self.first_seen_done = call.name

    def end(self, no_wait=False):
        """``no_wait``: the host must have come here while the delay kernel was still running."""
        if no_wait:
            assert self.after_delay is not None
            assert self.first_seen_done is None and not self.after_delay.query(), (
                "the host waited for the stream: the event behind the delay kernel was first seen complete after "
                f"{self.first_seen_done or 'the last call'}")

    def run(self, order, delay=False, no_wait=False):
        self.begin(delay)
        for c in order:
            self.issue(c)
        self.end(no_wait)

    def finish(self, expect=None, calls=None, label=""):
        """The one check (``expect``: the error code a queue plants on purpose, reported once), then every call's results
        (``label``: which pass this is, for the failure message)."""
        if expect is None:
            self.ws.check()
        else:
            try:
                self.ws.check()
            except self.sm.MinimizerError as e:
                assert e.code == expect, e
            else:
                raise AssertionError(f"mm_workspace_check returned MM_OK, {expect} was planted")
            self.ws.check()
        wrong = []
        for c in (self.calls if calls is None else calls):
            if c.verify is not None:
                try:
                    c.verify()
                except AssertionError as e:
                    wrong.append(f"{c.name}: {str(e)[:300]}")
        assert not wrong, f"{label}{len(wrong)} call(s) with wrong results:\n" + "\n".join(wrong)


def check_positions(name, out, count, want, cap=None, fill=-7):
    """``count`` (an Output of one uint64) holds len(want); ``out[:min(count, cap)]`` are the oracle's; everything behind
    them, slack included, is untouched."""
    got, cnt = out.host(), count.host()
    assert int(cnt[0]) == len(want), (name, "count", int(cnt[0]), len(want))
    assert (cnt[1:] == -7).all(), (name, "the count word's neighbours were written")
    m = len(want) if cap is None else min(len(want), cap)
    assert np.array_equal(got[:m].view(np.uint32), np.asarray(want[:m], dtype=np.uint32)), (name, "positions")
    assert (got[m:] == fill).all(), (name, "written at or past the count")


def check_exact(name, out, want, what="values"):
    """``out[:len(want)]`` equals ``want`` (compared as raw bits), the rest is untouched."""
    got = out.host()
    want = np.ascontiguousarray(want)
    head = got[: len(want)]
    assert np.array_equal(head.view(want.dtype) if head.dtype.itemsize == want.dtype.itemsize else head, want), (name, what)
    assert (got[len(want):] == out.fill).all(), (name, what, "written past the end")
