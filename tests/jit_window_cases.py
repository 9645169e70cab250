"""Window sizes 34 .. 128 without a prebuilt kernel: what tests/test_jit_windows_cpu.py and tests/test_gpu_jit_windows.py
share - which sizes those are (from the library), the kernel's compile-time choices per size (from the library:
mm_debug_walk_traits), the class representatives, and the inputs.

Every w <= 128 without a prebuilt instance is a kernel of its own, compiled with hiprtc at first use from a source that
branches on W at compile time (wide loads, view words, the strand vote, the skip-ambiguous landing area, ...).  The GPU file
runs EVERY such size with minimizers on both strands, and every other flavour at one size per distinct combination of those
branches (REPS).  Nothing here touches a device."""
import math

import numpy as np

from test_long_w_cpu import feasible, pack_at, plan_k, tie_heavy_codes  # noqa: F401 (re-exported to the two test files)

W_LO, W_HI = 34, 128
K_MAIN = 21   # (canonical plans: plan_k moves it to 22 where l would be even)
SENTINEL = -7

# One window size per distinct tuple of walk traits over the sizes of jit_windows() (tests/test_jit_windows_cpu.py checks
# that against the library); odd wherever its class has an odd member, so that open syncmers apply.  The classes: up to 35
# | 36, 37 (no lazy vote, chunked window bits of 8 rows) | 38 .. 47 (11 rows) | 48 | 49 .. 54 (four view words, five-dword
# wide loads, shallower table look-ahead) | 55 .. 63 (16 rows) | 64 | 65 .. 79 (no wide loads, no landing area, shift 7) |
# 80 | 81 .. 95 | 96 | 97 .. 111 (four words of ambiguity bits) | 112 | 113 .. 127 | 128 (shift 8).
REPS = [35, 37, 43, 48, 53, 59, 64, 71, 80, 87, 96, 105, 112, 121, 128]

# The flavours tests/test_gpu_jit_windows.py runs: name -> (mode, super-k-mer indices, reads mode, skip-ambiguous walk).
KINDS = {
    "minimizers": (0, False, False, False),
    "closed syncmers": (1, False, False, False),
    "open syncmers": (2, False, False, False),
    "super-k-mers": (0, True, False, False),          # (sequence mode and the batch call)
    "reads": (0, False, True, False),                 # (fixed stride and the lane table)
    "reads super-k-mers": (0, True, True, False),
    "reads closed syncmers": (1, False, True, False),
    "skip-ambiguous": (0, False, False, True),
    "skip-ambiguous closed syncmers": (1, False, False, True),
    "skip-ambiguous reads": (0, False, True, True),
}
# MM_TRAIT_LAST_VIEW_BASES is no branch: it takes every value within one combination of the others and names the edge a
# window size sits at (w = 49 and w = 65 have one base there).  That is why test_every_window_size runs every size.
NOT_A_CLASS = ("last_view_bases",)


def jit_windows(sm):
    """Every w in 34 .. 128 that mm_prebuilt_window_sizes does not list (the same on both strands: asserted)."""
    pre = set(sm.prebuilt_window_sizes(True))
    assert pre == set(sm.prebuilt_window_sizes(False))
    return [w for w in range(W_LO, W_HI + 1) if w not in pre]


def walk_class(sm, w, canonical, kind):
    """The trait tuple of one flavour at one window size, without the field that is no branch."""
    mode, sk, reads, amb = KINDS[kind]
    t = sm.walk_traits(w, canonical, mode, sk, reads, amb)
    return tuple(t[f] for f in sm.WALK_TRAITS if f not in NOT_A_CLASS)


def tie_input(w, k, extra=60_000):
    """The tie-heavy codes of one window size: l + `extra` bases (tests/test_long_w_cpu.py::tie_heavy_codes: A / G only up
    to base 20 000, C / T only from 24 000, a homopolymer from 38 000 to 44 000, per 50 000 bases)."""
    return tie_heavy_codes(k + w - 1 + extra, 9000 + w)


def tied_windows(oracle, packed, n, k, w, base_offset=0):
    """Windows whose minimum - the upper 16 bits of the canonical hash, what the kernel and the oracle compare - is taken by
    two or more of their k-mers: there the strand vote decides which one is the minimizer."""
    h = oracle.hash_kmers(packed, n, k, oracle.default_hasher(True), base_offset=base_offset) >> 16
    v = np.lib.stride_tricks.sliding_window_view(h[: n - k + 1], w)
    return int(((v == v.min(axis=1, keepdims=True)).sum(axis=1) >= 2).sum())


def offsets_for_every_residue(S):
    """Base offsets such that offset + lane * S takes all 16 residues mod 16 (hence all 4 byte phases) over the lanes of a
    tile: lane * S runs through the multiples of gcd(S, 16)."""
    return list(range(math.gcd(S, 16)))


def lane_start_residues(offsets, S, lanes=256):
    return {(o + j * S) % 16 for o in offsets for j in range(lanes)}


_CHILD_WS = []


def prepare_one(k, w, canonical, mode, sequence, reads, sk):
    """In a worker process: Builder.prepare of one plan - compiles what is missing, which leaves the code object in the
    library's disk cache (where it has one), and launches nothing."""
    try:
        import simd_minimizers_amd as sm
        if not _CHILD_WS:
            _CHILD_WS.append(sm.Workspace(0))
        b = sm.Builder(plan_k(k, w, canonical), w, canonical, mode)
        return b.prepare(ws=_CHILD_WS[0], sequence=sequence, reads=reads, super_kmers=sk)
    except Exception as e:  # noqa: BLE001 (reported as text: the library's exception does not survive pickling)
        return f"{type(e).__name__}: {e}"


def prepare_ahead(jobs, workers=8):
    """A cold hiprtc compile of a kernel for w = 34 .. 128 takes 0.7 s (forward, w = 35) to 4.4 s (canonical, w = 128), the
    GPU files need some 350 of them, and compiles from several THREADS of one process do not overlap (measured: 8 threads,
    8 kernels, 24 s - hiprtc serialises them).  So up to `workers` fresh worker processes (spawned, never forked) prepare
    the jobs in order, each with a workspace of its own; the test process then finds the code objects in the library's disk
    cache.  Only the time depends on it: with the cache off or a worker lost, a kernel is compiled at its first launch as
    for any caller - which is why wait() ignores what the workers report.  Returns (pool, futures in the order of the jobs)."""
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    pool = ProcessPoolExecutor(max_workers=workers, mp_context=multiprocessing.get_context("spawn"))
    return pool, [pool.submit(prepare_one, *job) for job in jobs]


def wait(futures):
    """Until the workers are done with these jobs, whatever became of them."""
    for f in futures:
        try:
            f.result()
        except Exception:  # noqa: BLE001 (a lost worker costs time, nothing else)
            pass
