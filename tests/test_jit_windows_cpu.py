"""Window sizes 34 .. 128 without a prebuilt kernel, on the CPU: the class representatives of tests/jit_window_cases.py
cover every combination of the kernel's compile-time choices (read from the library: mm_debug_walk_traits), and the oracle
that judges those kernels in tests/test_gpu_jit_windows.py is pinned at every one of the sizes first - its streaming flavour
equals its naive flavour (a plain argmin per window) on the input where the strand vote decides.  tests/test_oracle.py pins
the oracle at small w, tests/test_long_w_cpu.py above 128."""
import ctypes as C

import numpy as np
import pytest

import jit_window_cases as jw


def test_jit_window_sizes_come_from_the_library(sm):
    """ALL is what mm_prebuilt_window_sizes leaves of 34 .. 128; the representatives are among them."""
    all_w = jw.jit_windows(sm)
    assert all_w and 34 in all_w and 128 in all_w
    assert len(jw.REPS) == 15 and jw.REPS == sorted(set(jw.REPS)) and set(jw.REPS) <= set(all_w)


def test_walk_traits_export(sm):
    """mm_debug_walk_traits against the rules as mm_fused_impl.h states them in words, at sizes on both sides of each."""
    L = sm.lib()
    assert L.mm_debug_walk_traits(0, 1, 0, 0, 0, 0, None, 0) == 0 and L.mm_debug_walk_traits(40, 1, 3, 0, 0, 0, None, 0) == 0
    assert L.mm_debug_walk_traits(40, 1, 0, 0, 0, 0, None, 0) == len(sm.WALK_TRAITS)
    buf = (C.c_uint32 * 3)(9, 9, 9)   # a short buffer takes the first values only
    assert L.mm_debug_walk_traits(40, 1, 0, 0, 0, 0, buf, 2) == len(sm.WALK_TRAITS) and buf[2] == 9 and buf[1] in (4, 5)
    t = lambda w, c=True, m=0, sk=False, r=False, a=False: sm.walk_traits(w, c, m, sk, r, a)
    for w in range(1, 129):
        x = t(w)
        assert x["view_words"] == -(-w // 16) and x["last_view_bases"] == w - 16 * (x["view_words"] - 1) + 1
        assert t(w, False)["last_view_bases"] == x["last_view_bases"] - 1
        assert x["v2_load"] == (w % 16 == 0) and t(w, False)["v2_load"] == 0
        assert (x["wide_group_blocks"] == 0) == (w % 16 == 0 or w >= 64) or w < 16, (w, x)
        assert x["wide_dwords"] in (4, 5) and x["two_bodies"] == (w <= 12) and x["one_stream"] == 0
        assert x["sk_shift"] == 0 and t(w, sk=True)["sk_shift"] == w.bit_length() and t(w, m=1, sk=True)["sk_shift"] == 0
        assert x["amb_view_words"] == 1 and t(w, a=True)["amb_view_words"] == -(-w // 32)
        assert x["lazy_vote"] == (w not in (36, 37)) and t(w, False)["lazy_vote"] == 0
        assert t(w, False)["entry8"] == (w <= 13) and t(w, False, r=True)["entry8"] == 0 and x["entry8"] == 0
        a = t(w, a=True)
        assert a["ambi_land"] == (32 <= w <= 96 and x["wide_group_blocks"] != 0) and x["ambi_land"] == 0
        assert a["ambi_rows"] == (a["ambi_land"] and w >= 36)
        assert a["amb_row_dwords"] == (0 if not a["ambi_rows"] else 8 if w <= 37 else 11 if w <= 54 else 16)
    assert t(47)["table_prefetch"] == 2 and t(48)["table_prefetch"] == 1 and t(48, False)["table_prefetch"] == 12
    # the comment at wide_group_blocks_nd: w = 49 has one base (and the strand window's) in its last view, and needs the fifth dword
    assert t(49)["last_view_bases"] == 2 and t(49)["wide_dwords"] == 5 and t(49)["wide_group_blocks"] == 1
    assert t(65)["last_view_bases"] == 2 and t(65)["wide_group_blocks"] == 0
    assert t(11)["wide_group_blocks"] == 4 and t(51)["wide_group_blocks"] == 1


def test_representatives_cover_every_class(sm):
    """Every trait tuple over the library's own list of sizes, per flavour of tests/test_gpu_jit_windows.py::test_flavours and
    strand, is the tuple of a representative; the representatives are one per class.  A rule that changes
    (MM_AMBI_ROWS_MINW, another wide-load width) shows here as a class without a representative until REPS follows."""
    all_w = jw.jit_windows(sm)
    for kind in jw.KINDS:
        for canonical in (False, True):
            if jw.KINDS[kind][3] and not canonical:
                continue  # (the skip-ambiguous calls are canonical)
            have = {jw.walk_class(sm, w, canonical, kind) for w in jw.REPS}
            missing = [w for w in all_w if jw.walk_class(sm, w, canonical, kind) not in have]
            assert not missing, (kind, canonical, missing)
    whole = lambda w: tuple(jw.walk_class(sm, w, c, kind) for kind in jw.KINDS for c in (False, True))
    classes = {whole(w) for w in all_w}
    assert len(classes) == len(jw.REPS) == len({whole(w) for w in jw.REPS}), len(classes)
    # odd wherever the class has an odd member: open syncmers apply
    for r in jw.REPS:
        members = [w for w in all_w if whole(w) == whole(r)]
        assert r % 2 == 1 or all(w % 2 == 0 for w in members), (r, members)


def _jit_window_ids():
    import simd_minimizers_amd as sm
    return jw.jit_windows(sm)


@pytest.mark.parametrize("w", _jit_window_ids())
def test_oracle_streaming_equals_naive(oracle, w):
    """l + 60 000 tie-heavy bases (the input of the GPU tests): both strands where l is odd, every mode w admits, the
    super-k-mer indices of minimizers; and the vote decides in at least 1 000 windows of the canonical input."""
    done = 0
    for canonical in (False, True):
        k = jw.plan_k(jw.K_MAIN, w, canonical)
        n = k + w - 1 + 60_000
        packed = jw.pack_at(jw.tie_input(w, k))
        h = oracle.default_hasher(canonical)
        if canonical:
            assert jw.tied_windows(oracle, packed, n, k, w) >= 1000
        for mode in (0, 1, 2):
            if not jw.feasible(k, w, canonical, mode):
                continue
            if mode == 0:
                wp, wsk = oracle.run(packed, n, k, w, h, canonical, mode, flavour=oracle.NAIVE, super_kmers=True)
                gp, gsk = oracle.run(packed, n, k, w, h, canonical, mode, flavour=oracle.STREAMING, super_kmers=True)
                assert len(wp) >= 100 and np.array_equal(gp, wp) and np.array_equal(gsk, wsk), (w, canonical)
                assert np.array_equal(oracle.run(packed, n, k, w, h, canonical, mode), gp), (w, canonical)
                assert np.all(np.diff(wsk.astype(np.int64)) > 0) and wsk[0] == 0 and wsk[-1] <= 60_000
            else:
                want = oracle.run(packed, n, k, w, h, canonical, mode, flavour=oracle.NAIVE)
                got = oracle.run(packed, n, k, w, h, canonical, mode, flavour=oracle.STREAMING)
                assert np.array_equal(got, want) and len(want) >= (100 if mode == 1 else 1), (w, canonical, mode, len(want))
            done += 1
    assert done == 2 * (2 + w % 2)
