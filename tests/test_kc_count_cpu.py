"""The strand count of a tied window in the fixed-k canonical walk (DESIGN.md 4.1 "lazy vote"): that walk keeps no running
count, it counts the window's T|G bases from its two sequence buffers through a compile-time plan (kc_count_plan in
mm_fused_impl.h).  mm_debug_kc_count runs the same plan on the host over buffers built as a lane builds them; here it is
compared with a direct count of the window's bases.  No GPU."""
import ctypes as C

import numpy as np

K, W = 21, 11
GROUP_BLOCKS = 4  # blocks of w = 11 that share one 16-byte load (mm_debug_walk_traits: wide_group_blocks)


def _kc_count(L, w, k, kn, jj, group, data, lane_base):
    c = C.c_uint32(0xdeadbeef)
    r = L.mm_debug_kc_count(w, k, kn, jj, group, data.ctypes.data_as(C.POINTER(C.c_uint8)), len(data), lane_base, C.byref(c))
    return r, c.value


def _tg(data, first, n):
    """T|G bases (the high bit of a 2-bit code) among bases [first, first + n) of packed bytes; 0 past their end"""
    j = np.arange(first, first + n)
    byte = j >> 2
    code = np.where(byte < len(data), (data[np.minimum(byte, len(data) - 1)] >> (2 * (j & 3))) & 3, 0)
    return int(((code >> 1) & 1).sum())


def test_the_rule_holds_for_the_headline_and_only_inside_kc_rule(sm):
    L = sm.lib()
    assert sm.walk_traits(W, True)["wide_group_blocks"] == GROUP_BLOCKS
    r, _ = _kc_count(L, W, K, 0, 0, 0, np.zeros(64, dtype=np.uint8), 0)
    assert r == 7, r  # one load stream, a count plan, and the count was written
    assert L.mm_debug_kc_count(W, K, 0, 0, 0, None, 0, 0, None) == 3
    # kc_rule false -> kc_count_rule false, over every (w, k) up to 64
    for w in range(1, 65):
        for k in range(1, 65):
            r = L.mm_debug_kc_count(w, k, 0, 0, 0, None, 0, 0, None)
            assert r in (0, 1, 3), (w, k, r)
    assert L.mm_debug_kc_count(51, 31, 0, 0, 0, None, 0, 0, None) == 0
    # out of the plan's range: nothing is written
    data = np.zeros(64, dtype=np.uint8)
    for kn, jj, base in ((GROUP_BLOCKS, 0, 0), (0, W, 0), (0, 0, -2)):
        r, c = _kc_count(L, W, K, kn, jj, 0, data, base)
        assert r == 3 and c == 0xdeadbeef, (kn, jj, base, r)


def test_plan_counts_the_window_at_every_step_and_alignment(sm):
    """every kn, every jj, every lane base position modulo 16 (byte part x bit part of the loads), the lane whose element 0 is
    the base before the buffer, the first load group (whose earlier buffer the warm-up fills) and a later one; random bytes
    with the bytes behind the data reading 0"""
    L = sm.lib()
    rng = np.random.default_rng(11)
    l = K + W - 1
    checked = 0
    for trial in range(3):
        data = rng.integers(0, 256, size=(96, 44, 40)[trial], dtype=np.uint8)
        for group in (0, 1, 2):
            for base in [-1] + list(range(0, 16)) + list(range(37, 53)):
                for kn in range(GROUP_BLOCKS):
                    for jj in range(W):
                        r, c = _kc_count(L, W, K, kn, jj, group, data, base)
                        first = base + (kn + group * GROUP_BLOCKS) * W + jj + 1
                        assert r == 7 and c == _tg(data, first, l), (trial, group, base, kn, jj, c)
                        checked += 1
    assert checked == 3 * 3 * 33 * GROUP_BLOCKS * W
    # all-T|G and no-T|G bytes: the plan's pieces cover every base of the window once
    for byte, want in ((0xAA, l), (0xFF, l), (0x55, 0), (0x00, 0)):
        data = np.full(96, byte, dtype=np.uint8)
        for kn in range(GROUP_BLOCKS):
            for jj in range(W):
                for base in (-1, 0, 5, 14):
                    assert _kc_count(L, W, K, kn, jj, 1, data, base) == (7, want), (byte, kn, jj, base)
