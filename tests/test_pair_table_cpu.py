"""The pair table of the fixed-k canonical walk (canonical k=21 w=11; DESIGN.md 4.1 "Pair look-ups"): the walk looks its
rolling-hash contributions up two bases at a time, from a 256-entry table indexed by two consecutive bases of each stream.
mm_debug_pair_table makes the table on the host with the function the kernel's threads run; here it is compared with a
restatement from the one-base table, two one-base steps are compared with the pair step, and the launch geometry is checked:
the table is 4 KB of static LDS, and the default lanes of the launches that take that kernel have to leave room for it four
times per CU, while every other flavour keeps the lanes it had.  No GPU."""
import ctypes as C

import numpy as np

K, W = 21, 11
M32 = 0xFFFFFFFF
PAIR_TABLE_BYTES = 256 * 16
STATIC_ALLOWANCE = 512  # the kernel's hash tables and counters (tests/test_abi.py budgets the same)


def _rotl(x, r):
    r &= 31
    return ((x << r) | (x >> (32 - r))) & M32 if r else x


def _rotr(x, r):
    return _rotl(x, 32 - (r & 31))


def _t_in_out(h, k):
    """The one-base table of the walk, index (out << 2) | in -> (fw, rc) contribution of a step that takes base `in` into
    the k-mer and drops base `out` (the header's formulas for h_fw / h_rc, the constant XOR terms folded in)."""
    R = h.rot & 31
    df, dr = _rotl(h.fw_xor, R) ^ h.fw_xor, _rotr(h.rc_xor, R) ^ h.rc_xor
    t = []
    for out in range(4):
        for inn in range(4):
            fw = h.fw[inn] ^ _rotl(h.fw[out], (R * k) & 31) ^ df
            rc = _rotl(h.rc[inn], (R * (k - 1)) & 31) ^ _rotr(h.rc[out], R) ^ dr
            t.append((fw, rc))
    return t


def _hashers(sm):
    rng = np.random.default_rng(2112)
    hs = [("nt", sm.NtHasher(K, True))]
    for rot in (1, 5, 16, 31):
        fw, rc = rng.integers(0, 1 << 32, 4, dtype=np.uint64), rng.integers(0, 1 << 32, 4, dtype=np.uint64)
        hs.append((f"random rot={rot}", sm.Hasher.from_tables(fw, rc, rot=rot, canonical=True,
                                                              fw_xor=int(rng.integers(0, 1 << 32)), rc_xor=int(rng.integers(0, 1 << 32)))))
    return hs


def _table(sm, h):
    out = (C.c_uint32 * 1024)()
    sm._check(sm.lib().mm_debug_pair_table(C.byref(h), out))
    return np.frombuffer(out, dtype=np.uint32).reshape(256, 4).copy()


def test_entries_restate_the_one_base_table(sm):
    L = sm.lib()
    assert "mm_debug_pair_table" in sm.EXPORTED_SYMBOLS
    assert L.mm_debug_pair_table(None, (C.c_uint32 * 1024)()) == sm.ERR["NULL"]
    for name, h in _hashers(sm):
        t, got = _t_in_out(h, K), _table(sm, h)
        for idx in range(256):
            in4, out4 = idx & 15, idx >> 4
            t1 = t[((out4 & 3) << 2) | (in4 & 3)]
            t2 = t[((out4 >> 2) << 2) | (in4 >> 2)]
            want = (t1[0], t1[1], _rotl(t1[0], h.rot) ^ t2[0], _rotr(t1[1], h.rot) ^ t2[1])
            assert tuple(int(x) for x in got[idx]) == want, (name, idx)


def test_two_one_base_steps_equal_the_pair_step(sm):
    rng = np.random.default_rng(7)
    for name, h in _hashers(sm):
        t, tab = _t_in_out(h, K), _table(sm, h)
        R = h.rot & 31
        for idx in range(256):
            in4, out4 = idx & 15, idx >> 4
            e = [int(x) for x in tab[idx]]
            for fw0, rc0 in [(0, 0), (M32, M32)] + [tuple(int(x) for x in rng.integers(0, 1 << 32, 2, dtype=np.uint64)) for _ in range(6)]:
                a = t[((out4 & 3) << 2) | (in4 & 3)]
                b = t[((out4 >> 2) << 2) | (in4 >> 2)]
                fw1, rc1 = _rotl(fw0, R) ^ a[0], _rotr(rc0, R) ^ a[1]
                fw2, rc2 = _rotl(fw1, R) ^ b[0], _rotr(rc1, R) ^ b[1]
                # the pair step: the even step from the entry's first half, the odd one from the state the even one started from
                assert (_rotl(fw0, R) ^ e[0], _rotr(rc0, R) ^ e[1]) == (fw1, rc1), (name, idx)
                assert (_rotl(fw0, 2 * R) ^ e[2], _rotr(rc0, 2 * R) ^ e[3]) == (fw2, rc2), (name, idx)


def _geometry(sm, w, canonical, mode, n_windows):
    L = sm.lib()
    out2, out7 = (C.c_uint64 * 2)(), (C.c_uint64 * 7)()
    nw = (C.c_uint64 * 1)(n_windows)
    sm._check(L.mm_debug_launch_lds(w, canonical, mode, nw[0], out2))
    sm._check(L.mm_debug_launch_plan(w, canonical, mode, 0, nw, out7, None, None, None, 0, None))
    return int(out7[0]), int(out2[0]), int(out2[1])


def test_lanes_leave_room_for_the_table_four_times_per_cu(sm):
    """canonical k=21 w=11, minimizers, sequence mode (the planner's stand-in plan has k = 21): lists + static LDS <= 40 960
    bytes, a quarter of the CU's 160 KB - with and without ambiguity bits, which take the same kernel."""
    assert sm.lib().mm_debug_fixed_k_kernel(K, W, 1) == 1
    for mode in (0, 4):
        nblk, lists, landing = _geometry(sm, W, 1, mode, 3 * 10**9)
        assert landing == 0
        assert lists + PAIR_TABLE_BYTES + STATIC_ALLOWANCE <= 40_960, (mode, nblk, lists)
        assert nblk == 26 and lists == 69 * 2 * 258, (mode, nblk, lists)  # 69 entries, rows of 258 16-bit slots
        # a shorter run's lanes were below the bound already
        assert _geometry(sm, W, 1, mode, 50_000_000) == (17, 24768, 0)


# (w, canonical, mode, windows) -> (blocks per lane, bytes of the lists, bytes of the landing area), recorded from the build
# before the pair table: no other flavour's geometry moves
PARENT_GEOMETRY = {
    (11, 0, 0, 3 * 10**9): (22, 15600, 0), (11, 1, 3, 3 * 10**9): (28, 38184, 0), (11, 1, 1, 3 * 10**9): (26, 38700, 0),
    (11, 0, 2, 3 * 10**9): (22, 9360, 0), (9, 1, 0, 3 * 10**9): (29, 38700, 0), (13, 1, 0, 3 * 10**9): (28, 38700, 0),
    (19, 1, 0, 3 * 10**9): (27, 38184, 0), (25, 1, 0, 3 * 10**9): (21, 30960, 0), (31, 1, 4, 3 * 10**9): (12, 19608, 0),
    (51, 1, 0, 3 * 10**9): (27, 39216, 0), (51, 1, 4, 3 * 10**9): (27, 39216, 13312), (7, 0, 0, 3 * 10**9): (23, 15600, 0),
    (11, 0, 0, 50_000_000): (17, 12480, 0), (11, 1, 3, 50_000_000): (17, 24768, 0), (13, 1, 0, 50_000_000): (14, 21156, 0),
    (51, 1, 4, 50_000_000): (6, 11868, 13312),
}


def test_other_flavours_keep_their_geometry(sm):
    for (w, canonical, mode, nw), want in PARENT_GEOMETRY.items():
        assert _geometry(sm, w, canonical, mode, nw) == want, (w, canonical, mode, nw)
