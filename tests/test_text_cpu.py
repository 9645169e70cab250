"""CPU checks of the byte-text path (``&[u8]`` input, src/lib.rs:59): the numpy checker pinned to the oracle, the text
plan's validation, the text hashers' tables, and the Python dispatch of byte input up to the C call."""
import ctypes as C

import numpy as np
import pytest

import text_checker as tc


def _dna_text_hasher(sm, oracle, canonical):
    fw, rc = tc.text_tables_from_dna(oracle.default_hasher(canonical))
    return sm.TextHasher.from_tables(fw, rc, rot=7, canonical=canonical)


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_checker_equals_oracle_on_code_bytes(sm, oracle, canonical, mode):
    """The checker on the code bytes 0..3 with fw[c] = nt.fw[c & 3] equals the oracle's naive flavour on the same codes
    packed: hash, tie rules, strand vote (c & 2), collectors and super-k-mer indices."""
    rng = np.random.default_rng(7 + mode + 10 * canonical)
    n = 20_000
    codes = rng.integers(0, 4, n, dtype=np.uint8)
    codes[5000:5600] = 1  # a low-complexity stretch: ties everywhere
    codes[9000:9600:2] = 2
    packed = tc.pack_codes(codes)
    th = _dna_text_hasher(sm, oracle, canonical)
    for k, w in [(1, 1), (1, 6), (5, 7), (5, 11), (21, 11), (31, 5), (19, 19), (63, 3), (4, 34)]:
        if canonical and (k + w - 1) % 2 == 0:
            continue
        if mode == 2 and w % 2 == 0:
            continue
        want = oracle.run(packed, n, k, w, oracle.default_hasher(canonical), canonical, mode, flavour=oracle.NAIVE)
        got = tc.run(codes, k, w, th, canonical, mode)
        assert np.array_equal(got, want), (k, w)
        if mode == 0:
            wp, wsk = oracle.run(packed, n, k, w, oracle.default_hasher(canonical), canonical, mode,
                                 flavour=oracle.NAIVE, super_kmers=True)
            gp, gsk = tc.run(codes, k, w, th, canonical, mode, super_kmers=True)
            assert np.array_equal(gp, wp) and np.array_equal(gsk, wsk), (k, w)


def test_checker_xor_constants_match_oracle(sm, oracle):
    """Nonzero fw_xor / rc_xor (the AntiLexHasher form): the checker's hash equals the oracle's on code bytes."""
    n, k = 5000, 9
    codes = np.random.default_rng(3).integers(0, 4, n, dtype=np.uint8)
    h = oracle.antilex_hasher(k, True)
    th = sm.TextHasher.from_tables(*tc.text_tables_from_dna(h), rot=h.rot, canonical=True, fw_xor=h.fw_xor,
                                   rc_xor=h.rc_xor)
    assert np.array_equal(tc.hashes(codes, k, th), oracle.hash_kmers(tc.pack_codes(codes), n, k, h))


def test_text_plan_validation(sm):
    E = sm.ERR
    cases = [
        ((0, 5, False, 0), E["K_ZERO"]),
        ((5, 0, False, 0), E["W_ZERO"]),
        ((5, 1 << 15, False, 0), E["W_TOO_LARGE"]),
        ((5, 6, True, 0), E["EVEN_L"]),
        ((5, 6, False, 2), E["OPEN_EVEN_W"]),
        ((5, 7, False, 3), E["BAD_MODE"]),
    ]
    for (k, w, canon, mode), code in cases:
        with pytest.raises(sm.MinimizerError) as e:
            sm.Plan(k, w, canon, mode, None, text=True)
        assert e.value.code == code, (k, w, canon, mode)
    with pytest.raises(sm.MinimizerError) as e:
        sm.Plan(5, 7, True, 0, sm.TextMulHasher(5, canonical=False), text=True)
    assert e.value.code == E["HASHER_NOT_CANONICAL"]
    assert sm.Plan(5, 7, True, 0, None, text=True).value_len() == 5
    assert sm.Plan(5, 7, True, 1, sm.TextMulHasher(5), text=True).value_len() == 11


def test_text_plan_refused_by_packed_entry_points(sm):
    """A text plan passed to a packed entry point returns MM_ERR_BAD_MODE before anything else is looked at."""
    L = sm.lib()
    p = sm.Plan(5, 7, False, 0, None, text=True)
    cnt = C.c_uint64()
    assert L.mm_run_host(p.h, None, None, 0, 0, None, None, 0, C.byref(cnt)) == sm.ERR["BAD_MODE"]
    assert L.mm_run_device(p.h, None, None, 0, 0, 0, 0, 0, None, None, 0, C.byref(cnt)) == sm.ERR["BAD_MODE"]
    assert L.mm_run_host_ascii(p.h, None, None, 0, None, None, 0, C.byref(cnt)) == sm.ERR["BAD_MODE"]


def test_text_hasher_from_dna_tables(sm):
    for canon in (False, True):
        nt = sm.NtHasher(21, canon)
        th = sm.TextHasher.from_dna(nt)
        for c in range(256):
            assert th.fw[c] == nt.fw[(c >> 1) & 3] and th.rc[c] == nt.rc[(c >> 1) & 3], c
        assert (th.rot, th.canonical, th.fw_xor, th.rc_xor, th.kind) == (nt.rot, nt.canonical, nt.fw_xor, nt.rc_xor,
                                                                          nt.kind)
        # ASCII DNA maps onto the packed codes A0 C1 T2 G3, either case
        for i, ch in enumerate(b"ACTG"):
            assert th.fw[ch] == nt.fw[i] and th.fw[ch | 0x20] == nt.fw[i]


def test_text_mul_hasher_tables(sm):
    comp = {ord(a): ord(b) for a, b in zip("ACGTacgt", "TGCAtgca")}
    for canon in (False, True):
        h = sm.TextMulHasher(21, canon)
        assert h.canonical == int(canon) and h.rot == 7 and h.fw_xor == h.rc_xor == 0
        for c in range(256):
            assert h.fw[c] == (c * 0x9E3779B1) & 0xFFFFFFFF
            assert h.rc[c] == (comp.get(c, c) * 0x9E3779B1) & 0xFFFFFFFF


class _RecordingLib:
    """The real library, with the text entry point replaced by a recorder."""

    def __init__(self, real):
        self._real = real
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def mm_run_text_host(self, plan, ws, text, n, pos, sk, cap, cnt):
        self.calls.append((plan, ws, bytes(C.string_at(text, n)) if n else b"", n, cap, sk is not None))
        return 0


class _FakeWorkspace:
    h = C.c_void_p(0x1234)


@pytest.mark.parametrize("kind", ["bytes", "bytearray", "numpy"])
def test_builder_dispatches_bytes_to_the_text_entry_point(sm, monkeypatch, kind):
    rec = _RecordingLib(sm.lib())
    monkeypatch.setattr(sm, "lib", lambda: rec)
    raw = bytes(range(256)) * 3
    seq = {"bytes": raw, "bytearray": bytearray(raw), "numpy": np.frombuffer(raw, dtype=np.uint8)}[kind]
    b = sm.minimizers(5, 11).workspace(_FakeWorkspace())
    assert b.run_once(seq) == []
    sk = []
    b.super_kmers(sk).run(seq, [])
    assert len(rec.calls) == 2
    plan, ws, text, n, cap, has_sk = rec.calls[0]
    assert text == raw and n == len(raw) and cap == len(raw) - 15 + 1 and not has_sk
    assert rec.calls[1][5]
    # a TextHasher goes to the text plan, the packed plan keeps its hasher
    th = sm.TextMulHasher(5, canonical=True)
    b2 = sm.canonical_minimizers(5, 11).hasher(th).workspace(_FakeWorkspace())
    assert b2._text_hasher is th and b2._hasher is None
    b2.run_once(seq)
    assert len(rec.calls) == 3
