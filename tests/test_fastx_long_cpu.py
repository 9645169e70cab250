"""FASTA records longer than a chunk (MM_FASTX_LONG_RECORDS), what needs no device: the split rule of csrc/mm_fastx_cut.h
(mm_debug_fastx_split, the function the trim kernel calls) against a plain Python restatement on generated texts, its
agreement with mm_debug_fastx_cut wherever the old rule decides, the new create-time refusal in its documented place, the
exported symbols, fastx_join on hand-made batches, and a sanitizer build of a stand-alone program over the header."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------- the rule restated
def split_py(text: bytes, l: int, last: bool):
    """The rule, plainly.  Returns (cut, T, open, overlap)."""
    n = len(text)
    if last:
        return n, 0, 0, 0
    lines, at = [], 0          # (start, end) of every line; end = the offset of its '\n', or n
    while at < n:
        e = text.find(b"\n", at)
        e = n if e < 0 else e
        lines.append((at, e))
        at = e + 1
    heads = [a for a, e in lines if e > a and text[a:a + 1] == b">"]
    if len(heads) >= 2 or (len(heads) == 1 and heads[0] > 0):
        return heads[-1], 0, 0, 0                      # the old rule: the last record is carried whole
    if not heads:
        cut = text.rfind(b"\n") + 1                    # no record: behind the last newline (0 if none)
        return cut, 0, 0, 0
    # one record, from the first byte on
    h = text.find(b"\n")
    if h < 0:
        return 0, 0, 0, 0                              # the header line is not complete: nothing is cut
    seq = [i for i in range(h + 1, n) if text[i] not in b"\r\n"]
    if l == 1:
        T, overlap = n, 0                              # nothing is repeated
    elif len(seq) >= l - 1:
        T, overlap = seq[len(seq) - (l - 1)], l - 1
    else:
        T, overlap = (seq[0] if seq else n), len(seq)
    return n, T, 1, overlap


def _record(rng, n_bases, width, nl=b"\n", header=b">chr1 test", blank_every=0, final_newline=True):
    s = rng.choice(list(b"ACGTN"), size=n_bases).astype(np.uint8).tobytes()
    out = bytearray(header + nl)
    if width == 0:
        out += s + nl
    else:
        for j, i in enumerate(range(0, len(s), width)):
            out += s[i:i + width] + nl
            if blank_every and j % blank_every == blank_every - 1:
                out += nl
    if not final_newline and out.endswith(nl):
        del out[-len(nl):]
    return bytes(out)


def _check(sm, text, l, last):
    got = sm.fastx_split(text, l, last)
    want = split_py(text, l, last)
    assert (got["cut"], got["T"], got["open"], got["overlap"]) == want, (text[:80], len(text), l, last, got, want)
    return got


def test_symbols_exported_and_declared(sm):
    L = sm.lib()
    header = open(os.path.join(HERE, "..", "include", "simd_minimizers_amd.h")).read()
    for name in ("mm_fastx_stream_pieces", "mm_debug_fastx_split"):
        assert hasattr(L, name) and name + "(" in header
    assert "MM_FASTX_LONG_RECORDS = 16" in header and sm.FASTX_LONG_RECORDS == 16
    assert C.sizeof(sm._FastxPiecesC) == 24


@pytest.mark.parametrize("nl", [b"\n", b"\r\n"])
@pytest.mark.parametrize("width", [1, 10, 60, 0])
def test_split_rule_on_every_prefix_of_a_record(sm, width, nl):
    """Every prefix of one record as a chunk (so chunks end in the header line, on a line end, between '\\r' and '\\n', in a
    sequence line), l from 1 to more bases than the record has: fewer than l - 1 bases, an overlap that would reach into
    the header line, line ends between the overlap's bases."""
    rng = np.random.default_rng(width + len(nl))
    text = _record(rng, 150 if width != 1 else 40, width, nl, blank_every=3 if width == 10 else 0)
    opens = 0
    for n in range(len(text) + 1):
        for l in (1, 2, 11, 31, 200):
            opens += _check(sm, text[:n], l, False)["open"]
            _check(sm, text[:n], l, True)
    assert opens > len(text)


def test_split_rule_small_cases(sm):
    f = lambda t, l=11, last=False: tuple(sm.fastx_split(t, l, last)[k] for k in ("cut", "T", "open", "overlap"))  # noqa: E731
    assert f(b"") == (0, 0, 0, 0)
    assert f(b">chr1") == (0, 0, 0, 0)                         # the header line is not complete
    assert f(b">chr1 a long header line without its end" * 3) == (0, 0, 0, 0)
    assert f(b">chr1\n") == (6, 6, 1, 0)                       # complete, no base yet: T = n
    assert f(b">chr1\n\n\r\n") == (9, 9, 1, 0)
    assert f(b">chr1\nACGT") == (10, 6, 1, 4)                  # fewer than l - 1 bases: the first sequence byte
    assert f(b">chr1\n\nACGT\n") == (12, 7, 1, 4)              # ... behind the blank line
    assert f(b">chr1\nACGTACGTACGTA") == (19, 9, 1, 10)
    assert f(b">chr1\nACGTACGTACG\nTA\n\n") == (22, 9, 1, 10)  # line ends are not counted
    assert f(b">chr1\nACGTACGTACG\r\nTA\r\n") == (23, 9, 1, 10)
    assert f(b">\nACGTACGTACGTA") == (15, 5, 1, 10)            # the synthetic header line of a continuing chunk
    assert f(b">\nACGTACGTAC") == (12, 2, 1, 10)               # exactly l - 1 bases: T stays behind the header line
    assert f(b">\nACGTACGTAC", l=12) == (12, 2, 1, 10)
    assert f(b">AAAAAAAAAAAAAAAAAAAA\nAC") == (24, 22, 1, 2)    # the overlap never reaches back into the header line
    assert f(b">chr1\nACGTACGTACGTA", last=True) == (19, 0, 0, 0)
    # the old rule decides: a second header, a record that does not start the chunk, no record
    assert f(b">chr1\nACGT\n>chr2\nAC") == (11, 0, 0, 0)
    assert f(b"GT\n>chr2\nACGTACGTACGTACGT") == (3, 0, 0, 0)
    assert f(b"ACGT\nACGT\nAC") == (10, 0, 0, 0)
    assert f(b"ACGTACGT") == (0, 0, 0, 0)
    assert sm.lib().mm_debug_fastx_split(None, 5, 11, 0, (C.c_uint64 * 4)()) == sm.ERR["NULL"]
    assert sm.lib().mm_debug_fastx_split(b"x", 1, 11, 0, None) == sm.ERR["NULL"]


def test_old_rule_decides_with_a_complete_record_in_front(sm):
    """Several records, every prefix that holds a complete record in front of its last header: the split call gives
    mm_debug_fastx_cut's cut and no piece; and for EVERY prefix, a piece is cut only where the old rule gives cut == 0."""
    rng = np.random.default_rng(5)
    text = b"".join(_record(rng, int(nb), 60, header=b">r%d" % i) for i, nb in enumerate([0, 1, 130, 59, 61, 300]))
    second = text.index(b">", 1)
    for n in range(len(text) + 1):
        chunk = text[:n]
        old = sm.fastx_cut(chunk, "fasta", False)
        new = _check(sm, chunk, 31, False)
        if old["cut"] > 0:
            assert (new["cut"], new["open"], new["T"], new["overlap"]) == (old["cut"], 0, 0, 0)
        else:
            assert new["cut"] in (0, n)
        if n > second + 1:
            assert old["cut"] > 0 and new["open"] == 0
        assert sm.fastx_split(chunk, 31, True)["cut"] == sm.fastx_cut(chunk, "fasta", True)["cut"] == n


def test_pieces_chain_reproduces_the_record(sm):
    """The stream's own use of the rule, on the host: chunk = ">\\n" + text[T, n) + the next new bytes.  Whatever the chunk
    size and line form, the bases of the pieces minus their overlaps are the record's bases, every piece but the first
    starts with the l - 1 bases in front of it, and every chunk brings new bases (the stream never spins)."""
    rng = np.random.default_rng(9)
    for width, nl in ((60, b"\n"), (1, b"\r\n"), (0, b"\n"), (7, b"\n")):
        text = _record(rng, 1000, width, nl, blank_every=5 if width == 7 else 0, final_newline=False)
        bases = bytes(c for c in text[text.index(b"\n") + 1:] if c not in b"\r\n")
        for l, C_ in ((11, 64), (11, 100), (31, 124), (16, 65)):
            got, carry, at, overlap_in = b"", b"", 0, 0
            while True:
                new = text[at:at + C_]
                at += len(new)
                chunk = carry + new
                last = at >= len(text)
                r = sm.fastx_split(chunk, l, last)
                seq = bytes(c for c in chunk[chunk.index(b"\n") + 1:] if c not in b"\r\n")
                assert seq[:overlap_in] == got[len(got) - overlap_in:]
                if not last:
                    assert r["open"] == 1 and r["cut"] == len(chunk) and len(seq) > overlap_in
                got += seq[overlap_in:]
                if last:
                    break
                carry = b">\n" + chunk[r["T"]:]
                overlap_in = r["overlap"]
                assert overlap_in == min(l - 1, len(seq)) and len(carry) <= C_ + 2
            assert got == bases


# ---------------------------------------------------------------- create-time refusals
def _plan(sm, k=21, w=11, canonical=0, mode=0):
    h = C.c_void_p()
    assert sm.lib().mm_plan_create(C.byref(h), k, w, canonical, mode, None) == 0
    return h


def test_the_new_refusal_stands_behind_the_old_ones_and_before_the_device(sm):
    L, E = sm.lib(), sm.ERR
    LONG, SK, SKIP, U64, U128 = sm.FASTX_LONG_RECORDS, sm.FASTX_SK, sm.FASTX_SKIP_AMBIGUOUS, sm.FASTX_VALUES_U64, sm.FASTX_VALUES_U128
    fwd = _plan(sm)                       # l = 31: 4 l = 124
    small = _plan(sm, k=5, w=7)           # l = 11: 4 l = 44 < 64, the old lower bound of chunk_bytes
    sync_fwd = _plan(sm, k=15, w=17, mode=1)
    wide = _plan(sm, w=129)

    def create(plan, flags, chunk_bytes, max_records=5, device=-1, fmt=0, slots=0):
        c = sm.FastxStreamConfig(device, fmt, flags, slots, chunk_bytes, max_records, 0, 0)
        h = C.c_void_p()
        r = L.mm_fastx_stream_create(C.byref(h), plan, C.byref(c))
        if r == 0:
            L.mm_fastx_stream_destroy(h)
        else:
            assert not h.value
        return r

    try:
        # the old refusals win, in their order, with the flag set and chunk_bytes too small for it
        assert create(fwd, LONG, 63) == E["LEN_TOO_LARGE"]
        assert create(fwd, LONG, 100, max_records=1 << 31) == E["LEN_TOO_LARGE"]
        assert create(sync_fwd, LONG | SK, 100) == E["BAD_MODE"]
        assert create(fwd, LONG | SKIP, 100) == E["HASHER_NOT_CANONICAL"]
        assert create(fwd, LONG | U64 | U128, 100) == E["BAD_MODE"]
        assert create(wide, LONG, 100) == E["BAD_MODE"]
        assert create(fwd, LONG, 100, fmt=3) == E["BAD_MODE"]
        assert create(fwd, LONG, 100, slots=9) == E["BAD_MODE"]
        assert create(fwd, LONG | 32, 100) == E["BAD_MODE"]           # (the next unknown flag)
        # the new one: before any device is asked for
        assert create(fwd, LONG, 100) == E["CAPACITY"]
        assert b"4 * (k + w - 1) = 124" in L.mm_last_error()
        assert create(fwd, LONG, 123) == E["CAPACITY"]
        assert create(fwd, LONG, 123, fmt=sm.FASTX_FASTQ) == E["CAPACITY"]   # (a property of the flag, whatever the text)
        assert create(fwd, LONG, 124) == E["NO_DEVICE"]
        assert create(small, LONG, 64) == E["NO_DEVICE"]
        assert create(fwd, 0, 100) == E["NO_DEVICE"]                  # (without the flag: as ever)
    finally:
        for h in (fwd, small, sync_fwd, wide):
            L.mm_plan_destroy(h)


def test_pieces_of_no_stream(sm):
    L, E = sm.lib(), sm.ERR
    p = sm._FastxPiecesC()
    assert L.mm_fastx_stream_pieces(None, C.byref(p)) == E["NULL"]


# ---------------------------------------------------------------- fastx_join
def _batch(rec_text_pos, lens, slices, first_continues=False, last_open=False, first_overlap=0, sk=False):
    b = types.SimpleNamespace()
    b.n_records = len(lens)
    b.rec_text_pos = np.array(rec_text_pos, dtype=np.uint64)
    b.rec_base = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    b.offsets = np.concatenate([[0], np.cumsum([len(s) for s in slices])]).astype(np.uint64)
    b.pos = np.array([x for s in slices for x in s], dtype=np.uint32)
    b.sk = b.pos + 1 if sk else None
    b.values = None
    b.u128 = False
    b.first_continues, b.last_open, b.first_overlap, b.first_base = first_continues, last_open, first_overlap, 0
    return b


def test_fastx_join_on_hand_made_batches(sm):
    batches = [
        _batch([0, 10], [5, 7], [[1], [2, 3]], sk=True),
        _batch([30], [100], [[4, 50]], last_open=True, sk=True),
        _batch([30], [110], [[120, 130]], first_continues=True, last_open=True, first_overlap=10, sk=True),
        _batch([30, 400], [10, 3], [[], [0]], first_continues=True, first_overlap=10, sk=True),
        _batch([500], [40], [[7]], last_open=True, sk=True),
        _batch([500], [12], [[41]], first_continues=True, first_overlap=10, sk=True),
    ]
    got = list(sm.fastx_join(batches))
    assert [(g[0], g[1], list(g[2])) for g in got] == [(0, 5, [1]), (10, 7, [2, 3]), (30, 200, [4, 50, 120, 130]), (400, 3, [0]),
                                                        (500, 42, [7, 41])]
    assert all(list(g[3]) == [x + 1 for x in g[2]] and g[4] is None for g in got)
    with pytest.raises(ValueError):
        list(sm.fastx_join(batches[2:]))


# ---------------------------------------------------------------- the rule under sanitizers
def test_split_rule_walk_under_sanitizers(tmp_path):
    """tests/cxx/fastx_split_check.cpp: a stand-alone program over mm_fastx_cut.h, built with AddressSanitizer and UBSan
    and run as it is."""
    exe = str(tmp_path / "fastx_split_check")
    src = os.path.join(HERE, "cxx", "fastx_split_check.cpp")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                        "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "fastx_split_check: OK" in r.stdout
