"""The FASTA / FASTQ stream (mm_fastx_stream_*) without a GPU: the cut rule on the host (mm_debug_fastx_cut, the function
the trim kernel calls) is chunk-invariant against the oracle's readers for every chunk length, the exported symbols and
their declarations, the refusals of mm_fastx_stream_create in the documented order, and a sanitizer build of a stand-alone
program that walks the rule (tests/cxx/fastx_cut_check.cpp: nothing preloaded, nothing loaded into Python)."""
import ctypes as C
import os
import random
import re
import subprocess

import mm_oracle as oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ["mm_fastx_stream_create", "mm_fastx_stream_feed", "mm_fastx_stream_finish", "mm_fastx_stream_next",
       "mm_debug_fastx_cut"]


def test_symbols_exported_and_declared(sm):
    L = sm.lib()
    with open(os.path.join(ROOT, "include", "simd_minimizers_amd.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "include", "simd_minimizers_amd.hpp")) as f:
        mirror = f.read()
    for name in NEW:
        assert name in sm.EXPORTED_SYMBOLS, name
        assert hasattr(L, name), name
        assert re.search(r"\bint +%s\(" % name, header), name
    assert "mm_fastx_stream_destroy" in sm.EXPORTED_SYMBOLS and hasattr(L, "mm_fastx_stream_destroy")
    assert re.search(r"\bvoid mm_fastx_stream_destroy\(", header)
    assert "stream_fastx" in mirror
    for name in ("FastxStream", "stream_fastx", "fastx_cut"):
        assert callable(getattr(sm, name)), name


# ---------------------------------------------------------------- texts

def _seq(rng, n):
    return bytes(rng.choice(b"ACGTN") for _ in range(n))


def _fastq(rng, form):
    """A small FASTQ.  ``form``: 'plain', 'crlf', 'nonl' (no final newline), 'blank_end' (blank lines behind the last
    record), 'blank_slot' (a blank four-line slot in the middle), 'qual' (quality lines that begin with '@' / '>')."""
    nl = b"\r\n" if form == "crlf" else b"\n"
    out = []
    n = rng.randint(1, 6)
    for r in range(n):
        length = rng.choice([0, 0, 1, 2, 5, 9])
        qual = bytes(rng.choice(b"I#5") for _ in range(length))
        if form == "qual" and length:
            qual = bytes([rng.choice(b"@>")]) + qual[1:]
        out += [b"@r%d" % r, _seq(rng, length), b"+", qual]
        if form == "blank_slot" and r == n // 2:
            out += [b"", b"", b"", b""]
    text = nl.join(out) + nl
    if form == "nonl":
        text = text[:-len(nl)]
    if form == "blank_end":
        text += nl * rng.randint(1, 5)
    return text


def _fasta(rng, form):
    """A small FASTA.  ``form``: 'plain', 'crlf', 'nonl', 'blank_end', 'junk' (bytes in front of the first header),
    'empty' (records without a sequence)."""
    nl = b"\r\n" if form == "crlf" else b"\n"
    out = []
    if form == "junk":
        out += [b"junk line", b"", b" >not a header"][: rng.randint(1, 3)]
    for r in range(rng.randint(1, 5)):
        out.append(b">s%d d" % r)
        if form == "empty" and rng.random() < 0.5:
            continue
        for _ in range(rng.randint(0, 3)):
            out.append(_seq(rng, rng.choice([0, 1, 4, 7])))
    text = nl.join(out) + nl
    if form == "nonl":
        text = text[:-len(nl)]
    if form == "blank_end":
        text += nl * rng.randint(1, 4)
    return text


def _walk(sm, text, fmt, reader, length, phases=None):
    """Feeds ``text`` through the rule in chunks of ``length`` new bytes, the tail carried (a chunk without a cut carries
    everything, as the rule says; the stream itself refuses such a chunk), and returns the records of the kept pieces with
    absolute offsets."""
    got = []
    begin, at, tail = 0, 0, b""
    while True:
        new = text[at:at + length]
        at += len(new)
        last = at >= len(text)
        chunk = tail + new
        v = sm.fastx_cut(chunk, fmt, last)
        cut = v["cut"]
        assert 0 <= cut <= len(chunk)
        piece = chunk[:cut]
        recs = reader(piece)
        assert v["kept"] == len(recs), (text, length, v)
        assert v["dropped"] == len(reader(chunk)) - len(recs) <= (0 if last else 1), (text, length, v)
        if last:
            assert cut == len(chunk)
        elif phases is not None and cut:
            phases.add(chunk.count(b"\n") % 4)
        got += [(p + begin, h, s) for p, h, s in recs]
        begin += cut
        tail = chunk[cut:]
        if last:
            return got


def test_cut_rule_is_chunk_invariant_fastq(sm):
    rng = random.Random(20261019)
    forms = ["plain", "crlf", "nonl", "blank_end", "blank_slot", "qual"]
    phases = set()
    n_texts = 0
    for i in range(150):
        text = _fastq(rng, forms[i % len(forms)])
        want = oracle.fastq_records(text)
        for length in range(1, len(text) + 2):
            assert _walk(sm, text, "fastq", oracle.fastq_records, length, phases) == want, (text, length)
        n_texts += 1
    # cuts fell while the chunk ended in each of the four line phases
    assert phases == {0, 1, 2, 3}, phases
    assert n_texts == 150


def test_cut_rule_is_chunk_invariant_fasta(sm):
    rng = random.Random(7)
    forms = ["plain", "crlf", "nonl", "blank_end", "junk", "empty"]
    for i in range(150):
        text = _fasta(rng, forms[i % len(forms)])
        want = oracle.fasta_records(text)
        for length in range(1, len(text) + 2):
            assert _walk(sm, text, "fasta", oracle.fasta_records, length) == want, (text, length)


def test_cut_rule_small_cases(sm):
    L, E = sm.lib(), sm.ERR
    out = (C.c_uint64 * 3)()
    assert L.mm_debug_fastx_cut(None, 0, 2, 0, out) == 0 and list(out) == [0, 0, 0]
    assert L.mm_debug_fastx_cut(None, 0, 2, 0, None) == E["NULL"]
    assert L.mm_debug_fastx_cut(None, 5, 2, 0, out) == E["NULL"]
    assert L.mm_debug_fastx_cut(b"@a\n", 3, 0, 0, out) == E["BAD_MODE"]
    # fewer than four newlines: no cut; exactly four: behind the fourth; five: still behind the fourth
    assert sm.fastx_cut(b"@a\nAC\n+\nII", "fastq") == {"cut": 0, "kept": 0, "dropped": 1}
    assert sm.fastx_cut(b"@a\nAC\n+\nII\n", "fastq") == {"cut": 11, "kept": 1, "dropped": 0}
    assert sm.fastx_cut(b"@a\nAC\n+\nII\n@b\nA", "fastq") == {"cut": 11, "kept": 1, "dropped": 1}
    assert sm.fastx_cut(b"@a\nAC\n+\nII\n@b\nA", "fastq", last=True) == {"cut": 15, "kept": 2, "dropped": 0}
    # FASTA: the last record waits for the next header; without a record, behind the last newline
    assert sm.fastx_cut(b">a\nAC\n>b\nGG\n", "fasta") == {"cut": 6, "kept": 1, "dropped": 1}
    assert sm.fastx_cut(b"junk\nmore", "fasta") == {"cut": 5, "kept": 0, "dropped": 0}
    assert sm.fastx_cut(b"junk", "fasta") == {"cut": 0, "kept": 0, "dropped": 0}


# ---------------------------------------------------------------- refusals

def _plan(sm, k=21, w=11, canonical=0, mode=0):
    h = C.c_void_p()
    assert sm.lib().mm_plan_create(C.byref(h), k, w, canonical, mode, None) == 0
    return h


def test_refusals_before_any_device_in_the_documented_order(sm):
    """NULL arguments, a text plan, chunk_bytes / max_records out of range, super-k-mers with syncmers or with the
    skip-ambiguous form, a forward plan in the skip-ambiguous form, both values flags, a value length beyond the word, a
    plan without a lane-table launch, no device: each wins over everything behind it."""
    L, E = sm.lib(), sm.ERR
    SK, SKIP, U64, U128 = sm.FASTX_SK, sm.FASTX_SKIP_AMBIGUOUS, sm.FASTX_VALUES_U64, sm.FASTX_VALUES_U128
    fwd = _plan(sm)
    canon = _plan(sm, canonical=1)
    sync_fwd = _plan(sm, k=15, w=17, mode=1)
    long_k = _plan(sm, k=40, w=12, canonical=1)
    long_sync = _plan(sm, k=40, w=32, canonical=1, mode=1)   # value length 71
    wide = _plan(sm, w=129)
    th = sm.TextMulHasher(canonical=False)
    text = C.c_void_p()
    assert L.mm_plan_create_text(C.byref(text), 7, 11, 0, 0, C.byref(th)) == 0
    no_device = L.mm_device_count() <= 0

    def create(plan, flags=0, chunk_bytes=1 << 16, max_records=100, device=0, cfg=True, out=True, fmt=0, slots=0):
        c = sm.FastxStreamConfig(device, fmt, flags, slots, chunk_bytes, max_records, 0, 0)
        h = C.c_void_p()
        r = L.mm_fastx_stream_create(C.byref(h) if out else None, plan, C.byref(c) if cfg else None)
        if r == 0:
            L.mm_fastx_stream_destroy(h)
        else:
            assert not h.value
        return r

    try:
        every = SK | SKIP | U64 | U128
        # every argument wrong at once: the first documented refusal wins, one fix at a time
        assert create(None, every, 1, 1 << 31, -1) == E["NULL"]
        assert create(text, every, 1, 1 << 31, -1, cfg=False) == E["NULL"]
        assert create(text, every, 1, 1 << 31, -1, out=False) == E["NULL"]
        assert create(text, every, 1, 1 << 31, -1) == E["BAD_MODE"]
        assert create(sync_fwd, every, 63, 1 << 31, -1) == E["LEN_TOO_LARGE"]
        assert create(sync_fwd, every, 1 << 31, 5, -1) == E["LEN_TOO_LARGE"]
        assert create(sync_fwd, every, 64, 1 << 31, -1) == E["LEN_TOO_LARGE"]   # (max_records alone)
        assert create(sync_fwd, every, 64, 5, -1) == E["BAD_MODE"]              # (super-k-mers with syncmers)
        assert create(fwd, every, 64, 5, -1) == E["BAD_MODE"]                   # (... with the skip-ambiguous form)
        assert create(fwd, SKIP | U64 | U128, 64, 5, -1) == E["HASHER_NOT_CANONICAL"]
        assert create(sync_fwd, SKIP | U64 | U128, 64, 5, -1) == E["HASHER_NOT_CANONICAL"]
        assert create(long_sync, SKIP | U64 | U128, 64, 5, -1) == E["BAD_MODE"]  # (both values flags)
        assert create(long_sync, SKIP | U128, 64, 5, -1) == E["VALUE_LEN"]       # (71 > 64)
        assert create(long_k, SKIP | U64, 64, 5, -1) == E["VALUE_LEN"]           # (40 > 32)
        assert create(wide, U64, 64, 5, -1) == E["BAD_MODE"]                     # (w = 129: no lane-table launch)
        assert b"mm_run_packed_reads_device" in L.mm_last_error()
        assert create(fwd, U64, 64, 5, -1, fmt=3) == E["BAD_MODE"]
        assert create(fwd, U64, 64, 5, -1, slots=1) == E["BAD_MODE"]
        assert create(fwd, U64, 64, 5, -1, slots=9) == E["BAD_MODE"]
        assert create(long_k, SKIP | U128, 64, 5, -1) == E["NO_DEVICE"]          # (device -1, or no device at all)
        assert create(fwd, SK | U64, 64, 5, 1 << 20) == E["NO_DEVICE"]
        if no_device:
            assert create(canon, 0) == E["NO_DEVICE"]
    finally:
        for h in (fwd, canon, sync_fwd, long_k, long_sync, wide, text):
            L.mm_plan_destroy(h)


def test_lane_table_switched_off_is_refused(sm, monkeypatch):
    L, E = sm.lib(), sm.ERR
    plan = _plan(sm)
    try:
        c = sm.FastxStreamConfig(-1, 0, 0, 0, 1 << 16, 100, 0, 0)
        h = C.c_void_p()
        assert L.mm_fastx_stream_create(C.byref(h), plan, C.byref(c)) == E["NO_DEVICE"]
        monkeypatch.setenv("MM_LANE_TABLE", "0")
        assert L.mm_fastx_stream_create(C.byref(h), plan, C.byref(c)) == E["BAD_MODE"]
        assert b"MM_LANE_TABLE" in L.mm_last_error()
    finally:
        L.mm_plan_destroy(plan)


def test_null_stream_calls(sm):
    L, E = sm.lib(), sm.ERR
    took = C.c_uint64(7)
    assert L.mm_fastx_stream_feed(None, b"x", 1, C.byref(took)) == E["NULL"] and took.value == 0
    assert L.mm_fastx_stream_finish(None) == E["NULL"]
    assert L.mm_fastx_stream_next(None, None) == E["NULL"]
    L.mm_fastx_stream_destroy(None)


# ---------------------------------------------------------------- the rule under sanitizers

def test_cut_rule_walk_under_sanitizers(tmp_path):
    """tests/cxx/fastx_cut_check.cpp: a stand-alone program over mm_fastx_cut.h, built with AddressSanitizer and UBSan and
    run as it is."""
    exe = str(tmp_path / "fastx_cut_check")
    src = os.path.join(HERE, "cxx", "fastx_cut_check.cpp")
    # (the sanitizer runtimes linked statically: the program does not depend on what else the process loads first)
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                        "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "fastx_cut_check: OK" in r.stdout
