"""FASTA records longer than a chunk through the stream (MM_FASTX_LONG_RECORDS, FastxStream(long_records=True)): the
pieces of every record, joined by fastx_join, equal the CPU oracle on the WHOLE record bit for bit - positions, super-k-mer
indices, values and counts - whatever the chunk size.  Every case also checks rec_text_pos, that the batches'
[text_begin, text_end) tile the fed bytes, and that last_open of one batch is first_continues of the next.  The texts are
the smallest at which each part can go wrong: a few KB with chunks of 64 to 200 bytes (tens of seams), up to about 87 KB
where the packers' 16 KB unit and the lane table are to be crossed."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLANS = {
    "canon_min_k5_w7": dict(ctor="canonical_minimizers", k=5, w=7, canonical=True, mode=0, sk=False, values=None),
    "canon_min_k21_w11": dict(ctor="canonical_minimizers", k=21, w=11, canonical=True, mode=0, sk=False, values=None),
    "fwd_min_sk_k21_w11": dict(ctor="minimizers", k=21, w=11, canonical=False, mode=0, sk=True, values=None),
    "canon_closed_k15_w17": dict(ctor="canonical_closed_syncmers", k=15, w=17, canonical=True, mode=1, sk=False, values=None),
    "fwd_open_k5_w7": dict(ctor="open_syncmers", k=5, w=7, canonical=False, mode=2, sk=False, values=None),
    "canon_min_k21_w11_u64": dict(ctor="canonical_minimizers", k=21, w=11, canonical=True, mode=0, sk=False, values="u64"),
    "fwd_min_k40_w11_u128": dict(ctor="minimizers", k=40, w=11, canonical=False, mode=0, sk=False, values="u128"),
}
FEED = (1, 4095, 70000)


def _l(p):
    return p["k"] + p["w"] - 1


def _builder(sm, p):
    return getattr(sm, p["ctor"])(p["k"], p["w"])


def _bases(seed, n, alphabet=b"ACGT"):
    return np.random.default_rng(seed).choice(list(alphabet), size=int(n)).astype(np.uint8).tobytes()


def _fasta(records, width=60, nl=b"\n", final_newline=True):
    """records: (header bytes without '>', bases).  width 0: one line."""
    out = bytearray()
    for name, s in records:
        out += b">" + name + nl
        step = width or max(len(s), 1)
        for j in range(0, len(s), step):
            out += s[j:j + step] + nl
    if not final_newline and out.endswith(nl):
        del out[-len(nl):]
    return bytes(out)


def _expected_record(oracle, s, p, skip=False):
    """The oracle on one whole record: (positions, indices or None, values or None)."""
    ln = p["k"] if p["mode"] == 0 else _l(p)
    idx = None
    if skip:
        pk, am = oracle.pack_ascii_n(s)
        got = oracle.run_skip_ambiguous(pk, am, len(s), p["k"], p["w"], canonical=True, mode=p["mode"])
    else:
        pk = oracle.pack_ascii(s) if s else np.zeros(1, dtype=np.uint8)
        got = oracle.run(pk, len(s), p["k"], p["w"], canonical=p["canonical"], mode=p["mode"], super_kmers=p["sk"])
    if p["sk"]:
        got, idx = got
    vals = None
    if p["values"]:
        f = oracle.values_u128 if p["values"] == "u128" else oracle.values_u64
        vals = np.asarray(f(pk, ln, got, p["canonical"]), dtype=np.uint64).reshape(-1) if len(got) else np.zeros(0, np.uint64)
    return np.asarray(got, dtype=np.uint32), None if idx is None else np.asarray(idx, dtype=np.uint32), vals


def _stream(sm, p, text, chunk_bytes, max_records=64, feed=FEED, long_records=True, **options):
    """Feeds the text in pieces of the given sizes; returns the batches (copies, with their pieces fields)."""
    out = []
    with sm.FastxStream(_builder(sm, p), chunk_bytes, max_records, values=p["values"], super_kmers=p["sk"],
                        long_records=long_records, **options) as st:
        at, turn = 0, 0
        view = memoryview(text)
        while at < len(text):
            n = min(feed[turn % len(feed)], len(text) - at)
            turn += 1
            done = 0
            while done < n:
                done += st.feed(view[at + done: at + n])
                if done < n:
                    b = st.next()
                    if b is not None:
                        out.append(b.copy())
            at += n
        st.finish()
        for b in st:
            out.append(b.copy())
    return out


def _check_batches(batches, first, end):
    at, open_before = first, False
    for b in batches:
        assert b.text_begin == at and b.text_end >= at, (b.text_begin, b.text_end, at)
        at = b.text_end
        assert b.first_continues == open_before
        open_before = b.last_open
        assert len(b.rec_text_pos) == b.n_records and len(b.rec_base) == b.n_records + 1 == len(b.offsets)
        assert int(b.offsets[0]) == 0 and int(b.offsets[-1]) == b.n_positions == len(b.pos)
        assert int(b.rec_base[0]) == 0 and int(b.rec_base[-1]) == b.n_bases
        if b.last_open:
            assert b.n_records == 1
        if not b.first_continues:
            assert b.first_base == 0 and b.first_overlap == 0
        else:
            assert b.n_records >= 1 and b.first_overlap <= int(b.rec_base[1]) and b.first_base > 0
    assert at == end and not open_before


def _check(sm, oracle, p, text, batches, skip=False, first_byte=0, want=None):
    """Tiling and the pieces chain, then every joined record against the oracle on the whole record."""
    _check_batches(batches, first_byte, first_byte + len(text))
    recs = oracle.fasta_records(text)
    joined = list(sm.fastx_join(batches))
    assert [j[0] for j in joined] == [first_byte + o for o, _, _ in recs]
    assert [j[1] for j in joined] == [len(s) for _, _, s in recs]
    want = want if want is not None else [_expected_record(oracle, s, p, skip) for _, _, s in recs]
    for r, ((_, n_bases, pos, sk, vals), (wpos, widx, wvals)) in enumerate(zip(joined, want)):
        assert len(pos) == len(wpos), (r, len(pos), len(wpos))
        assert np.array_equal(pos, wpos), r
        if p["sk"]:
            assert np.array_equal(sk, widx), r
        else:
            assert sk is None
        if p["values"]:
            assert np.array_equal(vals, wvals), r
        else:
            assert vals is None
    return want


# ------------------------------------------------------------------------------------------------------- 1. many seams
# One record of 3 000 bases in lines of 60: chunks of 64 (the minimum) and 100 bytes at l = 11, of 128 bytes at l = 31, of
# 4 l = 200 bytes at l = 50 (the smallest the stream takes there) - about 45, 30, 24 and 15 seams.
SEAMS = [("canon_min_k5_w7", 64), ("canon_min_k5_w7", 100), ("fwd_open_k5_w7", 64), ("fwd_open_k5_w7", 100),
         ("canon_min_k21_w11", 128), ("fwd_min_sk_k21_w11", 128), ("canon_closed_k15_w17", 128), ("canon_min_k21_w11_u64", 128),
         ("fwd_min_k40_w11_u128", 200)]


@pytest.mark.parametrize("name,chunk_bytes", SEAMS)
def test_many_seams(sm, gpu, oracle, name, chunk_bytes):
    p = PLANS[name]
    text = _fasta([(b"chr1 one record", _bases(31, 3000))])
    batches = _stream(sm, p, text, chunk_bytes)
    assert len(batches) >= len(text) // chunk_bytes and all(b.last_open for b in batches[:-1])
    assert all(b.first_overlap == _l(p) - 1 for b in batches[1:])
    # (positions are record-global: they reach beyond what a piece holds)
    assert max(int(b.pos[-1]) for b in batches if b.n_positions) > 2500
    _check(sm, oracle, p, text, batches)


# ------------------------------------------------------------------------------------------------------- 2. a repeat on the seam
@pytest.mark.parametrize("name", ["canon_min_k5_w7", "fwd_min_sk_k21_w11"])
def test_a_position_chosen_on_both_sides_of_a_seam_is_delivered_once(sm, gpu, oracle, name):
    p = PLANS[name]
    l, chunk_bytes = _l(p), 64 if _l(p) == 11 else 128
    s = b"A" * 200 + _bases(37, 2800)
    text = _fasta([(b"low", s)])
    batches = _stream(sm, p, text, chunk_bytes)
    want = _check(sm, oracle, p, text, batches)
    whole = want[0][0]
    assert np.all(whole[1:] != whole[:-1])

    def window(i):  # the minimizer of window i alone
        got = oracle.run(oracle.pack_ascii(s[i:i + l]), l, p["k"], p["w"], canonical=p["canonical"], mode=0)
        assert len(got) == 1
        return int(got[0]) + i

    # the case is reached: at some seam the piece's first window chooses what the window before it chose - the piece began
    # with a position that the whole record holds once - and at some seam it does not
    firsts = [(window(b.first_base), window(b.first_base - 1)) for b in batches[1:] if b.first_base + l <= len(s)]
    same = [q == before for q, before in firsts]
    assert sum(same) >= 5 and not all(same), same
    assert any(np.count_nonzero(whole == q) == 1 for q, before in firsts if q == before)


# ------------------------------------------------------------------------------------------------------- 3. skip-ambiguous
@pytest.mark.parametrize("name", ["canon_min_k21_w11", "canon_closed_k15_w17"])
def test_runs_of_n_on_the_cuts(sm, gpu, oracle, name):
    """One base per line, so that a chunk of 128 bytes holds 64 bases and a run of 3 l = 93 N spans a whole chunk.  Runs of
    l - 1 N that END with a chunk's last base, of l N that BEGIN with a chunk's first base, of 3 l that cover a chunk, of 1."""
    p = PLANS[name]
    l, chunk_bytes = _l(p), 128
    s = bytearray(_bases(41, 3000))
    head = b">n\n"
    first_base_of = lambda j: -(-(j * chunk_bytes - len(head)) // 2)  # noqa: E731  (chunk j's first base; base b is byte 3 + 2 b)
    a, b_, c, d = first_base_of(5), first_base_of(10), first_base_of(15), first_base_of(20)
    s[a - (l - 1):a] = b"N" * (l - 1)
    s[b_:b_ + l] = b"N" * l
    s[c - 5:c - 5 + 3 * l] = b"N" * (3 * l)
    s[d - 1:d] = b"N"
    s[d + 30:d + 31] = b"N"
    s = bytes(s)
    text = _fasta([(b"n", s)], width=1)
    assert text[:3] == head and len(text) == 3 + 2 * len(s)
    assert text[5 * chunk_bytes - 2:5 * chunk_bytes + 3] in (b"\nN\n" + s[a:a + 1] + b"\n", b"N\n" + s[a:a + 1] + b"\n" + s[a + 1:a + 2])
    assert text[10 * chunk_bytes:10 * chunk_bytes + 2] in (b"N\n", b"\nN") and s[b_ - 1:b_] != b"N"
    assert set(text[15 * chunk_bytes:16 * chunk_bytes]) == set(b"N\n")
    batches = _stream(sm, p, text, chunk_bytes, skip_ambiguous=True)
    assert len(batches) >= 45 and any(b.n_positions == 0 for b in batches[1:-1])
    _check(sm, oracle, p, text, batches, skip=True)


# ------------------------------------------------------------------------------------------------------- 4. the record ends on the cut
@pytest.mark.parametrize("ends_the_file", [False, True])
def test_a_record_whose_last_base_ends_a_chunk(sm, gpu, oracle, ends_the_file):
    p = PLANS["canon_min_k21_w11_u64"]
    l, chunk_bytes, first = _l(p), 128, 1000
    text = b">r\n" + _bases(43, 3 * chunk_bytes - 3)
    assert len(text) == 3 * chunk_bytes
    if not ends_the_file:
        text += b"\n" + _fasta([(b"next", _bases(47, 150)), (b"more", _bases(53, 40))])
    batches = _stream(sm, p, text, chunk_bytes, first_byte=first)
    _check(sm, oracle, p, text, batches, first_byte=first)
    # the continuation piece holds the overlap and nothing else: no window, no position
    tail = batches[3]
    assert batches[2].last_open and tail.first_continues and not tail.last_open
    assert int(tail.rec_base[1]) == tail.first_overlap == l - 1 and int(tail.offsets[1]) == 0
    assert int(tail.rec_text_pos[0]) == first and tail.first_base == 3 * chunk_bytes - 3 - (l - 1)
    if ends_the_file:
        assert len(batches) == 4 and tail.text_begin == tail.text_end == first + len(text) and tail.n_positions == 0


# ------------------------------------------------------------------------------------------------------- 5. a mixed file
def _mixed_text(l):
    rng = np.random.default_rng(59)
    menu = [0, 1, l - 1, l, l + 1, 150]
    short = lambda n, tag: [(b"%s%d some description" % (tag, i), _bases(1000 + i + len(tag), int(x)))  # noqa: E731
                            for i, x in enumerate(list(rng.choice(menu, size=n - len(menu))) + menu)]
    recs = short(120, b"a") + [(b"chrA", _bases(61, 20000))] + short(120, b"bb") + [(b"chrB", _bases(67, 50000))]
    text = _fasta(recs, final_newline=False)
    # (chunks of 40 000 bytes: the second starts with chrB's header and is not the last, so chrB is split there too)
    assert text.index(b">chrB") < 40000 and len(text) > 80000
    return text


@pytest.fixture(scope="module")
def mixed(oracle):
    """Per plan: the text and the oracle's results per record, computed once and shared by chunk sizes and slots."""
    cache = {}

    def get(name):
        if name not in cache:
            p = PLANS[name]
            text = _mixed_text(_l(p))
            cache[name] = (text, [_expected_record(oracle, s, p) for _, _, s in oracle.fasta_records(text)])
        return cache[name]
    return get


@pytest.mark.parametrize("chunk_bytes", [4096, 40000])
@pytest.mark.parametrize("name", ["canon_min_k21_w11_u64", "fwd_min_sk_k21_w11"])
def test_mixed_file_with_two_and_eight_slots(sm, gpu, oracle, mixed, name, chunk_bytes):
    p = PLANS[name]
    text, want = mixed(name)
    assert not text.endswith(b"\n")
    got = {}
    for slots in (2, 8):
        batches = _stream(sm, p, text, chunk_bytes, max_records=400, slots=slots, fmt="auto" if slots == 8 else "fasta")
        _check(sm, oracle, p, text, batches, want=want)
        got[slots] = batches
        # both long records come in pieces (at 4 096 several each), and batches of whole records lie between them
        assert sum(b.first_continues for b in batches) >= (12 if chunk_bytes == 4096 else 1)
        assert any(b.n_records > 1 and not b.first_continues for b in batches)
    assert len(got[2]) == len(got[8])
    for x, y in zip(got[2], got[8]):
        for field in ("n_records", "n_bases", "n_positions", "text_begin", "text_end", "first_continues", "last_open", "first_base",
                      "first_overlap"):
            assert getattr(x, field) == getattr(y, field), field
        for field in ("rec_text_pos", "rec_base", "offsets", "pos", "sk", "values"):
            u, v = getattr(x, field), getattr(y, field)
            assert (u is None and v is None) or np.array_equal(u, v), field


# ------------------------------------------------------------------------------------------------------- 6. the flag without a long record
def _short_fasta(seed):
    rng = np.random.default_rng(seed)
    recs = []
    for i, n in enumerate(rng.choice([0, 1, 59, 60, 61, 150, 700, 1500], size=60)):
        s = bytearray(_bases(seed + i, int(n)))
        if i % 3 == 0 and len(s) > 100:
            a, m = int(rng.integers(0, len(s) - 40)), int(rng.integers(1, 40))
            s[a:a + m] = b"N" * m
        recs.append((b"seq%d some description" % i, bytes(s)))
    return b"junk in front\nof the first header\n" + _fasta(recs)


@pytest.mark.parametrize("name,skip", [("fwd_min_sk_k21_w11", False), ("canon_min_k21_w11_u64", False), ("canon_min_k21_w11", True)])
def test_the_flag_changes_nothing_when_every_record_fits(sm, gpu, name, skip):
    p = PLANS[name]
    text = _short_fasta(71)
    for chunk_bytes in (4000, 16385):
        plain = _stream(sm, p, text, chunk_bytes, long_records=False, fmt="fasta", skip_ambiguous=skip)
        flagged = _stream(sm, p, text, chunk_bytes, long_records=True, fmt="fasta", skip_ambiguous=skip)
        assert len(plain) == len(flagged) >= len(text) // chunk_bytes
        for x, y in zip(plain, flagged):
            for field in ("n_records", "n_bases", "n_positions", "text_begin", "text_end"):
                assert getattr(x, field) == getattr(y, field), field
            for field in ("rec_text_pos", "rec_base", "offsets", "pos", "sk", "values"):
                u, v = getattr(x, field), getattr(y, field)
                assert (u is None and v is None) or np.array_equal(u, v), field
            assert (y.first_continues, y.last_open, y.first_base, y.first_overlap) == (False, False, 0, 0)


# ------------------------------------------------------------------------------------------------------- 7. failures
def _fails_with(sm, st, text, code, needle):
    """Feeds and drains until the stream fails; the stream then stays failed."""
    L = sm.lib()
    with pytest.raises(sm.MinimizerError) as e:
        at = 0
        while at < len(text):
            at += st.feed(memoryview(text)[at:])
            if at < len(text):
                st.next()
        st.finish()
        for _ in st:
            pass
    assert e.value.code == code and needle in str(e.value), str(e.value)
    took = C.c_uint64(5)
    batch = sm._FastxBatchC()
    pieces = sm._FastxPiecesC()
    assert L.mm_fastx_stream_feed(st.h, b">", 1, C.byref(took)) == code and took.value == 0
    assert L.mm_fastx_stream_finish(st.h) == code
    assert L.mm_fastx_stream_next(st.h, C.byref(batch)) == code
    assert needle.encode() in L.mm_last_error()
    assert L.mm_fastx_stream_pieces(st.h, C.byref(pieces)) == 0
    st.close()


def test_failures_leave_the_stream_failed(sm, gpu, oracle):
    E = sm.ERR
    p = PLANS["canon_min_k21_w11"]
    b = _builder(sm, p)
    long_fasta = _fasta([(b"a", _bases(73, 150)), (b"chr", _bases(79, 9000)), (b"b", _bases(83, 150))])
    # a chunk too small to move past its own overlap: refused at create
    with pytest.raises(sm.MinimizerError) as e:
        sm.FastxStream(b, 123, 10, long_records=True)
    assert e.value.code == E["CAPACITY"] and "4 * (k + w - 1)" in str(e.value)
    # a header line longer than a chunk
    _fails_with(sm, sm.FastxStream(b, 128, 10, long_records=True), b">" + b"h" * 300 + b"\n" + _bases(89, 500) + b"\n", E["CAPACITY"],
                "a record longer than chunk_bytes")
    # a piece that brings no new base: a chunk of line ends inside a record
    _fails_with(sm, sm.FastxStream(b, 128, 10, long_records=True), b">r\n" + _bases(97, 300) + b"\n" * 400 + _bases(101, 300) + b"\n",
                E["CAPACITY"], "cannot advance")
    # the same long record without the flag: as ever
    _fails_with(sm, sm.FastxStream(b, 4096, 10), long_fasta, E["CAPACITY"], "a record longer than chunk_bytes")
    # FASTQ takes no notice of the flag, explicit or found
    fastq = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, _bases(103 + i, n), b"I" * n) for i, n in enumerate([150] * 5 + [9000] + [150] * 40))
    for fmt in ("fastq", "auto"):
        _fails_with(sm, sm.FastxStream(b, 4096, 100, long_records=True, fmt=fmt), fastq, E["CAPACITY"], "a record longer than chunk_bytes")
    # ... and with the flag the long FASTA goes through, on a stream made after all that
    _check(sm, oracle, p, long_fasta, _stream(sm, p, long_fasta, 4096))


# ------------------------------------------------------------------------------------------------------- 8. current device
def test_the_current_device_is_left_alone(sm, gpu):
    import torch
    other = 1 if torch.cuda.device_count() >= 2 else 0
    p = PLANS["canon_min_k21_w11"]
    text = _fasta([(b"chr", _bases(107, 20000)), (b"b", _bases(109, 150))])
    torch.cuda.set_device(other)
    try:
        current = torch.cuda.current_device
        st = sm.FastxStream(_builder(sm, p), 4096, 10, device=0, long_records=True)
        assert current() == other
        at, seen = 0, 0
        while at < len(text):
            at += st.feed(memoryview(text)[at:at + 5000])
            assert current() == other
            b = st.next()
            seen += b is not None and b.first_continues
            assert current() == other
        st.finish()
        assert current() == other
        for b in st:
            seen += b.first_continues
            assert current() == other
        st.close()
        assert current() == other and seen >= 3
    finally:
        torch.cuda.set_device(0)
