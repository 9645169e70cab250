"""FASTA / FASTQ text streamed through the device in chunks (mm_fastx_stream_*, FastxStream): the concatenated batches
equal the CPU oracle per record and, bit for bit, what the one-shot route (fastx_pipeline_device) gives for the whole
text.  Texts of tens to hundreds of KB: the smallest that cross the packers' 16 KB work unit and 32-byte pieces with one
record per lane and the lane table both in play.  The oracle's results and the one-shot route's are computed once per plan
and shared by the chunk sizes."""
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
    # (k = 40 with the prebuilt w = 11: a forward plan - a canonical one needs k + w - 1 odd)
    "fwd_min_k40_w11_u128": dict(ctor="minimizers", k=40, w=11, canonical=False, mode=0, sk=False, values="u128"),
}
PIECES = (1, 4095, 70000)


def _builder(sm, p):
    return getattr(sm, p["ctor"])(p["k"], p["w"])


def _reads(seed, lengths, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    return [rng.choice(list(alphabet), size=int(n)).astype(np.uint8).tobytes() for n in lengths]


def _lengths(l, n=400):
    menu = [0, 1, l - 1, l, l + 1, 31, 32, 33, 150, 1000, 5000]
    rng = np.random.default_rng(l)
    # (mostly the short ones, so that the text stays at a few hundred KB; every length of the menu occurs)
    weights = np.array([3, 3, 3, 3, 3, 3, 3, 3, 6, 2, 0.4])
    lens = list(rng.choice(menu, size=n - len(menu), p=weights / weights.sum())) + menu
    rng.shuffle(lens)
    return [int(x) for x in lens]


def _fastq(reads, nl=b"\n", final_newline=True, blank_end=0):
    """Four lines per read.  Every third read has a description of up to 300 bytes in the header line, every third a '+'
    line that long (so that chunks end in all four kinds of line), every fifth a quality line that begins with '@'."""
    out = bytearray()
    for i, s in enumerate(reads):
        head = b"@r%d" % i + (b" " + b"d" * min(len(s), 300) if i % 3 == 1 else b"")
        plus = b"+" + (b"r%d " % i + b"x" * min(len(s), 300) if i % 3 == 2 else b"")
        qual = (b"@" if i % 5 == 0 and s else b"") + b"I" * (len(s) - (1 if i % 5 == 0 and s else 0))
        out += head + nl + s + nl + plus + nl + qual + nl
    if not final_newline:
        del out[-len(nl):]
    out += nl * blank_end
    return bytes(out)


def _expected(oracle, reads, p, amb=False):
    """Per-record oracle results, concatenated: positions, indices or None, values or None, offsets."""
    ln = p["k"] if p["mode"] == 0 else p["k"] + p["w"] - 1
    pos, idx, vals, offs = [], [], [], [0]
    for s in reads:
        if amb:
            pk, am = oracle.pack_ascii_n(s)
            got = oracle.run_skip_ambiguous(pk, am, len(s), p["k"], p["w"], canonical=True, mode=p["mode"])
        else:
            pk = oracle.pack_ascii(s) if s else np.zeros(1, dtype=np.uint8)
            got = oracle.run(pk, len(s), p["k"], p["w"], canonical=p["canonical"], mode=p["mode"], super_kmers=p["sk"])
        if p["sk"]:
            idx.append(got[1])
            got = got[0]
        pos.append(got)
        if p["values"] and len(got):
            f = oracle.values_u128 if p["values"] == "u128" else oracle.values_u64
            vals.append(np.asarray(f(pk, ln, got, p["canonical"]), dtype=np.uint64).reshape(-1))
        offs.append(offs[-1] + len(got))
    cat = lambda xs, t: np.concatenate(xs).astype(t) if xs else np.zeros(0, t)  # noqa: E731
    return (cat(pos, np.uint32), cat(idx, np.uint32) if p["sk"] else None, cat(vals, np.uint64) if p["values"] else None,
            np.array(offs, dtype=np.uint64))


class Streamed:
    """Everything a stream delivered, concatenated, and the batches' byte ranges."""

    def __init__(self):
        self.rec_text_pos, self.lens, self.offsets = [], [], [0]
        self.pos, self.sk, self.values = [], [], []
        self.ranges = []
        self.last_records = []

    def add(self, b):
        self.ranges.append((b.text_begin, b.text_end))
        assert len(b.rec_text_pos) == b.n_records and len(b.rec_base) == b.n_records + 1 == len(b.offsets)
        assert int(b.offsets[0]) == 0 and int(b.offsets[-1]) == b.n_positions == len(b.pos)
        assert int(b.rec_base[0]) == 0 and int(b.rec_base[-1]) == b.n_bases
        base = self.offsets[-1]
        self.rec_text_pos += [int(x) for x in b.rec_text_pos]
        self.lens += [int(x) for x in np.diff(b.rec_base.astype(np.int64))]
        self.offsets += [base + int(x) for x in b.offsets[1:]]
        self.pos.append(np.array(b.pos, copy=True))
        if b.sk is not None:
            self.sk.append(np.array(b.sk, copy=True))
        if b.values is not None:
            self.values.append(np.array(b.values, copy=True))

    def cat(self, name, t):
        xs = getattr(self, name)
        return np.concatenate(xs).astype(t) if xs else np.zeros(0, t)


def _stream(sm, builder, text, chunk_bytes, max_records, pieces=PIECES, **options):
    got = Streamed()
    with sm.FastxStream(builder, chunk_bytes, max_records, **options) as st:
        at, turn = 0, 0
        view = memoryview(text)
        while at < len(text):
            n = min(pieces[turn % len(pieces)], len(text) - at)
            turn += 1
            done = 0
            while done < n:
                done += st.feed(view[at + done: at + n])
                if done < n:
                    b = st.next()
                    if b is not None:
                        got.add(b)
            at += n
        st.finish()
        for b in st:
            got.add(b)
    return got


def _tiles(ranges, first, end):
    at = first
    for b, e in ranges:
        assert b == at and e >= b, (ranges, first, end)
        at = e
    assert at == end, (at, end)


def _phases(text, ranges, chunk_bytes, first=0):
    """Newlines mod 4 of every chunk that is not the last: chunk i ends with the new bytes [i * C, (i + 1) * C)."""
    out = set()
    for i, (b, _) in enumerate(ranges[:-1]):
        out.add(text[b - first:(i + 1) * chunk_bytes].count(b"\n") % 4)
    return out


def _compare(got, want_text_pos, want_lens, want, p):
    want_pos, want_idx, want_vals, want_offs = want
    assert got.rec_text_pos == want_text_pos
    assert got.lens == want_lens
    assert np.array_equal(np.array(got.offsets, dtype=np.uint64), want_offs)
    assert np.array_equal(got.cat("pos", np.uint32), want_pos)
    if p["sk"]:
        assert np.array_equal(got.cat("sk", np.uint32), want_idx)
    else:
        assert not got.sk
    if p["values"]:
        assert np.array_equal(got.cat("values", np.uint64), want_vals)
    else:
        assert not got.values


def _one_shot(sm, p, text, fmt, max_records, with_amb=False):
    """What fastx_pipeline_device gives for the whole text: (text positions, lengths, positions, indices, values, offsets)."""
    import torch
    b = _builder(sm, p)
    if p["sk"]:
        # (the pipeline call has no super-k-mer output: the same three calls it queues, with one)
        pipe = sm.fastx_pipeline_device(b, text, max_records, fmt)
        recs, cnt, pos, offs, _ = pipe.finish()
        sk = torch.zeros(max(len(text), 1), dtype=torch.int32, device="cuda")
        pos2 = torch.zeros(max(len(text), 1), dtype=torch.int32, device="cuda")
        offs2 = torch.zeros(max_records + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        out = sm.run_packed_reads_counts_device(b, pipe.packed, pipe.starts, pipe.counts, pos2, offs2, out_sk=sk, max_bases=len(text),
                                                max_records=max_records)
        assert out[0] == cnt
        idx = sk[:cnt].cpu().numpy().view(np.uint32)
        vals = None
    else:
        pipe = sm.fastx_pipeline_device(b, text, max_records, fmt, with_amb=with_amb, values=bool(p["values"]), u128=p["values"] == "u128")
        recs, cnt, pos, offs, vals = pipe.finish()
        idx = None
        vals = vals.cpu().numpy().view(np.uint64) if vals is not None else None
    return ([int(x) for x in recs.text_pos], recs.lengths(), pos.cpu().numpy().view(np.uint32), idx, vals,
            offs.cpu().numpy().view(np.uint64))


def _same_as_one_shot(got, shot, p):
    tp, lens, pos, idx, vals, offs = shot
    assert got.rec_text_pos == tp and got.lens == list(lens)
    assert np.array_equal(np.array(got.offsets, dtype=np.uint64), offs)
    assert np.array_equal(got.cat("pos", np.uint32), pos)
    if p["sk"]:
        assert np.array_equal(got.cat("sk", np.uint32), idx)
    if p["values"]:
        assert np.array_equal(got.cat("values", np.uint64), vals)


@pytest.fixture(scope="module")
def fastq_case(sm, gpu, oracle):
    """Per plan: the reads, the text, the oracle's results and the one-shot route's, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            p = PLANS[name]
            reads = _reads(11, _lengths(p["k"] + p["w"] - 1))
            text = _fastq(reads)
            recs = oracle.fastq_records(text)
            assert [s for _, _, s in recs] == reads
            cache[name] = dict(p=p, reads=reads, text=text, text_pos=[o for o, _, _ in recs], lens=[len(s) for s in reads],
                               want=_expected(oracle, reads, p), shot=_one_shot(sm, p, text, "fastq", len(reads) + 3))
        return cache[name]
    return get


# ------------------------------------------------------------------------------------------------------- 1. FASTQ parity
@pytest.mark.parametrize("name", list(PLANS))
def test_fastq_parity(sm, fastq_case, name):
    c = fastq_case(name)
    p, text = c["p"], c["text"]
    phases = set()
    for chunk_bytes in (11000, 16384, 16385, 40000, len(text) + 1):
        got = _stream(sm, _builder(sm, p), text, chunk_bytes, len(c["reads"]) + 3, values=p["values"], super_kmers=p["sk"])
        _tiles(got.ranges, 0, len(text))
        _compare(got, c["text_pos"], c["lens"], c["want"], p)
        _same_as_one_shot(got, c["shot"], p)
        phases |= _phases(text, got.ranges, chunk_bytes)
        if chunk_bytes > len(text):
            assert len(got.ranges) == 1
        else:
            assert len(got.ranges) >= len(text) // chunk_bytes
    assert phases == {0, 1, 2, 3}, phases


# ------------------------------------------------------------------------------------------------------- 2. FASTQ edge forms
@pytest.mark.parametrize("form", ["crlf", "no_final_newline", "blank_lines_at_the_end"])
def test_fastq_edge_forms(sm, gpu, oracle, form):
    p = PLANS["canon_min_k21_w11_u64"]
    reads = _reads(13, _lengths(p["k"] + p["w"] - 1, n=150))
    text = _fastq(reads, nl=b"\r\n" if form == "crlf" else b"\n", final_newline=form != "no_final_newline",
                  blank_end=5 if form == "blank_lines_at_the_end" else 0)
    recs = oracle.fastq_records(text)
    assert [s for _, _, s in recs] == reads
    want = _expected(oracle, reads, p)
    shot = _one_shot(sm, p, text, "fastq", len(reads) + 3)
    for chunk_bytes in (11000, 16385, len(text) + 1):
        got = _stream(sm, _builder(sm, p), text, chunk_bytes, len(reads) + 3, values=p["values"])
        _tiles(got.ranges, 0, len(text))
        _compare(got, [o for o, _, _ in recs], [len(s) for s in reads], want, p)
        _same_as_one_shot(got, shot, p)


def test_fastq_blank_bytes_in_front_and_the_explicit_format(sm, gpu, oracle):
    p = PLANS["canon_min_k21_w11"]
    reads = _reads(17, [150] * 40)
    body = _fastq(reads)
    text = b"\n \r\n\t" + body
    recs = oracle.fastq_records(body)
    want = _expected(oracle, reads, p)
    for fmt in ("auto", "fastq"):
        got = _stream(sm, _builder(sm, p), text, 4096, 64, fmt=fmt, first_byte=1000)
        _tiles(got.ranges, 1000, 1000 + len(text))
        _compare(got, [1000 + 5 + o for o, _, _ in recs], [150] * 40, want, p)


def test_empty_and_blank_streams_end_without_a_batch(sm, gpu):
    b = _builder(sm, PLANS["canon_min_k21_w11"])
    for text in (b"", b"\n\n  \r\n"):
        for fmt in ("auto", "fastq"):
            got = _stream(sm, b, text, 4096, 64, fmt=fmt)
            assert got.ranges == []


# ------------------------------------------------------------------------------------------------------- 3. FASTA
def _fasta_text(seed):
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in rng.choice([0, 1, 59, 60, 61, 150, 700, 1500], size=60)]
    reads = _reads(seed, lens)
    reads = [bytearray(s) for s in reads]
    for s in reads[::3]:
        if len(s) > 100:
            a, m = int(rng.integers(0, len(s) - 40)), int(rng.integers(1, 40))
            s[a:a + m] = b"N" * m
    reads = [bytes(s) for s in reads]
    out = bytearray(b"junk in front\nof the first header\n")
    starts = []
    for i, s in enumerate(reads):
        starts.append(len(out))
        out += b">seq%d some description\n" % i
        for j in range(0, len(s), 60):
            out += s[j:j + 60] + b"\n"
    return reads, bytes(out), starts


@pytest.mark.parametrize("skip", [False, True])
def test_fasta_multi_line_records_with_n(sm, gpu, oracle, skip):
    p = PLANS["canon_min_k21_w11"]
    reads, text, starts = _fasta_text(19)
    recs = oracle.fasta_records(text)
    assert [s for _, _, s in recs] == reads and [o for o, _, _ in recs] == starts
    want = _expected(oracle, reads, p, amb=skip)
    shot = _one_shot(sm, p, text, "fasta", len(reads) + 3, with_amb=skip)
    # chunk borders exactly on a '>', inside that header line, inside the sequence line behind it; records are at most
    # 1 500 bases, so every chunk of 4 000 bytes or more holds a header
    h = next(o for o, r in zip(starts, reads) if o >= 4000 and len(r) > 100)
    header = text[h:text.index(b"\n", h) + 1]
    sizes = (h, h + 3, h + len(header) + 10, len(text) + 1)
    assert text[h:h + 1] == b">" and b"\n" not in text[h:h + 4] and b"\n" not in text[h + len(header):h + len(header) + 11]
    for chunk_bytes in sizes:
        got = _stream(sm, _builder(sm, p), text, chunk_bytes, len(reads) + 3, fmt="fasta", skip_ambiguous=skip)
        _tiles(got.ranges, 0, len(text))
        _compare(got, starts, [len(s) for s in reads], want, p)
        _same_as_one_shot(got, shot, p)
        if chunk_bytes <= len(text):
            assert got.ranges[0][1] < chunk_bytes  # (the first chunk's last record waits for the next header)
    # the format found by the stream: the text from its first '>' on (bytes in front of it are MM_ERR_FORMAT there)
    junk = starts[0]
    for chunk_bytes in (sizes[1], len(text) + 1):
        got = _stream(sm, _builder(sm, p), text[junk:], chunk_bytes, len(reads) + 3, fmt="auto", skip_ambiguous=skip, first_byte=junk)
        _tiles(got.ranges, junk, len(text))
        _compare(got, starts, [len(s) for s in reads], want, p)
        _same_as_one_shot(got, shot, p)


# ------------------------------------------------------------------------------------------------------- 4. offsets beyond 2^32
def test_offsets_cross_two_to_the_32(sm, fastq_case):
    c = fastq_case("canon_min_k21_w11")
    first = (1 << 32) - 5000
    got = _stream(sm, _builder(sm, c["p"]), c["text"], 16384, len(c["reads"]) + 3, first_byte=first)
    _tiles(got.ranges, first, first + len(c["text"]))
    assert got.rec_text_pos == [first + o for o in c["text_pos"]]
    assert got.rec_text_pos[0] < (1 << 32) < got.rec_text_pos[-1]
    assert np.array_equal(got.cat("pos", np.uint32), c["want"][0])


# ------------------------------------------------------------------------------------------------------- 5. batch lifetime
def test_a_batch_stays_unchanged_until_the_following_next(sm, fastq_case):
    c = fastq_case("canon_min_k21_w11_u64")
    text = c["text"]
    with sm.FastxStream(_builder(sm, c["p"]), 16384, len(c["reads"]) + 3, values="u64") as st:
        at = 0
        held = None
        checked = 0
        while at < len(text):
            took = st.feed(memoryview(text)[at:at + 3000])
            at += took
            if held is not None:
                view, copy = held
                for name in ("rec_text_pos", "rec_base", "offsets", "pos", "values"):
                    assert np.array_equal(getattr(view, name), copy[name]), name
                checked += 1
            if took < 3000 and at < len(text):
                b = st.next()
                if b is not None:
                    held = (b, {n: np.array(getattr(b, n), copy=True) for n in ("rec_text_pos", "rec_base", "offsets", "pos", "values")})
        assert checked > 10
        st.finish()
        for _ in st:
            pass


# ------------------------------------------------------------------------------------------------------- 6. slots
def test_two_and_eight_slots_give_the_same(sm, fastq_case):
    c = fastq_case("canon_min_k21_w11_u64")
    for slots in (2, 8):
        got = _stream(sm, _builder(sm, c["p"]), c["text"], 16384, len(c["reads"]) + 3, values="u64", slots=slots)
        _tiles(got.ranges, 0, len(c["text"]))
        _same_as_one_shot(got, c["shot"], c["p"])


# ------------------------------------------------------------------------------------------------------- 7. error returns
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
    assert L.mm_fastx_stream_feed(st.h, b"@", 1, C.byref(took)) == code and took.value == 0
    assert L.mm_fastx_stream_finish(st.h) == code
    assert L.mm_fastx_stream_next(st.h, C.byref(batch)) == code
    assert needle.encode() in L.mm_last_error()
    st.close()


def test_error_returns_leave_the_stream_failed(sm, gpu):
    E = sm.ERR
    b = _builder(sm, PLANS["canon_min_k21_w11"])
    reads = _reads(23, [150] * 200)
    text = _fastq(reads)
    long_text = _fastq(_reads(29, [150] * 20 + [9000] + [150] * 200))
    # a record longer than the chunk
    _fails_with(sm, sm.FastxStream(b, 8192, 1000), long_text, E["CAPACITY"], "a record longer than chunk_bytes")
    # more records in a chunk than the table holds
    _fails_with(sm, sm.FastxStream(b, 16384, 20), text, E["CAPACITY"], "max_records = 20")
    # more positions in a chunk than asked for
    _fails_with(sm, sm.FastxStream(b, 16384, 1000, max_positions=50), text, E["CAPACITY"], "max_positions = 50")
    # neither '@' nor '>'
    _fails_with(sm, sm.FastxStream(b, 16384, 1000), b"\n  xyz\n" + text, E["FORMAT"], "neither")
    # ... and a stream after all that works
    got = _stream(sm, b, text, 16384, 1000)
    assert got.lens == [150] * 200


# ------------------------------------------------------------------------------------------------------- 8. current device
def test_the_current_device_is_left_alone(sm, fastq_case):
    import torch
    if torch.cuda.device_count() < 2:
        other = 0
    else:
        other = 1
    c = fastq_case("canon_min_k21_w11")
    text = c["text"]
    torch.cuda.set_device(other)
    try:
        def current():
            return torch.cuda.current_device()

        assert current() == other
        st = sm.FastxStream(_builder(sm, c["p"]), 16384, len(c["reads"]) + 3, device=0)
        assert current() == other
        at = 0
        while at < len(text):
            at += st.feed(memoryview(text)[at:at + 5000])
            assert current() == other
            st.next()
            assert current() == other
        st.finish()
        assert current() == other
        n = 0
        for b in st:
            n += b.n_records
            assert current() == other
        st.close()
        assert current() == other
    finally:
        torch.cuda.set_device(0)
