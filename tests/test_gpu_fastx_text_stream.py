"""The byte-text FASTA stream on the GPU (mm_fastx_text_stream_create; FastxTextStream): every record of every batch
against the oracle's reader (oracle.fasta_records) and the text checker, the whole stream against the one-shot pipeline
(fasta_text_pipeline_device), the DNA stream on ASCII DNA, edge forms, independence of the feeding, errors."""
import ctypes as C

import numpy as np
import pytest

import one_minimizer_cases as oc
import text_checker as tc

pytestmark = pytest.mark.gpu

ALPHABET = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYacdxy*\x00\t\xff\x80\xa5", dtype=np.uint8)
PIECES = (1, 7, 4096, 333, 20000)


def _protein_fasta(rng, lens, width=60, nl=b"\n", final_newline=True):
    parts = []
    for i, m in enumerate(lens):
        s = ALPHABET[rng.integers(0, len(ALPHABET), m)].tobytes()
        parts.append(b">sp|Q%05d|NAME_%d some protein" % (i, i) + nl)
        parts += [s[q:q + width] + nl for q in range(0, m, width)]
    text = b"".join(parts)
    return text if final_newline else text[:-len(nl)]


class Streamed:
    """Per record, in the order of delivery; copies."""

    def __init__(self):
        self.rec_text_pos, self.seqs, self.pos, self.sk, self.values, self.one_min, self.ranges = [], [], [], [], [], [], []
        self.n_batches = 0
        self.n_chars = 0

    def add(self, b, per):
        self.n_batches += 1
        self.n_chars += b.n_bases
        self.ranges.append((b.text_begin, b.text_end))
        assert b.offsets[0] == 0 and int(b.offsets[b.n_records]) == b.n_positions and b.rec_base[0] == 0
        assert int(b.rec_base[b.n_records]) == b.n_bases
        for r in range(b.n_records):
            o0, o1 = int(b.offsets[r]), int(b.offsets[r + 1])
            self.rec_text_pos.append(int(b.rec_text_pos[r]))
            self.pos.append(np.array(b.pos[o0:o1], copy=True))
            self.sk.append(None if b.sk is None else np.array(b.sk[o0:o1], copy=True))
            self.values.append(None if b.values is None else np.array(b.values[per * o0:per * o1], copy=True))
            self.one_min.append(None if b.one_min is None else int(b.one_min[r]))
            self.seqs.append(None if b.seq is None else bytes(b.seq[int(b.rec_base[r]):int(b.rec_base[r + 1])]))
            if b.seq is None:
                self.seqs[-1] = int(b.rec_base[r + 1]) - int(b.rec_base[r])


def _stream(sm, builder, text, chunk_bytes, max_records, pieces=PIECES, **options):
    got = Streamed()
    per = 2 if options.get("values") == "u128" else 1
    with sm.FastxTextStream(builder, chunk_bytes, max_records, **options) as st:
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
                        got.add(b, per)
            at += n
        st.finish()
        for b in st:
            got.add(b, per)
    return got


def _tiles(ranges, first, end):
    at = first
    for b, e in ranges:
        assert b == at and e >= b, (ranges, first, end)
        at = e
    assert at == end, (at, end)


def _reduced_hasher(sm):
    """A custom 256-entry table: a reduced alphabet - every byte hashes as its class c % 11 does."""
    rng = np.random.default_rng(77)
    base_fw, base_rc = rng.integers(0, 1 << 32, 11, dtype=np.uint64), rng.integers(0, 1 << 32, 11, dtype=np.uint64)
    return sm.TextHasher.from_tables([int(base_fw[c % 11]) for c in range(256)], [int(base_rc[c % 11]) for c in range(256)],
                                     rot=5, canonical=False)


CONFIGS = {
    # name: (builder maker, mode, stream options)
    "fwd_sk_u64_one_seq": (lambda sm: sm.minimizers(7, 11).hasher(sm.TextMulHasher(canonical=False)), 0,
                           dict(super_kmers=True, values="u64", one_minimizer=True, seq=True)),
    "closed_syncmers": (lambda sm: sm.closed_syncmers(5, 9).hasher(sm.TextMulHasher(canonical=False)), 1,
                        dict(one_minimizer=True)),
    "k12_u128": (lambda sm: sm.minimizers(12, 5).hasher(sm.TextMulHasher(canonical=False)), 0, dict(values="u128", seq=True)),
    "reduced_alphabet": (lambda sm: sm.minimizers(7, 11).hasher(_reduced_hasher(sm)), 0,
                         dict(values="u64", one_minimizer=True)),
}


@pytest.fixture(scope="module")
def protein_case(oracle):
    rng = np.random.default_rng(9)
    l = 7 + 11 - 1
    lens = [0, 1, l - 1, l, l + 1, 2000, 0, 0, 60, 61, 120] + [int(x) for x in rng.integers(0, 2001, 289)]
    text = _protein_fasta(rng, lens)
    recs = oracle.fasta_records(text)
    assert [len(s) for _, _, s in recs] == lens and len(lens) == 300 and 250_000 < len(text) < 400_000
    return text, recs, {}


def _expected(sm, case, name):
    """Per record: positions, indices, values, one minimizer - from the checker, computed once per configuration."""
    text, recs, cache = case
    if name in cache:
        return cache[name]
    make, mode, opt = CONFIGS[name]
    b = make(sm)
    th = b._text_hasher
    k, w = b.k, b.w
    vlen = k if mode == 0 else k + w - 1
    out = []
    for _, _, s in recs:
        a = np.frombuffer(s, dtype=np.uint8)
        if opt.get("super_kmers"):
            pos, idx = tc.run(s, k, w, th, super_kmers=True)
        else:
            pos, idx = tc.run(s, k, w, th, mode=mode), None
        vals = None
        if opt.get("values"):
            a64 = a.astype(np.uint64)
            p = pos.astype(np.int64)
            lo, hi = np.zeros(len(p), dtype=np.uint64), np.zeros(len(p), dtype=np.uint64)
            for j in range(vlen):
                if j < 8:
                    lo |= a64[p + j] << np.uint64(8 * j)
                else:
                    hi |= a64[p + j] << np.uint64(8 * (j - 8))
            vals = lo if opt["values"] == "u64" else np.stack([lo, hi], axis=1).reshape(-1)
        one = None
        if opt.get("one_minimizer"):
            one = int(oc.expect_text(a, np.array([0, len(a)], dtype=np.uint64), k, th)[0])
        out.append((pos, idx, vals, one))
    cache[name] = out
    return out


@pytest.mark.parametrize("chunk_bytes", [4096, 10000, 65536])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_stream_parity(sm, gpu, protein_case, name, chunk_bytes):
    text, recs, _ = protein_case
    make, mode, opt = CONFIGS[name]
    want = _expected(sm, protein_case, name)
    got = _stream(sm, make(sm), text, chunk_bytes, 512, **opt)
    assert got.n_batches >= len(text) // (2 * chunk_bytes)
    assert got.rec_text_pos == [p for p, _, _ in recs]
    _tiles(got.ranges, 0, len(text))
    assert got.n_chars == sum(len(s) for _, _, s in recs)
    for r, ((_, _, s), (pos, idx, vals, one)) in enumerate(zip(recs, want)):
        assert np.array_equal(got.pos[r], pos), (r, got.pos[r][:8], pos[:8])
        if idx is not None:
            assert np.array_equal(got.sk[r], idx), r
        else:
            assert got.sk[r] is None
        if vals is not None:
            assert np.array_equal(got.values[r], vals), r
        else:
            assert got.values[r] is None
        assert got.one_min[r] == one, (r, got.one_min[r], one)
        if opt.get("seq"):
            assert got.seqs[r] == s, r
        else:
            assert got.seqs[r] == len(s), r


@pytest.mark.parametrize("name", ["fwd_sk_u64_one_seq", "k12_u128"])
def test_whole_stream_equals_the_one_shot_pipeline(sm, gpu, protein_case, name):
    """Bit for bit: positions, offsets and values of fasta_text_pipeline_device on the same text."""
    text, recs, _ = protein_case
    make, mode, opt = CONFIGS[name]
    b = make(sm)
    u128 = opt["values"] == "u128"
    shot_recs, cnt, pos, offsets, vals = sm.fasta_text_pipeline_device(b, text, 512, encoding=sm.TEXT_VALUES_BYTES,
                                                                      u128=u128).finish()
    got = _stream(sm, b, text, 10000, 512, **opt)
    assert np.array_equal(np.concatenate(got.pos), pos.cpu().numpy().view(np.uint32))
    assert np.array_equal(np.concatenate(got.values), vals.cpu().numpy().view(np.uint64))
    assert np.array_equal(np.cumsum([0] + [len(p) for p in got.pos]), offsets.cpu().numpy())
    assert b"".join(got.seqs) == bytes(shot_recs.seq.cpu().numpy())
    assert got.rec_text_pos == [int(x) for x in shot_recs.text_pos]


def _dna_streams(sm, b, text):
    """(the text stream's records, the DNA stream's (positions, values, lengths, text positions)) on the same bytes."""
    got = _stream(sm, b, text, 10000, 512, values="u64", encoding=sm.TEXT_VALUES_DNA)
    dna_pos, dna_vals, dna_lens, dna_where = [], [], [], []
    for batch in sm.stream_fastx(b, [text], 10000, 512, values="u64"):
        for r in range(batch.n_records):
            o0, o1 = int(batch.offsets[r]), int(batch.offsets[r + 1])
            dna_pos.append(batch.pos[o0:o1])
            dna_vals.append(batch.values[o0:o1])
            dna_lens.append(int(batch.rec_base[r + 1] - batch.rec_base[r]))
            dna_where.append(int(batch.rec_text_pos[r]))
    return got, (dna_pos, dna_vals, dna_lens, dna_where)


def _dna_fasta(seqs):
    return b"".join(b">r%d\n" % i + b"".join(s[q:q + 70] + b"\n" for q in range(0, len(s), 70)) for i, s in enumerate(seqs))


def test_dna_cross_check(sm, oracle, gpu):
    """ASCII DNA without N: the text stream with mm_text_hasher_from_dna, canonical k=21 w=11 and DNA values gives the
    positions and u64 values of the DNA stream on the same bytes.

    The input.  The two paths are DEFINED apart in one respect: byte text votes the strand on bit 1 of the byte (c & 2 on the
    characters of a `&[u8]`, src/canonical.rs:26-28: ASCII C and G), the packed path on bit 1 of the 2-bit code (T and G).
    The hashes are the same, so the two definitions - the oracle and tests/text_checker.py, both on the CPU - give other
    positions only in a window whose minimal key is tied between two k-mers, where the vote picks the leftmost or the
    rightmost of them; on random DNA that is about one window in 10^4 (of 204 random records of up to 900 bases, two).  A
    record enters the cross-check when the two DEFINITIONS agree on it - decided by the references, never by a stream's
    output - and every record drawn that they disagree on goes into a second file, on which each stream must equal its own
    definition: the difference is the text path's, as specified before this stream existed, and not the stream's to
    change.  The draw goes on until both files have records."""
    rng = np.random.default_rng(31)
    k, w = 21, 11
    nt = sm.NtHasher(k, True)
    th = sm.TextHasher.from_dna(nt)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    lens = [int(x) for x in rng.integers(0, 900, 200)] + [20, 31, 32, 0]
    agree, differ, drawn = [], [], 0
    while len(agree) < len(lens) or not differ:
        m = lens[len(agree)] if len(agree) < len(lens) else 900
        s = letters[rng.integers(0, 4, m)].tobytes()
        drawn += 1
        assert drawn < 2000
        packed_way = oracle.run(oracle.pack_ascii(s), m, k, w, canonical=True) if m else np.zeros(0, np.uint32)
        text_way = tc.run(s, k, w, th, canonical=True)
        if np.array_equal(packed_way, text_way):
            if len(agree) < len(lens):
                agree.append(s)
        else:
            differ.append((s, packed_way, text_way))
    assert len(differ) * 20 < drawn  # (rare: the cross-check covers what was drawn but for these)
    b = sm.canonical_minimizers(k, w).hasher(nt).hasher(th)
    # the cross-check
    got, (dna_pos, dna_vals, dna_lens, dna_where) = _dna_streams(sm, b, _dna_fasta(agree))
    assert dna_lens == lens and got.seqs == lens and got.rec_text_pos == dna_where
    assert sum(len(p) for p in dna_pos) > 1000
    for r in range(len(lens)):
        assert np.array_equal(got.pos[r], dna_pos[r]), r
        assert np.array_equal(got.values[r], dna_vals[r]), r
    # where the definitions part: each stream keeps to its own
    got, (dna_pos, _, _, _) = _dna_streams(sm, b, _dna_fasta([s for s, _, _ in differ]))
    for r, (_, packed_way, text_way) in enumerate(differ):
        assert np.array_equal(dna_pos[r], packed_way), r
        assert np.array_equal(got.pos[r], text_way), r


def _check_records(sm, oracle, text, chunk_bytes=64, pieces=PIECES, **kw):
    k, w = 3, 4
    th = sm.TextMulHasher(canonical=False)
    b = sm.minimizers(k, w).hasher(th)
    recs = oracle.fasta_records(text)
    got = _stream(sm, b, text, chunk_bytes, 64, pieces=pieces, one_minimizer=True, seq=True, values="u64", **kw)
    first = kw.get("first_byte", 0)
    assert got.rec_text_pos == [first + p for p, _, _ in recs], (text, chunk_bytes)
    assert got.seqs == [s for _, _, s in recs], (text, chunk_bytes)
    for r, (_, _, s) in enumerate(recs):
        assert np.array_equal(got.pos[r], tc.run(s, k, w, th)), (text, chunk_bytes, r)
        a = np.frombuffer(s, dtype=np.uint8)
        assert got.one_min[r] == int(oc.expect_text(a, np.array([0, len(a)], dtype=np.uint64), k, th)[0])
    if text.strip(b" \t\r\n"):
        _tiles(got.ranges, first, first + len(text))
    return got


def test_forms(sm, gpu, oracle):
    rng = np.random.default_rng(5)
    lens = [int(x) for x in rng.integers(0, 40, 30)]
    _check_records(sm, oracle, _protein_fasta(rng, lens, width=13, nl=b"\r\n"), 128)                 # CRLF lines
    _check_records(sm, oracle, _protein_fasta(rng, lens, width=13, final_newline=False), 128)        # no final newline
    _check_records(sm, oracle, b"junk in front\nmore junk\n" + _protein_fasta(rng, lens, width=13), 128, fmt="fasta")
    _check_records(sm, oracle, b"\n\n>a\nAC\n>b\n>c\n\n>d\nxyz\x80\xff\n>e", 64)           # headers with no sequence
    got = _check_records(sm, oracle, b">lower\nacdEF\x80\x81\xfe\xffgh\n>two\nAa\n", 64)   # kept as they are
    assert got.seqs == [b"acdEF\x80\x81\xfe\xffgh", b"Aa"]
    b = sm.minimizers(3, 4).hasher(sm.TextMulHasher(canonical=False))
    for text in (b"", b" \n\t\r\n  \n"):                                                   # empty, blank: no batch
        assert _stream(sm, b, text, 64, 8).n_batches == 0


def test_independence_of_the_feeding(sm, gpu, oracle):
    rng = np.random.default_rng(6)
    lens = [int(x) for x in rng.integers(0, 50, 40)]
    text = _protein_fasta(rng, lens, width=17)
    ref = _check_records(sm, oracle, text, 256, pieces=(len(text),))
    for pieces in ((1,), (7,), (4096,)):
        got = _check_records(sm, oracle, text, 256, pieces=pieces)
        assert got.ranges == ref.ranges
    for slots in (2, 8):
        _check_records(sm, oracle, text, 256, slots=slots)
    # every chunk-boundary phase of one small text
    small = text[:700]
    for chunk_bytes in range(100, 164):
        _check_records(sm, oracle, small, chunk_bytes, pieces=(len(small),))
    # offsets past 2^32
    first = (1 << 32) - 1000
    got = _check_records(sm, oracle, text, 256, first_byte=first)
    assert got.rec_text_pos[-1] > (1 << 32) and got.ranges[0][0] == first


def test_a_batch_stays_unchanged_until_the_following_next(sm, gpu, protein_case):
    text, recs, _ = protein_case
    make, mode, opt = CONFIGS["fwd_sk_u64_one_seq"]
    names = ("rec_text_pos", "rec_base", "offsets", "pos", "sk", "values", "one_min", "seq")
    with sm.FastxTextStream(make(sm), 10000, 512, **opt) as st:
        held, snap, n = None, None, 0
        at = 0
        while at < len(text):
            at += st.feed(memoryview(text)[at:at + 5000])
            if held is not None:  # (more chunks were uploaded and launched meanwhile)
                for name in names:
                    assert np.array_equal(getattr(held, name), snap[name]), name
            b = st.next()
            if b is not None:
                held, snap, n = b, {name: np.array(getattr(b, name), copy=True) for name in names}, n + 1
        assert n >= 5


def _fails_with(sm, st, text, code, needle):
    with pytest.raises(sm.MinimizerError) as e:
        at = 0
        while at < len(text):
            at += st.feed(memoryview(text)[at:])
            if at < len(text):
                st.next()
        st.finish()
        for _ in st:
            pass
    assert e.value.code == sm.ERR[code] and needle in str(e.value), e.value
    for call in (lambda: st.feed(b">x\nAC\n"), st.finish, st.next):  # the stream stays failed
        with pytest.raises(sm.MinimizerError) as again:
            call()
        assert again.value.code == sm.ERR[code]


def test_errors_leave_the_stream_failed(sm, gpu):
    import torch
    b = sm.minimizers(3, 4).hasher(sm.TextMulHasher(canonical=False))
    dev_before = torch.cuda.current_device()
    many = b"".join(b">r%d\nACDEFGHIKL\n" % i for i in range(60))
    with sm.FastxTextStream(b, 128, 64) as st:
        _fails_with(sm, st, b">long\n" + b"ACDEFGHIKLMNPQRSTVWY\n" * 40 + many, "CAPACITY", "a record longer than chunk_bytes")
    with sm.FastxTextStream(b, 1024, 8) as st:
        _fails_with(sm, st, many * 3, "CAPACITY", "max_records")
    with sm.FastxTextStream(b, 1024, 512, max_positions=5) as st:
        _fails_with(sm, st, many * 3, "CAPACITY", "max_positions")
    with sm.FastxTextStream(b, 1024, 512) as st:
        _fails_with(sm, st, b"\n@r0\nACGT\n+\nIIII\n", "FORMAT", "FASTQ")
    with sm.FastxTextStream(b, 1024, 512) as st:
        _fails_with(sm, st, b"ACGT\n>r\nAC\n", "FORMAT", "first non-blank byte")
    with pytest.raises(sm.MinimizerError) as e:
        sm.FastxTextStream(b, 1024, 512, fmt="fastq")
    assert e.value.code == sm.ERR["FORMAT"]
    assert torch.cuda.current_device() == dev_before
