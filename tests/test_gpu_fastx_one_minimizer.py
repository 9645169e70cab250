"""MM_FASTX_ONE_MINIMIZER of the DNA stream (FastxStream(one_minimizer=True), mm_fastx_stream_one_minimizer): a FASTQ and
a FASTA of 3000 reads with N fed in pieces of 1000 bytes to a stream of 4096-byte chunks and 3 slots - dozens of chunks and
carried tails.  The concatenated one_min equals the expectation built from the oracle's hashes over all reads, in order;
positions and values are those of the same stream without the flag."""
import ctypes as C

import numpy as np
import pytest

import one_minimizer_amb_cases as ac
import one_minimizer_cases as oc

pytestmark = pytest.mark.gpu
K, W = 21, 11
CHUNK, SLOTS, PIECE, MAX_RECORDS = 4096, 3, 1000, 600


def _reads(seed, n=3000):
    """Lengths 30 to 400, every 40th read shorter than k, about 2 % of the reads with N (one base, a run, or all)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ln = int(rng.integers(1, K)) if i % 40 == 7 else int(rng.integers(30, 401))
        s = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=ln).tobytes())
        if i % 50 == 3:
            kind = (i // 50) % 3
            if kind == 0:
                s[int(rng.integers(0, ln))] = ord("N")
            elif kind == 1:
                a = int(rng.integers(0, ln))
                s[a:a + 25] = b"N" * len(s[a:a + 25])
            else:
                s[:] = b"N" * ln
        out.append(bytes(s))
    return out


def _fastq(reads):
    return b"".join(b"@r%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n" for i, s in enumerate(reads))


def _fasta(reads):
    return b"".join(b">r%d\n" % i + b"".join(s[j:j + 60] + b"\n" for j in range(0, len(s), 60)) for i, s in enumerate(reads))


@pytest.fixture(scope="module")
def case(oracle):
    """The reads and the two expectations, computed once: plain (N packed as the packers pack it) and over clean k-mers."""
    reads = _reads(11)
    seq = b"".join(reads)
    starts = np.concatenate([[0], np.cumsum([len(s) for s in reads])]).astype(np.uint64)
    packed, amb = oracle.pack_ascii_n(seq)
    ho = oracle.default_hasher(True)
    plain = oc.expect_packed(oracle, oracle.pack_ascii(seq), starts, K, ho)
    clean = ac.expect_packed_amb(oracle, packed, starts, K, ho, amb)
    with_n = [i for i, s in enumerate(reads) if b"N" in s]
    assert 40 <= len(with_n) <= 80 and (clean[with_n] != plain[with_n]).any()
    assert (clean == oc.NO_MINIMIZER).sum() > (plain == oc.NO_MINIMIZER).sum() >= 70
    return {"reads": reads, "plain": plain, "clean": clean, "fastq": _fastq(reads), "fasta": _fasta(reads)}


def _stream(sm, text, **options):
    """(one_min or None, pos, values or None, records, batches) of the whole text, fed in pieces of PIECE bytes."""
    b = sm.canonical_minimizers(K, W)
    one, pos, vals, n_rec, n_batches = [], [], [], 0, 0
    for batch in sm.stream_fastx(b, [text[i:i + PIECE] for i in range(0, len(text), PIECE)], CHUNK, MAX_RECORDS, slots=SLOTS,
                                 **options):
        n_batches += 1
        n_rec += batch.n_records
        if batch.one_min is not None:
            assert len(batch.one_min) == batch.n_records
            one.append(batch.one_min)
        pos.append(batch.pos)
        if batch.values is not None:
            vals.append(batch.values)
    cat = lambda xs, t: np.concatenate(xs).astype(t) if xs else None  # noqa: E731
    return cat(one, np.uint32), cat(pos, np.uint32), cat(vals, np.uint64), n_rec, n_batches


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
@pytest.mark.parametrize("skip", [False, True])
def test_stream_one_minimizer(sm, case, fmt, skip):
    text, n = case[fmt], len(case["reads"])
    want = case["clean"] if skip else case["plain"]
    base_one, base_pos, base_vals, base_n, batches = _stream(sm, text, skip_ambiguous=skip, values="u64")
    assert base_one is None and base_n == n and batches >= 24  # (dozens of chunks)
    for values in (None, "u64"):
        one, pos, vals, n_rec, _ = _stream(sm, text, skip_ambiguous=skip, values=values, one_minimizer=True)
        assert n_rec == n and len(one) == n
        bad = np.nonzero(one != want)[0]
        assert not len(bad), (fmt, skip, values, bad[:8], one[bad[:8]], want[bad[:8]])
        # positions and values: unchanged from the same stream without the flag
        assert np.array_equal(pos, base_pos)
        if values:
            assert np.array_equal(vals, base_vals)
        else:
            assert vals is None


def test_delivery_entry(sm, case):
    """NULL and 0 without the flag and before the first batch; the batch's words with it."""
    L = sm.lib()
    b = sm.canonical_minimizers(K, W)
    text = case["fastq"][: 3 * CHUNK]
    text = text[: text.rfind(b"\n@") + 1]
    for flag in (False, True):
        with sm.FastxStream(b, CHUNK, MAX_RECORDS, slots=SLOTS, one_minimizer=flag) as st:
            words, n = C.c_void_p(1), C.c_uint64(9)
            assert L.mm_fastx_stream_one_minimizer(st.h, C.byref(words), C.byref(n)) == 0
            assert not words.value and n.value == 0  # (before the first batch)
            assert st.feed(text) == len(text)
            st.finish()
            seen = 0
            for batch in st:
                words, n = C.c_void_p(1), C.c_uint64(9)
                assert L.mm_fastx_stream_one_minimizer(st.h, C.byref(words), C.byref(n)) == 0
                if flag:
                    assert words.value and n.value == batch.n_records and len(batch.one_min) == batch.n_records
                    assert np.array_equal(batch.one_min, case["plain"][seen:seen + batch.n_records])
                else:
                    assert not words.value and n.value == 0 and batch.one_min is None
                seen += batch.n_records
            assert seen == text.count(b"\n") // 4
