"""FASTA / FASTQ text with N on the device: the packers that also write the ambiguity bits of a PackedNSeq
(mm_fasta_pack_n_device, mm_fastq_pack_n_device_async) and the skip-ambiguous run over the records they write
(mm_run_packed_reads_skip_ambiguous_*; Builder::run_skip_ambiguous_windows per record, src/lib.rs:451-496).  Every
expectation comes from the oracle - its restated readers (fasta_records / fastq_records), pack_ascii_n and
run_skip_ambiguous - and every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 16384   # text bytes per workgroup of the pack kernels (mm_text.h)
PIECE = 8192    # ... per piece of a workgroup
GROUP = 256     # chunks per group of the resolve step


def expect(oracle, text, fastq=False):
    if fastq:  # (blank bytes in front of the first '@' are cut off, text positions stay absolute: mm_fasta_pack_device)
        lead = len(text) - len(text.lstrip(b" \t\r\n"))
        recs = [(p + lead, h, s) for p, h, s in oracle.fastq_records(text[lead:])]
    else:
        recs = oracle.fasta_records(text)
    seq = b"".join(s for _, _, s in recs)
    base = np.cumsum([0] + [len(s) for _, _, s in recs]).astype(np.uint64)
    packed, amb = oracle.pack_ascii_n(seq)
    return recs, seq, base, packed[: (len(seq) + 3) // 4], amb[: (len(seq) + 7) // 8]


def check(sm, oracle, text, fastq=False, d_text=None, **kw):
    """The N packer against the oracle and, byte for byte over everything both clear, against the plain packer."""
    recs, seq, base, packed, amb = expect(oracle, text, fastq)
    src = text if d_text is None else d_text
    plain = sm.fasta_pack_device(src, **kw)
    got = sm.fasta_pack_n_device(src, **kw)
    n = len(text)
    assert len(got) == len(recs) == len(plain), (len(got), len(recs), len(plain))
    assert np.array_equal(got.base, base) and np.array_equal(got.base, plain.base)
    assert [int(p) for p in got.text_pos] == [p for p, _, _ in recs] == [int(p) for p in plain.text_pos]
    cleared = n // 4 + 8 if n else 0  # (what either packer clears at least; an empty text's packed bytes are left unwritten by both)
    gp = got.packed[:cleared].cpu().numpy()
    assert np.array_equal(gp[: len(packed)], packed)
    assert np.array_equal(gp, plain.packed[:cleared].cpu().numpy())
    # counts[0] bits exactly: the last byte's bits past the last base and every byte up to the cleared length are zero
    ga = got.amb[: (n // 8 + 8 + 3) // 4 * 4].cpu().numpy()
    assert np.array_equal(ga[: len(amb)], amb)
    assert not ga[len(amb):].any()
    return got


FASTA_CASES = [
    b"",
    b"\n",
    b">only a header",
    b">h\n",
    b">n\nNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN\nNNNN\n",  # a record of only N
    b">lower\nacgtnacgtnnacgtacgtacgtacgtacgtacgtnacgtacgtacgtacgtacgtacgtacgtacgtn\nacgtn\n",
    b">iupac\nACGTRYSWKMBDHVNU-*.acgtryswkmbdhvnu\nAC-GT*AC\n>b\n-\n",
    b">a\r\nACGTN\r\nGGNN\r\n>b\r\nTTNAC\r\nN\r\n",
    b">a\nACNGT\nNAC",                                   # no final newline
    b"junk NNNN before\nNNNN\n>chr1\nACGTNNNN\n\n\nacgt\n>c2\n>c3\nGG>T\nNA",  # bytes (and N) before the first header
    b">x\n" + b"ACGTN" * 5000,                              # one long line over a chunk seam
    b">x\n" + b"\n".join(b"ACNGTTGNCA"[: 1 + i % 10] for i in range(6000)) + b"\n>y\nGATTNACA\n",  # lines shorter than a piece
]

FASTQ_CASES = [
    b"@only a header",
    b"@h\n",
    b"@n\nNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n",
    b"@lower\nacgtnacgtn\n+\nIIIIIIIIII\n@r2\nnnacg\n+\nNNNNN\n",
    b"@iupac\nACGTRYSWKMBDHVNU-*.acgtryswkmbdhvnu\n+\nNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN\n",
    b"@a\r\nACGTN\r\n+\r\nNNNNN\r\n@b\r\nTTNAC\r\n+b\r\n@>N@>\r\n",
    b"@a\nACNGT\n+\nIIIII\n@b\nNAC\n+\nNN>",               # no final newline
    b"\n \n@a\nACNGT\n+\n@@@@@\n@b\nNAC\n+\n>>>\n\n\n",    # blank bytes before the first record, blank lines after the last
]


def test_known_small_texts(sm, oracle, gpu):
    for text in FASTA_CASES:
        check(sm, oracle, text)
    for text in FASTQ_CASES:
        check(sm, oracle, text, fastq=True)


# ------------------------------------------------------------------------------------------------------------ seams
RUNS = (1, 31, 32, 33, 70)


def put_runs(text, is_seq, run):
    """Overwrites sequence bytes of `text` (bytearray; is_seq marks them) with runs of `run` N - each run consecutive in the
    OUTPUT, whatever line ends or header bytes lie between its bytes - that straddle: a 32-byte thread piece, the 8 KB
    piece boundary, both chunk boundaries, an output base that starts a 32-base ambiguity dword and one that starts a
    16-base code dword in the middle of an ambiguity dword.  Returns the output bases of the run starts."""
    seq_pos = np.flatnonzero(is_seq)  # text position of output base j
    starts = []

    def at_output(j0):
        j0 = max(0, min(int(j0), len(seq_pos) - run))
        for j in range(j0, j0 + run):
            text[seq_pos[j]] = ord("N")
        starts.append(j0)

    def at_text(p):  # the run's middle on the first sequence byte at or behind text position p
        j = int(np.searchsorted(seq_pos, p))
        at_output(j - run // 2)

    for p in (4000 // 32 * 32, PIECE, CHUNK, CHUNK + PIECE, 2 * CHUNK):
        at_text(p)
    total = len(seq_pos)
    for j in (total // 5 // 32 * 32, total // 3 // 32 * 32 + 16, total // 2 // 32 * 32 + 16, total * 3 // 4 // 32 * 32):
        at_output(j - run // 2 if run > 1 else j)
        at_output(j + 200 - (run - 1))  # ... and one that ENDS on base j + 200 (the last bit of its dword when j + 200 = 31 mod 32)
    return starts


def seam_fasta(rng, n_target):
    """Random FASTA of about n_target bytes, line lengths 1..200 (many shorter than a thread's 32 bytes: the bit-by-bit
    path), a new record now and then; returns (bytearray, is_seq)."""
    out, mask = bytearray(), []

    def add(b, seq):
        out.extend(b)
        mask.extend([seq] * len(b))

    add(b">first record\n", False)
    while len(out) < n_target:
        if rng.random() < 0.03:
            add(b">r%d x\n" % len(out), False)
        m = int(rng.integers(1, 201)) if rng.random() < 0.7 else int(rng.integers(1, 32))
        add(rng.choice(list(b"ACGTacgt"), size=m).astype(np.uint8).tobytes(), True)
        add(b"\n", False)
    return out, np.array(mask, dtype=np.int64)


def seam_fastq(rng, n_target):
    """The FASTQ twin: reads of 1..200 bases whose quality lines hold 'N', '>' and '@' (no bases: they must set no bit)."""
    out, mask = bytearray(), []

    def add(b, seq):
        out.extend(b)
        mask.extend([seq] * len(b))

    r = 0
    while len(out) < n_target:
        m = int(rng.integers(1, 201)) if rng.random() < 0.7 else int(rng.integers(1, 32))
        add(b"@read%d\n" % r, False)
        add(rng.choice(list(b"ACGTacgt"), size=m).astype(np.uint8).tobytes(), True)
        add(b"\n+\n", False)
        add(rng.choice(list(b"N>@IF#"), size=m).astype(np.uint8).tobytes(), False)
        add(b"\n", False)
        r += 1
    return out, np.array(mask, dtype=np.int64)


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_seams(sm, oracle, gpu, fastq):
    """40 KB of text (three chunks, two 16 KB seams) per run length; then one of them again from odd device addresses."""
    import torch
    rng = np.random.default_rng(77 + fastq)
    last = None
    for run in RUNS:
        text, is_seq = (seam_fastq if fastq else seam_fasta)(rng, 40_000)
        assert len(text) > 2 * CHUNK + 200
        starts = put_runs(text, is_seq, run)
        text = bytes(text)
        got = check(sm, oracle, text, fastq=fastq, max_records=1 << 12)
        # (the construction did what it says: every run is in the bits, whole)
        bits = np.unpackbits(got.amb[: (int(got.base[-1]) + 7) // 8].cpu().numpy(), bitorder="little")
        for j in starts:
            assert bits[j: j + run].all(), (run, j)
        last = text
    buf = torch.zeros(len(last) + 64, dtype=torch.uint8, device="cuda")
    for off in (1, 3, 6):
        buf[off: off + len(last)] = torch.from_numpy(np.frombuffer(last, dtype=np.uint8).copy()).cuda()
        check(sm, oracle, last, fastq=fastq, d_text=buf[off: off + len(last)], max_records=1 << 12)


def test_state_and_run_across_a_group(sm, oracle, gpu):
    """Just over 4 MB (256 chunks = one group of the resolve step): a record whose bases, and an N run inside them, lie
    across the group boundary."""
    rng = np.random.default_rng(31)
    acgt = np.frombuffer(b"ACGTacgt", dtype=np.uint8)
    edge = GROUP * CHUNK

    def lines(n):
        s = acgt[rng.integers(0, 8, n)].tobytes()
        return b"\n".join(s[i: i + 60] for i in range(0, n, 60)) + b"\n"

    head = b">a\n" + lines(4_200_000)
    head = head[: edge - 200]
    head = head[: head.rfind(b"\n") + 1]
    text = head + b">b spans the group boundary\n" + acgt[rng.integers(0, 8, edge - len(head) - 28 - 30)].tobytes() + b"N" * 70 + \
        lines(20_000) + b">c\nNNNN\n"
    assert text[edge - 1: edge + 1] == b"NN" and len(text) > edge
    got = check(sm, oracle, text)
    assert len(got) == 3


# ------------------------------------------------------------------------------------------------------------- runs
def n_fasta(rng, l, n_records=300):
    """About 300 records: shorter than l, exactly l, l + 1, 150, a few kbp and one of 40 kbp; 1 % of the bases N, in runs of
    1, l - 1, l and 500 (cut at the record's end), half of the runs in records drawn by length, half in records drawn
    evenly - so that the short records get theirs - and a run of 500 in the longest record; 60-base lines."""
    lens = [int(x) for x in rng.choice([l - 1, l, l + 1, 150, 3000], size=n_records - 1, p=[0.1, 0.15, 0.15, 0.5, 0.1])]
    lens.insert(n_records // 3, 40_000)
    seqs = [bytearray(rng.choice(list(b"ACGT"), size=m).astype(np.uint8).tobytes()) for m in lens]
    weights = np.array(lens, dtype=np.float64) / sum(lens)

    def put(i, run):
        p = int(rng.integers(0, lens[i]))
        seqs[i][p: p + run] = b"N" * len(seqs[i][p: p + run])

    put(n_records // 3, 500)
    placed, evenly = 500, False
    while placed < sum(lens) // 100:
        run = int(rng.choice([1, l - 1, l, 500], p=[0.8, 0.08, 0.08, 0.04]))
        put(int(rng.integers(0, n_records)) if evenly else int(rng.choice(n_records, p=weights)), run)
        placed += run
        evenly = not evenly
    parts = [b">rec%d\n" % i + b"\n".join(bytes(s[j: j + 60]) for j in range(0, len(s), 60)) + b"\n" for i, s in enumerate(seqs)]
    return b"".join(parts), lens


PLANS = [(21, 11, 0), (31, 51, 0), (15, 17, 1)]  # (k, w, mode): minimizers; landing area and row chunks; closed syncmers


def builder_of(sm, k, w, mode):
    return sm.canonical_minimizers(k, w) if mode == 0 else sm.canonical_closed_syncmers(k, w)


def oracle_runs(oracle, text, k, w, mode, fastq=False):
    out = []
    for _, _, s in (oracle.fastq_records if fastq else oracle.fasta_records)(text):
        p, a = oracle.pack_ascii_n(s)
        out.append(oracle.run_skip_ambiguous(p, a, len(s), k, w, canonical=True, mode=(oracle.MINIMIZERS, oracle.CLOSED_SYNCMERS)[mode]))
    return out


def run_records(sm, b, recs, skip=True):
    import torch
    total = int(recs.base[-1]) if len(recs) else 0
    out = torch.zeros(total + 64, dtype=torch.int32, device="cuda")
    offs = torch.zeros(len(recs) + 1, dtype=torch.int64, device="cuda")
    if skip:
        cnt = sm.run_packed_reads_skip_ambiguous_device(b, recs, out, offs)
    else:
        cnt = sm.run_packed_reads_device(b, recs, out, offs)
    offs = offs.cpu().numpy()
    assert int(offs[-1]) == cnt
    return out[:cnt].cpu().numpy().view(np.uint32), offs


@pytest.mark.parametrize("k,w,mode", PLANS)
def test_file_to_minimizers(sm, oracle, gpu, monkeypatch, k, w, mode):
    rng = np.random.default_rng(1000 + k)
    text, lens = n_fasta(rng, k + w - 1)
    want = oracle_runs(oracle, text, k, w, mode)
    want_offs = np.cumsum([0] + [len(x) for x in want])
    want_pos = np.concatenate(want)
    recs = sm.fasta_pack_n_device(text)
    assert recs.lengths() == lens
    b = builder_of(sm, k, w, mode)
    for policy in (None, "1", "0"):  # MM_LANE_TABLE: the policy, the lane table forced, switched off
        if policy is None:
            monkeypatch.delenv("MM_LANE_TABLE", raising=False)
        else:
            monkeypatch.setenv("MM_LANE_TABLE", policy)
        pos, offs = run_records(sm, b, recs)
        assert np.array_equal(offs, want_offs), policy
        assert np.array_equal(pos, want_pos), policy


def test_no_leak_between_neighbours(sm, oracle, gpu):
    """A window inside a record covers that record's bases only: an N at the end of the record in front, or at the start of
    the record behind, changes nothing in a clean record - its output is the plain run of that record alone."""
    rng = np.random.default_rng(3)
    k, w = 21, 11

    def clean(m):
        return rng.choice(list(b"ACGT"), size=m).astype(np.uint8).tobytes()

    a, c, e = clean(200), clean(333), clean(5000)
    dirty_end, dirty_start = clean(150) + b"N" * 40, b"N" * 35 + clean(150)
    text = b"".join(b">r%d\n" % i + s + b"\n" for i, s in enumerate([dirty_end, a, dirty_start, dirty_end, c, dirty_start, e, dirty_end]))
    recs = sm.fasta_pack_n_device(text)
    pos, offs = run_records(sm, sm.canonical_minimizers(k, w), recs)
    for i, s in ((1, a), (4, c), (6, e)):
        alone = oracle.run(oracle.pack_ascii(s), len(s), k, w, canonical=True)
        assert np.array_equal(pos[offs[i]: offs[i + 1]], alone), i
    want = oracle_runs(oracle, text, k, w, 0)
    assert np.array_equal(pos, np.concatenate(want))


def test_clean_text_equals_the_plain_run(sm, oracle, gpu):
    rng = np.random.default_rng(8)
    parts = []
    for i in range(200):
        m = int(rng.choice([20, 31, 150, 400, 2500]))
        parts.append(b">c%d\n" % i + rng.choice(list(b"ACGTacgt"), size=m).astype(np.uint8).tobytes() + b"\n")
    recs = sm.fasta_pack_n_device(b"".join(parts))
    assert not recs.amb[: (int(recs.base[-1]) + 7) // 8].any()
    b = sm.canonical_minimizers(21, 11)
    pos, offs = run_records(sm, b, recs)
    pos0, offs0 = run_records(sm, b, recs, skip=False)
    assert len(pos) > 0 and np.array_equal(offs, offs0) and np.array_equal(pos, pos0)


def test_host_reads(sm, oracle, gpu):
    rng = np.random.default_rng(21)
    k, w = 21, 11
    reads = []
    for i in range(1000):
        s = bytearray(rng.choice(list(b"ACGTacgt"), size=int(rng.integers(30, 301))).astype(np.uint8).tobytes())
        for _ in range(int(rng.integers(0, 3))):
            p, run = int(rng.integers(0, len(s))), int(rng.choice([1, 2, 30, 31]))
            s[p: p + run] = b"N" * len(s[p: p + run])
        reads.append(bytes(s))
    pos, offs = sm.run_reads_skip_ambiguous_host(sm.canonical_minimizers(k, w), reads)
    assert len(offs) == len(reads) + 1
    for i, s in enumerate(reads):
        p, a = oracle.pack_ascii_n(s)
        assert np.array_equal(pos[offs[i]: offs[i + 1]], oracle.run_skip_ambiguous(p, a, len(s), k, w)), i
    pos, offs = sm.run_reads_skip_ambiguous_host(sm.canonical_minimizers(k, w), [])
    assert len(pos) == 0 and offs == [0]


def test_capacity(sm, oracle, gpu):
    """A d_amb one dword too small: MM_ERR_CAPACITY, the counts say what is needed, the dwords that fit are right and the
    guard words behind the buffer are untouched.  A misaligned d_amb is refused with a live workspace too."""
    import torch
    rng = np.random.default_rng(4)
    seq = rng.choice(list(b"ACGTN"), size=4000).astype(np.uint8).tobytes()
    for fastq in (False, True):
        text = (b"@r\n" + seq + b"\n+\n" + b"N" * len(seq) + b"\n") if fastq else (b">r\n" + seq[:1990] + b"\n" + seq[1990:] + b"\n")
        _, amb = oracle.pack_ascii_n(seq)
        need = (len(seq) + 31) // 32 * 4  # bytes, whole dwords
        guard = 0xA5
        t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
        packed = torch.zeros(len(text) // 4 + 64, dtype=torch.uint8, device="cuda")
        d_amb = torch.full((need + 64,), guard, dtype=torch.uint8, device="cuda")
        base = torch.zeros(9, dtype=torch.int64, device="cuda")
        tpos = torch.zeros(8, dtype=torch.int64, device="cuda")
        counts = torch.zeros(2, dtype=torch.int64, device="cuda")
        out = (C.c_uint64 * 2)()
        torch.cuda.synchronize()

        def pack(amb_ptr, cap):
            return sm.lib().mm_fasta_pack_n_device(gpu.h, C.c_void_p(t.data_ptr()), len(text), C.c_void_p(packed.data_ptr()),
                                                   packed.numel() // 4 * 4, C.c_void_p(amb_ptr), cap,
                                                   C.c_void_p(base.data_ptr()), C.c_void_p(tpos.data_ptr()), 8,
                                                   C.c_void_p(counts.data_ptr()), out)

        assert pack(d_amb.data_ptr(), need - 4) == sm.ERR["CAPACITY"]
        assert (out[0], out[1]) == (len(seq), 1) and out[0] > (need - 4) * 8
        host = d_amb.cpu().numpy()
        assert np.array_equal(host[: need - 4], amb[: need - 4])
        assert (host[need - 4:] == guard).all()
        assert pack(d_amb.data_ptr(), need) == 0
        host = d_amb.cpu().numpy()
        assert np.array_equal(host[:need], amb[:need]) and (host[need:] == guard).all()
        assert pack(d_amb.data_ptr() + 2, need) == sm.ERR["NULL"]
