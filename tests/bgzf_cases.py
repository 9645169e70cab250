"""BGZF test material, built from raw bytes with Python's zlib (never with the code under test): whole BGZF blocks, a bit
writer that hand-assembles deflate payloads for the codes zlib never emits, the malformed payloads of the decoder's error
list, the mutation sweep, and the input file of tests/cxx/bgzf_inflate_check.cpp."""
import random
import struct
import zlib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def deflate(raw: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        return c.compress(raw) + c.flush()
    return c.compress(raw[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(raw[flush_at:]) + c.flush()


def member(payload: bytes, raw: bytes, extra_first=b"") -> bytes:
    """One BGZF block around a deflate payload; `extra_first`: another extra subfield in front of BC."""
    xlen = len(extra_first) + 6
    bsize = 12 + xlen + len(payload) + 8 - 1
    assert bsize < 65536
    head = struct.pack("<4BI2BH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, xlen) + extra_first + b"BC" + struct.pack("<HH", 2, bsize)
    return head + payload + struct.pack("<II", zlib.crc32(raw) & 0xffffffff, len(raw))


def block(raw: bytes, **kw) -> bytes:
    return member(deflate(raw, **kw), raw)


def bgzf(raw: bytes, sizes, eof=True, **kw) -> bytes:
    """raw cut into blocks of the given raw sizes (the last size repeats)."""
    out, at, i = [], 0, 0
    while at < len(raw):
        n = sizes[min(i, len(sizes) - 1)]
        out.append(block(raw[at:at + n], **kw))
        at += n
        i += 1
    return b"".join(out) + (EOF_BLOCK if eof else b"")


def zlib_inflate(payload: bytes):
    """What zlib makes of a raw deflate payload: its bytes when the final block's end was reached, else None."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload)
    except zlib.error:
        return None
    return out if d.eof else None


# ---- text
def fastq(n_reads: int, read_len: int, seed: int, with_n=False) -> bytes:
    rng = random.Random(seed)
    out = []
    for i in range(n_reads):
        seq = "".join(rng.choice("ACGT") for _ in range(read_len))
        if with_n and i % 3 == 0:
            p = rng.randrange(read_len)
            seq = seq[:p] + "N" * min(rng.randint(1, 4), read_len - p) + seq[p + 4:]
            seq = seq[:read_len].ljust(read_len, "A")
        qual = "".join(chr(33 + rng.randrange(2, 41)) for _ in range(read_len))
        out.append(f"@read{i} sample:{rng.randrange(1000)}\n{seq}\n+\n{qual}\n")
    return "".join(out).encode()


def fastq_bytes(n: int, seed: int) -> bytes:
    return fastq(n // 200 + 2, 100, seed)[:n]


# ---- hand-assembled deflate
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value: int, n: int):  # as deflate packs numbers: least significant bit first
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, n: int):  # a Huffman code: most significant bit first
        for i in range(n - 1, -1, -1):
            self.bits((code >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def done(self) -> bytes:
        self.align()
        return bytes(self.out)


def canon(lens):
    """canonical codes of a list of code lengths: {symbol: (code, length)}"""
    out, code = {}, 0
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


FIXED_LIT = canon([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canon([5] * 32)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def put_match(bw, length, dist, lit=FIXED_LIT, dcodes=FIXED_DIST, len_code=None):
    c = len_code if len_code is not None else max(i for i in range(29) if LEN_BASE[i] <= length and (i == 28 or length < 258))
    bw.code(*lit[257 + c])
    bw.bits(length - LEN_BASE[c], LEN_EXTRA[c])
    d = max(i for i in range(30) if DIST_BASE[i] <= dist)
    bw.code(*dcodes[d])
    bw.bits(dist - DIST_BASE[d], DIST_EXTRA[d])


def fixed_payload(ops, final=1) -> bytes:
    """ops: bytes (literals) or (length, dist) matches, in one fixed-Huffman block"""
    bw = BitWriter()
    bw.bits(final, 1)
    bw.bits(1, 2)
    for op in ops:
        if isinstance(op, (bytes, bytearray)):
            for b in op:
                bw.code(*FIXED_LIT[b])
        else:
            put_match(bw, *op)
    bw.code(*FIXED_LIT[256])
    return bw.done()


def dynamic_header(bw, hlit_field, hdist_field, cl_lens, cl_syms, final=1):
    """a dynamic block's header: the code-length code's 19 lengths, then code-length symbols (sym, extra value)"""
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    bw.bits(final, 1)
    bw.bits(2, 2)
    bw.bits(hlit_field, 5)
    bw.bits(hdist_field, 5)
    bw.bits(15, 4)
    for s in order:
        bw.bits(cl_lens[s], 3)
    codes = canon(cl_lens)
    for sym, extra in cl_syms:
        bw.code(*codes[sym])
        if sym >= 16:
            bw.bits(extra, {16: 2, 17: 3, 18: 7}[sym])


CL_PLAIN = [4] * 16 + [0, 0, 0]            # lengths 0..15 as four bits each, no repeat codes
CL_REPEAT = [4] * 14 + [0, 0, 4, 4, 0]     # lengths 0..13, and the repeat codes 16 and 17


def dynamic_payload(lit_lens, dist_lens, body, cl_lens=CL_PLAIN) -> bytes:
    """one dynamic block: the two sets' lengths written one by one, then body(bw, lit_codes, dist_codes)"""
    bw = BitWriter()
    dynamic_header(bw, len(lit_lens) - 257, len(dist_lens) - 1, cl_lens, [(l, 0) for l in list(lit_lens) + list(dist_lens)])
    body(bw, canon(lit_lens), canon(dist_lens))
    return bw.done()


def hand_assembled():
    """(name, payload): valid payloads with the codes zlib never emits; zlib says what they hold"""
    rng = random.Random(77)
    lits = bytes(rng.randrange(256) for _ in range(32768))
    out = [
        ("len285", fixed_payload([b"A", (258, 1)])),
        ("dist29_max", fixed_payload([lits, (200, 32768)])),
        ("dist_equals_produced", fixed_payload([b"0123456789", (20, 10)])),
    ]
    for d in (63, 64, 65):
        out.append((f"dist{d}_len258", fixed_payload([bytes(range(70)), (258, d), b"xyz", (258, d + 200)])))
    # a literal/length set of three codes and a distance set of ONE code of length 1 (incomplete; zlib writes such sets)
    lit = [0] * 258
    lit[65], lit[256], lit[257] = 1, 2, 2

    def body(bw, lc, dc):
        bw.code(*lc[65])
        bw.code(*lc[257])
        bw.code(*dc[0])
        bw.code(*lc[256])

    out.append(("single_dist_code", dynamic_payload(lit, [1], body)))
    # repeat codes 16 and 17 filling the sets exactly
    bw = BitWriter()
    syms = [(8, 0)] + [(16, 3)] * 23 + [(16, 2)]   # 144 eights: 1 + 23 * 6 + 5
    syms += [(9, 0)] + [(16, 3)] * 18 + [(16, 0)]  # 112 nines: 1 + 18 * 6 + 3
    syms += [(7, 0)] * 24 + [(8, 0)] * 4 + [(7, 0)] * 2   # 256 .. 285 (complete without 286 and 287)
    syms += [(4, 0)] * 2 + [(5, 0)] * 28                  # (complete without 30 and 31)
    dynamic_header(bw, 286 - 257, 30 - 1, CL_REPEAT, syms)
    lc, dc = canon([8] * 144 + [9] * 112 + [7] * 24 + [8] * 4 + [7] * 2), canon([4] * 2 + [5] * 28)
    for b in b"repeat codes":
        bw.code(*lc[b])
    put_match(bw, 30, 12, lc, dc)
    bw.code(*lc[256])
    out.append(("repeat_codes", bw.done()))
    return out


def valid_blocks():
    """[(name, raw, payload)]: about 60 payloads with every block type (the issue's list)"""
    rng = random.Random(5)
    out = [(f"tiny{n}", b"AC"[:n], deflate(b"AC"[:n])) for n in (0, 1, 2)]
    fq3, fq60 = fastq_bytes(3000, 1), fastq_bytes(60000, 2)
    out.append(("fastq3000_stored", fq3, deflate(fq3, level=0)))
    out.append(("fastq3000_fixed", fq3, deflate(fq3, strategy=zlib.Z_FIXED)))
    out.append(("fastq60000_dynamic", fq60, deflate(fq60)))
    out.append(("fastq60000_flush", fq60, deflate(fq60, flush_at=20000)))
    out.append(("run_of_A", b"A" * 65280, deflate(b"A" * 65280)))
    r30 = bytes(rng.randrange(256) for _ in range(30000))
    out.append(("random_twice", r30 + r30, deflate(r30 + r30, level=9)))
    r65 = bytes(rng.randrange(256) for _ in range(65180))
    out.append(("random_level1", r65, deflate(r65, level=1)))
    for name, payload in hand_assembled():
        raw = zlib_inflate(payload)
        assert raw is not None, name
        out.append((name, raw, payload))
    text = fastq(1600, 150, 9)
    at = 0
    for i in range(40):
        n = rng.randint(300, 65280) if i else 300  # (the smallest size is there for certain)
        if at + n > len(text):
            at = 0
        out.append((f"fastq_block{i}", text[at:at + n], deflate(text[at:at + n])))
        at += n
    return out


def malformed():
    """[(name, payload, isize)]: one hand-built payload per entry of the decoder's error list"""
    fq = fastq_bytes(3000, 3)
    good = deflate(fq)
    out = [
        ("input_exhausted", good[:len(good) // 2], len(fq)),
        ("input_exhausted_empty", b"", 5),
        ("output_passes_isize", good, len(fq) - 1),
        ("output_passes_isize_match", fixed_payload([b"A", (258, 1)]), 100),
        ("ends_short", good, len(fq) + 1),
        ("distance_too_far", fixed_payload([b"abc", (3, 4)]), 6),
        ("distance_at_start", fixed_payload([(3, 1)]), 3),
    ]
    bw = BitWriter()
    bw.bits(1, 1), bw.bits(3, 2)
    out.append(("block_type_3", bw.done() + b"\0" * 8, 4))
    out.append(("stored_len_nlen", b"\x01" + struct.pack("<HH", 4, 4 ^ 0xfff0) + b"abcd", 4))
    out.append(("stored_past_input", b"\x01" + struct.pack("<HH", 9, 9 ^ 0xffff) + b"abcd", 9))
    out.append(("stored_past_output", b"\x01" + struct.pack("<HH", 4, 4 ^ 0xffff) + b"abcd", 3))
    for code in (286, 287):
        bw = BitWriter()
        bw.bits(1, 1), bw.bits(1, 2)
        bw.code(*FIXED_LIT[65]), bw.code(*FIXED_LIT[code]), bw.bits(0, 16)
        out.append((f"litlen_code_{code}", bw.done(), 300))
    for code in (30, 31):
        bw = BitWriter()
        bw.bits(1, 1), bw.bits(1, 2)
        bw.code(*FIXED_LIT[65]), bw.code(*FIXED_LIT[257]), bw.code(*FIXED_DIST[code]), bw.bits(0, 16)
        out.append((f"dist_code_{code}", bw.done(), 300))
    eob_only = [0] * 256 + [1, 1]
    for name, hl, hd in (("hlit_287", 30, 0), ("hlit_288", 31, 0), ("hdist_31", 1, 30), ("hdist_32", 1, 31)):
        bw = BitWriter()
        dynamic_header(bw, hl, hd, CL_PLAIN, [(l, 0) for l in eob_only + [1] * 40])
        out.append((name, bw.done() + b"\0" * 4, 0))
    bw = BitWriter()
    dynamic_header(bw, 0, 0, CL_REPEAT, [(16, 0)] + [(1, 0)] * 300)
    out.append(("repeat_nothing", bw.done(), 0))
    bw = BitWriter()
    dynamic_header(bw, 0, 0, CL_REPEAT, [(0, 0)] * 255 + [(1, 0), (16, 3), (1, 0)])  # 256 + 6 > 257 + 1
    out.append(("repeat_past_end", bw.done(), 0))
    bw = BitWriter()
    dynamic_header(bw, 0, 0, CL_REPEAT, [(0, 0)] * 250 + [(17, 7), (1, 0)])  # 250 + 10 > 258
    out.append(("zeros_past_end", bw.done(), 0))
    lit = [0] * 257
    lit[65], lit[66] = 1, 1
    out.append(("no_end_of_block", dynamic_payload(lit, [1], lambda bw, lc, dc: bw.code(*lc[65])), 1))
    bw = BitWriter()
    dynamic_header(bw, 0, 0, [1, 1, 1] + [0] * 16, [])
    out.append(("oversubscribed_code_lengths", bw.done() + b"\0" * 40, 0))
    lit = [0] * 257
    lit[65], lit[66], lit[256] = 1, 1, 1
    out.append(("oversubscribed_litlen", dynamic_payload(lit, [1], lambda bw, lc, dc: None) + b"\0" * 4, 0))
    out.append(("oversubscribed_dist", dynamic_payload([0] * 256 + [1, 1], [1, 1, 1], lambda bw, lc, dc: None) + b"\0" * 4, 0))
    bw = BitWriter()
    dynamic_header(bw, 0, 0, [1] + [0] * 18, [])
    out.append(("incomplete_code_lengths", bw.done() + b"\0" * 40, 0))
    lit = [0] * 257
    lit[65], lit[256] = 2, 2
    out.append(("incomplete_litlen", dynamic_payload(lit, [1], lambda bw, lc, dc: bw.code(*lc[256])) + b"\0" * 4, 0))
    out.append(("incomplete_dist", dynamic_payload([0] * 256 + [1, 1], [2, 2, 0], lambda bw, lc, dc: bw.code(*lc[256])) + b"\0" * 4, 0))
    # the other bit of a set with ONE code of length 1 is no code
    lit = [0] * 258
    lit[65], lit[256], lit[257] = 1, 2, 2

    def body(bw, lc, dc):
        bw.code(*lc[65]), bw.code(*lc[257]), bw.bits(1, 1), bw.bits(0, 16)

    out.append(("no_such_distance_code", dynamic_payload(lit, [1], body), 4))
    for name, payload, isize in out:
        raw = zlib_inflate(payload)
        assert raw is None or len(raw) != isize, f"{name}: zlib takes it"
    return out


# The decoder's error (csrc/mm_inflate.h, kInflate*) that each case of malformed() is built for.
INFLATE_INPUT, INFLATE_OUTPUT, INFLATE_SHORT, INFLATE_DISTANCE, INFLATE_TYPE, INFLATE_STORED, INFLATE_LIT_CODE = 1, 2, 3, 4, 5, 6, 7
INFLATE_DIST_CODE, INFLATE_COUNTS, INFLATE_REPEAT, INFLATE_NO_END, INFLATE_OVER, INFLATE_INCOMPLETE, INFLATE_NO_CODE = 8, 9, 10, 11, 12, 13, 14
MALFORMED_CODES = {
    "input_exhausted": INFLATE_INPUT, "input_exhausted_empty": INFLATE_INPUT, "stored_past_input": INFLATE_INPUT,
    "output_passes_isize": INFLATE_OUTPUT, "output_passes_isize_match": INFLATE_OUTPUT, "stored_past_output": INFLATE_OUTPUT,
    "ends_short": INFLATE_SHORT, "distance_too_far": INFLATE_DISTANCE, "distance_at_start": INFLATE_DISTANCE,
    "block_type_3": INFLATE_TYPE, "stored_len_nlen": INFLATE_STORED,
    "litlen_code_286": INFLATE_LIT_CODE, "litlen_code_287": INFLATE_LIT_CODE,
    "dist_code_30": INFLATE_DIST_CODE, "dist_code_31": INFLATE_DIST_CODE,
    "hlit_287": INFLATE_COUNTS, "hlit_288": INFLATE_COUNTS, "hdist_31": INFLATE_COUNTS, "hdist_32": INFLATE_COUNTS,
    "repeat_nothing": INFLATE_REPEAT, "repeat_past_end": INFLATE_REPEAT, "zeros_past_end": INFLATE_REPEAT,
    "no_end_of_block": INFLATE_NO_END,
    "oversubscribed_code_lengths": INFLATE_OVER, "oversubscribed_litlen": INFLATE_OVER, "oversubscribed_dist": INFLATE_OVER,
    "incomplete_code_lengths": INFLATE_INCOMPLETE, "incomplete_litlen": INFLATE_INCOMPLETE, "incomplete_dist": INFLATE_INCOMPLETE,
    "no_such_distance_code": INFLATE_NO_CODE,
}


def mutations(n_payloads=20, n_positions=200, seed=11):
    """[(payload, isize, want)]: valid payloads with one byte changed; want = zlib's bytes when it reaches the final
    block's end with exactly isize bytes, else None (our decoder must fail: it shares zlib's rules and has no history)."""
    rng = random.Random(seed)
    small = [(raw, p) for _, raw, p in valid_blocks() if 0 < len(p) <= 20000][:n_payloads]
    out = []
    for raw, payload in small:
        for _ in range(n_positions):
            at = rng.randrange(len(payload))
            m = bytearray(payload)
            m[at] ^= 1 << rng.randrange(8) if rng.random() < 0.5 else rng.randrange(1, 256)
            got = zlib_inflate(bytes(m))
            out.append((bytes(m), len(raw), got if got is not None and len(got) == len(raw) else None))
    return out


def write_check_file(path, cases):
    """the input of tests/cxx/bgzf_inflate_check.cpp: cases (payload, isize, want or None); little-endian words
    {comp_len, isize, has_want} then the payload then, with has_want, isize bytes"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for payload, isize, want in cases:
            f.write(struct.pack("<III", len(payload), isize, 0 if want is None else 1))
            f.write(payload)
            if want is not None:
                assert len(want) == isize
                f.write(want)


def all_check_cases():
    cases = [(p, len(raw), raw) for _, raw, p in valid_blocks()]
    cases += [(p, isize, None) for _, p, isize in malformed()]
    return cases + mutations()
