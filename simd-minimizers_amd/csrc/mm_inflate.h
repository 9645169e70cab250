// mm_inflate.h - RFC 1951 inflate of ONE BGZF payload into ONE output slot, written once for host and device: the kernel
// (mm_bgzf.hip, one wavefront per BGZF block), the host debug entry (mm_debug_bgzf_inflate), the stream's first block and
// the stand-alone check program (tests/cxx/bgzf_inflate_check.cpp) all run this code.  Plain C++, no HIP header needed.
// The reference reads compressed files through its loader's own gzip support on the CPU (needletail::parse_fastx_file,
// bench/src/lib.rs:51-82) and has no other counterpart.
//
// Contract of inflate_payload:
//   input  [payload, payload + comp_len), output [out, out + isize): nothing outside either range is loaded or stored,
//   whatever the bytes hold (the Io object does every access; the decoder hands it in-range offsets only).
//   0 = the final block's end-of-block code was reached and exactly isize bytes were produced.  Payload bytes BEHIND the
//   final block are ignored (BGZF's trailer follows there; a longer payload is the caller's matter).
//   Every other outcome is an error code (kInflate*), never undefined behaviour: input exhausted; output would pass isize
//   or ends short of it; a match distance larger than the bytes produced so far in THIS payload (there is no history across
//   BGZF blocks); block type 3; a stored block whose LEN / NLEN disagree; literal/length codes 286 / 287, distance codes
//   30 / 31; HLIT above 286 or HDIST above 30; a repeat code with nothing to repeat or one that runs past HLIT + HDIST; no
//   end-of-block code in the literal/length set; an over-subscribed code-length set; an incomplete one, other than what
//   zlib allows (a literal/length or distance set with at most one code, of length 1); bits that are no code of such a set.
//   Work is bounded: every step of the symbol loop consumes at least one input bit or ends, a match copies at most isize
//   bytes, a stored block at most comp_len.
//   The decoder verifies ISIZE and the deflate structure.  The CRC32 of the gzip trailer is verified ON REQUEST by code of
//   its own over the text written here: mm_crc32.h, the kernel mm_crc32.hip (mm_bgzf_crc32_device_async,
//   mm_bgzf_inflate_verify_host, the stream's MM_FASTX_BGZF_CRC).
//
// The decode state (bit buffer, offsets, tables) is the same in every lane of a wavefront: MM_INFLATE_UNIFORM makes that
// provable for what comes back from LDS, so the symbol loop is wave-uniform.  The Io object does the byte traffic:
//   uint32_t byte(i)                 payload[i], i < comp_len
//   void lit(pos, b)                 out[pos] = b
//   void copy(pos, dist, len)        out[pos + j] = out[pos + j - dist], j = 0 .. len - 1 in order (runs may overlap)
//   void stored(pos, in_off, len)    out[pos + j] = payload[in_off + j]
//   uint32_t lane(), lanes(); void sync()   who fills table entries (host: 0, 1, nothing)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MM_INFLATE_HD __host__ __device__ __forceinline__
#else
#define MM_INFLATE_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define MM_INFLATE_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define MM_INFLATE_UNIFORM(x) ((uint32_t)(x))
#endif

namespace mm {

enum {
    kInflateOk = 0,
    kInflateInput = 1,       // input exhausted
    kInflateOutput = 2,      // output would pass isize
    kInflateShort = 3,       // the stream ends short of isize
    kInflateDistance = 4,    // a match distance beyond the bytes produced so far
    kInflateType = 5,        // block type 3
    kInflateStored = 6,      // LEN / NLEN disagree
    kInflateLitCode = 7,     // literal/length code 286 or 287
    kInflateDistCode = 8,    // distance code 30 or 31
    kInflateCounts = 9,      // HLIT above 286 or HDIST above 30
    kInflateRepeat = 10,     // a repeat code with nothing to repeat, or past HLIT + HDIST
    kInflateNoEnd = 11,      // no end-of-block code
    kInflateOver = 12,       // over-subscribed code lengths
    kInflateIncomplete = 13, // incomplete code lengths
    kInflateNoCode = 14,     // bits that are no code of an incomplete set
    kInflateTable = 100      // (the kernel: a block-table entry beyond the buffers; nothing was read or written)
};

constexpr uint32_t kInflateLitFast = 9, kInflateDistFast = 8;  // bits of the first-level tables
constexpr uint32_t kBgzfMaxIsize = 65536;

// One wavefront's (or the host's) tables: canonical codes as counts per length + symbols in code order (the bit-serial
// decode, and what the first-level tables are filled from), and first-level tables indexed by the next bits of the
// stream: (symbol << 4) | length, 0 = the code is longer than the table's bits (or no code).
struct InflateTables {
    uint16_t lcount[16], lsym[288], lfast[1u << kInflateLitFast];
    uint16_t dcount[16], dsym[32], dfast[1u << kInflateDistFast];  // (also the code-length code, while a header is read)
    uint16_t offs[16];
    uint8_t lens[288 + 32];
};

// The bit-serial canonical decode of the code that `v` begins with (bit 0 first), codes of up to max_len bits:
// (symbol << 4) | length, or 0.
MM_INFLATE_HD uint32_t inflate_slow(const uint16_t *count, const uint16_t *sym, uint32_t v, uint32_t max_len) {
    int code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len <= max_len; ++len) {
        code |= (int)(v & 1u);
        v >>= 1;
        const int c = count[len];
        if (code - c < first) return ((uint32_t)sym[index + (code - first)] << 4) | len;
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return 0;
}

// Tables of the n code lengths lens[0 .. n).  `codes`: the code-length code, which must be complete.
template <class Io>
MM_INFLATE_HD int inflate_build(Io &io, const uint8_t *lens, uint32_t n, uint16_t *count, uint16_t *offs, uint16_t *sym, uint16_t *fast,
                                uint32_t fast_bits, bool codes) {
    for (uint32_t l = 0; l < 16; ++l) count[l] = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t l = MM_INFLATE_UNIFORM(lens[i]) & 15u;
        count[l] = (uint16_t)(MM_INFLATE_UNIFORM(count[l]) + 1u);
    }
    int left = 1;
    uint32_t max_len = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        const uint32_t c = MM_INFLATE_UNIFORM(count[l]);
        left = (left << 1) - (int)c;
        if (left < 0) return kInflateOver;
        if (c) max_len = l;
    }
    if (left > 0 && (codes || max_len > 1)) return kInflateIncomplete;
    uint32_t o = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        offs[l] = (uint16_t)o;
        o += MM_INFLATE_UNIFORM(count[l]);
    }
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t l = MM_INFLATE_UNIFORM(lens[i]) & 15u;
        if (l) {
            const uint32_t at = MM_INFLATE_UNIFORM(offs[l]);
            sym[at] = (uint16_t)i;
            offs[l] = (uint16_t)(at + 1u);
        }
    }
    io.sync();
    for (uint32_t e = io.lane(); e < (1u << fast_bits); e += io.lanes()) fast[e] = (uint16_t)inflate_slow(count, sym, e, fast_bits);
    io.sync();
    return kInflateOk;
}

// The bit buffer: bytes enter at the top, bits leave at bit 0.  Behind the input's end the buffer holds zeros, and `bits`
// says how many are real: a code that needs more than `bits` is "input exhausted".
struct InflateBits {
    uint64_t hold = 0;
    uint32_t bits = 0, in = 0, n = 0;
    template <class Io>
    MM_INFLATE_HD void fill(Io &io) {
        while (bits <= 56 && in < n) {
            hold |= (uint64_t)io.byte(in) << bits;
            ++in;
            bits += 8;
        }
    }
    MM_INFLATE_HD uint32_t peek(uint32_t k) const { return (uint32_t)hold & ((1u << k) - 1u); }
    MM_INFLATE_HD void drop(uint32_t k) {
        hold >>= k;
        bits -= k;
    }
};

// (the order in which a dynamic header lists the code-length code's lengths, five bits per entry)
MM_INFLATE_HD uint32_t inflate_clen_order(uint32_t i) {
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                        5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// One symbol of a set: first-level table, then the bit-serial decode.  0 = no code; else (symbol << 4) | length.
MM_INFLATE_HD uint32_t inflate_symbol(const InflateBits &b, const uint16_t *count, const uint16_t *sym, const uint16_t *fast,
                                      uint32_t fast_bits) {
    uint32_t e = MM_INFLATE_UNIFORM(fast[b.peek(fast_bits)]);
    if (!e) e = MM_INFLATE_UNIFORM(inflate_slow(count, sym, b.peek(15), 15));
    return e;
}

template <class Io>
MM_INFLATE_HD int inflate_dynamic_header(Io &io, InflateTables *t, InflateBits &b) {
    b.fill(io);
    if (b.bits < 14) return kInflateInput;
    const uint32_t hlit = b.peek(5) + 257u;
    b.drop(5);
    const uint32_t hdist = b.peek(5) + 1u;
    b.drop(5);
    const uint32_t hclen = b.peek(4) + 4u;
    b.drop(4);
    if (hlit > 286 || hdist > 30) return kInflateCounts;
    for (uint32_t i = 0; i < 19; ++i) t->lens[i] = 0;
    for (uint32_t i = 0; i < hclen; ++i) {
        b.fill(io);
        if (b.bits < 3) return kInflateInput;
        t->lens[inflate_clen_order(i)] = (uint8_t)b.peek(3);
        b.drop(3);
    }
    int r = inflate_build(io, t->lens, 19, t->dcount, t->offs, t->dsym, t->dfast, 7, true);
    if (r) return r;
    const uint32_t total = hlit + hdist;
    uint32_t i = 0, prev = 0;
    while (i < total) {
        b.fill(io);
        const uint32_t e = inflate_symbol(b, t->dcount, t->dsym, t->dfast, 7);
        if (!e) return kInflateNoCode;
        if ((e & 15u) > b.bits) return kInflateInput;
        b.drop(e & 15u);
        const uint32_t s = e >> 4;
        if (s < 16) {
            t->lens[i++] = (uint8_t)s;
            prev = s;
            continue;
        }
        uint32_t rep, val = 0, extra;
        if (s == 16) {
            if (i == 0) return kInflateRepeat;
            val = prev, extra = 2, rep = 3;
        } else if (s == 17) {
            extra = 3, rep = 3;
        } else {
            extra = 7, rep = 11;
        }
        if (b.bits < extra) return kInflateInput;  // (filled above: 15 + 7 bits fit behind one fill)
        rep += b.peek(extra);
        b.drop(extra);
        if (i + rep > total) return kInflateRepeat;
        for (uint32_t j = 0; j < rep; ++j) t->lens[i++] = (uint8_t)val;
        prev = val;
    }
    io.sync();
    if (MM_INFLATE_UNIFORM(t->lens[256]) == 0) return kInflateNoEnd;
    r = inflate_build(io, t->lens, hlit, t->lcount, t->offs, t->lsym, t->lfast, kInflateLitFast, false);
    if (r) return r;
    return inflate_build(io, t->lens + hlit, hdist, t->dcount, t->offs, t->dsym, t->dfast, kInflateDistFast, false);
}

template <class Io>
MM_INFLATE_HD int inflate_fixed_tables(Io &io, InflateTables *t) {
    for (uint32_t i = io.lane(); i < 288 + 32; i += io.lanes())
        t->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
    io.sync();
    int r = inflate_build(io, t->lens, 288, t->lcount, t->offs, t->lsym, t->lfast, kInflateLitFast, false);
    if (r) return r;
    return inflate_build(io, t->lens + 288, 32, t->dcount, t->offs, t->dsym, t->dfast, kInflateDistFast, false);
}

template <class Io>
MM_INFLATE_HD int inflate_payload(Io &io, InflateTables *t, uint32_t comp_len, uint32_t isize) {
    InflateBits b;
    b.n = comp_len;
    uint32_t pos = 0;
    for (;;) {
        b.fill(io);
        if (b.bits < 3) return kInflateInput;
        const uint32_t final_block = b.peek(1), type = (b.peek(3) >> 1);
        b.drop(3);
        if (type == 3) return kInflateType;
        if (type == 0) {
            b.drop(b.bits & 7u);
            b.fill(io);
            if (b.bits < 32) return kInflateInput;
            const uint32_t len = (uint32_t)b.hold & 0xffffu, nlen = ((uint32_t)b.hold >> 16) & 0xffffu;
            b.drop(32);
            if ((len ^ 0xffffu) != nlen) return kInflateStored;
            // (the buffer holds whole bytes now: they go back to the input)
            b.in -= b.bits >> 3;
            b.hold = 0;
            b.bits = 0;
            if (len > comp_len - b.in) return kInflateInput;
            if (len > isize - pos) return kInflateOutput;
            if (len) io.stored(pos, b.in, len);
            b.in += len;
            pos += len;
        } else {
            const int r = type == 1 ? inflate_fixed_tables(io, t) : inflate_dynamic_header(io, t, b);
            if (r) return r;
            for (;;) {
                b.fill(io);
                uint32_t e = inflate_symbol(b, t->lcount, t->lsym, t->lfast, kInflateLitFast);
                if (!e) return kInflateNoCode;
                if ((e & 15u) > b.bits) return kInflateInput;
                b.drop(e & 15u);
                uint32_t s = e >> 4;
                if (s < 256) {
                    if (pos >= isize) return kInflateOutput;
                    io.lit(pos, s);
                    ++pos;
                    continue;
                }
                if (s == 256) break;
                if (s > 285) return kInflateLitCode;
                // (length codes 257 .. 285: 3 .. 258; code c = s - 257 has (c >> 2) - 1 extra bits from c = 8 on)
                s -= 257;
                uint32_t len, extra = 0;
                if (s < 8) len = 3 + s;
                else if (s == 28) len = 258;
                else {
                    extra = (s >> 2) - 1;
                    len = 3 + ((4 + (s & 3u)) << extra);
                }
                if (b.bits < extra) return kInflateInput;  // (at least 56 - 15 bits stand behind the code when the input has them)
                len += b.peek(extra);
                b.drop(extra);
                b.fill(io);
                e = inflate_symbol(b, t->dcount, t->dsym, t->dfast, kInflateDistFast);
                if (!e) return kInflateNoCode;
                if ((e & 15u) > b.bits) return kInflateInput;
                b.drop(e & 15u);
                s = e >> 4;
                if (s > 29) return kInflateDistCode;
                // (distance codes 0 .. 29: 1 .. 32768; code c has (c >> 1) - 1 extra bits from c = 4 on)
                uint32_t dist;
                extra = 0;
                if (s < 4) dist = 1 + s;
                else {
                    extra = (s >> 1) - 1;
                    dist = 1 + ((2 + (s & 1u)) << extra);
                }
                if (b.bits < extra) return kInflateInput;
                dist += b.peek(extra);
                b.drop(extra);
                if (dist > pos) return kInflateDistance;
                if (len > isize - pos) return kInflateOutput;
                io.copy(pos, dist, len);
                pos += len;
            }
        }
        if (final_block) break;
    }
    return pos == isize ? kInflateOk : kInflateShort;
}

// The host's Io: plain loops over the two ranges.
struct InflateHostIo {
    const uint8_t *in;
    uint8_t *out;
    uint32_t byte(uint32_t i) const { return in[i]; }
    void lit(uint32_t pos, uint32_t b) { out[pos] = (uint8_t)b; }
    void copy(uint32_t pos, uint32_t dist, uint32_t len) {
        for (uint32_t j = 0; j < len; ++j) out[pos + j] = out[pos + j - dist];
    }
    void stored(uint32_t pos, uint32_t in_off, uint32_t len) {
        for (uint32_t j = 0; j < len; ++j) out[pos + j] = in[in_off + j];
    }
    uint32_t lane() const { return 0; }
    uint32_t lanes() const { return 1; }
    void sync() {}
};

inline int inflate_payload_host(const uint8_t *payload, uint32_t comp_len, uint8_t *out, uint32_t isize) {
    InflateTables t;
    InflateHostIo io{payload, out};
    return inflate_payload(io, &t, comp_len, isize);
}

// ---- the BGZF container (host): one gzip member's header.  0 = a whole member lies in data[0 .. n): *total its size,
// *payload_off / *comp_len its deflate payload, *isize its text size; 1 = incomplete (more bytes needed); -1 = a bad
// header; -2 = a gzip member without a BC subfield (plain gzip).
inline int bgzf_member(const uint8_t *d, uint64_t n, uint64_t *total, uint32_t *payload_off, uint32_t *comp_len, uint32_t *isize) {
    if (n >= 1 && d[0] != 0x1f) return -1;
    if (n >= 2 && d[1] != 0x8b) return -1;
    if (n >= 3 && d[2] != 8) return -1;
    if (n >= 4 && !(d[3] & 4)) return (d[3] & 0xe0) ? -1 : -2;
    if (n < 12) return 1;
    const uint32_t xlen = d[10] | (uint32_t)d[11] << 8;
    if (n < 12 + (uint64_t)xlen) return 1;
    uint32_t at = 0, bsize = 0;
    bool found = false;
    while (at + 4 <= xlen) {
        const uint8_t *f = d + 12 + at;
        const uint32_t slen = f[2] | (uint32_t)f[3] << 8;
        if (at + 4 + slen > xlen) return -1;
        if (f[0] == 'B' && f[1] == 'C' && slen == 2 && !found) {
            bsize = f[4] | (uint32_t)f[5] << 8;
            found = true;
        }
        at += 4 + slen;
    }
    if (at != xlen) return -1;
    if (!found) return -2;
    if (d[3] & ~5u) return -1;  // (FNAME / FCOMMENT / FHCRC: no BGZF writer sets them, and comp_len would count their bytes)
    const uint64_t size = (uint64_t)bsize + 1;
    if (size < 12ull + xlen + 8) return -1;
    if (n < size) return 1;
    *total = size;
    *payload_off = 12 + xlen;
    *comp_len = (uint32_t)(size - xlen - 20);
    *isize = d[size - 4] | (uint32_t)d[size - 3] << 8 | (uint32_t)d[size - 2] << 16 | (uint32_t)d[size - 1] << 24;
    return 0;
}
// the CRC32 of a whole member's trailer (d and total as bgzf_member found them): the four bytes in front of ISIZE
inline uint32_t bgzf_trailer_crc(const uint8_t *d, uint64_t total) {
    return d[total - 8] | (uint32_t)d[total - 7] << 8 | (uint32_t)d[total - 6] << 16 | (uint32_t)d[total - 5] << 24;
}

}  // namespace mm
