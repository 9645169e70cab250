// mm_fastx_cut.h - where a chunk of FASTA / FASTQ text is cut so that no record is split (the stream of
// mm_fastx_stream.hip hands a file of any size to the packers chunk by chunk; the reference has no counterpart beyond
// "the loader reads any file", bench/src/lib.rs:51-82).  ONE rule, called by the trim kernel (mm_fastx_cut.hip) and by the
// host (mm_debug_fastx_cut, tests/cxx/fastx_cut_check.cpp): plain C++, no HIP header needed.
//
// A chunk handed to the packers starts at a line whose global index is a multiple of 4 (FASTQ) or at the start of a line
// (FASTA).  With `last` everything is kept.  Otherwise
//   FASTQ  N = newlines of the chunk: cut = the offset behind the 4 * floor(N / 4)-th newline (0 when N < 4) - a line's
//          role is its index mod 4, so cuts on multiples of four lines leave every later line its role, blank lines or
//          not.  Kept records R' = tabulated records with rec_text_pos < cut (at most the last one is dropped).
//   FASTA  the last record is complete only when the next header has been seen: with R >= 1 records cut =
//          rec_text_pos[R - 1] and R' = R - 1; with R == 0 (only bytes in front of the first header) cut = the offset
//          behind the last newline (0 if there is none).
// Kept bases B' = rec_base[R'].  The rule needs table entry R - 1 (FASTQ: only to compare it with the cut), so it cannot
// be applied to a chunk with R > max_records: `overflow`.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MM_FASTX_HD __host__ __device__ __forceinline__
#else
#define MM_FASTX_HD inline
#endif

namespace mm {

constexpr int kFastxFasta = 1;  // (MM_FASTX_FASTA / MM_FASTX_FASTQ of the C header)
constexpr int kFastxFastq = 2;

struct FastxCut {
    uint64_t cut;       // bytes of the chunk that are kept: the next chunk starts with text[cut, n)
    uint64_t records;   // R'
    uint64_t bases;     // B' (0 when no rec_base table was given)
    uint32_t overflow;  // 1: R > max_records, the rule was not applied (cut = 0, the counts as they were)
};

// Which newline of the chunk the cut lies behind, counted from the END of the text (1 = the last one); 0 = the rule
// needs no newline (cut 0, `last`, or a FASTA chunk with records).
MM_FASTX_HD uint32_t fastx_cut_newline(int format, int last, uint64_t n_newlines, uint64_t n_records) {
    if (last) return 0u;
    if (format == kFastxFastq) return n_newlines < 4 ? 0u : (uint32_t)(n_newlines & 3u) + 1u;
    return (n_records == 0 && n_newlines != 0) ? 1u : 0u;
}

// The rule.  `newline_pos`: the offset of the newline fastx_cut_newline() names (unused when it names none);
// n_bases / n_records: the packer's counts; last_rec_text_pos: its rec_text_pos[n_records - 1] (the one entry of that table
// the rule reads; anything when there is no record or more than max_records); rec_base [max_records + 1] or null.
MM_FASTX_HD FastxCut fastx_cut_rule(int format, int last, uint64_t n, uint64_t n_newlines, uint64_t newline_pos,
                                    uint64_t n_bases, uint64_t n_records, uint64_t max_records,
                                    uint64_t last_rec_text_pos, const uint64_t *rec_base) {
    FastxCut c;
    c.cut = 0;
    c.records = n_records;
    c.bases = n_bases;
    c.overflow = 0;
    if (n_records > max_records) {
        c.overflow = 1;
        return c;
    }
    if (last) {
        c.cut = n;
        return c;
    }
    const uint32_t which = fastx_cut_newline(format, last, n_newlines, n_records);
    if (format == kFastxFastq) {
        c.cut = which ? newline_pos + 1 : 0;
        if (n_records && last_rec_text_pos >= c.cut) c.records = n_records - 1;
    } else if (n_records) {
        c.cut = last_rec_text_pos;
        c.records = n_records - 1;
    } else {
        c.cut = which ? newline_pos + 1 : 0;
    }
    if (c.records != n_records) c.bases = rec_base ? rec_base[c.records] : 0;
    return c;
}

// The rule on a text in HOST memory, the tables made by a plain reading of the text (the readers of the packers restated:
// FASTQ - a line 4r that holds a byte other than '\r' starts a record at that byte; FASTA - a line that begins with '>').
// out = {cut, kept records, dropped records}.
inline void fastx_cut_host(const uint8_t *text, uint64_t n, int format, int last, uint64_t out[3]) {
    uint64_t n_newlines = 0, n_records = 0, last_rec_pos = 0, line = 0;
    uint64_t nl[4] = {0, 0, 0, 0};  // the offsets of the last four newlines, nl[n_newlines % 4] the oldest
    uint64_t i = 0;
    while (i < n) {
        uint64_t e = i;
        while (e < n && text[e] != '\n') ++e;
        if (format == kFastxFastq) {
            if ((line & 3u) == 0) {
                uint64_t f = i;
                while (f < e && text[f] == '\r') ++f;
                if (f < e) {
                    ++n_records;
                    last_rec_pos = f;
                }
            }
        } else if (e > i && text[i] == '>') {
            ++n_records;
            last_rec_pos = i;
        }
        if (e < n) {
            nl[n_newlines & 3u] = e;
            ++n_newlines;
        }
        ++line;
        i = e + 1;
    }
    const uint32_t which = fastx_cut_newline(format, last, n_newlines, n_records);
    // (the which-th newline from the end: newline number n_newlines - which, counted from 0)
    const uint64_t newline_pos = which ? nl[(n_newlines - which) & 3u] : 0;
    const FastxCut c = fastx_cut_rule(format, last, n, n_newlines, newline_pos, 0, n_records, n_records, last_rec_pos, nullptr);
    out[0] = c.cut;
    out[1] = c.records;
    out[2] = n_records - c.records;
}

// ---- FASTA records longer than a chunk (MM_FASTX_LONG_RECORDS): the split rule.
// The rule above still decides whenever it gives cut > 0.  Where it gives cut == 0 in a chunk that is not the last and
// the chunk IS one record from its first byte on (R == 1, rec_text_pos[0] == 0) whose header line is complete (the chunk
// has a newline), the whole chunk is kept as a PIECE of an OPEN record: cut = n, and the next chunk's text begins with a
// synthetic header line ">\n" followed by text[T, n), the piece's last l - 1 sequence bytes (l = k + w - 1; a sequence
// byte is any byte of a sequence line but '\n' and '\r', as the packers read it).  T never lies inside the header line:
// a piece with fewer than l - 1 sequence bytes gives T = its first sequence byte (n when it has none).  Everything else
// with cut == 0 stays what it is today, a chunk that cannot be cut (a header line that is not complete, no record).
struct FastxSplit {
    FastxCut c;
    uint64_t T;        // 0 unless open
    uint32_t open;     // 1: the chunk is a piece of a record that goes on
    uint32_t overlap;  // sequence bytes in text[T, n): l - 1, or all the piece has (0 unless open)
};

// Is the split scan needed (the counts of the packer and of the newline pass decide; the scan is what costs)?
MM_FASTX_HD bool fastx_split_open(int format, int last, int long_records, uint64_t n_newlines, uint64_t n_records,
                                  uint64_t max_records, uint64_t first_rec_text_pos) {
    return long_records && !last && format == kFastxFasta && n_records == 1 && n_records <= max_records && first_rec_text_pos == 0 &&
           n_newlines != 0;
}

// The rule.  As fastx_cut_rule, plus: first_rec_text_pos = rec_text_pos[0] (anything without a record); scan_T / scan_seq =
// what the backward scan found (fastx_split_scan_* below: host and kernel count the same bytes), read only when
// fastx_split_open() holds.
MM_FASTX_HD FastxSplit fastx_split_rule(int format, int last, int long_records, uint64_t n, uint64_t n_newlines, uint64_t newline_pos,
                                        uint64_t n_bases, uint64_t n_records, uint64_t max_records, uint64_t first_rec_text_pos,
                                        uint64_t last_rec_text_pos, const uint64_t *rec_base, uint64_t scan_T, uint32_t scan_seq) {
    FastxSplit s;
    s.c = fastx_cut_rule(format, last, n, n_newlines, newline_pos, n_bases, n_records, max_records, last_rec_text_pos, rec_base);
    s.T = 0;
    s.open = 0;
    s.overlap = 0;
    if (s.c.overflow || s.c.cut != 0) return s;
    if (!fastx_split_open(format, last, long_records, n_newlines, n_records, max_records, first_rec_text_pos)) return s;
    s.c.cut = n;  // (the one record the old rule carries over is kept, all of it)
    s.c.records = n_records;
    s.c.bases = n_bases;
    s.T = scan_T;
    s.open = 1;
    s.overlap = scan_seq;
    return s;
}

MM_FASTX_HD bool fastx_is_line_end(uint8_t c) { return c == '\n' || c == '\r'; }

// The scan on a text in HOST memory, byte by byte from the end: stops at the (l - 1)-th sequence byte or at the FIRST
// newline of the text (the end of the header line of a chunk that fastx_split_open() accepts), whichever comes first; in
// the second case T moves forward over line ends to the first sequence byte.
inline void fastx_split_scan_host(const uint8_t *text, uint64_t n, uint64_t n_newlines, uint32_t l, uint64_t *scan_T, uint32_t *scan_seq) {
    const uint32_t want = l ? l - 1 : 0;
    uint64_t seen_nl = 0, i = n, T = n;
    uint32_t seq = 0;
    bool header = false;
    while (i > 0 && seq < want) {
        const uint8_t c = text[i - 1];
        if (c == '\n' && ++seen_nl == n_newlines) {
            header = true;
            break;
        }
        --i;
        if (!fastx_is_line_end(c)) {
            ++seq;
            T = i;
        }
    }
    if (header || want == 0) {
        // (want == 0 cannot be asked for through a plan: l >= 1 + 1 - 1; kept total for the debug call)
        T = header ? i : n;
        while (T < n && fastx_is_line_end(text[T])) ++T;
    }
    *scan_T = T;
    *scan_seq = seq;
}

// The split rule on a text in HOST memory, the tables made by a plain reading of the text as in fastx_cut_host.
// out = {cut, T, open, overlap}.
inline void fastx_split_host(const uint8_t *text, uint64_t n, uint32_t l, int last, uint64_t out[4]) {
    uint64_t n_newlines = 0, n_records = 0, first_rec_pos = 0, last_rec_pos = 0, last_nl = 0;
    uint64_t i = 0;
    while (i < n) {
        uint64_t e = i;
        while (e < n && text[e] != '\n') ++e;
        if (e > i && text[i] == '>') {
            if (n_records == 0) first_rec_pos = i;
            ++n_records;
            last_rec_pos = i;
        }
        if (e < n) {
            last_nl = e;
            ++n_newlines;
        }
        i = e + 1;
    }
    uint64_t scan_T = 0;
    uint32_t scan_seq = 0;
    if (fastx_split_open(kFastxFasta, last, 1, n_newlines, n_records, n_records, first_rec_pos))
        fastx_split_scan_host(text, n, n_newlines, l, &scan_T, &scan_seq);
    const FastxSplit s = fastx_split_rule(kFastxFasta, last, 1, n, n_newlines, last_nl, 0, n_records, n_records, first_rec_pos, last_rec_pos,
                                          nullptr, scan_T, scan_seq);
    out[0] = s.c.cut;
    out[1] = s.T;
    out[2] = s.open;
    out[3] = s.overlap;
}

}  // namespace mm
