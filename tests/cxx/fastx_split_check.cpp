/* The split rule for FASTA records longer than a chunk (simd-minimizers_amd/csrc/mm_fastx_cut.h) walked over a few
 * records on the host, for every chunk length from 4 * l up, the pieces chained as the stream chains them: the next chunk
 * is ">\n" + text[T, n) + the new bytes.  A stand-alone program for a sanitizer build (-fsanitize=address,undefined): every
 * chunk lies in a heap block of exactly its size, so a read past either end is reported.  Checks that T lies inside the
 * chunk and behind its header line, that the overlap is what text[T, n) holds, that every piece brings new bases, and that
 * the pieces' bases minus their overlaps are the record's bases.  Exit code 0 = fine. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../simd-minimizers_amd/csrc/mm_fastx_cut.h"

static std::string bases_of(const std::string &chunk, size_t from) {
    std::string s;
    for (size_t i = from; i < chunk.size(); ++i)
        if (chunk[i] != '\n' && chunk[i] != '\r') s.push_back(chunk[i]);
    return s;
}

static int walk(const std::string &text, uint32_t l) {
    const std::string want = bases_of(text, text.find('\n') + 1);
    // (the stream's lower bound, and the header line with a base behind it in the first chunk)
    for (size_t len = 4 * (size_t)l < 16 ? 16 : 4 * (size_t)l; len <= text.size() + 1; ++len) {
        std::string carry, got;
        uint64_t overlap_in = 0;
        for (size_t at = 0;;) {
            const size_t m = text.size() - at < len ? text.size() - at : len;
            const int last = at + m >= text.size();
            const std::string chunk = carry + text.substr(at, m);
            at += m;
            uint8_t *exact = (uint8_t *)malloc(chunk.size() ? chunk.size() : 1);
            if (!exact) return 99;
            memcpy(exact, chunk.data(), chunk.size());
            uint64_t out[4] = {0, 0, 0, 0};
            mm::fastx_split_host(exact, chunk.size(), l, last, out);
            free(exact);
            const size_t header_end = chunk.find('\n') + 1;
            const std::string seq = bases_of(chunk, header_end);
            if (seq.compare(0, overlap_in, got, got.size() - overlap_in, overlap_in) != 0) return 1;
            got += seq.substr(overlap_in);
            if (last) {
                if (out[0] != chunk.size() || out[2] != 0) return 2;
                break;
            }
            if (out[2] != 1 || out[0] != chunk.size()) return 3;
            if (out[1] > chunk.size() || out[1] < header_end) return 4;
            if (bases_of(chunk, out[1]).size() != out[3] || out[3] != (seq.size() < l - 1 ? seq.size() : l - 1)) return 5;
            if (seq.size() <= overlap_in) return 6;
            carry = ">\n" + chunk.substr(out[1]);
            if (carry.size() > len + 2) return 7;
            overlap_in = out[3];
        }
        if (got != want) {
            printf("l %u, chunk length %zu: %zu bases joined, %zu in the record\n", l, len, got.size(), want.size());
            return 8;
        }
    }
    return 0;
}

int main() {
    std::string acgt;
    for (int i = 0; i < 700; ++i) acgt.push_back("ACGTN"[(i * 7 + i / 5) % 5]);
    auto fold = [&](size_t width, const char *nl, bool blank, bool final_nl) {
        std::string t = std::string(">chr1 test") + nl;
        for (size_t i = 0, j = 0; i < acgt.size(); i += width, ++j) {
            t += acgt.substr(i, width) + nl;
            if (blank && j % 3 == 2) t += nl;
        }
        if (!final_nl) t.resize(t.size() - strlen(nl));
        return t;
    };
    const std::string texts[] = {
        fold(60, "\n", false, true), fold(60, "\r\n", false, false), fold(1, "\r\n", false, true),
        fold(10, "\n", true, true),  fold(700, "\n", false, false),  fold(7, "\n", true, false),
    };
    const uint32_t ls[] = {2, 11, 31};
    for (const std::string &t : texts)
        for (uint32_t l : ls) {
            const int r = walk(t, l);
            if (r) return printf("text failed: %d\n", r), 10 + r;
        }
    // texts the rule does not open: an unfinished header line, no record, a record that does not start the chunk
    const char *closed[] = {">chr1 and no end", "ACGT", "", "AC\n>b\nACGT", ">a\nAC\n>b\nGT"};
    for (const char *t : closed) {
        const size_t n = strlen(t);
        uint8_t *exact = (uint8_t *)malloc(n ? n : 1);
        if (!exact) return 99;
        memcpy(exact, t, n);
        uint64_t out[4] = {9, 9, 9, 9}, old[3];
        mm::fastx_split_host(exact, n, 11, 0, out);
        mm::fastx_cut_host(exact, n, mm::kFastxFasta, 0, old);
        free(exact);
        if (out[2] != 0 || out[1] != 0 || out[3] != 0 || out[0] != old[0]) return printf("closed text failed: %s\n", t), 30;
    }
    printf("fastx_split_check: OK\n");
    return 0;
}
