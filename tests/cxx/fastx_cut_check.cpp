/* The cut rule of the FASTA / FASTQ stream (simd-minimizers_amd/csrc/mm_fastx_cut.h) walked over a few texts on the host,
 * for every chunk length, with the tail carried as the stream carries it.  A stand-alone program for a sanitizer build
 * (-fsanitize=address,undefined): every chunk lies in a heap block of exactly its size, so a read past either end is
 * reported.  Checks that a cut never lies past the chunk, that the kept records of all pieces add up to the records of the
 * whole text, and that a last chunk keeps everything.  Exit code 0 = fine. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../simd-minimizers_amd/csrc/mm_fastx_cut.h"

static int walk(const std::string &text, int format) {
    uint64_t whole[3];
    {
        std::vector<uint8_t> exact(text.begin(), text.end());
        mm::fastx_cut_host(exact.data(), exact.size(), format, 1, whole);
    }
    if (whole[0] != text.size() || whole[2] != 0) return 1;
    for (size_t len = 1; len <= text.size() + 1; ++len) {
        std::string tail;
        uint64_t kept = 0;
        for (size_t at = 0; at < text.size() || !tail.empty();) {
            const size_t m = text.size() - at < len ? text.size() - at : len;
            const int last = at + m >= text.size();
            const std::string chunk = tail + text.substr(at, m);
            at += m;
            uint8_t *exact = (uint8_t *)malloc(chunk.size() ? chunk.size() : 1);
            if (!exact) return 99;
            memcpy(exact, chunk.data(), chunk.size());
            uint64_t out[3] = {0, 0, 0};
            mm::fastx_cut_host(exact, chunk.size(), format, last, out);
            free(exact);
            if (out[0] > chunk.size()) return 2;
            if (last && (out[0] != chunk.size() || out[2] != 0)) return 3;
            if (!last && out[2] > 1) return 4;
            if (!last && out[0] != 0 && format == mm::kFastxFastq && chunk[out[0] - 1] != '\n') return 5;
            kept += out[1];
            tail = chunk.substr(out[0]);
            if (last) break;
        }
        if (kept != whole[1]) {
            printf("format %d, chunk length %zu: %llu records kept, %llu in the text\n", format, len, (unsigned long long)kept,
                   (unsigned long long)whole[1]);
            return 6;
        }
    }
    return 0;
}

int main() {
    const char *fastq[] = {
        "@a\nACGT\n+\nIIII\n@b\nAC\n+\nII\n@c\n\n+\n\n",
        "@a\r\nACGT\r\n+\r\nIIII\r\n@b\r\nACGTAC\r\n+\r\n@@@@@@\r\n",
        "@a\nACGT\n+\n@III\n@b\nGG\n+\n>I",
        "@a\nAC\n+\nII\n\n\n\n\n@b\nACG\n+\nIII\n\n\n",
        "",
        "\n",
        "@only",
    };
    const char *fasta[] = {
        ">a\nACGT\nAC\n>b\n>c\nAAAA\n",
        "junk\nmore junk\n>a desc\nACGT\r\nGG\r\n>b\nTT",
        "no header at all\nnone\n",
        ">a",
        "",
        "\n\n>x\nA\n\n>y\n\nC\n",
    };
    for (const char *t : fastq) {
        const int r = walk(t, mm::kFastxFastq);
        if (r) return printf("FASTQ text failed: %d\n", r), 10 + r;
    }
    for (const char *t : fasta) {
        const int r = walk(t, mm::kFastxFasta);
        if (r) return printf("FASTA text failed: %d\n", r), 20 + r;
    }
    printf("fastx_cut_check: OK\n");
    return 0;
}
