// bgzf_inflate_check.cpp - the inflate of csrc/mm_inflate.h (the code the BGZF kernel runs) on the host, under
// AddressSanitizer and UBSan: tests/test_bgzf_cpu.py compiles this file with g++ -fsanitize=address,undefined, writes the
// cases (tests/bgzf_cases.py: the valid set, the malformed list, the mutation sweep) into a file and runs it.
// Every payload and every output slot is a heap allocation of EXACTLY its size, so a load outside the payload or a store
// outside the slot, whatever the bytes hold, is a sanitizer report.  No device, no library: only the header.
//
// The file: u32 n_cases, then per case u32 comp_len, u32 isize, u32 has_want, the payload, and with has_want isize bytes
// the decoder must produce; without it the decoder must fail.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../simd-minimizers_amd/csrc/mm_inflate.h"

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    uint32_t n_cases = 0;
    if (!read_exact(f, &n_cases, 4)) return 2;
    uint32_t ok = 0, refused = 0, bad = 0;
    for (uint32_t c = 0; c < n_cases; ++c) {
        uint32_t head[3];
        if (!read_exact(f, head, sizeof head)) return 2;
        const uint32_t comp_len = head[0], isize = head[1], has_want = head[2];
        if (isize > mm::kBgzfMaxIsize || comp_len > (1u << 20)) return 2;
        uint8_t *payload = static_cast<uint8_t *>(malloc(comp_len ? comp_len : 1));
        uint8_t *out = static_cast<uint8_t *>(malloc(isize ? isize : 1));
        uint8_t *exact_payload = comp_len ? payload : nullptr, *exact_out = isize ? out : nullptr;
        std::vector<uint8_t> want(has_want ? isize : 0);
        if (!read_exact(f, payload, comp_len) || !read_exact(f, want.data(), want.size())) return 2;
        if (isize) memset(out, 0xa5, isize);
        const int r = mm::inflate_payload_host(exact_payload, comp_len, exact_out, isize);
        if (has_want) {
            if (r != 0 || (isize && memcmp(out, want.data(), isize) != 0)) {
                fprintf(stderr, "case %u: comp_len %u isize %u: error %d or wrong bytes, the reference inflates it\n", c, comp_len, isize, r);
                ++bad;
            } else {
                ++ok;
            }
        } else if (r == 0) {
            fprintf(stderr, "case %u: comp_len %u isize %u: accepted, the reference does not give isize bytes\n", c, comp_len, isize);
            ++bad;
        } else {
            ++refused;
        }
        free(payload);
        free(out);
    }
    fclose(f);
    if (bad) {
        fprintf(stderr, "bgzf_inflate_check: %u of %u cases wrong\n", bad, n_cases);
        return 1;
    }
    printf("bgzf_inflate_check OK: %u inflated, %u refused\n", ok, refused);
    return 0;
}
