// crc32_check.cpp - the CRC32 of csrc/mm_crc32.h (the code the BGZF verify kernel runs) on the host, under AddressSanitizer
// and UBSan: tests/test_crc32_cpu.py compiles this file with g++ -fsanitize=address,undefined, writes messages and the
// CRC32s zlib gives them into a file and runs it.  Every message is a heap allocation of EXACTLY its size.  No device, no
// library: only the header.
//
// The file: u32 n_cases, then per case u32 length, u32 zlib's CRC32, the bytes.  Per case the bit-wise, byte-wise and
// sliced registers and the segment plan (at every start offset 0..15 behind a 16-byte boundary) must all give zlib's value.
// The case of 70 bytes is also split into 1..8 segments in EVERY way, empty segments included: the splits are walked as a
// table over (segments so far, bytes so far) that keeps the SET of registers the splits reaching that cell produce, so every
// distinct combine step of every split is computed once, and every cell must hold the one value of its prefix.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "../../simd-minimizers_amd/csrc/mm_crc32.h"

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static_assert(mm::crc32_table_entry(0, 1) == 0x77073096u, "table 0, entry 1 of the gzip CRC32");
static_assert(mm::crc32_xpow8(0) == mm::kCrc32One && mm::crc32_xpow8(1) == 0x00800000u, "x^0 and x^8");
static_assert(mm::crc32_mulmod(mm::kCrc32One, 0x12345678u) == 0x12345678u, "x^0 is the unit");

static uint32_t every_split(const uint8_t *p, uint32_t n, uint32_t max_segments, uint32_t want) {
    uint32_t bad = 0;
    std::vector<std::set<uint32_t>> reach(n + 1), next(n + 1);
    reach[0].insert(0xFFFFFFFFu);  // (the initial value, folded in once in front of the first segment)
    for (uint32_t k = 1; k <= max_segments; ++k) {
        for (auto &s : next) s.clear();
        for (uint32_t i = 0; i <= n; ++i)
            for (uint32_t v : reach[i])
                for (uint32_t j = i; j <= n; ++j) next[j].insert(mm::crc32_combine(v, mm::crc32_linear(0, p + i, j - i), j - i));
        for (uint32_t j = 0; j <= n; ++j) {
            const uint32_t prefix = mm::crc32_linear_bitwise(0xFFFFFFFFu, p, j);
            if (next[j].size() != 1 || *next[j].begin() != prefix) {
                fprintf(stderr, "splits into %u segments: %zu different registers for the first %u bytes\n", k, next[j].size(), j);
                ++bad;
            }
        }
        if (next[n].empty() || ~*next[n].begin() != want) ++bad;
        reach.swap(next);
    }
    return bad;
}

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
    for (uint32_t k = 0; k < 4; ++k)
        for (uint32_t i = 0; i < 256; ++i)
            if (mm::kCrc32Tables.t[256 * k + i] != mm::crc32_table_entry(k, i)) {
                fprintf(stderr, "table %u entry %u differs from its definition\n", k, i);
                return 1;
            }
    uint32_t n_cases = 0;
    if (!read_exact(f, &n_cases, 4)) return 2;
    uint32_t bad = 0, splits = 0;
    for (uint32_t c = 0; c < n_cases; ++c) {
        uint32_t head[2];
        if (!read_exact(f, head, sizeof head)) return 2;
        const uint32_t n = head[0], want = head[1];
        if (n > 65536) return 2;
        uint8_t *alloc = static_cast<uint8_t *>(malloc(n ? n : 1));
        const uint8_t *p = n ? alloc : nullptr;
        if (!read_exact(f, alloc, n)) return 2;
        const uint32_t bit = ~mm::crc32_linear_bitwise(0xFFFFFFFFu, p, n), byte = ~mm::crc32_linear_bytewise(0xFFFFFFFFu, p, n);
        const uint32_t sliced = mm::crc32_bytes(0, p, n);
        // (in two calls, the second continuing the first, as zlib's interface allows)
        const uint32_t two = mm::crc32_bytes(mm::crc32_bytes(0, p, n / 3), p + n / 3, n - n / 3);
        if (bit != want || byte != want || sliced != want || two != want) {
            fprintf(stderr, "case %u: %u bytes: bit-wise %08x byte-wise %08x sliced %08x in two calls %08x, zlib %08x\n", c, n, bit, byte,
                    sliced, two, want);
            ++bad;
        }
        for (uint32_t lo = 0; lo < 16; ++lo) {
            const uint32_t planned = mm::crc32_bytes_planned(p, n, lo);
            const mm::Crc32Plan plan = mm::crc32_plan(lo, n);
            if (planned != want || plan.T > mm::kCrc32Threads || (plan.S & 15u) || (n && (plan.r == 0 || plan.r > plan.S))) {
                fprintf(stderr, "case %u: %u bytes at offset %u: the plan (S %u T %u r %u) gives %08x, zlib %08x\n", c, n, lo, plan.S,
                        plan.T, plan.r, planned, want);
                ++bad;
            }
        }
        if (n == 70) {
            bad += every_split(p, n, 8, want);
            ++splits;
        }
        free(alloc);
    }
    fclose(f);
    if (splits == 0) {
        fprintf(stderr, "crc32_check: no case of 70 bytes to split\n");
        return 1;
    }
    if (bad) {
        fprintf(stderr, "crc32_check: %u checks of %u cases wrong\n", bad, n_cases);
        return 1;
    }
    printf("crc32_check OK: %u cases, %u split in every way\n", n_cases, splits);
    return 0;
}
