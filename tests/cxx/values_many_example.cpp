// Builder::values_u64_many / values_u128_many (one call for all reads) against Output::values_u64 / values_u128 of a
// loop over Builder::run (src/lib.rs:378, :584-629) through the C++ mirror of the builder.
// Exit code 0 = every read's values agree; 77 = no GPU (the engine has no CPU fallback).
#include <cstdio>
#include <vector>

#include "simd_minimizers_amd.hpp"

using namespace simd_minimizers;

// reads of lengths 0 .. 399 cut from one random sequence at every 2-bit phase, a few empty and too short ones among them
template <class B>
static int check_builder(const B &b, bool wide, int tag) {
    const uint64_t n = 40000;
    std::vector<uint8_t> data((n + 3) / 4 + 16, 0);
    uint64_t x = 0x9E3779B97F4A7C15ull * (uint64_t)(tag + 1);
    for (auto &byte : data) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        byte = (uint8_t)(x >> 32);
    }
    std::vector<PackedSeq> reads;
    uint64_t at = 3;
    for (int r = 0; r < 200; ++r) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        const uint64_t len = (r % 7 == 0) ? 0 : (r % 11 == 0 ? 9 : (x >> 40) % 400);
        if (at + len > n) break;
        reads.push_back(PackedSeq{data.data(), at, len});
        at += len + (r % 3);
    }
    std::vector<uint32_t> pos;
    std::vector<uint64_t> offsets;
    b.run_many(reads, pos, offsets);
    if (offsets.size() != reads.size() + 1 || offsets.back() != pos.size() || pos.empty()) return 10 * tag + 1;
    const std::vector<uint64_t> v64 = wide ? std::vector<uint64_t>() : b.values_u64_many(reads, pos, offsets);
    const std::vector<u128> v128 = wide ? b.values_u128_many(reads, pos, offsets) : std::vector<u128>();
    if ((wide ? v128.size() : v64.size()) != pos.size()) return 10 * tag + 2;
    for (size_t r = 0; r < reads.size(); ++r) {
        std::vector<uint32_t> one;
        auto out = b.run(reads[r], one);
        if (one.size() != offsets[r + 1] - offsets[r]) return 10 * tag + 3;
        for (size_t i = 0; i < one.size(); ++i)
            if (one[i] != pos[offsets[r] + i]) return 10 * tag + 4;
        if (wide) {
            const std::vector<u128> want = out.values_u128();
            for (size_t i = 0; i < want.size(); ++i)
                if (want[i] != v128[offsets[r] + i]) return 10 * tag + 5;
        } else {
            const std::vector<uint64_t> want = out.values_u64();
            for (size_t i = 0; i < want.size(); ++i)
                if (want[i] != v64[offsets[r] + i]) return 10 * tag + 6;
        }
    }
    return 0;
}

int main() {
    if (mm_device_count() <= 0) {
        printf("no GPU\n");
        return 77;
    }
    try {
        int r;
        if ((r = check_builder(canonical_minimizers(21, 11), false, 1))) return r;
        if ((r = check_builder(minimizers(5, 7), false, 2))) return r;
        if ((r = check_builder(closed_syncmers(15, 17), false, 3))) return r;            // len 31
        if ((r = check_builder(canonical_closed_syncmers(31, 33), true, 4))) return r;   // len 63
        if ((r = check_builder(canonical_minimizers(43, 9), true, 5))) return r;
        // no reads, and reads without a window: empty results
        std::vector<uint32_t> pos;
        std::vector<uint64_t> offsets;
        const auto b = canonical_minimizers(21, 11);
        b.run_many(std::vector<PackedSeq>(), pos, offsets);
        if (!b.values_u64_many(std::vector<PackedSeq>(), pos, offsets).empty()) return 90;
    } catch (const Error &e) {
        printf("error: %s (code %d)\n", e.what(), e.code);
        return 99;
    }
    printf("values_many_example: ok\n");
    return 0;
}
