// Builder::values_u64 / values_u128 of byte text (TextSeq) and their _many forms (one call for all records) through the
// C++ mirror of the builder: Output::values_* (src/lib.rs:584-629) of the Seq the text stands for - `&[u8]`
// (MM_TEXT_VALUES_BYTES, src/lib.rs:59-60) or packed-seq AsciiSeq (MM_TEXT_VALUES_DNA, src/lib.rs:59, :85-100) - checked
// per record against the single-text call and against the definitions written out below.
// Exit code 0 = every record's values agree; 77 = no GPU (the engine has no CPU fallback).
#include <cstdio>
#include <vector>

#include "simd_minimizers_amd.hpp"

using namespace simd_minimizers;

// the definitions: character j of the k-mer at bits 8j (BYTES) or its code (c >> 1) & 3 at bits 2j (DNA), canonical =
// min(forward, reverse complement); characters past the record's buffer do not occur here
static u128 value_of(const uint8_t *s, uint32_t len, int encoding, bool canonical) {
    u128 fwd = 0, rc = 0;
    for (uint32_t j = 0; j < len; ++j) {
        if (encoding == MM_TEXT_VALUES_BYTES) {
            fwd |= (u128)s[j] << (8 * j);
        } else {
            fwd |= (u128)((s[j] >> 1) & 3u) << (2 * j);
            rc |= (u128)(((s[len - 1 - j] >> 1) & 3u) ^ 2u) << (2 * j);
        }
    }
    return canonical && rc < fwd ? rc : fwd;
}

// records of lengths 0 .. 399 cut from one random ACGTacgt text, a few empty and too short ones among them
template <class B>
static int check_builder(const B &b, uint32_t len, bool canonical, int encoding, bool wide, int tag) {
    const uint64_t n = 40000;
    std::vector<uint8_t> data(n);
    uint64_t x = 0x9E3779B97F4A7C15ull * (uint64_t)(tag + 1);
    for (auto &c : data) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        c = (uint8_t)"ACGTacgt"[(x >> 32) & 7u];
    }
    std::vector<TextSeq> records;
    uint64_t at = 3;
    for (int r = 0; r < 200; ++r) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        const uint64_t rec = (r % 7 == 0) ? 0 : (r % 11 == 0 ? 6 : (x >> 40) % 400);
        if (at + rec > n) break;
        records.push_back(TextSeq{data.data() + at, rec});
        at += rec + (r % 3);
    }
    std::vector<uint32_t> pos;
    std::vector<uint64_t> offsets;
    b.run_many(records, pos, offsets);
    if (offsets.size() != records.size() + 1 || offsets.back() != pos.size() || pos.empty()) return 10 * tag + 1;
    const std::vector<uint64_t> v64 = wide ? std::vector<uint64_t>() : b.values_u64_many(records, pos, offsets, encoding);
    const std::vector<u128> v128 = wide ? b.values_u128_many(records, pos, offsets, encoding) : std::vector<u128>();
    if ((wide ? v128.size() : v64.size()) != pos.size()) return 10 * tag + 2;
    for (size_t r = 0; r < records.size(); ++r) {
        const std::vector<uint32_t> one(pos.begin() + offsets[r], pos.begin() + offsets[r + 1]);
        if (b.run_once(records[r]) != one) return 10 * tag + 3;
        const std::vector<uint64_t> s64 = wide ? std::vector<uint64_t>() : b.values_u64(records[r], one, encoding);
        const std::vector<u128> s128 = wide ? b.values_u128(records[r], one, encoding) : std::vector<u128>();
        if ((wide ? s128.size() : s64.size()) != one.size()) return 10 * tag + 4;
        for (size_t i = 0; i < one.size(); ++i) {
            const u128 want = value_of(records[r].data + one[i], len, encoding, canonical);
            const u128 many = wide ? v128[offsets[r] + i] : (u128)v64[offsets[r] + i];
            const u128 single = wide ? s128[i] : (u128)s64[i];
            if (many != want) return 10 * tag + 5;
            if (single != want) return 10 * tag + 6;
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
        if ((r = check_builder(canonical_minimizers(21, 11), 21, true, MM_TEXT_VALUES_DNA, false, 1))) return r;
        if ((r = check_builder(minimizers(5, 4), 5, false, MM_TEXT_VALUES_BYTES, false, 2))) return r;
        if ((r = check_builder(closed_syncmers(5, 4), 8, false, MM_TEXT_VALUES_BYTES, false, 3))) return r;  // len 8
        if ((r = check_builder(closed_syncmers(5, 4), 8, false, MM_TEXT_VALUES_BYTES, true, 4))) return r;
        if ((r = check_builder(closed_syncmers(15, 17), 31, false, MM_TEXT_VALUES_DNA, false, 5))) return r;
        if ((r = check_builder(canonical_closed_syncmers(31, 33), 63, true, MM_TEXT_VALUES_DNA, true, 6))) return r;
        if ((r = check_builder(minimizers(12, 5), 12, false, MM_TEXT_VALUES_BYTES, true, 7))) return r;
        // refusals carry the C ABI's codes: a canonical builder or a k-mer too long for `&[u8]` values
        const uint8_t text[32] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24};
        const std::vector<uint32_t> p = {0, 1};
        try {
            canonical_minimizers(5, 5).values_u64(TextSeq{text, 32}, p, MM_TEXT_VALUES_BYTES);
            return 91;
        } catch (const Error &e) {
            if (e.code != MM_ERR_BAD_MODE) return 92;
        }
        try {
            minimizers(9, 4).values_u64(TextSeq{text, 32}, p, MM_TEXT_VALUES_BYTES);
            return 93;
        } catch (const Error &e) {
            if (e.code != MM_ERR_VALUE_LEN) return 94;
        }
        // no records: empty results
        std::vector<uint32_t> pos;
        std::vector<uint64_t> offsets;
        const auto b = minimizers(5, 4);
        b.run_many(std::vector<TextSeq>(), pos, offsets);
        if (!b.values_u64_many(std::vector<TextSeq>(), pos, offsets, MM_TEXT_VALUES_BYTES).empty()) return 90;
    } catch (const Error &e) {
        printf("error: %s (code %d)\n", e.what(), e.code);
        return 99;
    }
    printf("values_text_example: ok\n");
    return 0;
}
