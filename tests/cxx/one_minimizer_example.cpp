// one_minimizer / one_minimizer_many of the C++ mirror (src/minimizers.rs:22-28) over a handful of records, packed bases
// and byte text, against a loop written from the definition: the leftmost position that minimises hash & 0xffff0000,
//   h_fw(i) = fw_xor ^ XOR_j rotl(fw[s[i+j]], rot*(k-1-j));  h_rc(i) = rc_xor ^ XOR_j rotl(rc[s[i+j]], rot*j)
//   h = canonical ? h_fw + h_rc : h_fw.
// Compiling it needs no device; running it needs one.
#include <cstdio>
#include <vector>

#include "simd_minimizers_amd.hpp"

namespace sm = simd_minimizers;

static uint32_t rotl(uint32_t x, uint32_t r) {
    r &= 31u;
    return r ? (x << r) | (x >> (32u - r)) : x;
}

template <class Tables>
static uint32_t by_definition(const Tables &t, const std::vector<uint8_t> &s, uint32_t k) {
    uint32_t want = MM_NO_MINIMIZER, best = 0;
    for (size_t p = 0; p + k <= s.size(); ++p) {
        uint32_t f = t.fw_xor, r = t.rc_xor;
        for (uint32_t j = 0; j < k; ++j) {
            f ^= rotl(t.fw[s[p + j]], t.rot * (k - 1 - j));
            r ^= rotl(t.rc[s[p + j]], t.rot * j);
        }
        const uint32_t m = (t.canonical ? f + r : f) & 0xffff0000u;
        if (want == MM_NO_MINIMIZER || m < best) want = (uint32_t)p, best = m;
    }
    return want;
}

int main() {
    const uint32_t k = 21;
    const size_t lens[] = {150, 0, 20, 21, 5000, 9000, 1, 333};
    uint64_t x = 88172645463325252ull;
    auto rnd = [&]() {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        return x;
    };
    int bad = 0;
    // packed bases: every record at its own base offset inside its own buffer
    std::vector<std::vector<uint8_t>> codes, packed;
    std::vector<sm::PackedSeq> reads;
    size_t r = 0;
    for (size_t len : lens) {
        const size_t off = r++ % 4;
        std::vector<uint8_t> c(len), p((off + len + 3) / 4 + 1, 0);
        for (size_t i = 0; i < len; ++i) {
            c[i] = (uint8_t)(rnd() & 3);
            p[(off + i) >> 2] |= (uint8_t)(c[i] << (2 * ((off + i) & 3)));
        }
        codes.push_back(c);
        packed.push_back(p);
    }
    for (size_t i = 0; i < packed.size(); ++i) reads.push_back(sm::PackedSeq{packed[i].data(), i % 4, codes[i].size()});
    const sm::NtHasher<true> nt(k);
    const std::vector<uint32_t> got = sm::one_minimizer_many(reads, nt, k);
    for (size_t i = 0; i < reads.size(); ++i) {
        const uint32_t want = by_definition(nt.tables, codes[i], k);
        if (got[i] != want) ++bad, printf("packed record %zu: got %u want %u\n", i, got[i], want);
        if (codes[i].size() >= k && sm::one_minimizer(reads[i], nt, k) != want) ++bad, printf("packed single %zu\n", i);
    }
    // byte text
    std::vector<std::vector<uint8_t>> texts;
    std::vector<sm::TextSeq> records;
    for (size_t len : lens) {
        std::vector<uint8_t> t(len);
        for (auto &b : t) b = (uint8_t)rnd();
        texts.push_back(t);
    }
    for (const auto &t : texts) records.push_back(sm::TextSeq{t.data(), t.size()});
    const sm::TextMulHasher<false> mul(k);
    const std::vector<uint32_t> tgot = sm::one_minimizer_many(records, mul, k);
    for (size_t i = 0; i < records.size(); ++i) {
        const uint32_t want = by_definition(mul.tables, texts[i], k);
        if (tgot[i] != want) ++bad, printf("text record %zu: got %u want %u\n", i, tgot[i], want);
        if (texts[i].size() >= k && sm::one_minimizer(records[i], mul, k) != want) ++bad, printf("text single %zu\n", i);
    }
    bool threw = false;
    try {
        sm::one_minimizer(reads[2], nt, k);  // (20 bases: the reference panics)
    } catch (const sm::Error &) {
        threw = true;
    }
    if (!threw) ++bad, printf("a record shorter than k did not throw\n");
    printf("one_minimizer_example: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
