// one_minimizer / one_minimizer_many of the C++ mirror over reads with ambiguity bits (PackedNSeq), and a FASTQ with N
// through Builder::stream_fastx with MM_FASTX_ONE_MINIMIZER | MM_FASTX_SKIP_AMBIGUOUS whose callback reads one_min - both
// against a loop written from the definition: the smallest position, among those whose k bases carry no ambiguity bit, that
// minimises hash & 0xffff0000 (MM_NO_MINIMIZER without one),
//   h_fw(i) = fw_xor ^ XOR_j rotl(fw[s[i+j]], rot*(k-1-j));  h_rc(i) = rc_xor ^ XOR_j rotl(rc[s[i+j]], rot*j);  h = h_fw + h_rc.
// Compiling it needs no device; running it needs one.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "simd_minimizers_amd.hpp"

namespace sm = simd_minimizers;

static uint32_t rotl(uint32_t x, uint32_t r) {
    r &= 31u;
    return r ? (x << r) | (x >> (32u - r)) : x;
}

// `s`: 2-bit codes, `n`: 1 where the base is ambiguous
static uint32_t by_definition(const mm_hasher_t &t, const std::vector<uint8_t> &s, const std::vector<uint8_t> &n, uint32_t k) {
    uint32_t want = MM_NO_MINIMIZER, best = 0;
    for (size_t p = 0; p + k <= s.size(); ++p) {
        uint32_t f = t.fw_xor, r = t.rc_xor;
        bool clean = true;
        for (uint32_t j = 0; j < k; ++j) {
            f ^= rotl(t.fw[s[p + j]], t.rot * (k - 1 - j));
            r ^= rotl(t.rc[s[p + j]], t.rot * j);
            clean = clean && !n[p + j];
        }
        const uint32_t m = (t.canonical ? f + r : f) & 0xffff0000u;
        if (clean && (want == MM_NO_MINIMIZER || m < best)) want = (uint32_t)p, best = m;
    }
    return want;
}

int main() {
    const uint32_t k = 21, w = 11;
    const size_t lens[] = {150, 0, 20, 21, 5000, 9000, 1, 333, 150, 150, 60};
    uint64_t x = 88172645463325252ull;
    auto rnd = [&]() {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        return x;
    };
    int bad = 0;
    // every read at its own base offset and its own bit offset inside its own buffers
    std::vector<std::vector<uint8_t>> codes, isn, packed, amb;
    std::vector<sm::PackedNSeq> reads;
    size_t r = 0;
    for (size_t len : lens) {
        const size_t off = r % 4, aoff = (3 * r + 5) % 11;
        std::vector<uint8_t> c(len), n(len, 0), p((off + len + 3) / 4 + 1, 0), a((aoff + len + 7) / 8 + 1, 0xff);
        for (size_t i = 0; i < len; ++i) {
            c[i] = (uint8_t)(rnd() & 3);
            n[i] = rnd() % 97 == 0;
            if (r == 8) n[i] = 1;                         // all N
            if (r == 9) n[i] = !(i >= 30 && i < 30 + k);  // one clean run of exactly k bases
            p[(off + i) >> 2] |= (uint8_t)(c[i] << (2 * ((off + i) & 3)));
            if (!n[i]) a[(aoff + i) >> 3] &= (uint8_t)~(1u << ((aoff + i) & 7));
        }
        codes.push_back(c), isn.push_back(n), packed.push_back(p), amb.push_back(a);
        ++r;
    }
    for (size_t i = 0; i < packed.size(); ++i)
        reads.push_back(sm::PackedNSeq{sm::PackedSeq{packed[i].data(), i % 4, codes[i].size()}, amb[i].data(), (3 * i + 5) % 11});
    const sm::NtHasher<true> nt(k);
    const std::vector<uint32_t> got = sm::one_minimizer_many(reads, nt, k);
    for (size_t i = 0; i < reads.size(); ++i) {
        const uint32_t want = by_definition(nt.tables, codes[i], isn[i], k);
        if (got[i] != want) ++bad, printf("read %zu: got %u want %u\n", i, got[i], want);
        if (codes[i].size() >= k && sm::one_minimizer(reads[i], nt, k) != want) ++bad, printf("single %zu\n", i);
    }
    if (got[8] != MM_NO_MINIMIZER || got[9] != 30) ++bad, printf("the all-N read or the exact run: %u %u\n", got[8], got[9]);

    // a FASTQ of the same reads (and more) through the stream: one_min in the callback
    std::string fastq;
    std::vector<uint32_t> want_stream;
    const char letters[] = "ACTG";  // (code c is letters[c]: A0 C1 T2 G3)
    for (int rep = 0; rep < 40; ++rep)
        for (size_t i = 0; i < codes.size(); ++i) {
            if (codes[i].empty()) continue;
            std::string s(codes[i].size(), 'A');
            for (size_t j = 0; j < s.size(); ++j) s[j] = isn[i][j] ? 'N' : letters[codes[i][j]];
            fastq += "@r\n" + s + "\n+\n" + std::string(s.size(), 'I') + "\n";
            want_stream.push_back(by_definition(nt.tables, codes[i], isn[i], k));
        }
    mm_fastx_stream_config_t cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.format = MM_FASTX_AUTO;
    cfg.flags = MM_FASTX_ONE_MINIMIZER | MM_FASTX_SKIP_AMBIGUOUS;
    cfg.chunk_bytes = 1 << 16;
    cfg.max_records = 4000;
    std::vector<uint32_t> got_stream;
    size_t at = 0;
    sm::canonical_minimizers(k, w).stream_fastx(
        [&](uint8_t *buf, size_t cap) {
            const size_t m = fastq.size() - at < cap ? fastq.size() - at : cap;
            memcpy(buf, fastq.data() + at, m);
            at += m;
            return m;
        },
        [&](const mm_fastx_batch_t &b, const uint32_t *one_min) {
            if (!one_min && b.n_records) ++bad, printf("a batch without one_min\n");
            for (uint64_t i = 0; one_min && i < b.n_records; ++i) got_stream.push_back(one_min[i]);
        },
        cfg, 5000);
    if (got_stream != want_stream) {
        ++bad;
        printf("stream: %zu words, %zu wanted\n", got_stream.size(), want_stream.size());
        for (size_t i = 0; i < got_stream.size() && i < want_stream.size(); ++i)
            if (got_stream[i] != want_stream[i]) {
                printf("stream record %zu: got %u want %u\n", i, got_stream[i], want_stream[i]);
                break;
            }
    }
    printf("one_minimizer_amb_example: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
