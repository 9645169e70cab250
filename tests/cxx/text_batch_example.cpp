// The C++ mirror of many byte-text records in one call: Builder::run_many(std::vector<TextSeq>, pos, offsets)
// (mm_run_text_batch_host).  Exit code 0 = all checks passed; 77 = no GPU (the engine has no CPU fallback).
#include <cstdio>
#include <random>

#include "simd_minimizers_amd.hpp"

using namespace simd_minimizers;

int main() {
    if (mm_device_count() <= 0) return 77;
    // records of random bytes, empty and short ones among them: each slice equals the record run alone
    std::mt19937 rng(3);
    std::vector<std::vector<uint8_t>> data;
    for (uint64_t n : {300ull, 0ull, 30ull, 31ull, 9000ull, 1ull, 0ull, 20000ull, 77ull}) {
        std::vector<uint8_t> v(n);
        for (auto &c : v) c = (uint8_t)rng();
        data.push_back(v);
    }
    std::vector<TextSeq> recs;
    for (auto &v : data) recs.push_back(TextSeq{v.data(), v.size()});
    std::vector<uint32_t> pos{1, 2, 3}, sk;
    std::vector<uint64_t> offsets{9};
    const auto b = minimizers(21, 11);
    b.super_kmers(&sk).run_many(recs, pos, offsets);  // (overwrites pos and offsets)
    if (offsets.size() != recs.size() + 1 || offsets.front() != 0 || offsets.back() != pos.size()) return 2;
    if (sk.size() != pos.size()) return 3;
    for (size_t r = 0; r < recs.size(); ++r) {
        const std::vector<uint32_t> one = b.run_once(recs[r]);
        if (std::vector<uint32_t>(pos.begin() + offsets[r], pos.begin() + offsets[r + 1]) != one) return 4;
    }
    // canonical closed syncmers with NtHasher's tables over ASCII DNA
    mm_text_hasher_t dna;
    const NtHasher<true> nt(21);
    check(mm_text_hasher_from_dna(&dna, &nt.tables));
    for (auto &v : data)
        for (auto &c : v) c = (uint8_t)"ACGT"[rng() & 3];
    const auto cs = canonical_closed_syncmers(21, 11).hasher(dna);
    cs.run_many(recs, pos, offsets);
    for (size_t r = 0; r < recs.size(); ++r) {
        const std::vector<uint32_t> one = cs.run_once(recs[r]);
        if (std::vector<uint32_t>(pos.begin() + offsets[r], pos.begin() + offsets[r + 1]) != one) return 5;
    }
    printf("text batch example ok (%zu positions)\n", pos.size());
    return 0;
}
