// The C++ mirror of many PackedNSeq reads in one call: Builder::run_many_skip_ambiguous_windows(reads, pos, offsets)
// (mm_run_packed_reads_skip_ambiguous_host).  Every read's slice equals run_skip_ambiguous_windows of that read alone.
// Exit code 0 = all checks passed; 77 = no GPU (the engine has no CPU fallback).
#include <cstdio>
#include <random>

#include "simd_minimizers_amd.hpp"

using namespace simd_minimizers;

int main() {
    if (mm_device_count() <= 0) return 77;
    // one buffer of codes and one of bits; the reads are views at odd base offsets, N in runs of 1, 30, 31 and 200
    std::mt19937 rng(11);
    const uint64_t total = 60000;
    std::vector<uint8_t> codes(total / 4 + 16), bits(total / 8 + 16, 0);
    for (auto &c : codes) c = (uint8_t)rng();
    const uint64_t runs[4] = {1, 30, 31, 200};
    for (int i = 0; i < 60; ++i) {
        const uint64_t run = runs[rng() & 3], p = rng() % (total - run);
        for (uint64_t j = p; j < p + run; ++j) bits[j >> 3] |= (uint8_t)(1u << (j & 7));
    }
    const PackedNSeq all{PackedSeq{codes.data(), 0, total}, bits.data(), 0};
    std::vector<PackedNSeq> reads;
    uint64_t at = 3;
    for (uint64_t n : {150ull, 0ull, 30ull, 31ull, 32ull, 9001ull, 1ull, 301ull, 40000ull, 77ull}) {
        reads.push_back(all.slice(at, at + n));
        at += n + 5;
    }
    std::vector<uint32_t> pos{1, 2, 3};
    std::vector<uint64_t> offsets{9};
    const auto b = canonical_minimizers(21, 11);
    b.run_many_skip_ambiguous_windows(reads, pos, offsets);  // (overwrites pos and offsets)
    if (offsets.size() != reads.size() + 1 || offsets.front() != 0 || offsets.back() != pos.size()) return 2;
    bool skipped = false;
    for (size_t r = 0; r < reads.size(); ++r) {
        const std::vector<uint32_t> one = b.run_skip_ambiguous_windows_once(reads[r]);
        if (std::vector<uint32_t>(pos.begin() + offsets[r], pos.begin() + offsets[r + 1]) != one) return 3;
        if (one != b.run_once(reads[r].seq)) skipped = true;
    }
    if (!skipped) return 4;  // (the bits were looked at)
    const auto cs = canonical_closed_syncmers(15, 17);
    cs.run_many_skip_ambiguous_windows(reads, pos, offsets);
    for (size_t r = 0; r < reads.size(); ++r)
        if (std::vector<uint32_t>(pos.begin() + offsets[r], pos.begin() + offsets[r + 1]) != cs.run_skip_ambiguous_windows_once(reads[r]))
            return 5;
    cs.run_many_skip_ambiguous_windows({}, pos, offsets);
    if (!pos.empty() || offsets != std::vector<uint64_t>{0}) return 6;
    printf("skip-ambiguous reads example ok (%zu reads)\n", reads.size());
    return 0;
}
