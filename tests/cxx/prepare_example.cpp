// The C++ mirror of mm_plan_prepare: Builder::prepare(what) gets a builder's kernels ready before its first run, then
// run_many with super-k-mer indices (reads mode) compiles nothing, and every read's slice equals run of that read alone.
// Prints the report.  Exit code 0 = all checks passed; 77 = no GPU (the engine has no CPU fallback).
#include <cstdio>
#include <random>

#include "simd_minimizers_amd.hpp"

using namespace simd_minimizers;

int main() {
    if (mm_device_count() <= 0) return 77;
    std::mt19937 rng(5);
    const uint64_t total = 40000;
    std::vector<uint8_t> codes(total / 4 + 16);
    for (auto &c : codes) c = (uint8_t)rng();
    const PackedSeq all{codes.data(), 0, total};
    std::vector<PackedSeq> reads;
    uint64_t at = 1;
    for (uint64_t n : {150ull, 0ull, 30ull, 31ull, 32ull, 6001ull, 151ull, 301ull}) {
        reads.push_back(all.slice(at, at + n));
        at += n + 3;
    }
    std::vector<uint32_t> sk;
    const auto b = canonical_minimizers(21, 11).super_kmers(&sk);
    uint64_t before[4], after[4];
    const mm_prepare_report_t rep = b.prepare(MM_PREPARE_SEQUENCE | MM_PREPARE_READS);
    printf("prepare: %u kernels, %u compiled, %u from disk, %u unavailable\n", rep.kernels, rep.compiled, rep.from_disk,
           rep.unavailable);
    if (rep.kernels < 4 || rep.unavailable != 0) return 2;
    if (mm_jit_stats(before) != MM_OK) return 3;
    std::vector<uint32_t> pos;
    std::vector<uint64_t> offsets;
    b.run_many(reads, pos, offsets);
    if (offsets.size() != reads.size() + 1 || offsets.back() != pos.size() || sk.size() != pos.size()) return 4;
    const std::vector<uint32_t> sk_many = sk;
    for (size_t r = 0; r < reads.size(); ++r) {
        std::vector<uint32_t> one;
        sk.clear();
        b.run_scalar(reads[r], one);
        if (std::vector<uint32_t>(pos.begin() + offsets[r], pos.begin() + offsets[r + 1]) != one) return 5;
        if (std::vector<uint32_t>(sk_many.begin() + offsets[r], sk_many.begin() + offsets[r + 1]) != sk) return 6;
    }
    if (mm_jit_stats(after) != MM_OK) return 3;
    if (after[0] != before[0] || after[1] != before[1]) return 7;  // (nothing compiled or read from disk after prepare)
    printf("prepare example ok (%zu reads, %zu positions)\n", reads.size(), pos.size());
    return 0;
}
