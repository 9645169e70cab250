// DeviceGroup::values_batch / batch_values (the k-mer values of a device-resident batch, every entry's sequences in one
// launch) against Output::values_u64 / values_u128 of a loop over Builder::run per contig (src/lib.rs:584-629,
// bench/src/bin/paper.rs:410-431) through the C++ mirror.  Prints a checksum of all values in sequence order, which the
// test-suite recomputes with its oracle.  Exit code 0 = every sequence's values agree; 77 = no GPU.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <vector>

#include "simd_minimizers_amd.hpp"

using namespace simd_minimizers;

static uint64_t g_x = 0x9E3779B97F4A7C15ull;
static uint8_t next_byte() {
    g_x ^= g_x << 13, g_x ^= g_x >> 7, g_x ^= g_x << 17;
    return (uint8_t)(g_x >> 32);
}
static void fnv(uint64_t &h, uint64_t v) { h = (h ^ v) * 0x100000001B3ull; }

// the values of sequence `seq` from the group's device buffer: `words` 64-bit words per value
static bool download(const DeviceGroup &g, const std::vector<int> &devices, uint64_t seq, int words, std::vector<uint64_t> &out) {
    const DeviceGroup::BatchValues v = g.batch_values(seq);
    out.assign(v.count * words, 0);
    if (v.count == 0) return true;
    if (hipSetDevice(devices[(size_t)v.entry]) != hipSuccess) return false;
    return hipMemcpy(out.data(), v.d_values, out.size() * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess;
}

template <class B>
static int check_builder(const B &b, bool wide, const std::vector<PackedSeq> &seqs, uint64_t &checksum, uint64_t &n_values) {
    const std::vector<int> devices = {0, 0};
    DeviceGroup g(devices);
    g.upload_batch(seqs);
    const std::vector<uint64_t> counts = g.run_batch_device(b, seqs);
    const uint64_t total = g.values_batch(b, wide);
    checksum = 0xCBF29CE484222325ull;
    n_values = 0;
    for (size_t s = 0; s < seqs.size(); ++s) {
        std::vector<uint64_t> got;
        if (!download(g, devices, s, wide ? 2 : 1, got)) return 1;
        std::vector<uint32_t> one;
        auto out = b.run(seqs[s], one);
        if (one.size() != counts[s] || got.size() != counts[s] * (wide ? 2 : 1)) return 2;
        if (wide) {
            const std::vector<u128> want = out.values_u128();
            for (size_t i = 0; i < want.size(); ++i)
                if ((uint64_t)want[i] != got[2 * i] || (uint64_t)(want[i] >> 64) != got[2 * i + 1]) return 3;
        } else {
            const std::vector<uint64_t> want = out.values_u64();
            for (size_t i = 0; i < want.size(); ++i)
                if (want[i] != got[i]) return 4;
        }
        for (uint64_t v : got) fnv(checksum, v);
        n_values += counts[s];
    }
    return n_values == total ? 0 : 5;
}

int main() {
    if (mm_device_count() <= 0) {
        printf("no GPU\n");
        return 77;
    }
    // 12 sequences of 500 + 977 s bases, sequence s from base s % 5 of its own buffer; two empty ones among them
    std::vector<std::vector<uint8_t>> data;
    std::vector<PackedSeq> seqs;
    for (uint64_t s = 0; s < 12; ++s) {
        const uint64_t len = (s == 3 || s == 7) ? 0 : 500 + 977 * s, offset = s % 5;
        data.emplace_back((offset + len + 3) / 4 + 1, 0);
        for (auto &byte : data.back()) byte = next_byte();
        seqs.push_back(PackedSeq{data.back().data(), offset, len});
    }
    try {
        uint64_t c64 = 0, n64 = 0, c128 = 0, n128 = 0;
        int r;
        if ((r = check_builder(canonical_minimizers(21, 11), false, seqs, c64, n64))) return r;
        if ((r = check_builder(canonical_minimizers(43, 9), true, seqs, c128, n128))) return 10 + r;
        printf("values_batch_example: u64 %llu values checksum %016llx; u128 %llu values checksum %016llx\n",
               (unsigned long long)n64, (unsigned long long)c64, (unsigned long long)n128, (unsigned long long)c128);
    } catch (const Error &e) {
        printf("error: %s (code %d)\n", e.what(), e.code);
        return 99;
    }
    return 0;
}
