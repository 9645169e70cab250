// File bytes in device memory -> records of byte text -> minimizer positions -> k-mer values, queued on ONE stream through
// the C ABI with a single wait at the end: mm_fasta_text_device_async, mm_run_text_batch_counts_device_async and
// mm_values_u64_text_batch_counts_device_async hand the loader's two counts on in device memory.  The reference does the
// same work in synchronous host code (the loader of bench/src/lib.rs:51-82, Builder::run per record src/lib.rs:378,
// Output::values_u64 src/lib.rs:584-629); the checks below restate it: the FASTA reader, the per-record offsets, and every
// value against the bytes at its position.  The positions themselves are compared with the synchronous batch call.
// Exit code 0 = everything agrees; 77 = no GPU (the engine has no CPU fallback).
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "simd_minimizers_amd.h"

#define HIP_OK(x)                                                     \
    do {                                                              \
        if ((x) != hipSuccess) {                                      \
            printf("HIP call failed at line %d\n", __LINE__);         \
            return 98;                                                \
        }                                                             \
    } while (0)
#define MM_OK_OR(x, ret)                                                               \
    do {                                                                               \
        const int mm_code = (x);                                                       \
        if (mm_code != MM_OK) {                                                        \
            printf("line %d: %s (%s)\n", __LINE__, mm_strerror(mm_code), mm_last_error()); \
            return ret;                                                                \
        }                                                                              \
    } while (0)

int main() {
    if (mm_device_count() <= 0) {
        printf("no GPU\n");
        return 77;
    }
    // a protein-like FASTA: 150 records of 0 .. 899 letters in 60-character lines, junk in front of the first header
    std::string file = "not a record\n";
    std::vector<std::string> seqs;
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (int r = 0; r < 150; ++r) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        const size_t len = r == 9 ? 0 : (size_t)((x >> 40) % 900);
        std::string s(len, 'A');
        for (auto &c : s) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            c = "ACDEFGHIKLMNPQRSTVWY"[(x >> 33) % 20];
        }
        file += ">sp|P" + std::to_string(r) + " protein\n";
        for (size_t q = 0; q < len; q += 60) file += s.substr(q, 60) + "\n";
        seqs.push_back(s);
    }
    const uint64_t n_bytes = file.size(), max_records = 256;
    const uint32_t k = 7, w = 11, l = k + w - 1;

    mm_text_hasher_t th;
    mm_plan_t *plan = nullptr;
    mm_workspace_t *ws = nullptr;
    MM_OK_OR(mm_text_mul_hasher(&th, 0), 1);
    MM_OK_OR(mm_plan_create_text(&plan, k, w, 0, MM_MINIMIZERS, &th), 2);
    MM_OK_OR(mm_workspace_create(&ws, 0, nullptr), 3);

    uint8_t *d_file = nullptr, *d_seq = nullptr;
    uint64_t *d_starts = nullptr, *d_counts = nullptr, *d_offsets = nullptr, *d_count = nullptr, *d_values = nullptr;
    uint32_t *d_pos = nullptr;
    HIP_OK(hipMalloc((void **)&d_file, n_bytes));
    HIP_OK(hipMalloc((void **)&d_seq, n_bytes));
    HIP_OK(hipMalloc((void **)&d_starts, (max_records + 1) * sizeof(uint64_t)));
    HIP_OK(hipMalloc((void **)&d_counts, 2 * sizeof(uint64_t)));
    HIP_OK(hipMalloc((void **)&d_offsets, (max_records + 1) * sizeof(uint64_t)));
    HIP_OK(hipMalloc((void **)&d_count, sizeof(uint64_t)));
    HIP_OK(hipMalloc((void **)&d_pos, n_bytes * sizeof(uint32_t)));  // (capacity = max_chars always suffices)
    HIP_OK(hipMalloc((void **)&d_values, n_bytes * sizeof(uint64_t)));
    HIP_OK(hipMemcpy(d_file, file.data(), n_bytes, hipMemcpyHostToDevice));

    // four queued calls, nothing in between ...
    MM_OK_OR(mm_fasta_text_device_async(ws, d_file, n_bytes, d_seq, n_bytes, d_starts, nullptr, max_records, d_counts), 4);
    MM_OK_OR(mm_run_text_batch_counts_device_async(plan, ws, d_seq, n_bytes, n_bytes, max_records, d_starts, d_counts, d_pos,
                                                   nullptr, n_bytes, d_offsets, d_count), 5);
    MM_OK_OR(mm_values_u64_text_batch_counts_device_async(ws, d_seq, n_bytes, n_bytes, max_records, d_starts, d_counts,
                                                          MM_TEXT_VALUES_BYTES, mm_plan_value_len(plan), 0, d_pos, d_offsets,
                                                          n_bytes, d_values), 6);
    // ... and the one check
    MM_OK_OR(mm_workspace_check(ws), 7);

    uint64_t counts[2] = {0, 0}, count = 0;
    HIP_OK(hipMemcpy(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&count, d_count, sizeof(count), hipMemcpyDeviceToHost));
    std::string all;
    for (const auto &s : seqs) all += s;
    if (counts[0] != all.size() || counts[1] != seqs.size()) return 10;
    std::vector<uint64_t> starts(seqs.size() + 1), offsets(seqs.size() + 1), values(count);
    std::vector<uint32_t> pos(count);
    std::vector<uint8_t> seq(all.size());
    HIP_OK(hipMemcpy(starts.data(), d_starts, starts.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(offsets.data(), d_offsets, offsets.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(seq.data(), d_seq, seq.size(), hipMemcpyDeviceToHost));
    if (count) {
        HIP_OK(hipMemcpy(pos.data(), d_pos, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(values.data(), d_values, count * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    if (memcmp(seq.data(), all.data(), all.size()) != 0) return 11;
    if (offsets[0] != 0 || offsets[seqs.size()] != count || count == 0) return 12;
    uint64_t at = 0;
    for (size_t r = 0; r < seqs.size(); ++r) {
        if (starts[r] != at) return 13;
        const uint64_t len = seqs[r].size();
        if (offsets[r] > offsets[r + 1]) return 14;
        if (len < l && offsets[r] != offsets[r + 1]) return 15;
        for (uint64_t i = offsets[r]; i < offsets[r + 1]; ++i) {
            if ((uint64_t)pos[i] + k > len) return 16;  // (record-local, its k-mer inside the record)
            if (i > offsets[r] && pos[i] <= pos[i - 1]) return 17;
            uint64_t want = 0;
            for (uint32_t j = 0; j < k; ++j) want |= (uint64_t)(uint8_t)seqs[r][pos[i] + j] << (8 * j);
            if (values[i] != want) return 18;
        }
        at += len;
    }
    if (starts[seqs.size()] != at) return 19;

    // the positions: bit for bit those of the synchronous batch call given the counts as host arguments
    uint32_t *d_pos2 = nullptr;
    uint64_t *d_offsets2 = nullptr, count2 = 0;
    HIP_OK(hipMalloc((void **)&d_pos2, n_bytes * sizeof(uint32_t)));
    HIP_OK(hipMalloc((void **)&d_offsets2, (max_records + 1) * sizeof(uint64_t)));
    MM_OK_OR(mm_run_text_batch_device(plan, ws, d_seq, n_bytes, counts[1], d_starts, counts[0], d_pos2, nullptr, n_bytes,
                                      d_offsets2, &count2), 20);
    if (count2 != count) return 21;
    std::vector<uint32_t> pos2(count);
    std::vector<uint64_t> offsets2(seqs.size() + 1);
    HIP_OK(hipMemcpy(pos2.data(), d_pos2, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(offsets2.data(), d_offsets2, offsets2.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (pos2 != pos || offsets2 != offsets) return 22;

    // the synchronous counts call: positions and both counts from one wait
    uint64_t out3[3] = {0, 0, 0};
    MM_OK_OR(mm_run_text_batch_counts_device(plan, ws, d_seq, n_bytes, n_bytes, max_records, d_starts, d_counts, d_pos2, nullptr,
                                             n_bytes, d_offsets2, out3), 23);
    if (out3[0] != count || out3[1] != counts[0] || out3[2] != counts[1]) return 24;

    // a table too small for the file: the loader counts on, the run refuses, the one check says MM_ERR_CAPACITY
    MM_OK_OR(mm_fasta_text_device_async(ws, d_file, n_bytes, d_seq, n_bytes, d_starts, nullptr, 100, d_counts), 25);
    MM_OK_OR(mm_run_text_batch_counts_device_async(plan, ws, d_seq, n_bytes, n_bytes, 100, d_starts, d_counts, d_pos, nullptr,
                                                   n_bytes, d_offsets, d_count), 26);
    if (mm_workspace_check(ws) != MM_ERR_CAPACITY) return 27;
    HIP_OK(hipMemcpy(&count, d_count, sizeof(count), hipMemcpyDeviceToHost));
    if (count != 0) return 28;
    MM_OK_OR(mm_workspace_check(ws), 29);

    hipFree(d_file), hipFree(d_seq), hipFree(d_starts), hipFree(d_counts), hipFree(d_offsets), hipFree(d_count);
    hipFree(d_pos), hipFree(d_values), hipFree(d_pos2), hipFree(d_offsets2);
    mm_workspace_destroy(ws);
    mm_plan_destroy(plan);
    printf("text_counts_example: ok (%llu records, %llu characters, %llu positions)\n", (unsigned long long)counts[1],
           (unsigned long long)counts[0], (unsigned long long)out3[0]);
    return 0;
}
