/* FASTQ bytes in device memory -> packed reads -> minimizer positions -> k-mer values, queued on ONE stream through the C
 * ABI with a single wait at the end: mm_fastq_pack_device_async, mm_run_packed_reads_counts_device_async and
 * mm_values_u64_reads_device_async (n_reads = max_records) hand the packer's two counts on in device memory.  The
 * reference does the same work in synchronous host code (the loader of bench/src/lib.rs:51-82, Builder::run per read
 * src/lib.rs:378, Output::values_u64 src/lib.rs:584-612).  The result is compared, bit for bit, with the synchronous
 * route: mm_fasta_pack_device, the counts on the host, mm_run_packed_reads_device, the values and a wait each.
 * Plain C against the header.  Exit code 0 = everything agrees; 77 = no GPU (the engine has no CPU fallback). */
#include <hip/hip_runtime_api.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "simd_minimizers_amd.h"

#define HIP_OK(x)                                             \
    do {                                                      \
        if ((x) != hipSuccess) {                              \
            printf("HIP call failed at line %d\n", __LINE__); \
            return 98;                                        \
        }                                                     \
    } while (0)
#define MM_OK_OR(x, ret)                                                                   \
    do {                                                                                   \
        const int mm_code = (x);                                                           \
        if (mm_code != MM_OK) {                                                            \
            printf("line %d: %s (%s)\n", __LINE__, mm_strerror(mm_code), mm_last_error()); \
            return ret;                                                                    \
        }                                                                                  \
    } while (0)

enum { N_READS = 400, MAX_RECORDS = 1000, K = 21, W = 11 };

int main(void) {
    if (mm_device_count() <= 0) {
        printf("no GPU\n");
        return 77;
    }
    /* 400 reads of 0 .. 699 bases, one of 20 000 */
    char *file = (char *)malloc((size_t)N_READS * 1500 + 50000);
    uint64_t n_bytes = 0, total_bases = 0, x = 0x9E3779B97F4A7C15ull;
    int r;
    if (!file) return 99;
    for (r = 0; r < N_READS; ++r) {
        uint64_t len, j;
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        len = r == 7 ? 0 : (r == 200 ? 20000 : (x >> 40) % 700);
        n_bytes += (uint64_t)sprintf(file + n_bytes, "@read%d\n", r);
        for (j = 0; j < len; ++j) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            file[n_bytes++] = "ACGT"[(x >> 33) & 3];
        }
        file[n_bytes++] = '\n', file[n_bytes++] = '+', file[n_bytes++] = '\n';
        memset(file + n_bytes, 'I', len);
        n_bytes += len;
        file[n_bytes++] = '\n';
        total_bases += len;
    }

    mm_plan_t *plan = NULL;
    mm_workspace_t *ws = NULL;
    MM_OK_OR(mm_plan_create(&plan, K, W, 1, MM_MINIMIZERS, NULL), 2);
    MM_OK_OR(mm_workspace_create(&ws, 0, NULL), 3);

    const uint64_t packed_cap = (n_bytes / 4 + 8 + 3) / 4 * 4;
    uint8_t *d_file = NULL, *d_packed = NULL, *d_packed2 = NULL;
    uint64_t *d_starts = NULL, *d_starts2 = NULL, *d_counts = NULL, *d_counts2 = NULL, *d_offsets = NULL, *d_offsets2 = NULL;
    uint64_t *d_count = NULL, *d_values = NULL, *d_values2 = NULL;
    uint32_t *d_pos = NULL, *d_pos2 = NULL;
    HIP_OK(hipMalloc((void **)&d_file, n_bytes));
    HIP_OK(hipMalloc((void **)&d_packed, packed_cap));
    HIP_OK(hipMalloc((void **)&d_packed2, packed_cap));
    HIP_OK(hipMalloc((void **)&d_starts, (MAX_RECORDS + 1) * sizeof(uint64_t)));
    HIP_OK(hipMalloc((void **)&d_starts2, (MAX_RECORDS + 1) * sizeof(uint64_t)));
    HIP_OK(hipMalloc((void **)&d_counts, 2 * sizeof(uint64_t)));
    HIP_OK(hipMalloc((void **)&d_counts2, 2 * sizeof(uint64_t)));
    HIP_OK(hipMalloc((void **)&d_offsets, (MAX_RECORDS + 1) * sizeof(uint64_t)));
    HIP_OK(hipMalloc((void **)&d_offsets2, (MAX_RECORDS + 1) * sizeof(uint64_t)));
    HIP_OK(hipMalloc((void **)&d_count, sizeof(uint64_t)));
    HIP_OK(hipMalloc((void **)&d_pos, n_bytes * sizeof(uint32_t)));
    HIP_OK(hipMalloc((void **)&d_pos2, n_bytes * sizeof(uint32_t)));
    HIP_OK(hipMalloc((void **)&d_values, n_bytes * sizeof(uint64_t)));
    HIP_OK(hipMalloc((void **)&d_values2, n_bytes * sizeof(uint64_t)));
    HIP_OK(hipMemcpy(d_file, file, n_bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_starts, 0xA5, (MAX_RECORDS + 1) * sizeof(uint64_t))); /* (nothing behind starts[n] may be used) */
    HIP_OK(hipMemset(d_values, 0, n_bytes * sizeof(uint64_t)));
    HIP_OK(hipMemset(d_values2, 0, n_bytes * sizeof(uint64_t)));
    HIP_OK(hipDeviceSynchronize());

    /* three queued calls, nothing in between: the bounds are the text length and the table's size ... */
    MM_OK_OR(mm_fastq_pack_device_async(ws, d_file, n_bytes, d_packed, packed_cap, d_starts, NULL, MAX_RECORDS, d_counts), 4);
    MM_OK_OR(mm_run_packed_reads_counts_device_async(plan, ws, d_packed, packed_cap, 0, n_bytes, MAX_RECORDS, d_starts, d_counts,
                                                     d_pos, NULL, n_bytes, d_offsets, d_count), 5);
    MM_OK_OR(mm_values_u64_reads_device_async(ws, d_packed, packed_cap, 0, MAX_RECORDS, d_starts, 0, mm_plan_value_len(plan), 1,
                                              d_pos, d_offsets, n_bytes, d_values), 6);
    /* ... and the one check */
    MM_OK_OR(mm_workspace_check(ws), 7);

    uint64_t counts[2] = {0, 0}, count = 0;
    HIP_OK(hipMemcpy(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&count, d_count, sizeof(count), hipMemcpyDeviceToHost));
    if (counts[0] != total_bases || counts[1] != N_READS || count == 0) return 10;

    /* the synchronous route: a wait after the packer (counts to the host), after the run, after the values */
    uint64_t counts2[2] = {0, 0}, count2 = 0;
    MM_OK_OR(mm_fasta_pack_device(ws, d_file, n_bytes, d_packed2, packed_cap, d_starts2, NULL, MAX_RECORDS, d_counts2, counts2), 20);
    if (counts2[0] != counts[0] || counts2[1] != counts[1]) return 21;
    MM_OK_OR(mm_run_packed_reads_device(plan, ws, d_packed2, packed_cap, 0, counts2[1], d_starts2, counts2[0], 0xffffffffu, d_pos2,
                                        NULL, n_bytes, d_offsets2, &count2), 22);
    if (count2 != count) return 23;
    MM_OK_OR(mm_values_u64_reads_device_async(ws, d_packed2, packed_cap, 0, counts2[1], d_starts2, 0, mm_plan_value_len(plan), 1,
                                              d_pos2, d_offsets2, n_bytes, d_values2), 24);
    MM_OK_OR(mm_workspace_sync(ws), 25);

    uint32_t *pos = (uint32_t *)malloc(count * sizeof(uint32_t)), *pos2 = (uint32_t *)malloc(count * sizeof(uint32_t));
    uint64_t *val = (uint64_t *)malloc(count * sizeof(uint64_t)), *val2 = (uint64_t *)malloc(count * sizeof(uint64_t));
    uint64_t offs[MAX_RECORDS + 1], offs2[N_READS + 1];
    if (!pos || !pos2 || !val || !val2) return 99;
    HIP_OK(hipMemcpy(pos, d_pos, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(pos2, d_pos2, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(val, d_values, count * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(val2, d_values2, count * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(offs, d_offsets, sizeof(offs), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(offs2, d_offsets2, sizeof(offs2), hipMemcpyDeviceToHost));
    if (memcmp(pos, pos2, count * sizeof(uint32_t)) != 0) return 30;
    if (memcmp(val, val2, count * sizeof(uint64_t)) != 0) return 31;
    if (memcmp(offs, offs2, sizeof(offs2)) != 0) return 32;
    for (r = N_READS; r <= MAX_RECORDS; ++r)
        if (offs[r] != count) return 33; /* (the tail is filled with the total) */

    /* the synchronous counts call: positions and both counts from one wait */
    uint64_t out3[3] = {0, 0, 0};
    MM_OK_OR(mm_run_packed_reads_counts_device(plan, ws, d_packed, packed_cap, 0, n_bytes, MAX_RECORDS, d_starts, d_counts, d_pos2,
                                               NULL, n_bytes, d_offsets2, out3), 40);
    if (out3[0] != count || out3[1] != counts[0] || out3[2] != counts[1]) return 41;

    /* a table too small for the file: the packer counts on, the run refuses, the one check says MM_ERR_CAPACITY */
    MM_OK_OR(mm_fastq_pack_device_async(ws, d_file, n_bytes, d_packed, packed_cap, d_starts, NULL, 100, d_counts), 50);
    MM_OK_OR(mm_run_packed_reads_counts_device_async(plan, ws, d_packed, packed_cap, 0, n_bytes, 100, d_starts, d_counts, d_pos, NULL,
                                                     n_bytes, d_offsets, d_count), 51);
    if (mm_workspace_check(ws) != MM_ERR_CAPACITY) return 52;
    HIP_OK(hipMemcpy(&count2, d_count, sizeof(count2), hipMemcpyDeviceToHost));
    if (count2 != 0) return 53;
    MM_OK_OR(mm_workspace_check(ws), 54);

    hipFree(d_file), hipFree(d_packed), hipFree(d_packed2), hipFree(d_starts), hipFree(d_starts2), hipFree(d_counts);
    hipFree(d_counts2), hipFree(d_offsets), hipFree(d_offsets2), hipFree(d_count), hipFree(d_pos), hipFree(d_pos2);
    hipFree(d_values), hipFree(d_values2);
    free(pos), free(pos2), free(val), free(val2), free(file);
    mm_workspace_destroy(ws);
    mm_plan_destroy(plan);
    printf("reads_counts_example: OK (%llu reads, %llu bases, %llu positions)\n", (unsigned long long)counts[1],
           (unsigned long long)counts[0], (unsigned long long)count);
    return 0;
}
