// mm_fastx_stream.h - what the FASTA / FASTQ stream (mm_fastx_stream.hip) shares with the kernel file of its trim step
// (mm_fastx_cut.hip) and asks of the host file that owns plans and workspaces (mm_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simd_minimizers_amd.h"

namespace mm {

// The trim step behind a packer, on `stream` (mm_fastx_cut.hip): d_counts {bases, records} rewritten in place to the kept
// ones, d_cut[0] = cut, d_cut[1] = 1 when records > max_records kept the rule from being applied.  d_newlines: one word of
// scratch.  The text may have any alignment; no byte outside [d_text, d_text + n_bytes) rounded to whole dwords is loaded.
// long_records (MM_FASTX_LONG_RECORDS on FASTA text) and l = k + w - 1: the split rule, d_cut[2..4] = {T, open, overlap}
// (zeros without it; d_cut has five words).  Returns 0, or -1 when a launch failed.
int launch_fastx_trim(const uint8_t *d_text, uint64_t n_bytes, int format, int last, int long_records, uint32_t l,
                      const unsigned long long *d_rec_base, const unsigned long long *d_rec_text_pos, uint64_t max_records,
                      unsigned long long *d_counts, unsigned long long *d_cut, unsigned long long *d_newlines, hipStream_t stream);
// The seam epilogue's device part, behind the run and the values on `stream`: pos[j] (and sk[j] when d_sk is not null)
// += bias for j < min(d_offsets[1], max_positions), record 0's slice; nothing when d_counts[1] is 0 or above max_records.
int launch_fastx_bias(const unsigned long long *d_counts, const unsigned long long *d_offsets, uint64_t max_records,
                      uint64_t max_positions, uint32_t bias, uint32_t *d_pos, uint32_t *d_sk, hipStream_t stream);

// ---- from mm_api.hip
struct ApiPlanInfo {
    uint32_t k, w, mode;
    int canonical_windows;  // the strand-vote tie-break (what the skip-ambiguous run asks for)
    int canonical_hasher;   // what the values calls take as `canonical`
    int text;               // a plan of mm_plan_create_text
};
ApiPlanInfo api_plan_info(const mm_plan_t *plan);
// What mm_run_packed_reads_counts_device_async would say to this plan and these bounds before it touches a device, pointers
// and workspace aside: MM_OK or its refusal (mm_last_error() set as that call sets it).
int api_reads_counts_refusal(const mm_plan_t *plan, uint64_t max_bases, uint64_t max_records, int want_sk, int want_amb);
// The byte-text stream (mm_fastx_text_stream_create).  What mm_run_text_batch_counts_device_async would say to this plan
// and these bounds before it touches a device, pointers and workspace aside (mm_last_error() set as that call sets it) ...
int api_text_counts_refusal(const mm_plan_t *plan, uint64_t max_chars, uint64_t max_records, int want_sk);
// ... and mm_one_minimizer_text_batch_counts_device_async with the text plan's own k and hasher tables (a plan keeps the
// tables of its hasher, not the mm_text_hasher_t they were made from).
int api_one_min_text_plan_counts(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_text, uint64_t text_bytes,
                                 uint64_t max_chars, uint64_t max_records, const uint64_t *d_starts, const uint64_t *d_counts,
                                 uint32_t *d_out_pos);
// The DNA stream (MM_FASTX_ONE_MINIMIZER): mm_one_minimizer_reads_counts_device_async - with d_amb (amb_bytes of bits,
// bit 0 = base 0) its skip-ambiguous form - with the plan's own k and hasher, base_offset 0.
int api_one_min_reads_plan_counts(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed, uint64_t packed_bytes,
                                  const void *d_amb, uint64_t amb_bytes, uint64_t max_bases, uint64_t max_records,
                                  const uint64_t *d_read_starts, const uint64_t *d_counts, uint32_t *d_out_pos);
hipStream_t api_workspace_stream(mm_workspace_t *ws);
void api_set_last_error(const char *text);

}  // namespace mm
