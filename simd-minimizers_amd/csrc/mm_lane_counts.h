// mm_lane_counts.h - a packed reads run whose two counts (bases, records) are read on the DEVICE
// (mm_run_packed_reads_counts_*): the host sizes the lane table, the walk's grid and the workspace buffers
// from the upper bounds it was given, every table kernel turns {counts, bounds} into the reads it tabulates with the one
// function below.  The host runs the same function for the tests (mm_debug_lane_counts_view): no device needed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MM_LC_HD __host__ __device__ __forceinline__
#else
#define MM_LC_HD inline
#endif

namespace mm {

struct LaneCountsView {
    uint32_t n_reads_eff;  // reads the table is built for (0 when refused)
    uint32_t n_bases_eff;  // bases they lie in: no start or end of a read is taken beyond it (0 when refused)
    uint32_t refused;      // a count exceeds its bound: an empty batch, and the fill kernel raises the error word once
};

// max_bases < 2^32 and max_records < 2^31 (the entry points' rule), so counts within the bounds fit 32 bits.  Counts
// within the bounds give the table of a launch with those counts as host arguments.
MM_LC_HD LaneCountsView lane_counts_view(uint64_t max_bases, uint64_t max_records, uint64_t n_bases, uint64_t n_records) {
    LaneCountsView v;
    v.refused = (n_bases > max_bases || n_records > max_records) ? 1u : 0u;
    v.n_reads_eff = v.refused ? 0u : (uint32_t)n_records;
    v.n_bases_eff = v.refused ? 0u : (uint32_t)n_bases;
    return v;
}

// lanes the reads can need at most at S windows per lane: every read owns at least one lane and ceil(windows / S) <=
// windows / S + 1 of them (fused_segments_plan sizes the walk's grid from it)
MM_LC_HD uint64_t lane_counts_bound(uint64_t max_bases, uint64_t max_records, uint32_t S) {
    return max_records + max_bases / (S ? S : 1u) + 1u;
}

}  // namespace mm
