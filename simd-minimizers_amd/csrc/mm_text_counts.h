// mm_text_counts.h - a text batch whose two counts (characters, records) are read on the DEVICE
// (mm_run_text_batch_counts_*, mm_values_*_text_batch_counts_*): the host sizes the launch from the upper
// bounds it was given, every workgroup turns {counts, bounds} into what it works on with the one function below.  The host
// runs the same function for the tests (mm_debug_text_counts_view): no device needed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MM_TC_HD __host__ __device__ __forceinline__
#else
#define MM_TC_HD inline
#endif

namespace mm {

constexpr uint32_t kTextCountsTile = 8192;  // = kTextTile (mm_text_walk_impl.h asserts it)

// tiles of a batch launch over n_chars characters: windows 0 .. n_chars inclusive, so that the records that start in the
// last l - 1 bytes get their offsets
MM_TC_HD uint64_t text_counts_tiles(uint64_t n_chars) { return (n_chars + 1 + kTextCountsTile - 1) / kTextCountsTile; }

struct TextCountsView {
    uint64_t n;          // characters the kernels work on (0 when refused)
    uint64_t n_records;  // records (0 when refused)
    uint64_t win_end;    // n >= l ? n - l + 1 : 0: never wraps
    uint64_t tiles;      // real tiles = text_counts_tiles(n) <= text_counts_tiles(max_chars): tickets at or past it leave at once
    uint32_t refused;    // a count exceeds its bound: ticket 0 writes count 0, offsets[0] = 0 and raises the error word
    uint32_t walk;       // 0: refused or no record - ticket 0 writes count 0 and offsets[0] = 0, nobody reads the starts
};

// l = k + w - 1.  Counts within the bounds give the view of a launch with those counts as host arguments.
MM_TC_HD TextCountsView text_counts_view(uint32_t l, uint64_t max_chars, uint64_t max_records, uint64_t n_chars,
                                         uint64_t n_records) {
    TextCountsView v;
    v.refused = (n_chars > max_chars || n_records > max_records) ? 1u : 0u;
    v.walk = (!v.refused && n_records != 0) ? 1u : 0u;
    v.n = v.refused ? 0 : n_chars;
    v.n_records = v.refused ? 0 : n_records;
    v.win_end = v.n >= l ? v.n - l + 1 : 0;
    v.tiles = text_counts_tiles(v.n);
    return v;
}

}  // namespace mm
