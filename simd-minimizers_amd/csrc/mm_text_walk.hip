// mm_text_walk.hip - instances and launcher of the fused text kernel (mm_text_walk_impl.h).
//
// Prebuilt with a fixed W (unrolled minimum) for the paper's windows w = 5, 11, 19 (bench/src/bin/paper.rs:343-361), forward
// and canonical windows, with and without the reverse-strand hash, for minimizers and both syncmer modes; every other
// w <= kTextMaxW runs in the W = 0 instances of the same kernel (w read at run time), larger w and k > kTextMaxK take the
// generic family's text kernels.  Each instance has a BATCH twin for mm_run_text_batch_* (records in one launch).
#include "mm_launch.h"
#include "mm_text_walk_impl.h"

namespace mm {

namespace {

typedef void (*TextWalkFn)(TextWalkParams);

template <int W, bool CANON, bool HASH_RC, bool BATCH>
TextWalkFn pick_mode(uint32_t mode) {
    if (mode == 0) return text_walk_kernel<W, CANON, HASH_RC, 0, BATCH>;
    if (mode == 1) return text_walk_kernel<W, CANON, HASH_RC, 1, BATCH>;
    return text_walk_kernel<W, CANON, HASH_RC, 2, BATCH>;
}
template <int W, bool BATCH>
TextWalkFn pick_strand(bool canon, bool hash_rc, uint32_t mode) {
    if (canon) return pick_mode<W, true, true, BATCH>(mode);  // (canonical windows need a canonical hasher: mm_plan_create_text)
    return hash_rc ? pick_mode<W, false, true, BATCH>(mode) : pick_mode<W, false, false, BATCH>(mode);
}
template <int W>
TextWalkFn pick(bool canon, bool hash_rc, uint32_t mode, bool batch) {
    return batch ? pick_strand<W, true>(canon, hash_rc, mode) : pick_strand<W, false>(canon, hash_rc, mode);
}

const uint32_t kTextPrebuiltW[] = {5, 11, 19};

}  // namespace

bool text_walk_supported(uint32_t k, uint32_t w) { return w <= kTextMaxW && k <= kTextMaxK; }

int text_prebuilt_windows(uint32_t *out, int capacity) {
    const int n = (int)(sizeof(kTextPrebuiltW) / sizeof(kTextPrebuiltW[0]));
    for (int i = 0; i < n && i < capacity; ++i)
        if (out) out[i] = kTextPrebuiltW[i];
    return n;
}

uint64_t text_walk_tiles(uint64_t windows) { return (windows + kTextTile - 1) / kTextTile; }
uint64_t text_batch_tiles(uint64_t n_chars) { return text_counts_tiles(n_chars); }

namespace {
TextWalkFn pick_window(uint32_t w, bool canon, bool hash_rc, uint32_t mode, bool batch) {
    switch (w) {
        case 5: return pick<5>(canon, hash_rc, mode, batch);
        case 11: return pick<11>(canon, hash_rc, mode, batch);
        case 19: return pick<19>(canon, hash_rc, mode, batch);
        default: return pick<0>(canon, hash_rc, mode, batch);
    }
}
}  // namespace

// mm_plan_prepare: the kernels of a text plan's single and batch launches, loaded on the current device without a launch
// (every instance is prebuilt: nothing to compile)
hipError_t text_walk_prepare(uint32_t w, bool canon, bool hash_rc, uint32_t mode, uint32_t *kernels) {
    return load_kernels({reinterpret_cast<const void *>(pick_window(w, canon, hash_rc, mode, false)),
                         reinterpret_cast<const void *>(pick_window(w, canon, hash_rc, mode, true)),
                         reinterpret_cast<const void *>(text_batch_tiles_kernel)},
                        kernels);
}

int launch_text_walk(const TextRunArgs &a, hipStream_t stream) {
    if (!text_walk_supported(a.k, a.w)) return -2;
    const bool canon = a.canonical_windows != 0;
    const bool hash_rc = a.hash_rc;
    const TextWalkFn fn = pick_window(a.w, canon, hash_rc, a.mode, a.batch);
    TextWalkParams p;
    p.text = a.text;
    p.n = a.n;
    p.tables = reinterpret_cast<const uint2 *>(a.tables);
    p.fw0 = a.fw0;
    p.rc0 = a.rc0;
    p.rot = a.rot;
    p.k = a.k;
    p.w = a.w;
    p.win_begin = a.win_begin;
    p.win_end = a.win_end;
    p.out = a.out;
    p.starts = a.starts;
    p.n_records = a.n_records;
    p.tile_rec = a.tile_rec;
    p.offsets = a.offsets;
    p.counts = a.batch ? a.counts : nullptr;
    // (a batch: windows 0 .. n inclusive, so that the records that start in the last l - 1 bytes get their offsets; with
    // a.counts, n and n_records are upper bounds: the grid, the status words and tile_rec are sized for the bound, the
    // kernels find the real tiles themselves)
    const uint64_t tiles = a.batch ? text_batch_tiles(a.n) : text_walk_tiles(a.win_end - a.win_begin);
    // (untagged look-back words and the ticket, cleared per launch as the generic family does)
    if (hipMemsetAsync(a.out.status, 0, sizeof(unsigned long long) * tiles, stream) != hipSuccess) return -1;
    if (hipMemsetAsync(a.out.ticket, 0, sizeof(uint32_t), stream) != hipSuccess) return -1;
    if (a.timing_start) hipEventRecord(a.timing_start, stream);
    if (a.batch)
        hipLaunchKernelGGL(text_batch_tiles_kernel, dim3((uint32_t)((tiles + 255) / 256)), dim3(256), 0, stream, a.starts,
                           a.n_records, a.k + a.w - 1, tiles, a.tile_rec, p.counts, a.n);
    hipLaunchKernelGGL(fn, dim3((uint32_t)tiles), dim3(kTextThreads), 0, stream, p);
    if (a.timing_stop) hipEventRecord(a.timing_stop, stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mm
