// mm_lanes.hip — the LANE TABLE of a reads-mode launch, built on the device (round 6).
//
// The reference's operator is `Builder::run` per read / contig (src/lib.rs:378), and its own `short` experiment spans
// sequence lengths 16 .. 16 384 (bench/src/bin/paper.rs:62-115).  The reads-mode kernel of rounds 2-5 gave every read one
// lane (sized for the longest read), so a batch with one read above about 1.5 kbp fell back to one launch per read,
// and the batch mode gave every contig tiles of its own, so a 10 kbp contig filled 33 of a tile's 256 lanes.  With a lane
// table (LaneSeg, mm_common.h) a tile's 256 lanes are ANY 256 consecutive segments: a read of n_w windows takes
// ceil(n_w / S) consecutive lanes of (almost) equal length, a short read one lane, a read without a window one empty
// lane (it stores the read's output offset).  Four small kernels on the run's stream (two for up to 2048 reads), no host round trip:
//   seg_count_kernel   segments per read, summed per block of 2048 reads
//   seg_scan_kernel    exclusive scan of the block sums (one workgroup)
//   seg_first_kernel   first lane of every read (seg_first[r], n_reads + 1 entries)
//   seg_fill_kernel    one thread per lane of the (padded) table: binary search for its read, its share of the read's
//                      windows, and the tile's origin (smallest start of its lanes)
// The grid of the walk is sized from an upper bound of the lane count (n_reads + total_bases / S), so nothing is read
// back; lanes behind the last real one are empty (count 0) and their tiles pass through the look-back with nothing.
//
// Counts on the device (mm_run_packed_reads_counts_*; SegSource::counts): the four kernels are instantiated a second time
// (COUNTS) for a run whose number of reads and bases lie in device memory, as the FASTQ / FASTA packers leave them.  The
// host sizes grids and buffers from upper bounds, the kernels tabulate the reads the counts name (mm_lane_counts.h); the
// lanes behind them are the empty lanes above.  seg_tail_kernel, queued behind the walk, fills the offsets of the reads
// between the real count and the bound with the total.
#include "mm_common.h"
#include "mm_lane_counts.h"
#include "mm_launch.h"

namespace mm {

namespace {

constexpr uint32_t kSegItems = 8;                               // reads per thread of the counting kernels
constexpr uint32_t kSegBlock = kBlockThreads * kSegItems;       // reads per workgroup

struct SegGeom {
    SegSource src;
    uint32_t n_reads;
    uint32_t l;  // k + w - 1: bases of a window
    uint32_t S;  // windows per lane at most
    uint32_t n_bases;  // (COUNTS) bases of the reads: starts are cut to it, so no lane leaves the span whatever they hold
};

// COUNTS: the reads and bases of the run come from src.counts (n_reads was the bound that sized the launch); *refused:
// the counts exceed their bounds - no read is tabulated
template <bool COUNTS>
__device__ __forceinline__ SegGeom seg_geom(const SegGeom &g_in, uint32_t *refused) {
    SegGeom g = g_in;
    *refused = 0u;
    if constexpr (COUNTS) {
        const LaneCountsView v = lane_counts_view(g.src.max_bases, g.src.max_records, g.src.counts[0], g.src.counts[1]);
        g.n_reads = v.n_reads_eff;
        g.n_bases = v.n_bases_eff;
        *refused = v.refused;
    }
    return g;
}

template <bool COUNTS>
__device__ __forceinline__ uint32_t seg_len(const SegGeom &g, uint32_t r) {
    if constexpr (COUNTS) {  // (reads back to back: starts[r] .. starts[r + 1], both cut to the bases the packer counted)
        unsigned long long s0 = g.src.starts[r], s1 = g.src.starts[r + 1];
        s0 = s0 < g.n_bases ? s0 : g.n_bases;
        s1 = s1 < g.n_bases ? s1 : g.n_bases;
        return s1 > s0 ? (uint32_t)(s1 - s0) : 0u;
    }
    unsigned long long len;
    if (g.src.lens) len = g.src.lens[r];
    else if (g.src.starts) {
        const unsigned long long s0 = g.src.starts[r], s1 = g.src.starts[r + 1];
        len = s1 > s0 ? s1 - s0 : 0ull;
    } else len = g.src.max_len;
    return len < (unsigned long long)g.src.max_len ? (uint32_t)len : g.src.max_len;
}
template <bool COUNTS>
__device__ __forceinline__ uint32_t seg_windows(const SegGeom &g, uint32_t r) {
    const uint32_t len = seg_len<COUNTS>(g, r);
    return len >= g.l ? len - g.l + 1u : 0u;
}
// lanes of a read: every read owns at least one (a read without a window: an empty lane that stores its offset)
template <bool COUNTS>
__device__ __forceinline__ uint32_t seg_lanes(const SegGeom &g, uint32_t r) {
    const uint32_t nw = seg_windows<COUNTS>(g, r);
    return nw ? (nw + g.S - 1u) / g.S : 1u;
}
template <bool COUNTS>
__device__ __forceinline__ unsigned long long seg_start(const SegGeom &g, uint32_t r) {
    if constexpr (COUNTS) {
        const unsigned long long s0 = g.src.starts[r];
        return s0 < g.n_bases ? s0 : g.n_bases;
    }
    return g.src.starts ? g.src.starts[r] : (unsigned long long)r * g.src.stride;
}

// sum over the workgroup (every thread gets it); `lds` holds kWavesPerBlock words
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *lds) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) lds[threadIdx.x / kWave] = v;
    __syncthreads();
    uint32_t t = 0;
#pragma unroll
    for (int i = 0; i < kWavesPerBlock; ++i) t += lds[i];
    __syncthreads();
    return t;
}

template <bool COUNTS>
__global__ __launch_bounds__(kBlockThreads) void seg_count_kernel(const SegGeom g_in, uint32_t *blk_sums) {
    __shared__ uint32_t lds[kWavesPerBlock];
    uint32_t refused;
    const SegGeom g = seg_geom<COUNTS>(g_in, &refused);
    const uint32_t r0 = (blockIdx.x * kBlockThreads + threadIdx.x) * kSegItems;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t i = 0; i < kSegItems; ++i)
        if (r0 + i < g.n_reads) v += seg_lanes<COUNTS>(g, r0 + i);
    const uint32_t t = block_sum(v, lds);
    if (threadIdx.x == 0) blk_sums[blockIdx.x] = t;
}

// exclusive scan of blk_sums[0 .. n) in place; blk_sums[n] receives the total
__global__ __launch_bounds__(1024) void seg_scan_kernel(uint32_t *blk_sums, uint32_t n) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry_s;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += 1024u) {
        const uint32_t i = base + tid;
        const uint32_t v = i < n ? blk_sums[i] : 0u;
        const uint32_t incl = wave_inclusive_sum(v);
        if (lane == kWave - 1) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = carry_s;
        for (uint32_t q = 0; q < wave; ++q) before += wsum[q];
        if (i < n) blk_sums[i] = before + incl - v;
        __syncthreads();
        if (tid == 1023u) carry_s = before + incl;
        __syncthreads();
    }
    if (tid == 0) blk_sums[n] = carry_s;
}

// (also: tile_r0[b] = the read that owns lane 256 b, the first lane of tile b - written by the read's own thread, so that
// seg_fill_kernel starts without a search of the whole array; a read that spans many tiles loops over them)
// (COUNTS: no read at all, or the counts refused - g.n_reads == 0 - leaves seg_first[0] = 0, the total the fill kernel reads)
template <bool COUNTS>
__global__ __launch_bounds__(kBlockThreads) void seg_first_kernel(const SegGeom g_in, const uint32_t *blk_sums, uint32_t n_blocks,
                                                                  uint32_t *seg_first, uint32_t *tile_r0, uint32_t n_tiles) {
    __shared__ uint32_t wsum[kWavesPerBlock];
    uint32_t refused;
    const SegGeom g = seg_geom<COUNTS>(g_in, &refused);
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t r0 = (blockIdx.x * kBlockThreads + tid) * kSegItems;
    uint32_t c[kSegItems], v = 0;
#pragma unroll
    for (uint32_t i = 0; i < kSegItems; ++i) {
        c[i] = r0 + i < g.n_reads ? seg_lanes<COUNTS>(g, r0 + i) : 0u;
        v += c[i];
    }
    const uint32_t incl = wave_inclusive_sum(v);
    if (lane == kWave - 1) wsum[wave] = incl;
    __syncthreads();
    // (n_blocks == 1 - up to 2048 reads: this workgroup is the whole scan, the counting and scanning kernels are not launched -
    // two launches less on a small batch's stream, 84 -> 78 us for 100 reads of 10 kbp, tools/gpu_lanes_small.py)
    uint32_t at = (n_blocks == 1u ? 0u : blk_sums[blockIdx.x]) + incl - v;
    for (uint32_t q = 0; q < wave; ++q) at += wsum[q];
#pragma unroll
    for (uint32_t i = 0; i < kSegItems; ++i) {
        if (r0 + i < g.n_reads) {
            seg_first[r0 + i] = at;
            for (uint32_t b = (at + kFusedThreads - 1u) / kFusedThreads; b < n_tiles && b * kFusedThreads < at + c[i]; ++b) tile_r0[b] = r0 + i;
        }
        at += c[i];
    }
    if (blockIdx.x == 0 && tid == 0) {
        uint32_t total = 0;
        if (n_blocks == 1u) {
#pragma unroll
            for (int q = 0; q < kWavesPerBlock; ++q) total += wsum[q];
        } else {
            total = blk_sums[n_blocks];
        }
        seg_first[g.n_reads] = total;
    }
}

template <bool COUNTS>
__global__ __launch_bounds__(kFusedThreads) void seg_fill_kernel(const SegGeom g_in, const uint32_t *seg_first, LaneSeg *table,
                                                                 uint32_t *tile_origin, uint32_t *error) {
    __shared__ uint32_t wmin[kFusedWaves];
    uint32_t refused;
    const SegGeom g = seg_geom<COUNTS>(g_in, &refused);
    const uint32_t lane_id = blockIdx.x * kFusedThreads + threadIdx.x;
    const uint32_t total = seg_first[g.n_reads];
    // counts beyond their bounds (a packer whose table or buffer was too small): the run is an empty batch and fails with
    // error code 7, raised once
    if (COUNTS && lane_id == 0 && refused) flag_error(error, 7u);
    // more lanes than the grid was sized for: the caller's total_bases understates its reads (the bound is n_reads +
    // total_bases / S).  The run fails with error code 5 instead of dropping the reads behind the table.
    if (lane_id == 0 && total > gridDim.x * kFusedThreads) flag_error(error, 5u);
    LaneSeg sg{0u, 1u, 0u, 0xffffffffu};  // (behind the table: no window, not a read's first lane)
    // The read a lane belongs to is the last r with seg_first[r] <= lane_id (strictly increasing: every read owns a lane).
    // The read r0 of the tile's first lane comes from seg_first_kernel (tile_origin[b] holds it until this kernel stores the
    // origin there); the tile's other lanes belong to reads r0 .. r0 + 255 at most, whose entries go to LDS in one coalesced
    // load and are searched there.  (A search of the whole array per lane - or per tile, by one thread - is a chain of 18
    // dependent loads per workgroup: 100 us per 8 M lanes, 7 % of the long-read row, profiles/r06_f_LONGREADS.txt.)
    __shared__ uint32_t s_first[kFusedThreads + 1];
    const uint32_t lane0 = blockIdx.x * kFusedThreads;
    uint32_t r0 = lane0 < total ? tile_origin[blockIdx.x] : 0u;
    r0 = r0 < g.n_reads ? r0 : (COUNTS && g.n_reads == 0u ? 0u : g.n_reads - 1u);  // (COUNTS: there may be no read at all)
    {
        const uint32_t i0 = r0 + threadIdx.x;
        s_first[threadIdx.x] = seg_first[i0 < g.n_reads ? i0 : g.n_reads];  // (behind the last read: the total, above every lane)
        if (threadIdx.x == 0) s_first[kFusedThreads] = seg_first[r0 + kFusedThreads < g.n_reads ? r0 + kFusedThreads : g.n_reads];
    }
    __syncthreads();
    if (lane_id < total) {
        uint32_t lo = 0, hi = kFusedThreads;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1u) / 2u;
            if (s_first[mid] <= lane_id) lo = mid;
            else hi = mid - 1u;
        }
        const uint32_t r = r0 + lo, f = s_first[lo], ns = s_first[lo + 1 <= kFusedThreads ? lo + 1 : kFusedThreads] - f, j = lane_id - f;
        const uint32_t nw = seg_windows<COUNTS>(g, r);
        // the read's windows in ns shares of (almost) equal length: share j = base + (j < rem) windows
        const uint32_t base = nw / ns, rem = nw % ns;
        sg.win0 = j * base + (j < rem ? j : rem);
        sg.count = base + (j < rem ? 1u : 0u);
        sg.start = (uint32_t)(seg_start<COUNTS>(g, r) + sg.win0);
        sg.read = r;
    }
    table[lane_id] = sg;
    uint32_t m = sg.count ? sg.start : 0xffffffffu;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, d, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0) wmin[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0xffffffffu;
#pragma unroll
        for (int i = 0; i < kFusedWaves; ++i) t = min(t, wmin[i]);
        tile_origin[blockIdx.x] = t == 0xffffffffu ? 0u : t;
    }
}

// Behind the walk of a COUNTS run: the walk was given the bound max_records as its number of reads and left the total in
// offsets[max_records]; the reads between the real count and the bound get it as their offset (they are empty), so that
// what follows on the stream (mm_values_*_reads_device_async with n_reads = max_records) sees a whole table.  16-byte
// stores where the address allows, a grid-stride loop over the tail.
__global__ __launch_bounds__(kBlockThreads) void seg_tail_kernel(const unsigned long long *counts, uint32_t max_bases,
                                                                 uint32_t max_records, unsigned long long *offsets) {
    const LaneCountsView v = lane_counts_view(max_bases, max_records, counts[0], counts[1]);
    const unsigned long long total = offsets[max_records];
    const uint32_t gid = blockIdx.x * kBlockThreads + threadIdx.x, stride = gridDim.x * kBlockThreads;
    uint32_t first = v.n_reads_eff;  // entries [first, max_records) are filled
    if (first >= max_records) return;
    if (reinterpret_cast<uintptr_t>(offsets + first) & 15u) {
        if (gid == 0) offsets[first] = total;
        ++first;
    }
    const uint32_t pairs = (max_records - first) / 2u;
    ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(offsets + first);
    for (uint32_t i = gid; i < pairs; i += stride) dst[i] = make_ulonglong2(total, total);
    if (((max_records - first) & 1u) && gid == 0) offsets[max_records - 1u] = total;
}

template <bool COUNTS>
int launch_lane_table_impl(const SegGeom &g, uint32_t nb, const SegPlan &plan, const SegBuffers &b, uint32_t *error,
                           hipStream_t stream) {
    if (nb > 1) {
        hipLaunchKernelGGL(seg_count_kernel<COUNTS>, dim3(nb), dim3(kBlockThreads), 0, stream, g, b.blk_sums);
        hipLaunchKernelGGL(seg_scan_kernel, dim3(1), dim3(1024), 0, stream, b.blk_sums, nb);
    }
    hipLaunchKernelGGL(seg_first_kernel<COUNTS>, dim3(nb), dim3(kBlockThreads), 0, stream, g, b.blk_sums, nb, b.seg_first,
                       b.tile_origin, (uint32_t)plan.tiles);
    hipLaunchKernelGGL(seg_fill_kernel<COUNTS>, dim3((uint32_t)plan.tiles), dim3(kFusedThreads), 0, stream, g, b.seg_first, b.table,
                       b.tile_origin, error);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace

uint64_t lane_table_blocks(uint64_t n_reads) { return (n_reads + kSegBlock - 1) / kSegBlock; }

// Queues the four kernels.  b.blk_sums holds lane_table_blocks(n_reads) + 1 words, b.seg_first n_reads + 1, b.table
// plan.tiles * 256 entries, b.tile_origin plan.tiles.  Returns 0 or -1.
// (src.counts: n_reads >= max(src.max_records, 1) is the bound the buffers and `plan` were sized for; the two-kernel
// shortcut is decided by it, the kernels work on the reads the counts name)
int launch_lane_table(const SegSource &src, uint64_t n_reads, uint32_t l, const SegPlan &plan, const SegBuffers &b,
                      uint32_t *error, hipStream_t stream) {
    if (n_reads == 0 || n_reads >= (1ull << 32) || plan.tiles == 0) return -1;
    if (src.counts && (!src.starts || src.lens || src.max_records > n_reads)) return -1;
    SegGeom g;
    g.src = src;
    g.n_reads = (uint32_t)n_reads;
    g.l = l;
    g.S = plan.S;
    g.n_bases = 0;
    const uint32_t nb = (uint32_t)lane_table_blocks(n_reads);
    return src.counts ? launch_lane_table_impl<true>(g, nb, plan, b, error, stream)
                      : launch_lane_table_impl<false>(g, nb, plan, b, error, stream);
}

// the epilogue of a counts run, queued behind the walk (max_records == 0: the walk's offsets[0] is the whole table)
int launch_lane_tail(const SegSource &src, unsigned long long *offsets, hipStream_t stream) {
    if (!src.counts || !offsets) return -1;
    if (src.max_records == 0) return 0;
    const uint64_t want = ((uint64_t)src.max_records / 2 + kBlockThreads - 1) / kBlockThreads;
    const uint32_t blocks = want > 1024 ? 1024u : (want ? (uint32_t)want : 1u);
    hipLaunchKernelGGL(seg_tail_kernel, dim3(blocks), dim3(kBlockThreads), 0, stream, src.counts, src.max_bases, src.max_records,
                       offsets);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// mm_plan_prepare: the table's kernels - both instantiations and the epilogue of a counts run - loaded on the current
// device without a launch
hipError_t lane_table_prepare(uint32_t *kernels) {
    return load_kernels({reinterpret_cast<const void *>(seg_count_kernel<false>), reinterpret_cast<const void *>(seg_scan_kernel),
                         reinterpret_cast<const void *>(seg_first_kernel<false>), reinterpret_cast<const void *>(seg_fill_kernel<false>),
                         reinterpret_cast<const void *>(seg_count_kernel<true>), reinterpret_cast<const void *>(seg_first_kernel<true>),
                         reinterpret_cast<const void *>(seg_fill_kernel<true>), reinterpret_cast<const void *>(seg_tail_kernel)},
                        kernels);
}

}  // namespace mm
