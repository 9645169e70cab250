// mm_one_min.hip — one minimizer per record in one call: one_minimizer(seq, hasher) (src/minimizers.rs:22-28, re-exported
// at src/lib.rs:211) of EVERY record of a packed buffer or of a byte text, the leftmost position that minimises
// hash & 0xffff_0000 over the record's k-mers.  It is a segmented argmin over records of any lengths laid back to back: a
// record may span thousands of workgroups or share one with thousands of others.
//
// The arithmetic and the per-lane walk are mm_one_min.h (shared with the host: mm_debug_one_minimizer_*).  Here:
//   - the k-mer start positions, numbered from the first record's start, are cut into tiles of kOneMinTile = 4096, one
//     workgroup of 256 lanes each, 16 consecutive positions per lane; the grid covers what the HOST knows (the buffer's
//     size), workgroups past the last record's end leave at once;
//   - thread 0 finds the records of the tile's first and last position (one search and one gallop over the starts), every
//     lane searches only between them;
//   - the tile's symbols - T + k - 1 of them, every k up to a tile's own size - are copied to LDS by whole dwords, so the
//     lanes' dependent chain of symbol and table look-ups never waits for global memory (a larger k reads them there);
//   - a lane hashes its first k-mer from the definition and rolls the rest (the "simple form": (k + 16) / 16 table steps per
//     position), tables in LDS; it keeps the minimum key per record and hands each (record, key) pair to an LDS slot
//     (ds_min_u64), slot = record - the tile's first record; pairs of records beyond kOneMinSlots slots - more than that
//     many records, empty ones included, inside a tile - go to global memory directly;
//   - after a barrier the used slots go out with ONE atomicMin(unsigned long long) per (tile, record) pair into the key
//     array (n words preset to all-ones on the same stream), a single global_atomic_umin_x2 without a return value;
//   - a second small kernel turns keys into positions: all-ones -> MM_NO_MINIMIZER;
//   - the COUNTS instances (mm_one_minimizer_*_counts_device_async) read the record and symbol counts on the device: grid
//     and keys are sized from the caller's bounds, thread 0 turns {counts, bounds} into (n, limit) with
//     one_min_counts_view (mm_one_min.h) where the others use a.n and a.avail, and a finish kernel of their own writes
//     MM_NO_MINIMIZER at and past n and raises kernel error 8 for counts beyond the bounds.  The host-n instances are the
//     code they were: the flag is a template parameter, the position loop has no run-time branch;
//   - the AMB instances (mm_one_minimizer_reads_skip_ambiguous_*: packed symbols only, starts x forward / canonical x
//     host-n / COUNTS and fixed stride x forward / canonical) skip every k-mer that holds an ambiguous base: the tile's
//     ambiguity bits, T + k - 1 of them, are staged in LDS next to the symbols (read from global memory where the symbols
//     are), a lane counts the clean run that ends at its newest symbol (mm_one_min.h) and a position has a key only when
//     the run holds its k symbols.  Again a template parameter: the other instances are the code they were.
// Nothing outside the symbols [0, limit), starts[0 .. n] and keys / out [0, n) is touched, whatever the starts hold: every
// record index is clamped to [0, n - 1] by the searches and every symbol index lies below the limit, which is itself
// clamped to the buffer - for the AMB instances to the bits of the ambiguity buffer as well (the host folds both into
// a.avail), so no byte outside [amb, amb + amb_bytes) is loaded.  All stores are vector stores or atomics; no inline assembly.
#include "mm_common.h"
#include "mm_launch.h"
#include "mm_one_min.h"

namespace mm {

namespace {

// A tile's symbols in LDS: the bytes [src, src + count) copied by whole dwords where the global address allows it (single
// bytes at both ends: no byte outside [src, src + count) is loaded).  dst has src's alignment modulo 4.
__device__ __forceinline__ void stage_bytes(uint8_t *dst, const uint8_t *src, uint32_t count, uint32_t tid) {
    uint32_t head = (4u - (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3u)) & 3u;
    if (head > count) head = count;
    const uint32_t dwords = (count - head) / 4, tail_at = head + 4 * dwords;
    if (tid < head) dst[tid] = src[tid];
    const uint32_t *s4 = reinterpret_cast<const uint32_t *>(src + head);
    uint32_t *d4 = reinterpret_cast<uint32_t *>(dst + head);
    for (uint32_t i = tid; i < dwords; i += kOneMinThreads) d4[i] = s4[i];
    if (tid < count - tail_at) dst[tail_at + tid] = src[tail_at + tid];
}

// The COUNTS instances' record count, from thread 0 to the workgroup.  A function of its own, called only under
// `if constexpr (COUNTS)`: the host-n instances never name the word, so their LDS is what it was by construction.
__device__ __forceinline__ unsigned long long &one_min_counts_n() {
    __shared__ unsigned long long s_n;
    return s_n;
}

// The AMB instances' ambiguity bits of a tile, T + k - 1 of them whenever the symbols are staged: at most 4 * kStage bits
// from any bit of a byte, placed at the global address's alignment modulo 4.  A function of its own for the reason above.
constexpr uint32_t kOneMinAmbStage = (2 * kOneMinTile / 4 + 4) / 2 + 1 + 3;  // bytes
__device__ __forceinline__ uint8_t *one_min_amb_stage() {
    __shared__ uint32_t s_amb[kOneMinAmbStage / 4 + 1];
    return reinterpret_cast<uint8_t *>(s_amb);
}

// TEXT: byte symbols and 256-entry tables (else 2-bit symbols, 4 entries).  kStage: bytes of a tile's symbols kept in LDS -
// every k up to a tile's own size; a larger k reads its symbols from global memory.
// COUNTS: a.n and a.avail are bounds, the true counts are read from a.counts (starts layout only).
// AMB (packed only): symbol i has the ambiguity bit a.amb0 + i of a.amb, a k-mer over a set bit has no key; a.avail is
// already cut to the bits the buffer holds, so no bit at or past the limit is loaded either.
template <bool TEXT, class Lay, bool CANON, bool COUNTS = false, bool AMB = false>
__global__ __launch_bounds__(kOneMinThreads) void one_min_kernel(Lay lay, OneMinArgs a) {
    constexpr int NTAB = TEXT ? 256 : 4;
    constexpr uint32_t kStage = TEXT ? 2 * kOneMinTile : 2 * kOneMinTile / 4 + 4;
    __shared__ OneMinPair s_in[NTAB], s_out[NTAB];
    __shared__ unsigned long long s_keys[kOneMinSlots];
    __shared__ uint32_t s_stage[kStage / 4 + 1];
    __shared__ OneMinTileRange s_range;
    __shared__ int s_any;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        if constexpr (COUNTS) {
            // (a refused view and one without a record have n = 0: the starts are not read, the tile leaves)
            const OneMinCountsView v = one_min_counts_view(lay.s, (uint64_t)a.avail, (uint64_t)a.n, (uint64_t)a.counts[0],
                                                           (uint64_t)a.counts[1]);
            one_min_counts_n() = v.n;
            s_any = v.n != 0 && one_min_tile_range(lay, v.n, v.limit, a.k, (uint64_t)blockIdx.x, kOneMinTile, &s_range) ? 1 : 0;
        } else {
            unsigned long long limit = lay.end(a.n - 1);
            if (limit > a.avail) limit = a.avail;
            s_any = one_min_tile_range(lay, (uint64_t)a.n, (uint64_t)limit, a.k, (uint64_t)blockIdx.x, kOneMinTile, &s_range) ? 1 : 0;
        }
    }
    __syncthreads();
    if (!s_any) return;
    [[maybe_unused]] unsigned long long n_counts = 0;
    if constexpr (COUNTS) n_counts = one_min_counts_n();
    const OneMinTileRange range = s_range;
    const uint64_t span = range.r_hi - range.r_lo + 1;
    const uint32_t n_slots = span < kOneMinSlots ? (uint32_t)span : kOneMinSlots;
    for (uint32_t i = tid; i < n_slots; i += kOneMinThreads) s_keys[i] = kOneMinNoKey;
    if (!TEXT) {
        if (tid < 4) {
            s_in[tid] = OneMinPair{a.small_in[tid].x, a.small_in[tid].y};
            s_out[tid] = OneMinPair{a.small_out[tid].x, a.small_out[tid].y};
        }
    } else {
        for (uint32_t i = tid; i < (uint32_t)NTAB; i += kOneMinThreads) {
            const uint2 e = a.tables->t_in[i], o = a.tables->t_out[i];
            s_in[i] = OneMinPair{e.x, e.y};
            s_out[i] = OneMinPair{o.x, o.y};
        }
    }
    // the symbols [g_begin, g_end + k - 1) of the tile (all below the limit): their bytes
    const uint64_t sym_lo = (TEXT ? 0 : a.base0) + range.g_begin, sym_hi = sym_lo + (range.g_end - range.g_begin) + a.k - 2;
    const uint64_t byte_lo = TEXT ? sym_lo : sym_lo >> 2, byte_hi = TEXT ? sym_hi : sym_hi >> 2;  // (inclusive)
    const bool staged = byte_hi - byte_lo < kStage;
    const uint8_t *const src = a.syms + byte_lo;
    uint8_t *const stage = reinterpret_cast<uint8_t *>(s_stage) + (reinterpret_cast<uintptr_t>(src) & 3u);
    if (staged) stage_bytes(stage, src, (uint32_t)(byte_hi - byte_lo + 1), tid);
    [[maybe_unused]] const uint8_t *amb_stage = nullptr;
    [[maybe_unused]] uint64_t amb_byte_lo = 0;
    if constexpr (AMB) {
        // the bits of the same symbols: [a.amb0 + g_begin, a.amb0 + g_end + k - 1), staged whenever the symbols are
        const uint64_t bit_lo = a.amb0 + range.g_begin, bit_hi = bit_lo + (range.g_end - range.g_begin) + a.k - 2;
        amb_byte_lo = bit_lo >> 3;
        const uint8_t *const amb_src = a.amb + amb_byte_lo;
        uint8_t *const dst = one_min_amb_stage() + (reinterpret_cast<uintptr_t>(amb_src) & 3u);
        if (staged) stage_bytes(dst, amb_src, (uint32_t)((bit_hi >> 3) - amb_byte_lo + 1), tid);
        amb_stage = dst;
    }
    __syncthreads();
    const uint64_t g0 = range.g_begin + (uint64_t)tid * kOneMinPerLane;
    if (g0 < range.g_end) {
        const uint64_t g1 = range.g_end - g0 < kOneMinPerLane ? range.g_end : g0 + kOneMinPerLane;
        OneMinTables t;
        t.t_in = s_in;
        t.t_out = s_out;
        t.fw0 = a.fw0;
        t.rc0 = a.rc0;
        t.rot = a.rot;
        t.canonical = CANON ? 1u : 0u;
        auto emit = [&](uint64_t r, uint64_t key) {
            const uint64_t slot = r - range.r_lo;
            if (slot < n_slots) atomicMin(&s_keys[slot], (unsigned long long)key);
            else if constexpr (COUNTS) {
                if (r < n_counts) atomicMin(a.keys + r, (unsigned long long)key);
            } else if (r < a.n) atomicMin(a.keys + r, (unsigned long long)key);
        };
        if constexpr (TEXT) {
            if (staged) one_min_lane(OneMinText{stage, range.g_begin}, lay, range, t, a.k, g0, g1, emit);
            else one_min_lane(OneMinText{a.syms, 0}, lay, range, t, a.k, g0, g1, emit);
        } else if constexpr (AMB) {
            // (the staged copies start at bytes byte_lo and amb_byte_lo: symbol i is base a.base0 + i - 4 * byte_lo of the
            // one, bit a.amb0 + i - 8 * amb_byte_lo of the other)
            if (staged)
                one_min_lane(OneMinPackedAmb{OneMinPacked{stage, a.base0 - 4 * byte_lo}, amb_stage, a.amb0 - 8 * amb_byte_lo}, lay,
                             range, t, a.k, g0, g1, emit);
            else one_min_lane(OneMinPackedAmb{OneMinPacked{a.syms, a.base0}, a.amb, a.amb0}, lay, range, t, a.k, g0, g1, emit);
        } else {
            // (the staged copy starts at byte byte_lo: symbol i is base a.base0 + i - 4 * byte_lo of it)
            if (staged) one_min_lane(OneMinPacked{stage, a.base0 - 4 * byte_lo}, lay, range, t, a.k, g0, g1, emit);
            else one_min_lane(OneMinPacked{a.syms, a.base0}, lay, range, t, a.k, g0, g1, emit);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < n_slots; i += kOneMinThreads) {
        const unsigned long long key = s_keys[i];
        if (key != kOneMinNoKey) atomicMin(a.keys + (range.r_lo + i), key);
    }
}

__global__ __launch_bounds__(256) void one_min_finish_kernel(const unsigned long long *__restrict__ keys, uint32_t *__restrict__ out,
                                                             unsigned long long n) {
    const unsigned long long r = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (r < n) out[r] = one_min_position(keys[r]);
}

// The counts form: the words [0, n) of the view from the keys, "none" at and past it up to the bound `max_records`; the
// view's refusal is raised here (this kernel always runs, the main one has no workgroup when max_sym < k) in the sticky
// error word mm_workspace_check reads.
__global__ __launch_bounds__(256) void one_min_finish_counts_kernel(const unsigned long long *__restrict__ keys,
                                                                    uint32_t *__restrict__ out, const uint64_t *starts,
                                                                    const unsigned long long *__restrict__ counts,
                                                                    unsigned long long max_sym, unsigned long long max_records,
                                                                    uint32_t *error) {
    const OneMinCountsView v = one_min_counts_view(starts, (uint64_t)max_sym, (uint64_t)max_records, (uint64_t)counts[0],
                                                   (uint64_t)counts[1]);
    const unsigned long long r = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (r < max_records) out[r] = r < v.n ? one_min_position(keys[r]) : 0xFFFFFFFFu;
    if (v.refused && r == 0) error[2] = 8u;
}

template <class Lay, bool COUNTS>
void launch_main_amb(const Lay &lay, const OneMinArgs &a, uint32_t blocks, hipStream_t stream) {
    if (a.canonical)
        hipLaunchKernelGGL((one_min_kernel<false, Lay, true, COUNTS, true>), dim3(blocks), dim3(kOneMinThreads), 0, stream, lay, a);
    else
        hipLaunchKernelGGL((one_min_kernel<false, Lay, false, COUNTS, true>), dim3(blocks), dim3(kOneMinThreads), 0, stream, lay, a);
}

template <bool TEXT>
void launch_main_counts(const OneMinStarts &lay, const OneMinArgs &a, uint32_t blocks, hipStream_t stream) {
    if (a.canonical)
        hipLaunchKernelGGL((one_min_kernel<TEXT, OneMinStarts, true, true>), dim3(blocks), dim3(kOneMinThreads), 0, stream, lay, a);
    else
        hipLaunchKernelGGL((one_min_kernel<TEXT, OneMinStarts, false, true>), dim3(blocks), dim3(kOneMinThreads), 0, stream, lay, a);
}

template <bool TEXT, class Lay>
void launch_main(const Lay &lay, const OneMinArgs &a, uint32_t blocks, hipStream_t stream) {
    if (a.canonical)
        hipLaunchKernelGGL((one_min_kernel<TEXT, Lay, true>), dim3(blocks), dim3(kOneMinThreads), 0, stream, lay, a);
    else
        hipLaunchKernelGGL((one_min_kernel<TEXT, Lay, false>), dim3(blocks), dim3(kOneMinThreads), 0, stream, lay, a);
}

}  // namespace

int launch_one_min(const OneMinArgs &a, hipStream_t stream) {
    if (a.n == 0) return 0;
    if (a.amb && a.text) return -1;  // (byte text has no ambiguity bits)
    const uint64_t finish_blocks = (a.n + 255) / 256;
    if (finish_blocks > 0x7fffffffull) return -3;
    if (hipMemsetAsync(a.keys, 0xff, a.n * sizeof(unsigned long long), stream) != hipSuccess) return -1;
    if (a.counts) {
        // grid, keys and the finish for the BOUNDS (a.avail symbols, a.n records); workgroups past the view's last tile
        // leave at once
        if (!a.starts || !a.error) return -1;
        const OneMinStarts by_starts{reinterpret_cast<const uint64_t *>(a.starts)};
        if (a.avail >= a.k) {
            const uint64_t tiles = one_min_tiles(a.avail - a.k + 1, kOneMinTile);
            if (tiles > 0x7fffffffull) return -3;
            if (a.text) launch_main_counts<true>(by_starts, a, (uint32_t)tiles, stream);
            else if (a.amb) launch_main_amb<OneMinStarts, true>(by_starts, a, (uint32_t)tiles, stream);
            else launch_main_counts<false>(by_starts, a, (uint32_t)tiles, stream);
            if (hipGetLastError() != hipSuccess) return -1;
        }
        hipLaunchKernelGGL(one_min_finish_counts_kernel, dim3((uint32_t)finish_blocks), dim3(256), 0, stream, a.keys, a.out,
                           by_starts.s, a.counts, a.avail, a.n, a.error);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    // what the host knows of the positions: the symbols of the buffer (a fixed-stride layout: up to its last read's end)
    uint64_t symbols = a.avail;
    if (!a.starts) {
        const uint64_t end = (a.n - 1) * a.stride + a.len;
        if (end < symbols) symbols = end;
    }
    if (symbols >= a.k && (a.starts || a.len >= a.k)) {
        const uint64_t tiles = one_min_tiles(symbols - a.k + 1, kOneMinTile);
        if (tiles > 0x7fffffffull) return -3;
        const OneMinStarts by_starts{reinterpret_cast<const uint64_t *>(a.starts)};
        if (a.text) launch_main<true>(by_starts, a, (uint32_t)tiles, stream);
        else if (a.amb && a.starts) launch_main_amb<OneMinStarts, false>(by_starts, a, (uint32_t)tiles, stream);
        else if (a.amb) launch_main_amb<OneMinStride, false>(OneMinStride{a.stride, a.len}, a, (uint32_t)tiles, stream);
        else if (a.starts) launch_main<false>(by_starts, a, (uint32_t)tiles, stream);
        else launch_main<false>(OneMinStride{a.stride, a.len}, a, (uint32_t)tiles, stream);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    hipLaunchKernelGGL(one_min_finish_kernel, dim3((uint32_t)finish_blocks), dim3(256), 0, stream, a.keys, a.out, a.n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mm
