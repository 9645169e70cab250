// mm_values_reads.hip — k-mer values of EVERY read's sampled positions in one launch: Output::values_u64 / values_u128
// (src/lib.rs:584-629) of what a loop over Builder::run (src/lib.rs:378) returns, for reads that share one packed
// buffer.  The reads entry points write read-LOCAL positions back to back plus the n_reads + 1 offsets that delimit
// them; value i belongs to the read r with offsets[r] <= i < offsets[r + 1] and its k-mer starts at base
// base_offset + start(r) + pos[i] of the buffer, start(r) = read_starts[r] (reads packed back to back) or
// r * read_stride (fixed-stride reads).
//
// The workgroup's shape and the read lookup are mm_values_block.h, the arithmetic mm_values.h.  This file's own:
//   - the TRUE count is offsets[n_reads], read on the device: the grid covers n_pos_max, workgroups and threads at or
//     past the true count store nothing, so the call queues behind the run that writes the offsets with no host wait;
//   - addressing is 64-bit throughout: a read may start at or beyond base 2^32, r * read_stride is a 64-bit product;
//   - the sequence loads are plain global loads of whole dwords that lie inside [d_packed, d_packed + packed_bytes); a
//     k-mer that touches the first or last partial dword, or leaves the buffer (a position past its read's end, a bad
//     start), takes the edge path, which reads single bytes inside the buffer and zeros outside.
#include "mm_common.h"
#include "mm_launch.h"
#include "mm_values.h"
#include "mm_values_block.h"
#include "mm_values_load.h"
#include "mm_values_reads.h"

namespace mm {

namespace {

__device__ __forceinline__ unsigned long long read_start(const ValuesReadsArgs &a, unsigned long long r) {
    return a.read_starts ? a.read_starts[r] : r * (unsigned long long)a.read_stride;
}

// VPT values per thread: 4 (u64) or 1 (u128)
template <int VPT, bool U128>
__global__ __launch_bounds__(kBlockThreads) void values_reads_kernel(ValuesReadsArgs a) {
    __shared__ unsigned long long stage[kValuesReadsStage];

    const unsigned long long *__restrict__ offsets = a.offsets;
    const unsigned long long total0 = offsets[a.n_reads];
    const unsigned long long total = total0 < a.n_pos_max ? total0 : a.n_pos_max;  // (never past what the buffers hold)
    const unsigned long long i0 = values_block_first<VPT>();
    if (i0 >= total) return;
    const uint32_t here = values_block_here<VPT>(i0, total);
    // one search per workgroup: a value's read is at most n_reads - 1 (the bounds: mm_values_block.h)
    const unsigned long long r_first = values_read_of(offsets, 0ull, a.n_reads - 1ull, i0);
    const unsigned long long r_last = values_read_of(offsets, r_first, a.n_reads - 1ull, i0 + here - 1u);
    const unsigned long long span = r_last - r_first + 2ull;  // offsets[r_first .. r_last + 1]
    const bool staged = span <= (unsigned long long)kValuesReadsStage;
    const ValuesBlock<VPT, U128> b(a.pos, a.out, i0, here);
    uint32_t ps[VPT];
    b.load_positions(ps);
    if (staged) {
        values_stage_offsets(stage, offsets, r_first, span);
        __syncthreads();
    }
    unsigned long long rd[VPT];
    MM_VALUES_RECORDS(VPT, rd, stage, offsets, r_first, r_last, span, staged, i0, here)

    unsigned long long p[VPT];
    values_by_record<VPT>(
        rd, [&](unsigned long long r) { return read_start(a, r); },
        [&](int u, unsigned long long start) { p[u] = a.view.base0 + start + ps[u]; });

    if constexpr (!U128) {
        const unsigned long long mask = a.len >= 32 ? ~0ull : ((1ull << (2u * a.len)) - 1ull);
        uint32_t w[VPT][3];
#pragma unroll
        for (int u = 0; u < VPT; ++u) load_dwords<3>(a.view, p[u] >> 4, w[u]);
        unsigned long long v[VPT];
#pragma unroll
        for (int u = 0; u < VPT; ++u)
            v[u] = value_of(w[u][0], w[u][1], w[u][2], 2u * (uint32_t)(p[u] & 15u), a.len, a.canonical, mask);
        b.store_u64(v);
    } else {
        uint32_t w32[5];
        load_dwords<5>(a.view, p[0] >> 4, w32);
        const unsigned long long w[5] = {w32[0], w32[1], w32[2], w32[3], w32[4]};
        unsigned long long lo, hi;
        value128_of(w, 2u * (uint32_t)(p[0] & 15u), a.len, a.canonical, lo, hi);
        b.store_u128(lo, hi);
    }
}

}  // namespace

int launch_values_reads(const ValuesReadsArgs &a, bool u128, hipStream_t stream) {
    if (a.n_pos_max == 0 || a.n_reads == 0) return 0;
    uint32_t blocks;
    if (values_grid(a.n_pos_max, u128, &blocks)) return -3;
    if (u128)
        hipLaunchKernelGGL((values_reads_kernel<1, true>), dim3(blocks), dim3(kBlockThreads), 0, stream, a);
    else
        hipLaunchKernelGGL((values_reads_kernel<4, false>), dim3(blocks), dim3(kBlockThreads), 0, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mm
