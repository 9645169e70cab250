// mm_values_batch.hip — k-mer values of EVERY sequence of a device batch in one launch: Output::values_u64 / values_u128
// (src/lib.rs:584-629) of what the loop over Builder::run per contig (bench/src/bin/paper.rs:410-431) returns, for
// sequences that lie in separately allocated device buffers.  mm_run_batch_device writes sequence-LOCAL positions back to
// back plus the n_seqs + 1 offsets that delimit them; value i belongs to the sequence s with offsets[s] <= i <
// offsets[s + 1] and its k-mer starts at base base_offset[s] + pos[i] of sequence s's own buffer.
//
// The workgroup's shape and the sequence lookup are mm_values_block.h, the arithmetic mm_values.h.  This file's own is
// where a value's bytes are found: a table of per-sequence descriptors (ValuesBatchSeq, mm_values_batch.h) in device
// memory.  On the LDS path the span's descriptors are staged beside its offsets; on the global path (ladders of tiny
// sequences, long runs of empty ones) a value's descriptor is read from the table.
// The bounds are PER SEQUENCE: the view of a value's sequence (aligned dword pointer, whole dwords [q_lo, q_hi), bytes
// [byte_lo, byte_hi), base0) is derived from its descriptor, the sequence loads are plain global loads of whole dwords
// inside it, and a k-mer that touches a partial first or last dword, or runs past the sequence's bytes, takes the rolled
// edge path of mm_values_load.h: single bytes inside, zeros outside.  No byte outside [d_packed[s], d_packed[s] +
// packed_bytes[s]) is loaded whatever the positions hold.  A sequence without values is never the answer of a lookup, so its
// descriptor (all zeros) is never dereferenced.  Addresses are 64-bit per sequence: the buffers may lie anywhere, in any order.
#include "mm_common.h"
#include "mm_launch.h"
#include "mm_values.h"
#include "mm_values_batch.h"
#include "mm_values_block.h"
#include "mm_values_load.h"

namespace mm {

namespace {

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

// VPT values per thread: 4 (u64) or 1 (u128)
template <int VPT, bool U128>
__global__ __launch_bounds__(kBlockThreads) void values_batch_kernel(ValuesBatchArgs a) {
    __shared__ unsigned long long stage_off[kValuesBatchStage];
    __shared__ __attribute__((aligned(16))) ValuesBatchSeq stage_seq[kValuesBatchStage];

    const unsigned long long *__restrict__ offsets = a.offsets;
    const unsigned long long i0 = values_block_first<VPT>();
    if (i0 >= a.total) return;
    const uint32_t here = values_block_here<VPT>(i0, a.total);
    // one search per workgroup: a value's sequence is at most n_seqs - 1 (the bounds: mm_values_block.h)
    const unsigned long long r_first = values_read_of(offsets, 0ull, a.n_seqs - 1ull, i0);
    const unsigned long long r_last = values_read_of(offsets, r_first, a.n_seqs - 1ull, i0 + here - 1u);
    const unsigned long long span = r_last - r_first + 2ull;  // offsets[r_first .. r_last + 1], seqs[r_first .. r_last]
    const bool staged = span <= (unsigned long long)kValuesBatchStage;
    const ValuesBlock<VPT, U128> b(a.pos, a.out, i0, here);
    uint32_t ps[VPT];
    b.load_positions(ps);
    if (staged) {
        values_stage_offsets(stage_off, offsets, r_first, span);
        // the span - 1 descriptors as 16-byte halves (the device table and the stage are 16-byte aligned)
        const u64x2 *src = reinterpret_cast<const u64x2 *>(a.seqs + r_first);
        u64x2 *dst = reinterpret_cast<u64x2 *>(stage_seq);
        for (uint32_t j = threadIdx.x; j < 2u * (uint32_t)(span - 1ull); j += kBlockThreads) dst[j] = src[j];
        __syncthreads();
    }
    unsigned long long rd[VPT];
    MM_VALUES_RECORDS(VPT, rd, stage_off, offsets, r_first, r_last, span, staged, i0, here)

    // per value: its sequence's view and the dwords that hold its k-mer
    constexpr int kDwords = U128 ? 5 : 3;
    unsigned long long p[VPT];
    uint32_t w[VPT][kDwords];
    {  // (the view derived anew only when the sequence changes)
        unsigned long long r_have = rd[0];
        PackedView v = view_of(staged ? stage_seq[rd[0] - r_first] : a.seqs[rd[0]]);
#pragma unroll
        for (int u = 0; u < VPT; ++u) {
            if (rd[u] != r_have) {
                r_have = rd[u];
                v = view_of(staged ? stage_seq[rd[u] - r_first] : a.seqs[rd[u]]);
            }
            p[u] = v.base0 + ps[u];
            load_dwords<kDwords>(v, p[u] >> 4, w[u]);
        }
    }

    if constexpr (!U128) {
        const unsigned long long mask = a.len >= 32 ? ~0ull : ((1ull << (2u * a.len)) - 1ull);
        unsigned long long v[VPT];
#pragma unroll
        for (int u = 0; u < VPT; ++u)
            v[u] = value_of(w[u][0], w[u][1], w[u][2], 2u * (uint32_t)(p[u] & 15u), a.len, a.canonical, mask);
        b.store_u64(v);
    } else {
        const unsigned long long w64[5] = {w[0][0], w[0][1], w[0][2], w[0][3], w[0][4]};
        unsigned long long lo, hi;
        value128_of(w64, 2u * (uint32_t)(p[0] & 15u), a.len, a.canonical, lo, hi);
        b.store_u128(lo, hi);
    }
}

}  // namespace

int launch_values_batch(const ValuesBatchArgs &a, bool u128, hipStream_t stream) {
    if (a.total == 0 || a.n_seqs == 0) return 0;
    uint32_t blocks;
    if (values_grid(a.total, u128, &blocks)) return -3;
    if (u128)
        hipLaunchKernelGGL((values_batch_kernel<1, true>), dim3(blocks), dim3(kBlockThreads), 0, stream, a);
    else
        hipLaunchKernelGGL((values_batch_kernel<4, false>), dim3(blocks), dim3(kBlockThreads), 0, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mm
