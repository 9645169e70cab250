// mm_values_batch.hip — k-mer values of EVERY sequence of a device batch in one launch: Output::values_u64 / values_u128
// (src/lib.rs:584-629) of what the loop over Builder::run per contig (bench/src/bin/paper.rs:410-431) returns, for
// sequences that lie in separately allocated device buffers.  mm_run_batch_device writes sequence-LOCAL positions back to
// back plus the n_seqs + 1 offsets that delimit them; value i belongs to the sequence s with offsets[s] <= i <
// offsets[s + 1] and its k-mer starts at base base_offset[s] + pos[i] of sequence s's own buffer.
//
// The arithmetic is mm_values.h and the lookup values_read_of (mm_values_reads.h), both shared with the reads kernel
// (mm_values_reads.hip), whose shape this kernel has: a workgroup of 256 threads takes 1024 consecutive values (u64: four
// per thread, one 16-byte position load and two 16-byte stores each) or 256 (u128: one per thread, one 16-byte store).
// What differs is where a value's bytes are found: a table of per-sequence descriptors (ValuesBatchSeq, mm_values_batch.h)
// in device memory instead of starts inside one buffer.
//   - ONE search per workgroup finds the sequences of its first and last value.  If the offsets and descriptors between
//     them fit the LDS stage (kValuesBatchStage entries) they are loaded once, every thread searches the staged offsets
//     for its first value and steps forward for the next three, skipping sequences without values (the LDS path);
//   - otherwise (ladders of tiny sequences, long runs of empty ones) every value is searched in global memory within that
//     span, each from its predecessor's sequence on, and its descriptor read from the table (the global path).
// The bounds are PER SEQUENCE: the view of a value's sequence (aligned dword pointer, whole dwords [q_lo, q_hi), bytes
// [byte_lo, byte_hi), base0) is derived from its descriptor, the sequence loads are plain global loads of whole dwords
// inside it, and a k-mer that touches a partial first or last dword, or runs past the sequence's bytes, takes the rolled
// edge path of mm_values_load.h: single bytes inside, zeros outside.  No byte outside [d_packed[s], d_packed[s] +
// packed_bytes[s]) is loaded whatever the positions hold.  A sequence without values is never the answer of a lookup, so its
// descriptor (all zeros) is never dereferenced.  Addresses are 64-bit per sequence: the buffers may lie anywhere, in any order.
// All stores are vector (buffer) stores.
#include "mm_common.h"
#include "mm_launch.h"
#include "mm_values.h"
#include "mm_values_batch.h"
#include "mm_values_load.h"

namespace mm {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ PackedView view_of(const ValuesBatchSeq &s) {
    PackedView v;
    v.d = reinterpret_cast<const uint32_t *>(s.d);
    v.q_lo = values_batch_q_lo(s);
    v.q_hi = values_batch_q_hi(s);
    v.byte_lo = s.byte_lo;
    v.byte_hi = s.byte_hi;
    v.base0 = s.base0;
    return v;
}

// VPT values per thread: 4 (u64) or 1 (u128)
template <int VPT, bool U128>
__global__ __launch_bounds__(kBlockThreads) void values_batch_kernel(ValuesBatchArgs a) {
    constexpr unsigned long long kPerBlock = (unsigned long long)kBlockThreads * VPT;
    constexpr uint32_t kOutBytes = U128 ? 16u : 8u;
    __shared__ unsigned long long stage_off[kValuesBatchStage];
    __shared__ __attribute__((aligned(16))) ValuesBatchSeq stage_seq[kValuesBatchStage];

    const unsigned long long *__restrict__ offsets = a.offsets;
    const unsigned long long total = a.total;
    const unsigned long long i0 = (unsigned long long)blockIdx.x * kPerBlock;  // first value of the workgroup
    if (i0 >= total) return;
    const unsigned long long left = total - i0;
    const uint32_t here = left < kPerBlock ? (uint32_t)left : (uint32_t)kPerBlock;

    // one search per workgroup: the sequences of its first and last value (uniform: scalar loads).  A value's sequence is at
    // most n_seqs - 1; searching no further keeps offsets[s + 1] and seqs[s] inside their arrays.
    const unsigned long long r_first = values_read_of(offsets, 0ull, a.n_seqs - 1ull, i0);
    const unsigned long long r_last = values_read_of(offsets, r_first, a.n_seqs - 1ull, i0 + here - 1u);
    const unsigned long long span = r_last - r_first + 2ull;  // offsets[r_first .. r_last + 1], seqs[r_first .. r_last]
    const bool staged = span <= (unsigned long long)kValuesBatchStage;

    // workgroup-local bounds-checked views: positions in, values out (lanes past the end load 0 / store nothing)
    const __amdgpu_buffer_rsrc_t rpos =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(a.pos + i0), 0, (int)(here * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rout =
        __builtin_amdgcn_make_buffer_rsrc(a.out + i0 * (U128 ? 2u : 1u), 0, (int)(here * kOutBytes), 0x00020000);
    const uint32_t t = threadIdx.x;
    uint32_t ps[VPT];
    if constexpr (VPT == 4) {
        // (the position array may start at any 4-byte boundary: a 16-byte load needs no more)
        const u32x4 pp = __builtin_amdgcn_raw_buffer_load_b128(rpos, t * 16u, 0, 0);
        ps[0] = pp.x, ps[1] = pp.y, ps[2] = pp.z, ps[3] = pp.w;
    } else {
        ps[0] = __builtin_amdgcn_raw_buffer_load_b32(rpos, t * 4u, 0, 0);
    }

    if (staged) {
        for (uint32_t j = t; j < (uint32_t)span; j += kBlockThreads) stage_off[j] = offsets[r_first + j];
        // the span - 1 descriptors as 16-byte halves (the device table and the stage are 16-byte aligned)
        const u64x2 *src = reinterpret_cast<const u64x2 *>(a.seqs + r_first);
        u64x2 *dst = reinterpret_cast<u64x2 *>(stage_seq);
        for (uint32_t j = t; j < 2u * (uint32_t)(span - 1ull); j += kBlockThreads) dst[j] = src[j];
        __syncthreads();
    }

    const uint32_t first = t * (uint32_t)VPT;  // workgroup-local index of the thread's first value
    const uint32_t mine = first < here ? (here - first < (uint32_t)VPT ? here - first : (uint32_t)VPT) : 0u;
    // the sequence of each of the thread's values (r_last for the lanes past the end: a sequence WITH values, nothing is stored)
    unsigned long long rd[VPT];
    if (staged) {
        // LDS path: search the stage for the first value, step forward for the others (stage_off[j] = offsets[r_first + j];
        // i < offsets[r_last + 1] = stage_off[span - 1] ends every step inside the stage, and so does the bound on j)
        uint32_t j = mine ? (uint32_t)values_read_of(stage_off, 0ull, span - 2ull, i0 + first) : (uint32_t)(span - 2ull);
#pragma unroll
        for (int u = 0; u < VPT; ++u) {
            if ((uint32_t)u < mine)
                while (j + 2u < (uint32_t)span && stage_off[j + 1u] <= i0 + first + (uint32_t)u) ++j;
            rd[u] = r_first + j;
        }
    } else {
        // global path: every value searched within the workgroup's span, from its predecessor's sequence on
        unsigned long long r = r_first;
#pragma unroll
        for (int u = 0; u < VPT; ++u) {
            if ((uint32_t)u < mine) r = values_read_of(offsets, r, r_last, i0 + first + (uint32_t)u);
            rd[u] = (uint32_t)u < mine ? r : r_last;
        }
    }

    // per value: its sequence's view (derived anew only when the sequence changes) and the dwords that hold its k-mer
    constexpr int kDwords = U128 ? 5 : 3;
    unsigned long long p[VPT];
    uint32_t w[VPT][kDwords];
    {
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
#pragma unroll
        for (int u = 0; u < VPT; u += 2) {
            u32x4 o;
            o.x = (uint32_t)v[u];
            o.y = (uint32_t)(v[u] >> 32);
            o.z = (uint32_t)v[u + 1];
            o.w = (uint32_t)(v[u + 1] >> 32);
            // (the last pair may be half inside: the bounds check works per dword, so its inner half is stored)
            __builtin_amdgcn_raw_buffer_store_b128(o, rout, t * 32u + (uint32_t)u * 8u, 0, 0);
        }
    } else {
        const unsigned long long w64[5] = {w[0][0], w[0][1], w[0][2], w[0][3], w[0][4]};
        unsigned long long lo, hi;
        value128_of(w64, 2u * (uint32_t)(p[0] & 15u), a.len, a.canonical, lo, hi);
        u32x4 o;
        o.x = (uint32_t)lo;
        o.y = (uint32_t)(lo >> 32);
        o.z = (uint32_t)hi;
        o.w = (uint32_t)(hi >> 32);
        __builtin_amdgcn_raw_buffer_store_b128(o, rout, t * 16u, 0, 0);
    }
}

}  // namespace

int launch_values_batch(const ValuesBatchArgs &a, bool u128, hipStream_t stream) {
    if (a.total == 0 || a.n_seqs == 0) return 0;
    const uint64_t per_block = (uint64_t)kBlockThreads * (u128 ? 1 : 4);
    const uint64_t blocks = (a.total + per_block - 1) / per_block;
    if (blocks > 0x7fffffffull) return -3;
    if (u128)
        hipLaunchKernelGGL((values_batch_kernel<1, true>), dim3((uint32_t)blocks), dim3(kBlockThreads), 0, stream, a);
    else
        hipLaunchKernelGGL((values_batch_kernel<4, false>), dim3((uint32_t)blocks), dim3(kBlockThreads), 0, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mm
