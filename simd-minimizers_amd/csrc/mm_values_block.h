// mm_values_block.h — the workgroup skeleton of the k-mer value kernels (mm_aux.hip, mm_values_reads.hip,
// mm_values_batch.hip, mm_values_text.hip), in pieces a kernel composes; what a record IS - a read of one buffer, a
// sequence with a descriptor, a record of a text - and the arithmetic of a value stay in the kernels.
//
// The shape.  A workgroup of 256 threads takes 1024 consecutive values (u64: four per thread, one 16-byte position load
// and two 16-byte stores each) or 256 (u128: one per thread, one 16-byte store) through two workgroup-local buffer
// resources: lanes past the end load 0 and store nothing.  All stores are vector (buffer) stores.
//
// The record lookup of the segmented kernels: value i belongs to the record r with offsets[r] <= i < offsets[r + 1]
// (values_read_of, mm_values_reads.h).
//   - ONE search per workgroup finds the records r_first and r_last of its first and last value (uniform: scalar
//     loads); span = r_last - r_first + 2 is the number of offsets[r_first .. r_last + 1];
//   - if they fit the kernel's LDS stage (staged) they are loaded once (values_stage_offsets; the barrier is the
//     kernel's), every thread searches LDS for its first value and steps forward for the others, skipping empty records
//     (the LDS path of MM_VALUES_RECORDS);
//   - otherwise (long runs of empty records) every value is searched in global memory within that span, from its
//     predecessor's record on (the global path).
// The bounds: a value's record is at most n - 1 (i < offsets[n], the true count), searching no further keeps
// offsets[r + 1] and what a kernel reads per record - starts[r], seqs[r] - inside their arrays whatever the offsets
// hold; every later lookup stays inside [r_first, r_last].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mm_common.h"
#include "mm_values_reads.h"

namespace mm {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// The launch grid: one workgroup per 1024 (u64) or 256 (u128) of `count` values.  0, or -3: more than a grid holds.
inline int values_grid(uint64_t count, bool u128, uint32_t *blocks) {
    const uint64_t per_block = (uint64_t)kBlockThreads * (u128 ? 1 : 4);
    const uint64_t n = (count + per_block - 1) / per_block;
    if (n > 0x7fffffffull) return -3;
    *blocks = (uint32_t)n;
    return 0;
}

// first value of the workgroup; VPT values per thread: 4 (u64) or 1 (u128)
template <int VPT>
__device__ __forceinline__ unsigned long long values_block_first() {
    return (unsigned long long)blockIdx.x * ((unsigned long long)kBlockThreads * VPT);
}

// values of the workgroup, of `total` in all (i0 = values_block_first() < total)
template <int VPT>
__device__ __forceinline__ uint32_t values_block_here(unsigned long long i0, unsigned long long total) {
    constexpr unsigned long long kPerBlock = (unsigned long long)kBlockThreads * VPT;
    const unsigned long long left = total - i0;
    return left < kPerBlock ? (uint32_t)left : (uint32_t)kPerBlock;
}

// The workgroup's slice, `here` values from i0 on, as workgroup-local bounds-checked views: positions in, values out.
template <int VPT, bool U128>
struct ValuesBlock {
    __amdgpu_buffer_rsrc_t rpos, rout;

    __device__ __forceinline__ ValuesBlock(const uint32_t *pos, unsigned long long *out, unsigned long long i0, uint32_t here) {
        rpos = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(pos + i0), 0, (int)(here * 4u), 0x00020000);
        rout = __builtin_amdgcn_make_buffer_rsrc(out + i0 * (U128 ? 2u : 1u), 0, (int)(here * (U128 ? 16u : 8u)), 0x00020000);
    }

    // the thread's positions (the position array may start at any 4-byte boundary: a 16-byte load needs no more)
    __device__ __forceinline__ void load_positions(uint32_t (&ps)[VPT]) const {
        if constexpr (VPT == 4) {
            const u32x4 pp = __builtin_amdgcn_raw_buffer_load_b128(rpos, threadIdx.x * 16u, 0, 0);
            ps[0] = pp.x, ps[1] = pp.y, ps[2] = pp.z, ps[3] = pp.w;
        } else {
            ps[0] = __builtin_amdgcn_raw_buffer_load_b32(rpos, threadIdx.x * 4u, 0, 0);
        }
    }

    // the thread's u64 values, a pair per store
    __device__ __forceinline__ void store_u64(const unsigned long long (&v)[VPT]) const {
#pragma unroll
        for (int u = 0; u < VPT; u += 2) {
            u32x4 o;
            o.x = (uint32_t)v[u];
            o.y = (uint32_t)(v[u] >> 32);
            o.z = (uint32_t)v[u + 1];
            o.w = (uint32_t)(v[u + 1] >> 32);
            // (the last pair may be half inside: the bounds check works per dword, so its inner half is stored)
            __builtin_amdgcn_raw_buffer_store_b128(o, rout, threadIdx.x * 32u + (uint32_t)u * 8u, 0, 0);
        }
    }

    // the thread's one u128 value
    __device__ __forceinline__ void store_u128(unsigned long long lo, unsigned long long hi) const {
        u32x4 o;
        o.x = (uint32_t)lo;
        o.y = (uint32_t)(lo >> 32);
        o.z = (uint32_t)hi;
        o.w = (uint32_t)(hi >> 32);
        __builtin_amdgcn_raw_buffer_store_b128(o, rout, threadIdx.x * 16u, 0, 0);
    }
};

// stage[j] = offsets[r_first + j] for the `span` entries of a staged span (no barrier: the caller's follows its own loads)
__device__ __forceinline__ void values_stage_offsets(unsigned long long *stage, const unsigned long long *offsets,
                                                     unsigned long long r_first, unsigned long long span) {
    for (uint32_t j = threadIdx.x; j < (uint32_t)span; j += kBlockThreads) stage[j] = offsets[r_first + j];
}

// The record of each of the thread's VPT values, into `unsigned long long rd[VPT]` (r_last for the lanes past the end: a
// record WITH values, nothing is stored), from the kernel's r_first, r_last, span and staged (above) and its stage.
// A macro: the same statements as a force-inlined function are simplified on their own before they reach the kernel
// and leave it with another block layout and instruction stream (profiles/values_block_isa.txt).  One block statement:
// nothing but rd[] leaves it.  Every argument is evaluated more than once and none may be named first, mine, j, r or u.
#define MM_VALUES_RECORDS(VPT, rd, stage, offsets, r_first, r_last, span, staged, i0, here)                                \
{                                                                                                                         \
    const uint32_t first = threadIdx.x * (uint32_t)(VPT); /* workgroup-local index of the thread's first value */         \
    const uint32_t mine = first < (here) ? ((here) - first < (uint32_t)(VPT) ? (here) - first : (uint32_t)(VPT)) : 0u;    \
    if (staged) {                                                                                                         \
        /* LDS path: search the stage for the first value, step forward for the others (i < offsets[r_last + 1] =      */ \
        /* stage[span - 1] ends every step inside the stage, and so does the bound on j)                               */ \
        uint32_t j = mine ? (uint32_t)values_read_of(stage, 0ull, (span) - 2ull, (i0) + first) : (uint32_t)((span) - 2ull); \
        _Pragma("unroll") for (int u = 0; u < (VPT); ++u) {                                                               \
            if ((uint32_t)u < mine)                                                                                       \
                while (j + 2u < (uint32_t)(span) && stage[j + 1u] <= (i0) + first + (uint32_t)u) ++j;                     \
            rd[u] = (r_first) + j;                                                                                        \
        }                                                                                                                 \
    } else {                                                                                                              \
        /* global path: every value searched within the workgroup's span, from its predecessor's record on */            \
        unsigned long long r = (r_first);                                                                                 \
        _Pragma("unroll") for (int u = 0; u < (VPT); ++u) {                                                               \
            if ((uint32_t)u < mine) r = values_read_of(offsets, r, (r_last), (i0) + first + (uint32_t)u);                 \
            rd[u] = (uint32_t)u < mine ? r : (r_last);                                                                    \
        }                                                                                                                 \
    }                                                                                                                     \
}

// body(u, of(rd[u])) for each of the thread's values, `of` evaluated anew only when the record changes
template <int VPT, class Of, class Body>
__device__ __forceinline__ void values_by_record(const unsigned long long (&rd)[VPT], Of of, Body body) {
    unsigned long long r_have = rd[0];
    auto have = of(rd[0]);
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
        if (rd[u] != r_have) r_have = rd[u], have = of(rd[u]);
        body(u, have);
    }
}

}  // namespace mm
