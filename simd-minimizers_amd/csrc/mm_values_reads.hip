// mm_values_reads.hip — k-mer values of EVERY read's sampled positions in one launch: Output::values_u64 / values_u128
// (src/lib.rs:584-629) of what a loop over Builder::run (src/lib.rs:378) returns, for reads that share one packed
// buffer.  The reads entry points write read-LOCAL positions back to back plus the n_reads + 1 offsets that delimit
// them; value i belongs to the read r with offsets[r] <= i < offsets[r + 1] and its k-mer starts at base
// base_offset + start(r) + pos[i] of the buffer, start(r) = read_starts[r] (reads packed back to back) or
// r * read_stride (fixed-stride reads).
//
// The arithmetic is mm_values.h, shared with the single-sequence kernels (mm_aux.hip); the shape is theirs too - a
// workgroup of 256 threads takes 1024 consecutive values (u64: four per thread, one 16-byte position load and two
// 16-byte stores each) or 256 (u128: one per thread, one 16-byte store).  What is new is the read lookup
// (values_read_of, mm_values_reads.h):
//   - the TRUE count is offsets[n_reads], read on the device: the grid covers n_pos_max, workgroups and threads at or
//     past the true count store nothing, so the call queues behind the run that writes the offsets with no host wait;
//   - ONE search per workgroup finds the reads of its first and last value.  If the offsets between them fit the LDS
//     stage (kValuesReadsStage entries) they are loaded once, every thread searches LDS for its first value and steps
//     forward for the next three, skipping empty reads (the LDS path);
//   - otherwise (long runs of empty reads) every value is searched in global memory within that span (the global path).
// Addressing is 64-bit throughout: a read may start at or beyond base 2^32, r * read_stride is a 64-bit product.  The
// sequence loads are plain global loads of whole dwords that lie inside [d_packed, d_packed + packed_bytes); a k-mer that
// touches the first or last partial dword, or leaves the buffer (a position past its read's end, a bad start), takes the
// edge path, which reads single bytes inside the buffer and zeros outside.  All stores are vector stores.
#include "mm_common.h"
#include "mm_launch.h"
#include "mm_values.h"
#include "mm_values_load.h"
#include "mm_values_reads.h"

namespace mm {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned long long read_start(const ValuesReadsArgs &a, unsigned long long r) {
    return a.read_starts ? a.read_starts[r] : r * (unsigned long long)a.read_stride;
}

// VPT values per thread: 4 (u64) or 1 (u128)
template <int VPT, bool U128>
__global__ __launch_bounds__(kBlockThreads) void values_reads_kernel(ValuesReadsArgs a) {
    constexpr unsigned long long kPerBlock = (unsigned long long)kBlockThreads * VPT;
    constexpr uint32_t kOutBytes = U128 ? 16u : 8u;
    __shared__ unsigned long long stage[kValuesReadsStage];

    const unsigned long long *__restrict__ offsets = a.offsets;
    const unsigned long long total0 = offsets[a.n_reads];
    const unsigned long long total = total0 < a.n_pos_max ? total0 : a.n_pos_max;  // (never past what the buffers hold)
    const unsigned long long i0 = (unsigned long long)blockIdx.x * kPerBlock;      // first value of the workgroup
    if (i0 >= total) return;
    const unsigned long long left = total - i0;
    const uint32_t here = left < kPerBlock ? (uint32_t)left : (uint32_t)kPerBlock;

    // one search per workgroup: the reads of its first and last value (uniform: scalar loads).  A value's read is at most
    // n_reads - 1 (i < offsets[n_reads]); searching no further keeps offsets[r + 1] and read_starts[r] inside their arrays
    // whatever the offsets hold.
    const unsigned long long r_first = values_read_of(offsets, 0ull, a.n_reads - 1ull, i0);
    const unsigned long long r_last = values_read_of(offsets, r_first, a.n_reads - 1ull, i0 + here - 1u);
    const unsigned long long span = r_last - r_first + 2ull;  // offsets[r_first .. r_last + 1]
    const bool staged = span <= (unsigned long long)kValuesReadsStage;

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
        for (uint32_t j = t; j < (uint32_t)span; j += kBlockThreads) stage[j] = offsets[r_first + j];
        __syncthreads();
    }

    const uint32_t first = t * (uint32_t)VPT;  // workgroup-local index of the thread's first value
    const uint32_t mine = first < here ? (here - first < (uint32_t)VPT ? here - first : (uint32_t)VPT) : 0u;
    // the read of each of the thread's values (r_last for the lanes past the end: a valid read, nothing is stored)
    unsigned long long rd[VPT];
    if (staged) {
        // LDS path: search the stage for the first value, step forward for the others (stage[j] = offsets[r_first + j];
        // i < offsets[r_last + 1] = stage[span - 1] ends every step inside the stage, and so does the bound on j)
        uint32_t j = mine ? (uint32_t)values_read_of(stage, 0ull, span - 2ull, i0 + first) : (uint32_t)(span - 2ull);
#pragma unroll
        for (int u = 0; u < VPT; ++u) {
            if ((uint32_t)u < mine)
                while (j + 2u < (uint32_t)span && stage[j + 1u] <= i0 + first + (uint32_t)u) ++j;
            rd[u] = r_first + j;
        }
    } else {
        // global path: every value searched within the workgroup's span, from its predecessor's read on
        unsigned long long r = r_first;
#pragma unroll
        for (int u = 0; u < VPT; ++u) {
            if ((uint32_t)u < mine) r = values_read_of(offsets, r, r_last, i0 + first + (uint32_t)u);
            rd[u] = (uint32_t)u < mine ? r : r_last;
        }
    }

    unsigned long long p[VPT];
    {
        unsigned long long r_have = rd[0], s_have = read_start(a, rd[0]);
#pragma unroll
        for (int u = 0; u < VPT; ++u) {
            if (rd[u] != r_have) r_have = rd[u], s_have = read_start(a, rd[u]);
            p[u] = a.view.base0 + s_have + ps[u];
        }
    }

    if constexpr (!U128) {
        const unsigned long long mask = a.len >= 32 ? ~0ull : ((1ull << (2u * a.len)) - 1ull);
        uint32_t w[VPT][3];
#pragma unroll
        for (int u = 0; u < VPT; ++u) load_dwords<3>(a.view, p[u] >> 4, w[u]);
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
        uint32_t w32[5];
        load_dwords<5>(a.view, p[0] >> 4, w32);
        const unsigned long long w[5] = {w32[0], w32[1], w32[2], w32[3], w32[4]};
        unsigned long long lo, hi;
        value128_of(w, 2u * (uint32_t)(p[0] & 15u), a.len, a.canonical, lo, hi);
        u32x4 o;
        o.x = (uint32_t)lo;
        o.y = (uint32_t)(lo >> 32);
        o.z = (uint32_t)hi;
        o.w = (uint32_t)(hi >> 32);
        __builtin_amdgcn_raw_buffer_store_b128(o, rout, t * 16u, 0, 0);
    }
}

}  // namespace

int launch_values_reads(const ValuesReadsArgs &a, bool u128, hipStream_t stream) {
    if (a.n_pos_max == 0 || a.n_reads == 0) return 0;
    const uint64_t per_block = (uint64_t)kBlockThreads * (u128 ? 1 : 4);
    const uint64_t blocks = (a.n_pos_max + per_block - 1) / per_block;
    if (blocks > 0x7fffffffull) return -3;
    if (u128)
        hipLaunchKernelGGL((values_reads_kernel<1, true>), dim3((uint32_t)blocks), dim3(kBlockThreads), 0, stream, a);
    else
        hipLaunchKernelGGL((values_reads_kernel<4, false>), dim3((uint32_t)blocks), dim3(kBlockThreads), 0, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mm
