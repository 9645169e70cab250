// mm_values_text.hip — k-mer values of byte text: Output::values_u64 / values_u128 (src/lib.rs:584-629) at the positions
// the text entry points write, for a single text (absolute positions) and for a batch of records in ONE launch
// (record-local positions plus the n_records + 1 offsets that delimit them; value i belongs to the record r with
// offsets[r] <= i < offsets[r + 1] and its k-mer starts at character starts[r] + pos[i]).  The text stands for one of two
// reference Seqs (mm_values_text.h): `&[u8]` at 8 bits per character, or packed-seq AsciiSeq at 2.
//
// The shape is that of the packed values kernels (mm_aux.hip, mm_values_reads.hip): a workgroup of 256 threads takes 1024
// consecutive values (u64: four per thread, one 16-byte position load and two 16-byte stores each) or 256 (u128: one per
// thread, one 16-byte store).  What is new:
//   - the gather: a k-mer is len bytes at ANY byte address.  A thread loads the whole dwords that cover it (NDW = 3 for 8
//     bytes, 5 for 16, 9 for 32 characters, 17 for 64: consecutive dwords, which the compiler merges into 16-byte
//     loads - a dword-aligned address is all those need) and shifts by the byte phase with v_alignbyte, the byte
//     counterpart of value_of's v_alignbit.  A thread with a dword not wholly inside [d_text, d_text + text_bytes) takes
//     the rolled edge path instead (edge_dword, mm_values_load.h): single bytes inside, zeros outside;
//   - the DNA compression: the four characters of a shifted dword become eight bits by SWAR (dna_codes_of), eight dwords
//     the 64-bit forward value; the canonical step is the packed kernels' (mm_values.h);
//   - BYTES is the gather plus a mask.
// The batch kernel looks records up as the reads kernel looks reads up (values_read_of, mm_values_reads.h): ONE search per
// workgroup for the records of its first and last value; if the offsets between them fit the LDS stage
// (kValuesTextStage) they are staged, every thread searches LDS once and steps forward, skipping empty records;
// otherwise every value is searched in global memory within that span, from its predecessor's record on.  The searches
// stay inside [0, n_records - 1] whatever the offsets hold, and the true count is offsets[n_records], read on the device.
// All stores are vector stores.
#include "mm_common.h"
#include "mm_launch.h"
#include "mm_values_reads.h"
#include "mm_values_text.h"

namespace mm {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// NDW dwords per value (mm_values_text.h); VPT values per thread: 4 (u64) or 1 (u128)
template <int NDW, bool DNA, bool U128, bool BATCH>
__global__ __launch_bounds__(kBlockThreads) void values_text_kernel(ValuesTextArgs a) {
    constexpr int VPT = U128 ? 1 : 4;
    constexpr unsigned long long kPerBlock = (unsigned long long)kBlockThreads * VPT;
    constexpr uint32_t kOutBytes = U128 ? 16u : 8u;

    unsigned long long total = a.n_pos_max;
    unsigned long long n_records = a.n_records;
    if constexpr (BATCH) {
        if (a.counts) {  // (uniform: the device's own counts, within the caller's bounds or nothing is written)
            const unsigned long long c_chars = a.counts[0], c_records = a.counts[1];
            if (c_chars > a.max_chars || c_records > n_records || c_records == 0ull) return;
            n_records = c_records;
        }
        const unsigned long long total0 = a.offsets[n_records];
        if (total0 < total) total = total0;  // (never past what the buffers hold)
    }
    const unsigned long long i0 = (unsigned long long)blockIdx.x * kPerBlock;  // first value of the workgroup
    if (i0 >= total) return;
    const unsigned long long left = total - i0;
    const uint32_t here = left < kPerBlock ? (uint32_t)left : (uint32_t)kPerBlock;

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

    // the byte of view.d at which each of the thread's k-mers starts
    unsigned long long p[VPT];
    if constexpr (!BATCH) {
#pragma unroll
        for (int u = 0; u < VPT; ++u) p[u] = a.view.base0 + ps[u];
    } else {
        __shared__ unsigned long long stage[kValuesTextStage];
        const unsigned long long *__restrict__ offsets = a.offsets;
        // one search per workgroup: the records of its first and last value (uniform: scalar loads).  A value's record is
        // at most n_records - 1 (i < offsets[n_records]); searching no further keeps offsets[r + 1] and starts[r] inside
        // their arrays whatever the offsets hold.
        const unsigned long long r_first = values_read_of(offsets, 0ull, n_records - 1ull, i0);
        const unsigned long long r_last = values_read_of(offsets, r_first, n_records - 1ull, i0 + here - 1u);
        const unsigned long long span = r_last - r_first + 2ull;  // offsets[r_first .. r_last + 1]
        const bool staged = span <= (unsigned long long)kValuesTextStage;
        if (staged) {
            for (uint32_t j = t; j < (uint32_t)span; j += kBlockThreads) stage[j] = offsets[r_first + j];
            __syncthreads();
        }
        const uint32_t first = t * (uint32_t)VPT;  // workgroup-local index of the thread's first value
        const uint32_t mine = first < here ? (here - first < (uint32_t)VPT ? here - first : (uint32_t)VPT) : 0u;
        // the record of each of the thread's values (r_last for the lanes past the end: a valid record, nothing is stored)
        unsigned long long rd[VPT];
        if (staged) {
            // LDS path: search the stage for the first value, step forward for the others (stage[j] = offsets[r_first + j];
            // the bound on j ends every step inside the stage)
            uint32_t j = mine ? (uint32_t)values_read_of(stage, 0ull, span - 2ull, i0 + first) : (uint32_t)(span - 2ull);
#pragma unroll
            for (int u = 0; u < VPT; ++u) {
                if ((uint32_t)u < mine)
                    while (j + 2u < (uint32_t)span && stage[j + 1u] <= i0 + first + (uint32_t)u) ++j;
                rd[u] = r_first + j;
            }
        } else {
            // global path: every value searched within the workgroup's span, from its predecessor's record on
            unsigned long long r = r_first;
#pragma unroll
            for (int u = 0; u < VPT; ++u) {
                if ((uint32_t)u < mine) r = values_read_of(offsets, r, r_last, i0 + first + (uint32_t)u);
                rd[u] = (uint32_t)u < mine ? r : r_last;
            }
        }
        unsigned long long r_have = rd[0], s_have = a.starts[rd[0]];
#pragma unroll
        for (int u = 0; u < VPT; ++u) {
            if (rd[u] != r_have) r_have = rd[u], s_have = a.starts[rd[u]];
            p[u] = a.view.base0 + s_have + ps[u];
        }
    }

    // the gathered characters of each value, unmasked.  Hot path: every k-mer of the thread lies in whole dwords inside
    // the text - all the loads are issued together, then shifted and compressed.  Otherwise (a thread at one of the
    // buffer's ends, a position past the text) each value goes through the rolled edge path.
    unsigned long long lo[VPT], hi[VPT];
    bool inside = true;
#pragma unroll
    for (int u = 0; u < VPT; ++u) inside = inside && dwords_inside<NDW>(a.view, p[u] >> 2);
    if (inside) {
        uint32_t w[VPT][NDW];
#pragma unroll
        for (int u = 0; u < VPT; ++u)
#pragma unroll
            for (int j = 0; j < NDW; ++j) w[u][j] = a.view.d[(p[u] >> 2) + (unsigned long long)j];
#pragma unroll
        for (int u = 0; u < VPT; ++u) text_value_bits<NDW, DNA>(w[u], (uint32_t)(p[u] & 3u), lo[u], hi[u]);
    } else {
#pragma unroll
        for (int u = 0; u < VPT; ++u) text_value_bits_edge<NDW, DNA>(a.view, p[u], lo[u], hi[u]);
    }

    if constexpr (!U128) {
        unsigned long long v[VPT];
#pragma unroll
        for (int u = 0; u < VPT; ++u) v[u] = text_value64<DNA>(lo[u], a.len, a.canonical);
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
        unsigned long long vlo = lo[0], vhi = hi[0];
        text_value128<DNA>(a.len, a.canonical, vlo, vhi);
        u32x4 o;
        o.x = (uint32_t)vlo;
        o.y = (uint32_t)(vlo >> 32);
        o.z = (uint32_t)vhi;
        o.w = (uint32_t)(vhi >> 32);
        __builtin_amdgcn_raw_buffer_store_b128(o, rout, t * 16u, 0, 0);
    }
}

template <int NDW, bool DNA, bool U128>
int launch_one(const ValuesTextArgs &a, bool batch, uint32_t blocks, hipStream_t stream) {
    if (batch)
        hipLaunchKernelGGL((values_text_kernel<NDW, DNA, U128, true>), dim3(blocks), dim3(kBlockThreads), 0, stream, a);
    else
        hipLaunchKernelGGL((values_text_kernel<NDW, DNA, U128, false>), dim3(blocks), dim3(kBlockThreads), 0, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace

int launch_values_text(const ValuesTextArgs &a, int encoding, bool u128, bool batch, hipStream_t stream) {
    if (a.n_pos_max == 0 || (batch && a.n_records == 0)) return 0;
    const uint64_t per_block = (uint64_t)kBlockThreads * (u128 ? 1 : 4);
    const uint64_t blocks64 = (a.n_pos_max + per_block - 1) / per_block;
    if (blocks64 > 0x7fffffffull) return -3;
    const uint32_t blocks = (uint32_t)blocks64;
    if (encoding == kTextValuesBytes)
        return u128 ? launch_one<text_value_dwords(16), false, true>(a, batch, blocks, stream)
                    : launch_one<text_value_dwords(8), false, false>(a, batch, blocks, stream);
    // DNA: half the dwords when the k-mer fits them at every byte phase
    if (u128)
        return a.len <= 32 ? launch_one<text_value_dwords(32), true, true>(a, batch, blocks, stream)
                           : launch_one<text_value_dwords(64), true, true>(a, batch, blocks, stream);
    return a.len <= 16 ? launch_one<text_value_dwords(16), true, false>(a, batch, blocks, stream)
                       : launch_one<text_value_dwords(32), true, false>(a, batch, blocks, stream);
}

void values_text_host_one(const PackedView &view, int encoding, uint32_t len, int canonical, bool u128, uint64_t abs_pos,
                          uint64_t *out) {
    const unsigned long long p = view.base0 + abs_pos;
    const uint32_t phase = (uint32_t)(p & 3u);
    unsigned long long lo = 0, hi = 0;
    auto one = [&](auto ndw, auto dna) {
        constexpr int NDW = decltype(ndw)::value;
        constexpr bool DNA = decltype(dna)::value;
        if (dwords_inside<NDW>(view, p >> 2)) {
            uint32_t w[NDW];
            load_dwords<NDW>(view, p >> 2, w);
            text_value_bits<NDW, DNA>(w, phase, lo, hi);
        } else {
            text_value_bits_edge<NDW, DNA>(view, p, lo, hi);
        }
        if (u128) text_value128<DNA>(len, canonical, lo, hi);
        else lo = text_value64<DNA>(lo, len, canonical);
    };
    using std::integral_constant;
    // (the instances the launches above choose)
    if (encoding == kTextValuesBytes) {
        if (u128) one(integral_constant<int, text_value_dwords(16)>{}, std::false_type{});
        else one(integral_constant<int, text_value_dwords(8)>{}, std::false_type{});
    } else if (u128) {
        if (len <= 32) one(integral_constant<int, text_value_dwords(32)>{}, std::true_type{});
        else one(integral_constant<int, text_value_dwords(64)>{}, std::true_type{});
    } else {
        if (len <= 16) one(integral_constant<int, text_value_dwords(16)>{}, std::true_type{});
        else one(integral_constant<int, text_value_dwords(32)>{}, std::true_type{});
    }
    out[0] = lo;
    if (u128) out[1] = hi;
}

}  // namespace mm
