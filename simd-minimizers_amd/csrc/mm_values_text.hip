// mm_values_text.hip — k-mer values of byte text: Output::values_u64 / values_u128 (src/lib.rs:584-629) at the positions
// the text entry points write, for a single text (absolute positions) and for a batch of records in ONE launch
// (record-local positions plus the n_records + 1 offsets that delimit them; value i belongs to the record r with
// offsets[r] <= i < offsets[r + 1] and its k-mer starts at character starts[r] + pos[i]).  The text stands for one of two
// reference Seqs (mm_values_text.h): `&[u8]` at 8 bits per character, or packed-seq AsciiSeq at 2.
//
// The workgroup's shape, and the batch kernels' record lookup, are mm_values_block.h.  This file's own:
//   - the gather: a k-mer is len bytes at ANY byte address.  A thread loads the whole dwords that cover it (NDW = 3 for 8
//     bytes, 5 for 16, 9 for 32 characters, 17 for 64: consecutive dwords, which the compiler merges into 16-byte
//     loads - a dword-aligned address is all those need) and shifts by the byte phase with v_alignbyte, the byte
//     counterpart of value_of's v_alignbit.  A thread with a dword not wholly inside [d_text, d_text + text_bytes) takes
//     the rolled edge path instead (edge_dword, mm_values_load.h): single bytes inside, zeros outside;
//   - the DNA compression: the four characters of a shifted dword become eight bits by SWAR (dna_codes_of), eight dwords
//     the 64-bit forward value; the canonical step is the packed kernels' (mm_values.h);
//   - BYTES is the gather plus a mask;
//   - the batch kernels' true count is offsets[n_records], read on the device, n_records itself the device's own when
//     the launch carries counts.
#include "mm_common.h"
#include "mm_launch.h"
#include "mm_values_block.h"
#include "mm_values_text.h"

namespace mm {

namespace {

// NDW dwords per value (mm_values_text.h); VPT values per thread: 4 (u64) or 1 (u128)
template <int NDW, bool DNA, bool U128, bool BATCH>
__global__ __launch_bounds__(kBlockThreads) void values_text_kernel(ValuesTextArgs a) {
    constexpr int VPT = U128 ? 1 : 4;

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
    const unsigned long long i0 = values_block_first<VPT>();
    if (i0 >= total) return;
    const uint32_t here = values_block_here<VPT>(i0, total);
    const ValuesBlock<VPT, U128> b(a.pos, a.out, i0, here);
    uint32_t ps[VPT];
    b.load_positions(ps);

    // the byte of view.d at which each of the thread's k-mers starts
    unsigned long long p[VPT];
    if constexpr (!BATCH) {
#pragma unroll
        for (int u = 0; u < VPT; ++u) p[u] = a.view.base0 + ps[u];
    } else {
        __shared__ unsigned long long stage[kValuesTextStage];
        const unsigned long long *__restrict__ offsets = a.offsets;
        // one search per workgroup: a value's record is at most n_records - 1 (the bounds: mm_values_block.h)
        const unsigned long long r_first = values_read_of(offsets, 0ull, n_records - 1ull, i0);
        const unsigned long long r_last = values_read_of(offsets, r_first, n_records - 1ull, i0 + here - 1u);
        const unsigned long long span = r_last - r_first + 2ull;  // offsets[r_first .. r_last + 1]
        const bool staged = span <= (unsigned long long)kValuesTextStage;
        if (staged) {
            values_stage_offsets(stage, offsets, r_first, span);
            __syncthreads();
        }
        unsigned long long rd[VPT];
        MM_VALUES_RECORDS(VPT, rd, stage, offsets, r_first, r_last, span, staged, i0, here)
        values_by_record<VPT>(
            rd, [&](unsigned long long r) { return a.starts[r]; },
            [&](int u, unsigned long long start) { p[u] = a.view.base0 + start + ps[u]; });
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
        b.store_u64(v);
    } else {
        unsigned long long vlo = lo[0], vhi = hi[0];
        text_value128<DNA>(a.len, a.canonical, vlo, vhi);
        b.store_u128(vlo, vhi);
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
    uint32_t blocks;
    if (values_grid(a.n_pos_max, u128, &blocks)) return -3;
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
