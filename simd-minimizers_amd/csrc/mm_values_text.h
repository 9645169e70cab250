// mm_values_text.h — one k-mer value of byte text (mm_values_text.hip; mm_debug_values_text runs the same functions on
// the host, on a host buffer): the gather of a k-mer's bytes from whole dwords, the 2-bit compression of ASCII DNA, and
// the assembly into Output::values_u64 / values_u128 (src/lib.rs:584-629) of the Seq the text stands for -
//   BYTES  `&[u8]` (src/lib.rs:59-60), 8 bits per character: value = sum text[p + j] << 8j.  PARITY UNPINNED: packed-seq
//          is not in the reference tree, the layout is inferred (first character in the low byte, as read_kmer puts the
//          first base in the low bits);
//   DNA    packed-seq AsciiSeq (src/lib.rs:59, :85-100), 2 bits per character, code = (c >> 1) & 3: bit for bit the value
//          of PackedSeqVec::from_ascii(text) at the same position (mm_values.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mm_launch.h"
#include "mm_values.h"
#include "mm_values_load.h"

namespace mm {

// Offsets a workgroup of the batch kernels stages in LDS (8 bytes each): a workgroup whose values span more records than
// this (runs of empty records) searches the offsets in global memory instead.  16 KiB per workgroup: ten workgroups fit
// the CU's 160 KiB where the 32-waves-per-CU cap admits eight, so the stage costs no occupancy at any register count.
constexpr uint32_t kValuesTextStage = 2048;

constexpr int kTextValuesBytes = 0, kTextValuesDna = 1;

// Dwords loaded per value: the whole dwords a k-mer of `chars` characters covers at the worst byte phase.
//   BYTES  u64: 8 characters -> 3, u128: 16 -> 5
//   DNA    u64: len <= 16 -> 5, len <= 32 -> 9; u128: len <= 32 -> 9, len <= 64 -> 17
constexpr int text_value_dwords(uint32_t chars) { return (int)(chars / 4u) + 1; }

// bytes [phase, phase + 4) of the eight bytes {lo, hi}
__host__ __device__ __forceinline__ uint32_t align_bytes(uint32_t hi, uint32_t lo, uint32_t phase) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, phase);
#else
    return (uint32_t)(((((unsigned long long)hi) << 32) | lo) >> (8u * (phase & 3u)));
#endif
}

// PackedSeqVec::from_ascii of the four characters of a dword: code (c >> 1) & 3 of character j at bits 2j
__host__ __device__ __forceinline__ uint32_t dna_codes_of(uint32_t x) {
    const uint32_t c = (x >> 1) & 0x03030303u;
    return (c | (c >> 6) | (c >> 12) | (c >> 18)) & 0xFFu;
}

// The 4 * (NDW - 1) characters from byte `phase` of w[0] on, as {lo, hi}: 8 bits (BYTES) or 2 bits (DNA) per character,
// first character lowest.  Nothing is masked yet.
template <int NDW, bool DNA>
__host__ __device__ __forceinline__ void text_value_bits(const uint32_t (&w)[NDW], uint32_t phase, unsigned long long &lo,
                                                         unsigned long long &hi) {
    static_assert(DNA ? NDW <= 17 : NDW <= 5, "a value holds at most 128 bits");
    lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j + 1 < NDW; ++j) {
        const uint32_t s = align_bytes(w[j + 1], w[j], phase);
        if constexpr (DNA) {
            const unsigned long long b = dna_codes_of(s);
            if (j < 8) lo |= b << (8 * j);
            else hi |= b << (8 * (j - 8));
        } else {
            if (j < 2) lo |= (unsigned long long)s << (32 * j);
            else hi |= (unsigned long long)s << (32 * (j - 2));
        }
    }
}

// The same for a k-mer whose dwords are not all inside the view, by the edge rules of mm_values_load.h (single bytes
// inside, zeros outside): one dword at a time, kept rolled and free of arrays - it runs for the few values at the
// buffer's ends, the registers are the hot path's.  p: the k-mer's first byte, counted from view.d.
template <int NDW, bool DNA>
__host__ __device__ __forceinline__ void text_value_bits_edge(const PackedView &view, unsigned long long p, unsigned long long &lo,
                                                     unsigned long long &hi) {
    const unsigned long long q = p >> 2;
    const uint32_t phase = (uint32_t)(p & 3u);
    lo = 0, hi = 0;
    uint32_t have = edge_dword(view, q);
#pragma nounroll
    for (uint32_t j = 0; j + 1u < (uint32_t)NDW; ++j) {
        const uint32_t next = edge_dword(view, q + j + 1u);
        const unsigned long long s = DNA ? dna_codes_of(align_bytes(next, have, phase)) : align_bytes(next, have, phase);
        constexpr uint32_t kPer = DNA ? 8u : 2u, kBits = DNA ? 8u : 32u;  // shifted dwords per 64-bit half, bits of each
        const bool low = j < kPer;
        const unsigned long long piece = s << (kBits * (low ? j : j - kPer));
        lo |= low ? piece : 0ull;  // (selects of values, not of which variable to update: both stay in registers)
        hi |= low ? 0ull : piece;
        have = next;
    }
}

// values_u64 from the gathered bits: BYTES len <= 8, DNA len <= 32; canonical is DNA's only
template <bool DNA>
__host__ __device__ __forceinline__ unsigned long long text_value64(unsigned long long lo, uint32_t len, int canonical) {
    const uint32_t bits = (DNA ? 2u : 8u) * len;
    const unsigned long long mask = bits >= 64 ? ~0ull : ((1ull << bits) - 1ull);
    lo &= mask;
    if (DNA && canonical) lo = canonical_value(lo, len, mask);
    return lo;
}

// values_u128 {lo, hi} from the gathered bits (BYTES len <= 16, DNA len <= 64)
template <bool DNA>
__host__ __device__ __forceinline__ void text_value128(uint32_t len, int canonical, unsigned long long &lo,
                                                       unsigned long long &hi) {
    // (a byte is four 2-bit groups: BYTES keeps 2 * (4 * len) bits and has no canonical step)
    finish_value128(DNA ? len : 4u * len, DNA ? canonical : 0, lo, hi);
}

// The text as whole dwords plus its byte range (packed_view, mm_values_reads.h): base0 = byte_lo, so character p of the
// text is byte base0 + p of d.
inline PackedView text_view(uint64_t address, uint64_t text_bytes) { return packed_view(address, text_bytes, 0, 1); }

struct ValuesTextArgs {
    PackedView view;
    unsigned long long n_records;              // batch: > 0
    const unsigned long long *starts;          // batch: [n_records + 1], record r = characters [starts[r], starts[r + 1])
    uint32_t len;
    int canonical;
    const uint32_t *pos;                       // single text: absolute positions; batch: record-local, back to back
    const unsigned long long *offsets;         // batch: [n_records + 1]; offsets[n_records] = the true count
    unsigned long long n_pos_max;              // what pos / out hold: the grid's size (single text: the count)
    unsigned long long *out;                   // u64: one word per value; u128: {lo, hi}
    // batch, or null: the true {characters, records} in device memory (mm_values_*_text_batch_counts_*); n_records and
    // max_chars are then their bounds - counts beyond them, or no record, and the kernel writes nothing
    const unsigned long long *counts = nullptr;
    unsigned long long max_chars = 0;
};
// 0, -1 (HIP failure), -3 (grid too large)
int launch_values_text(const ValuesTextArgs &a, int encoding, bool u128, bool batch, hipStream_t stream);

// One value on the host, of a host buffer: the functions above on (view, absolute position).
void values_text_host_one(const PackedView &view, int encoding, uint32_t len, int canonical, bool u128, uint64_t abs_pos,
                          uint64_t *out);

}  // namespace mm
