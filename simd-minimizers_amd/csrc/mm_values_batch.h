// mm_values_batch.h — what the host and the kernel of mm_values_batch.hip share: the per-sequence descriptor of a batch's
// separately allocated sequences, how it is derived from {device address, packed_bytes, base_offset}, and the size of the
// LDS stage.  Plain C++ up to the launch declaration: mm_debug_values_batch_view runs the derivation with no device.
#pragma once
#include <stdint.h>

#include "mm_values_reads.h"  // MM_HOST_DEVICE, values_read_of, PackedView

namespace mm {

// One sequence of the batch as the kernel addresses it (32 bytes, 16-byte aligned in the device table and in LDS): `d` is the
// sequence's device address rounded down to a dword, bytes [byte_lo, byte_hi) of `d` are the sequence's own, base0 =
// base_offset + 4 * byte_lo is the base of `d` at which the sequence's first base lies.  A sequence without values is all zeros:
// an empty byte range, so that even a stray look-up would load nothing.
struct ValuesBatchSeq {
    unsigned long long d;
    unsigned long long byte_lo, byte_hi;
    unsigned long long base0;
};

MM_HOST_DEVICE inline ValuesBatchSeq values_batch_seq(uint64_t address, uint64_t packed_bytes, uint64_t base_offset) {
    const PackedView v = packed_view(address, packed_bytes, base_offset, 4);
    return ValuesBatchSeq{(unsigned long long)reinterpret_cast<uintptr_t>(v.d), v.byte_lo, v.byte_hi, v.base0};
}
// the view again, as the kernel reads it out of a descriptor: the whole dwords are derived from the byte range
MM_HOST_DEVICE inline PackedView view_of(const ValuesBatchSeq &s) {
    PackedView v;
    v.d = reinterpret_cast<const uint32_t *>(s.d);
    v.byte_lo = s.byte_lo;
    v.byte_hi = s.byte_hi;
    v.base0 = s.base0;
    view_whole_dwords(v);
    return v;
}

// Entries of the LDS stage: an offset (8 bytes) and a descriptor (32 bytes) each, 20 KiB in all.  The kernels are
// register-bound at 8 workgroups of 256 threads per CU (the 32-wave cap); 8 x 20 KiB is exactly the CU's 160 KiB, so the
// stage is the largest that costs no occupancy.  A workgroup whose values span more sequences searches global memory.
constexpr uint32_t kValuesBatchStage = 512;

struct ValuesBatchArgs {
    unsigned long long n_seqs;                 // > 0
    const ValuesBatchSeq *seqs;                // device, [n_seqs]
    const unsigned long long *offsets;         // device, [n_seqs + 1], non-decreasing (the host checked them)
    unsigned long long total;                  // = offsets[n_seqs] > 0
    uint32_t len;
    int canonical;
    const uint32_t *pos;                       // sequence-local positions, back to back
    unsigned long long *out;                   // u64: one word per value; u128: {lo, hi}
};

}  // namespace mm

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace mm {
int launch_values_batch(const ValuesBatchArgs &a, bool u128, hipStream_t stream);  // 0, -1 (HIP failure), -3 (grid too large)
}
#endif
