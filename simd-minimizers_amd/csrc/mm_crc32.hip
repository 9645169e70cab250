// mm_crc32.hip - the CRC32 of every BGZF block's text, on the device, over the text the inflate kernel (mm_bgzf.hip) has
// just written: mm_bgzf_crc32_device_async and the stream's MM_FASTX_BGZF_CRC.  The arithmetic is mm_crc32.h, the code the
// host runs too.
//
// The reference's loader checks every gzip member's CRC32 on the CPU, inside its decompressor (needletail::parse_fastx_file,
// bench/src/lib.rs:51-82).  Here the check is a kernel of its own behind the inflate, not a tail phase of it: the inflate's
// rate hangs on its residency, which LDS for CRC tables would cost, and the two have nothing in common - the inflate is one
// serial symbol loop per block, this is a parallel pass over bytes.
//
// ONE WORKGROUP OF 256 THREADS PER BLOCK.  The slicing-by-4 tables (4 KiB) are made in LDS by the threads themselves, entry
// by definition (crc32_table_entry: no table in global memory, nothing to upload).  The block is cut by crc32_plan: a thread
// takes one contiguous segment of S bytes (a multiple of 16, counted from the 16-byte boundary at or in front of the block's
// first byte), runs it through the tables with 16-byte global loads - byte-wise up to the first boundary in thread 0, and
// byte-wise over the last segment's end - and the segments' registers are combined in log2 steps in LDS, in the order
// u = T - 2 - t so that every pair of a level takes the same multiplier, x^(8 S) squared per level; the short last segment's
// x^(8 r) is applied once at the end (mm_crc32.h has the algebra).  No byte outside [out_off, out_off + isize) is loaded.
// Table entries are checked on the device, as the inflate checks them.
#include <hip/hip_runtime.h>

#include "mm_bgzf.h"
#include "mm_crc32.h"
#include "mm_inflate.h"

namespace mm {
namespace {

__global__ __launch_bounds__(256) void bgzf_crc32_kernel(const uint8_t *d_text, uint64_t capacity, const mm_bgzf_block_t *d_blocks,
                                                         const uint32_t *d_expect, uint32_t *d_crc, uint32_t *d_status, uint32_t *error) {
    __shared__ uint32_t s_table[1024];
    __shared__ uint32_t s_red[kCrc32Threads];
    __shared__ uint32_t s_last;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    // (a block the inflate in front of this launch has failed keeps its code: it is not looked at)
    if (d_expect && d_status && d_status[b] != 0) return;
    const uint64_t out_off = d_blocks[b].out_off;
    const uint32_t isize = d_blocks[b].isize;
    if (out_off > capacity || isize > capacity - out_off || isize > kBgzfMaxIsize) {
        if (tid == 0) {
            if (d_status) d_status[b] = kInflateTable;
            atomicMax(&error[2], kErrBgzfTable);
        }
        return;
    }
    for (uint32_t k = 0; k < 4; ++k) s_table[256 * k + tid] = crc32_table_entry(k, tid);
    const uint8_t *const base = d_text + out_off;
    const uint32_t lo = (uint32_t)(reinterpret_cast<uintptr_t>(base) & 15u), hi = lo + isize;
    const uint8_t *const aligned = base - lo;  // (never dereferenced below `lo`)
    const Crc32Plan plan = crc32_plan(lo, isize);
    __syncthreads();
    uint32_t c = tid == 0 ? 0xFFFFFFFFu : 0u;
    if (tid < plan.T) {
        uint32_t p = tid ? tid * plan.S : lo;
        const uint32_t end = tid + 1 == plan.T ? hi : (tid + 1) * plan.S;
        for (; p < end && (p & 15u); ++p) c = crc32_step_byte(s_table, c, aligned[p]);
        for (; p + 16 <= end; p += 16) {
            const uint4 v = *reinterpret_cast<const uint4 *>(aligned + p);
            c = crc32_step_word(s_table, c, v.x);
            c = crc32_step_word(s_table, c, v.y);
            c = crc32_step_word(s_table, c, v.z);
            c = crc32_step_word(s_table, c, v.w);
        }
        for (; p < end; ++p) c = crc32_step_byte(s_table, c, aligned[p]);
    }
    // the combine: slot u = T - 2 - t holds segment t, the slots behind them zeros, the last segment stands aside
    if (tid + 2 <= plan.T) s_red[plan.T - 2 - tid] = c;
    else s_red[tid] = 0;  // (tid >= T - 1: a slot no segment fills)
    if (tid + 1 == plan.T) s_last = c;
    __syncthreads();
    uint32_t m = crc32_xpow8(plan.S);
    for (uint32_t stride = 1; stride + 1 < plan.T; stride <<= 1) {
        // (a thread writes its own slot only and reads one that no thread writes at this level)
        if ((tid & (2 * stride - 1)) == 0 && tid + stride < kCrc32Threads) s_red[tid] ^= crc32_mulmod(s_red[tid + stride], m);
        m = crc32_mulmod(m, m);
        __syncthreads();
    }
    if (tid == 0) {
        uint32_t crc = 0;
        if (plan.T) crc = ~(plan.T > 1 ? crc32_mulmod(s_red[0], crc32_xpow8(plan.r)) ^ s_last : s_last);
        if (d_crc) d_crc[b] = crc;
        if (d_expect && crc != d_expect[b]) {
            if (d_status) d_status[b] = kCrc32Mismatch;
            // (the sticky word mm_workspace_check reads; the larger code stays, so a launch with a mismatch and a bad table
            // entry reports the mismatch)
            atomicMax(&error[2], kErrBgzfCrc);
        }
    }
}

}  // namespace

int launch_bgzf_crc32(const uint8_t *d_text, uint64_t capacity, const mm_bgzf_block_t *d_blocks, uint64_t n_blocks,
                      const uint32_t *d_expect, uint32_t *d_crc, uint32_t *d_status, uint32_t *error, hipStream_t stream) {
    if (n_blocks == 0) return 0;
    hipLaunchKernelGGL(bgzf_crc32_kernel, dim3((uint32_t)n_blocks), dim3(kCrc32Threads), 0, stream, d_text, capacity, d_blocks,
                       d_expect, d_crc, d_status, error);
    return hipPeekAtLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mm
