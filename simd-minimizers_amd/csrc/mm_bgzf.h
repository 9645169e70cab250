// mm_bgzf.h - what the BGZF inflate (mm_bgzf.hip) offers the FASTA / FASTQ stream (mm_fastx_stream.hip) and asks of the
// host file that owns workspaces (mm_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simd_minimizers_amd.h"

namespace mm {

constexpr uint32_t kErrBgzfBlock = 9;   // kernel error 9: a BGZF block did not inflate (mm_workspace_check: MM_ERR_FORMAT)
constexpr uint32_t kErrBgzfTable = 10;  // kernel error 10: a block-table entry beyond the buffers (MM_ERR_CAPACITY)

// One wavefront per block of d_blocks[0 .. n_blocks) on `stream`: payload d_comp + comp_off inflated to d_out + out_off.
// An entry beyond comp_bytes / out_capacity (or with isize above 65536) is refused on the device, nothing of it is read
// or written.  d_status (or null) receives one word per block, 0 or the error (mm_inflate.h); `error`: the workspace's
// error words.  Returns 0, or -1 when the launch failed.
int launch_bgzf_inflate(const uint8_t *d_comp, uint64_t comp_bytes, const mm_bgzf_block_t *d_blocks, uint64_t n_blocks,
                        uint8_t *d_out, uint64_t out_capacity, uint32_t *d_status, uint32_t *error, hipStream_t stream);

// kernel error 11: a block's text does not have the CRC32 of its gzip trailer (MM_ERR_FORMAT, "CRC32").  The sticky word
// keeps the LARGEST code, so a queue with a mismatch and a bad table entry, or a block that did not inflate, reports the mismatch.
constexpr uint32_t kErrBgzfCrc = 11;
constexpr uint32_t kCrc32Mismatch = 15;  // d_status of such a block (behind the inflate's own codes 1..14, mm_inflate.h)

// The CRC32 of every block's text (mm_crc32.hip): one workgroup of 256 threads per block of d_blocks[0 .. n_blocks) on
// `stream`, over d_text + out_off [isize]; comp_off and comp_len are not read.  d_crc (or null) receives every block's CRC32.
// With d_expect (or null) a block whose CRC32 differs gets d_status[b] = 15 and raises kernel error 11, and a block whose
// d_status[b] is not 0 when the kernel comes to it is skipped (the inflate in front has failed it).  An entry beyond
// `capacity` (or with isize above 65536): nothing is read, d_status[b] = 100, kernel error 10.  d_status may be null.
// Returns 0, or -1 when the launch failed.
int launch_bgzf_crc32(const uint8_t *d_text, uint64_t capacity, const mm_bgzf_block_t *d_blocks, uint64_t n_blocks,
                      const uint32_t *d_expect, uint32_t *d_crc, uint32_t *d_status, uint32_t *error, hipStream_t stream);

// ---- from mm_api.hip
uint32_t *api_workspace_error(mm_workspace_t *ws);  // the error words of OutParams::error
int api_workspace_device(mm_workspace_t *ws);
void api_workspace_mark_async(mm_workspace_t *ws);  // an asynchronous call was queued: mm_workspace_check has news to read

}  // namespace mm
