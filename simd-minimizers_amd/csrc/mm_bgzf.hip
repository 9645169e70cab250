// mm_bgzf.hip - BGZF (blocked gzip: bgzip, htslib) inflated on the device, and the host calls around it (mm_bgzf_*).
//
// The reference reads compressed FASTA / FASTQ through its loader on the CPU (needletail::parse_fastx_file,
// bench/src/lib.rs:51-82), one serial inflate per file.  A BGZF file is a series of independent gzip members of at most
// 64 KiB of text, each saying its compressed size in its header (BSIZE) and its text size in its trailer (ISIZE), so the
// host lays out a whole chunk's output from 26 bytes per block (mm_bgzf_scan_host) and the device inflates the blocks side
// by side.
//
// The kernel: ONE WAVEFRONT PER BLOCK (one wave per workgroup, so no barrier anywhere: waves run different trip counts).
// The decoder is mm_inflate.h, the code the host runs too; its state - bit buffer, offsets, tables - is the same in every
// lane, and what comes back from LDS goes through readfirstlane, so the symbol loop is wave-uniform.  The 64 lanes do the
// byte traffic (WaveIo below):
//   input    64 payload bytes per load, one per lane, kept in a register; the bit buffer takes its bytes with readlane
//   literal  stored by lane pos % 64
//   match    64 bytes per step; a distance below 64 is a period, so byte j comes from out[pos - dist + j % dist], which
//            the match itself never writes; a distance of 64 or more reads only what earlier steps (or symbols) wrote
//   stored   64 bytes per step
//   tables   in LDS (2 592 bytes); the first-level tables' entries are filled lane-parallel
// A wave's loads see its own earlier stores of other lanes: vector memory operations of one wavefront execute in order,
// and the wavefront-scope fences keep the compiler from reordering them.  Every global store is a per-lane store.
// CRC32 is verified on request, by a kernel of its own behind this one (mm_crc32.hip): mm_bgzf_crc32_device_async,
// mm_bgzf_inflate_verify_host, the stream's MM_FASTX_BGZF_CRC.  This kernel accepts a block by its structure and ISIZE alone.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "mm_bgzf.h"
#include "mm_crc32.h"
#include "mm_fastx_stream.h"
#include "mm_inflate.h"

namespace mm {
namespace {

struct WaveIo {
    const uint8_t *in;
    uint32_t n;
    uint8_t *out;
    uint32_t ln;
    uint32_t cache_base, cache;
    __device__ __forceinline__ uint32_t byte(uint32_t i) {
        const uint32_t base = i & ~63u;
        if (base != cache_base) {
            cache_base = base;
            cache = base + ln < n ? in[base + ln] : 0u;
        }
        return (uint32_t)__builtin_amdgcn_readlane((int)cache, (int)(i & 63u));
    }
    __device__ __forceinline__ void lit(uint32_t pos, uint32_t b) {
        if (ln == (pos & 63u)) out[pos] = (uint8_t)b;
    }
    __device__ __forceinline__ void copy(uint32_t pos, uint32_t dist, uint32_t len) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (uint32_t off = 0; off < len; off += 64u) {
            const uint32_t j = off + ln;
            if (j < len) {
                const uint32_t src = dist >= 64u ? pos + j - dist : pos - dist + (j < dist ? j : j % dist);
                out[pos + j] = out[src];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
    }
    __device__ __forceinline__ void stored(uint32_t pos, uint32_t in_off, uint32_t len) {
        for (uint32_t j = ln; j < len; j += 64u) out[pos + j] = in[in_off + j];
    }
    __device__ __forceinline__ uint32_t lane() const { return ln; }
    __device__ __forceinline__ uint32_t lanes() const { return 64u; }
    __device__ __forceinline__ void sync() {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
};

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return (uint64_t)hi << 32 | lo;
}

__global__ __launch_bounds__(64) void bgzf_inflate_kernel(const uint8_t *d_comp, uint64_t comp_bytes, const mm_bgzf_block_t *d_blocks,
                                                          uint8_t *d_out, uint64_t out_capacity, uint32_t *d_status, uint32_t *error) {
    __shared__ InflateTables s_tables;
    const uint32_t b = blockIdx.x;
    const uint64_t comp_off = uniform64(d_blocks[b].comp_off), out_off = uniform64(d_blocks[b].out_off);
    const uint32_t comp_len = MM_INFLATE_UNIFORM(d_blocks[b].comp_len), isize = MM_INFLATE_UNIFORM(d_blocks[b].isize);
    uint32_t st;
    if (comp_off > comp_bytes || comp_len > comp_bytes - comp_off || isize > kBgzfMaxIsize || out_off > out_capacity ||
        isize > out_capacity - out_off) {
        st = kInflateTable;
    } else {
        WaveIo io{d_comp + comp_off, comp_len, d_out + out_off, threadIdx.x & 63u, 0xffffffffu, 0u};
        st = (uint32_t)inflate_payload(io, &s_tables, comp_len, isize);
    }
    if (threadIdx.x == 0) {
        if (d_status) d_status[b] = st;
        // (the sticky word mm_workspace_check reads: this call has no synchronous form that reads the per-launch word; the
        // larger code stays, so a bad table entry - kernel error 10 - is what a launch with both kinds of failure reports)
        if (st) atomicMax(&error[2], st == kInflateTable ? kErrBgzfTable : kErrBgzfBlock);
    }
}

struct DeviceGuard {  // every entry restores the caller's current device
    int saved = -1;
    DeviceGuard() {
        if (hipGetDevice(&saved) != hipSuccess) {
            (void)hipGetLastError();
            saved = -1;
        }
    }
    ~DeviceGuard() {
        if (saved >= 0) (void)hipSetDevice(saved);
    }
};

int refuse(int code, const std::string &why) {
    api_set_last_error(why.c_str());
    return code;
}

}  // namespace

int launch_bgzf_inflate(const uint8_t *d_comp, uint64_t comp_bytes, const mm_bgzf_block_t *d_blocks, uint64_t n_blocks,
                        uint8_t *d_out, uint64_t out_capacity, uint32_t *d_status, uint32_t *error, hipStream_t stream) {
    if (n_blocks == 0) return 0;
    hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((uint32_t)n_blocks), dim3(64), 0, stream, d_comp, comp_bytes, d_blocks, d_out,
                       out_capacity, d_status, error);
    return hipPeekAtLastError() == hipSuccess ? 0 : -1;
}

namespace {

// the walk of mm_bgzf_scan_host and mm_bgzf_scan_crc_host (with_crcs: crcs[i] = the CRC32 of listed block i's trailer)
int scan_host(const uint8_t *data, uint64_t n_bytes, uint64_t max_blocks, uint64_t max_out_bytes, mm_bgzf_block_t *blocks,
              uint64_t *n_blocks, uint64_t *consumed, uint64_t *out_bytes, bool with_crcs, uint32_t *crcs) {
    if (n_blocks) *n_blocks = 0;
    if (consumed) *consumed = 0;
    if (out_bytes) *out_bytes = 0;
    if (!n_blocks || !consumed || !out_bytes || (!data && n_bytes) || (!blocks && max_blocks) || (with_crcs && !crcs && max_blocks))
        return MM_ERR_NULL;
    uint64_t at = 0, nb = 0, ob = 0;
    while (at < n_bytes) {
        uint64_t total = 0;
        uint32_t payload_off = 0, comp_len = 0, isize = 0;
        const int r = mm::bgzf_member(data + at, n_bytes - at, &total, &payload_off, &comp_len, &isize);
        if (r > 0) break;  // (incomplete: the caller brings more bytes)
        if (r == -2)
            return mm::refuse(MM_ERR_FORMAT, "mm_bgzf_scan_host: a gzip member without a BC subfield at byte " + std::to_string(at) +
                                                 ": plain gzip is one serial stream; recompress with bgzip");
        if (r < 0) return mm::refuse(MM_ERR_FORMAT, "mm_bgzf_scan_host: no BGZF block header at byte " + std::to_string(at));
        if (isize > mm::kBgzfMaxIsize)
            return mm::refuse(MM_ERR_FORMAT, "mm_bgzf_scan_host: ISIZE " + std::to_string(isize) + " above 65536 in the block at byte " +
                                                 std::to_string(at));
        if (isize) {
            if (nb == max_blocks || isize > max_out_bytes - ob) break;
            blocks[nb].comp_off = at + payload_off;
            blocks[nb].comp_len = comp_len;
            blocks[nb].isize = isize;
            blocks[nb].out_off = ob;
            if (with_crcs) crcs[nb] = mm::bgzf_trailer_crc(data + at, total);
            ++nb;
            ob += isize;
        }
        at += total;
    }
    *n_blocks = nb;
    *consumed = at;
    *out_bytes = ob;
    return MM_OK;
}

}  // namespace
}  // namespace mm

extern "C" {

int mm_bgzf_scan_host(const uint8_t *data, uint64_t n_bytes, uint64_t max_blocks, uint64_t max_out_bytes, mm_bgzf_block_t *blocks,
                      uint64_t *n_blocks, uint64_t *consumed, uint64_t *out_bytes) {
    return mm::scan_host(data, n_bytes, max_blocks, max_out_bytes, blocks, n_blocks, consumed, out_bytes, false, nullptr);
}

int mm_bgzf_scan_crc_host(const uint8_t *data, uint64_t n_bytes, uint64_t max_blocks, uint64_t max_out_bytes, mm_bgzf_block_t *blocks,
                          uint64_t *n_blocks, uint64_t *consumed, uint64_t *out_bytes, uint32_t *crcs) {
    return mm::scan_host(data, n_bytes, max_blocks, max_out_bytes, blocks, n_blocks, consumed, out_bytes, true, crcs);
}

int mm_debug_crc32(const uint8_t *data, uint64_t n, uint32_t *crc) {
    if (!crc || (!data && n)) return MM_ERR_NULL;
    *crc = mm::crc32_bytes(0, data, n);
    return MM_OK;
}

int mm_debug_bgzf_inflate(const uint8_t *payload, uint32_t comp_len, uint8_t *out, uint32_t isize) {
    if ((!payload && comp_len) || (!out && isize)) return MM_ERR_NULL;
    if (isize > mm::kBgzfMaxIsize) return mm::refuse(MM_ERR_FORMAT, "mm_debug_bgzf_inflate: isize above 65536");
    const int r = mm::inflate_payload_host(payload, comp_len, out, isize);
    if (r) return mm::refuse(MM_ERR_FORMAT, "mm_debug_bgzf_inflate: BGZF block: inflate error " + std::to_string(r));
    return MM_OK;
}

int mm_bgzf_inflate_device_async(mm_workspace_t *ws, const void *d_comp, uint64_t comp_bytes, const mm_bgzf_block_t *d_blocks,
                                 uint64_t n_blocks, void *d_out, uint64_t out_capacity, uint32_t *d_status) {
    if (!ws || (n_blocks && (!d_comp || !d_blocks || !d_out))) return MM_ERR_NULL;
    if (n_blocks >= (1ull << 31)) return MM_ERR_LEN_TOO_LARGE;
    if (n_blocks == 0) return MM_OK;
    mm::DeviceGuard guard;
    if (hipSetDevice(mm::api_workspace_device(ws)) != hipSuccess)
        return mm::refuse(MM_ERR_HIP, std::string("mm_bgzf_inflate_device_async: hipSetDevice: ") + hipGetErrorString(hipGetLastError()));
    mm::api_workspace_mark_async(ws);
    if (mm::launch_bgzf_inflate(static_cast<const uint8_t *>(d_comp), comp_bytes, d_blocks, n_blocks, static_cast<uint8_t *>(d_out),
                                out_capacity, d_status, mm::api_workspace_error(ws), mm::api_workspace_stream(ws)))
        return mm::refuse(MM_ERR_HIP, std::string("mm_bgzf_inflate_device_async: ") + hipGetErrorString(hipGetLastError()));
    return MM_OK;
}

int mm_bgzf_crc32_device_async(mm_workspace_t *ws, const void *d_text, uint64_t text_capacity, const mm_bgzf_block_t *d_blocks,
                               uint64_t n_blocks, const uint32_t *d_expect, uint32_t *d_crc, uint32_t *d_status) {
    if (!ws || (!d_expect && !d_crc) || (n_blocks && (!d_text || !d_blocks))) return MM_ERR_NULL;
    if (n_blocks >= (1ull << 31)) return MM_ERR_LEN_TOO_LARGE;
    if (n_blocks == 0) return MM_OK;
    mm::DeviceGuard guard;
    if (hipSetDevice(mm::api_workspace_device(ws)) != hipSuccess)
        return mm::refuse(MM_ERR_HIP, std::string("mm_bgzf_crc32_device_async: hipSetDevice: ") + hipGetErrorString(hipGetLastError()));
    mm::api_workspace_mark_async(ws);
    if (mm::launch_bgzf_crc32(static_cast<const uint8_t *>(d_text), text_capacity, d_blocks, n_blocks, d_expect, d_crc, d_status,
                              mm::api_workspace_error(ws), mm::api_workspace_stream(ws)))
        return mm::refuse(MM_ERR_HIP, std::string("mm_bgzf_crc32_device_async: ") + hipGetErrorString(hipGetLastError()));
    return MM_OK;
}

}  // extern "C"

namespace mm {
namespace {

// mm_bgzf_inflate_host, and with `verify` mm_bgzf_inflate_verify_host: the trailers' CRC32s go up with the table, the inflate
// gets a status array and the verify kernel runs behind it
int inflate_host(mm_workspace_t *ws, const uint8_t *data, uint64_t n_bytes, uint8_t *out, uint64_t out_capacity, uint64_t *out_bytes,
                 bool verify) {
    if (out_bytes) *out_bytes = 0;
    if (!ws || !out_bytes || (!data && n_bytes) || (!out && out_capacity)) return MM_ERR_NULL;
    std::vector<mm_bgzf_block_t> blocks;
    std::vector<uint32_t> crcs;
    uint64_t at = 0, total_out = 0;
    while (at < n_bytes) {
        mm_bgzf_block_t part[256];
        uint32_t part_crc[256];
        uint64_t nb = 0, used = 0, ob = 0;
        const int r = scan_host(data + at, n_bytes - at, 256, ~0ull, part, &nb, &used, &ob, verify, part_crc);
        if (r) return r;
        if (used == 0)
            return mm::refuse(MM_ERR_FORMAT, "mm_bgzf_inflate_host: the last BGZF block is incomplete (a truncated file), at byte " +
                                                 std::to_string(at));
        for (uint64_t i = 0; i < nb; ++i) {
            part[i].comp_off += at;
            part[i].out_off += total_out;
            blocks.push_back(part[i]);
            if (verify) crcs.push_back(part_crc[i]);
        }
        at += used;
        total_out += ob;
    }
    *out_bytes = total_out;
    if (total_out > out_capacity) return MM_ERR_CAPACITY;
    if (blocks.empty()) return MM_OK;
    mm::DeviceGuard guard;
    hipStream_t stream = mm::api_workspace_stream(ws);
    uint8_t *d_comp = nullptr, *d_out = nullptr;
    mm_bgzf_block_t *d_blocks = nullptr;
    uint32_t *d_expect = nullptr, *d_status = nullptr;
    const uint64_t table_bytes = blocks.size() * sizeof(mm_bgzf_block_t), words_bytes = blocks.size() * sizeof(uint32_t);
    hipError_t e = hipSetDevice(mm::api_workspace_device(ws));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_comp), n_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_out), total_out);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_blocks), table_bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(d_comp, data, n_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_blocks, blocks.data(), table_bytes, hipMemcpyHostToDevice, stream);
    if (verify) {
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_expect), words_bytes);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_status), words_bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(d_expect, crcs.data(), words_bytes, hipMemcpyHostToDevice, stream);
    }
    int rc = MM_OK;
    if (e == hipSuccess) {
        // (the copies read pageable memory: they are done when the calls return, and the stream is waited for below)
        // (the inflate writes every block's status word, so the array needs no clearing)
        rc = mm_bgzf_inflate_device_async(ws, d_comp, n_bytes, d_blocks, blocks.size(), d_out, total_out, d_status);
        if (rc == MM_OK && verify) rc = mm_bgzf_crc32_device_async(ws, d_out, total_out, d_blocks, blocks.size(), d_expect, nullptr, d_status);
        if (rc == MM_OK) e = hipMemcpyAsync(out, d_out, total_out, hipMemcpyDeviceToHost, stream);
    }
    const hipError_t es = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = es;
    if (d_comp) (void)hipFree(d_comp);
    if (d_out) (void)hipFree(d_out);
    if (d_blocks) (void)hipFree(d_blocks);
    if (d_expect) (void)hipFree(d_expect);
    if (d_status) (void)hipFree(d_status);
    if (rc) return rc;
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return mm::refuse(e == hipErrorOutOfMemory ? MM_ERR_ALLOC : MM_ERR_HIP, std::string("mm_bgzf_inflate_host: ") + hipGetErrorString(e));
    }
    return mm_workspace_check(ws);
}

}  // namespace
}  // namespace mm

extern "C" {

int mm_bgzf_inflate_host(mm_workspace_t *ws, const uint8_t *data, uint64_t n_bytes, uint8_t *out, uint64_t out_capacity,
                         uint64_t *out_bytes) {
    return mm::inflate_host(ws, data, n_bytes, out, out_capacity, out_bytes, false);
}

int mm_bgzf_inflate_verify_host(mm_workspace_t *ws, const uint8_t *data, uint64_t n_bytes, uint8_t *out, uint64_t out_capacity,
                                uint64_t *out_bytes) {
    return mm::inflate_host(ws, data, n_bytes, out, out_capacity, out_bytes, true);
}

}  // extern "C"
