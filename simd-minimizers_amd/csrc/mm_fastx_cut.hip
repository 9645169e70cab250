// mm_fastx_cut.hip - the trim step of the FASTA / FASTQ stream (mm_fastx_stream.hip): behind a packer, on its stream,
// apply the cut rule of mm_fastx_cut.h to what the packer left and rewrite its counts in place, so that the counts run
// (mm_run_packed_reads_counts_device_async) sees only the records that lie whole inside the chunk.  The reference has no
// counterpart: its loader reads any file record by record on the host (bench/src/lib.rs:51-82).
//
// Two kernels.  fastx_newlines_kernel counts the chunk's newlines (a count of its own: one coalesced pass over the text,
// 32 bytes per thread as the packers read it - the FASTQ packer's resolve step holds the same number, but taking it from
// there would put an output into a kernel whose results this step must not touch).  fastx_trim_kernel, ONE workgroup:
// the newline the cut lies behind is among the last four of the chunk, so it is found by a scan from the END of the text,
// 8 KB per step (16-byte loads, 32-bit newline masks, a workgroup vote skips steps without a newline); thread 0 then
// calls the rule and stores d_counts = {B', R'}, d_cut = {cut, overflow, T, open, overlap}.  With MM_FASTX_LONG_RECORDS a
// chunk that is one open record is also scanned for T, the start of the l - 1 sequence bytes the next chunk repeats (the
// split rule of mm_fastx_cut.h), and fastx_bias_kernel makes a continuing record's positions record-global.
#include <hip/hip_runtime.h>

#include "mm_fastx_cut.h"
#include "mm_fastx_stream.h"
#include "mm_text.h"

namespace mm {
namespace {

// the '\n' bytes among the thread's 32 bytes of the 8 KB piece that starts at byte c0 (bit i = byte i), inside the text only:
// load32 reads whole dwords, so the text's last dword may bring bytes from behind it
__device__ __forceinline__ uint32_t newline_mask(const uint8_t *text, uint64_t n, uint64_t c0, uint32_t t) {
    const uint64_t first = c0 + (uint64_t)t * kFqBytesPerThread;
    if (first >= n) return 0u;
    const uint64_t nin = n - first;
    const uint32_t inside = nin >= 32u ? 0xffffffffu : ((1u << (uint32_t)nin) - 1u);
    return eq32(load32(text, n, c0, t), 0x0a0a0a0au) & inside;
}

__global__ __launch_bounds__(kFqThreads) void fastx_newlines_kernel(const uint8_t *__restrict__ text, uint64_t n,
                                                                   unsigned long long *__restrict__ d_newlines) {
    const uint64_t c0 = (uint64_t)blockIdx.x * kFqChunk;
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t p = 0; p < kFqPieces; ++p) {
        cnt += (uint32_t)__builtin_popcount(newline_mask(text, n, c0 + (uint64_t)p * kFqPiece, threadIdx.x));
    }
    // (one atomic per workgroup: a word takes about 90 of them per microsecond)
    __shared__ uint32_t s_part[kFqWaves];
    for (int d = kWave / 2; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) s_part[threadIdx.x / kWave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (int i = 0; i < kFqWaves; ++i) sum += s_part[i];
        if (sum) atomicAdd(d_newlines, (unsigned long long)sum);
    }
}

__global__ __launch_bounds__(kFqThreads) void fastx_trim_kernel(const uint8_t *__restrict__ text, uint64_t n, int format,
                                                               int last, const unsigned long long *__restrict__ d_newlines,
                                                               const unsigned long long *__restrict__ d_rec_base,
                                                               const unsigned long long *__restrict__ d_rec_text_pos,
                                                               uint64_t max_records, int long_records, uint32_t l,
                                                               unsigned long long *d_counts, unsigned long long *d_cut) {
    __shared__ uint32_t s_mask[kFqThreads];
    __shared__ uint32_t s_seq_mask[kFqThreads];
    __shared__ uint64_t s_T, s_nl_seen;
    __shared__ uint32_t s_seq, s_done;  // s_done: 1 the (l - 1)-th sequence byte was met, 2 the header line's newline
    __shared__ uint64_t s_found_pos;
    __shared__ uint32_t s_left;  // newlines still to pass, the one looked for included (0: found)
    const uint64_t n_newlines = d_newlines[0];
    const uint64_t n_bases = d_counts[0], n_records = d_counts[1];
    const uint32_t which = fastx_cut_newline(format, last, n_newlines, n_records);
    if (threadIdx.x == 0) {
        s_left = which;
        s_found_pos = 0;
    }
    __syncthreads();
    if (which) {
        // (which <= n_newlines: the scan meets its newline before it runs out of text)
        for (uint64_t piece = (n + kFqPiece - 1) / kFqPiece; piece-- > 0;) {
            const uint64_t c0 = piece * kFqPiece;
            const uint32_t m = newline_mask(text, n, c0, threadIdx.x);
            if (!__syncthreads_or(m != 0)) continue;
            s_mask[threadIdx.x] = m;
            __syncthreads();
            if (threadIdx.x == 0) {
                uint32_t left = s_left;
                for (int t = (int)kFqThreads - 1; t >= 0 && left; --t) {
                    uint32_t mt = s_mask[t];
                    const uint32_t c = (uint32_t)__builtin_popcount(mt);
                    if (c < left) {
                        left -= c;
                        continue;
                    }
                    for (; left > 1; --left) mt &= ~(0x80000000u >> __builtin_clz(mt));  // drop the highest set bit
                    s_found_pos = c0 + (uint64_t)t * kFqBytesPerThread + (31u - (uint32_t)__builtin_clz(mt));
                    left = 0;
                }
                s_left = left;
            }
            __syncthreads();
            if (s_left == 0) break;
        }
    }
    // The split scan (MM_FASTX_LONG_RECORDS; a chunk that is one open record): sequence bytes counted from the END of the
    // text, the same 8 KB steps, until the (l - 1)-th one or the text's FIRST newline (the end of the header line).
    const bool in_table = n_records && n_records <= max_records && d_rec_text_pos;
    const uint64_t first_pos = in_table ? d_rec_text_pos[0] : 0;
    const bool open = fastx_split_open(format, last, long_records, n_newlines, n_records, max_records, first_pos);  // (uniform)
    const uint32_t want = l ? l - 1 : 0;
    if (open) {
        if (threadIdx.x == 0) {
            s_T = n;
            s_nl_seen = 0;
            s_seq = 0;
            s_done = want == 0 ? 1u : 0u;
        }
        __syncthreads();
        for (uint64_t piece = (n + kFqPiece - 1) / kFqPiece; piece-- > 0 && s_done == 0;) {
            const uint64_t c0 = piece * kFqPiece;
            const uint64_t first = c0 + (uint64_t)threadIdx.x * kFqBytesPerThread;
            uint32_t nlm = 0, seqm = 0;
            if (first < n) {
                const uint64_t nin = n - first;
                const uint32_t inside = nin >= 32u ? 0xffffffffu : ((1u << (uint32_t)nin) - 1u);
                const Text32 v = load32(text, n, c0, threadIdx.x);
                nlm = eq32(v, 0x0a0a0a0au) & inside;
                seqm = inside & ~(nlm | eq32(v, 0x0d0d0d0du));
            }
            s_mask[threadIdx.x] = nlm;
            s_seq_mask[threadIdx.x] = seqm;
            __syncthreads();
            if (threadIdx.x == 0) {
                uint64_t T = s_T, seen = s_nl_seen;
                uint32_t seq = s_seq, done = 0;
                for (int t = (int)kFqThreads - 1; t >= 0 && !done; --t) {
                    const uint32_t nl = s_mask[t], sq = s_seq_mask[t];
                    if ((nl | sq) == 0u) continue;
                    const uint64_t base = c0 + (uint64_t)t * kFqBytesPerThread;
                    const uint32_t cs = (uint32_t)__builtin_popcount(sq), cn = (uint32_t)__builtin_popcount(nl);
                    if (seq + cs < want && seen + cn < n_newlines) {  // neither end lies in these 32 bytes
                        seq += cs;
                        seen += cn;
                        if (cs) T = base + (uint32_t)__builtin_ctz(sq);
                        continue;
                    }
                    for (int b = 31; b >= 0 && !done; --b) {
                        if ((nl >> b) & 1u) {
                            if (++seen == n_newlines) {
                                T = base + (uint32_t)b + 1u;
                                done = 2;
                            }
                        } else if ((sq >> b) & 1u) {
                            T = base + (uint32_t)b;
                            if (++seq == want) done = 1;
                        }
                    }
                }
                s_T = T;
                s_nl_seen = seen;
                s_seq = seq;
                s_done = done;
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        const uint64_t last_pos = in_table ? d_rec_text_pos[n_records - 1] : 0;
        uint64_t T = 0;
        if (open) {
            T = s_T;
            // (the header line was met first: forward over line ends to the piece's first sequence byte)
            if (s_done == 2)
                while (T < n && fastx_is_line_end(text[T])) ++T;
        }
        const FastxSplit sp = fastx_split_rule(format, last, long_records, n, n_newlines, s_found_pos, n_bases, n_records, max_records,
                                               first_pos, last_pos, reinterpret_cast<const uint64_t *>(d_rec_base), T, open ? s_seq : 0u);
        d_counts[0] = sp.c.bases;
        d_counts[1] = sp.c.records;
        d_cut[0] = sp.c.cut;
        d_cut[1] = sp.c.overflow;
        d_cut[2] = sp.T;
        d_cut[3] = sp.open;
        d_cut[4] = sp.overlap;
    }
}

// The seam epilogue's device part: record 0 of a chunk that continues an open record gets record-global positions (and
// window indices), pos + bias, 16 bytes per thread and step.  The record's slice is [0, offsets[1]) - read from the
// device, clamped to the buffer; a chunk whose counts are out of their bounds (the host refuses it) is left alone.
__global__ __launch_bounds__(256) void fastx_bias_kernel(const unsigned long long *__restrict__ d_counts,
                                                         const unsigned long long *__restrict__ d_offsets, uint64_t max_records,
                                                         uint64_t max_positions, uint32_t bias, uint32_t *__restrict__ d_pos,
                                                         uint32_t *__restrict__ d_sk) {
    const uint64_t n_records = d_counts[1];
    if (n_records == 0 || n_records > max_records) return;
    uint64_t n0 = d_offsets[1];
    if (n0 > max_positions) n0 = max_positions;
    const uint64_t quads = n0 / 4, stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    u32x4 *const pos4 = reinterpret_cast<u32x4 *>(d_pos), *const sk4 = reinterpret_cast<u32x4 *>(d_sk);
    for (uint64_t q = me; q < quads; q += stride) {
        pos4[q] = pos4[q] + bias;
        if (d_sk) sk4[q] = sk4[q] + bias;
    }
    const uint64_t j = quads * 4 + me;
    if (j < n0) {
        d_pos[j] += bias;
        if (d_sk) d_sk[j] += bias;
    }
}

}  // namespace

int launch_fastx_bias(const unsigned long long *d_counts, const unsigned long long *d_offsets, uint64_t max_records,
                      uint64_t max_positions, uint32_t bias, uint32_t *d_pos, uint32_t *d_sk, hipStream_t stream) {
    // (a chunk of 64 MiB of genome text gives about 12 M positions: 1024 workgroups take three steps each)
    uint64_t groups = (max_positions / 4 + 255) / 256;
    groups = groups < 1 ? 1 : (groups > 1024 ? 1024 : groups);
    hipLaunchKernelGGL(fastx_bias_kernel, dim3((unsigned)groups), dim3(256), 0, stream, d_counts, d_offsets, max_records, max_positions,
                       bias, d_pos, d_sk);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_fastx_trim(const uint8_t *d_text, uint64_t n_bytes, int format, int last, int long_records, uint32_t l,
                      const unsigned long long *d_rec_base, const unsigned long long *d_rec_text_pos, uint64_t max_records,
                      unsigned long long *d_counts, unsigned long long *d_cut, unsigned long long *d_newlines, hipStream_t stream) {
    if (n_bytes >= (1ull << 32)) return -1;
    if (hipMemsetAsync(d_newlines, 0, sizeof(unsigned long long), stream) != hipSuccess) return -1;
    const uint64_t chunks = (n_bytes + kFqChunk - 1) / kFqChunk;
    if (chunks && !last)
        hipLaunchKernelGGL(fastx_newlines_kernel, dim3((unsigned)chunks), dim3(kFqThreads), 0, stream, d_text, n_bytes, d_newlines);
    hipLaunchKernelGGL(fastx_trim_kernel, dim3(1), dim3(kFqThreads), 0, stream, d_text, n_bytes, format, last, d_newlines,
                       d_rec_base, d_rec_text_pos, max_records, long_records, l, d_counts, d_cut);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mm
