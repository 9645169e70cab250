// mm_text_walk_impl.h - the fused kernel of general byte text (mm_text_hasher_t).
//
// One workgroup = one tile of kTextTile consecutive windows (tiles taken from an atomic ticket, so the decoupled look-back
// only ever waits for tiles that have started), in ONE kernel:
//   1. stage: the tile's text (kTextTile + w + k - 1 bytes, from the byte before its first window) into LDS with 16-byte
//      raw-buffer loads (past the end of the text: zeros through the descriptor), the two rolling tables beside it;
//   2. hash: every thread rolls an odd-length run of k-mers (warm-up of k characters, then one t_in and one t_out look-up per
//      character) and stores key = (hash & 0xffff0000) | tile-local position - the reference's key (src/sliding_min.rs:
//      104-127); positions stay below 2^16 inside a tile, so min(key) IS the leftmost argmin and max(key ^ 0xffff0000) the
//      rightmost one (src/sliding_min.rs:196-197);
//   3. window minima: window u of the tile takes the minimum over keys u .. u+w-1; threads take windows round robin, so a
//      wave reads consecutive keys (no bank conflicts); the selected offsets (left | right << 8, w <= 128) go to LDS;
//   4. collect: every thread walks kTextPerThread consecutive windows with the lazy strand vote (2 #{c & 2} > l counted
//      over the window's bytes, one byte in and one out per window; src/canonical.rs:26-28), the dedup against the
//      previous window / the syncmer predicate (src/collect.rs:15-76, src/syncmers.rs:19-48), a block scan, the look-back
//      across tiles (lookback_exclusive) and the stores in window order.
// The first window of a tile dedups against the window in front of it (the tile computes one extra window), which is also
// the seam rule of a window range.
//
// BATCH (mm_run_text_batch_*): the text is n_records records [starts[r], starts[r+1]) back to back, each run as if alone.
// Stages 1-3 run straight across record boundaries (the rot-xor roll is exact, every k-mer of a valid window lies inside
// its record); only the collect stage knows the records: window g of record r is valid iff g + l <= starts[r+1], the
// first window of a record has no previous window, and positions / indices are record-local.  The tile's record starts
// come from text_batch_tiles_kernel (one binary search per tile) and are staged into LDS as 16-bit tile-local offsets
// (up to kTextBnd of them; a tile with more reads them from global memory instead); every thread finds its first
// window's record by a search in that list and steps forward.  The thread whose windows hold g == starts[r] writes
// offsets[r]; the grid spans windows 0 .. n_chars, so records that start in the last l - 1 bytes get theirs too.
//
// BATCH with p.counts (mm_run_text_batch_counts_*): the two counts are device words that an earlier call on the stream
// writes (mm_fasta_text_device_async), p.n and p.n_records are only their upper bounds and the grid is sized from them.
// Every workgroup reads the counts right behind its ticket (text_counts_view, mm_text_counts.h): a ticket at or past the
// real tile count leaves before it touches anything, "the last tile" is the last REAL tile, and counts beyond the bounds
// are refused by the workgroup that holds ticket 0 (count 0, offsets[0] = 0, error word 6).
#pragma once
#include "mm_common.h"
#include "mm_text_counts.h"

namespace mm {

constexpr uint32_t kTextThreads = 256;
constexpr uint32_t kTextPerThread = 32;                           // windows per thread in the collect stage
constexpr uint32_t kTextTile = kTextThreads * kTextPerThread;     // 8192 windows per workgroup
constexpr uint32_t kTextMaxW = 128;                               // (left | right << 8 offsets; key array size)
constexpr uint32_t kTextMaxK = 1024;                              // (LDS text buffer)
constexpr uint32_t kTextKeys = kTextTile + 1 + kTextMaxW;         // k-mers of a tile, with the window in front
constexpr uint32_t kTextHashRun = (kTextKeys + kTextThreads - 1) / kTextThreads;  // 33: odd, conflict-free key stores
// (the hash stage's runs read up to kTextHashRun * kTextThreads + k bytes: those past the tile's span feed k-mers that no
// window uses)
constexpr uint32_t kTextBytes = (kTextHashRun * kTextThreads + kTextMaxK + 32 + 15) & ~15u;
constexpr uint32_t kTextSelStride = kTextPerThread / 2 + 1;       // dwords per thread's 32 offsets (+1: no conflicts)
static_assert(kTextHashRun % 2 == 1, "odd runs keep the key stores of a wave on distinct banks");
static_assert(kTextThreads == 256, "one table entry per thread");
static_assert(kTextTile == kTextCountsTile, "text_counts_view counts tiles of kTextTile windows");
constexpr uint32_t kTextBnd = 2048;                               // BATCH: record starts of a tile held in LDS (4 KB)
static_assert(kTextTile + 1 + kTextMaxW + kTextMaxK < 0xffffu, "tile-local byte offsets fit 16 bits");

struct TextWalkParams {
    const uint8_t *text;       // caller's pointer (any alignment)
    uint64_t n;                // characters
    const uint2 *tables;       // device: t_in[256] then t_out[256] (TextTables)
    uint32_t fw0, rc0, rot;
    uint32_t k, w;             // (w: runtime value, also for the instances with a fixed W)
    uint64_t win_begin, win_end;
    OutParams out;
    // BATCH: records [starts[r], starts[r+1]), r < n_records; tile_rec[2 t], [2 t + 1]: the first index of starts past
    // tile t's front window, and the first past the last byte its windows reach (text_batch_tiles_kernel)
    const uint64_t *starts;
    uint64_t n_records;
    const unsigned long long *tile_rec;
    unsigned long long *offsets;  // [n_records + 1]
    // BATCH, or null: {characters, records} in device memory, read when the kernel runs; n and n_records are then their
    // upper bounds and win_end is not looked at
    const uint64_t *counts;
};

// One thread per tile of a BATCH launch: the range of record starts that tile t's collect stage needs (upper bounds of
// its front window t * kTextTile - 1 and of the last byte it reaches, in starts[0 .. n_records]).  Records in any order
// give some range inside [0, n_records + 1]: the walk never indexes outside it.
// counts (or null): the batch's true {characters, records}; n_chars and n_records are then their bounds, tiles the launched
// tiles, and only the real tiles get their range (a refused or record-less batch has none: the walk reads no range then).
__global__ __launch_bounds__(256) void text_batch_tiles_kernel(const uint64_t *starts, uint64_t n_records, uint32_t l,
                                                               uint64_t tiles, unsigned long long *tile_rec,
                                                               const uint64_t *counts, uint64_t n_chars) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (counts) {
        const TextCountsView v = text_counts_view(l, n_chars, n_records, counts[0], counts[1]);
        if (!v.walk) return;
        if (v.tiles < tiles) tiles = v.tiles;
        n_records = v.n_records;
    }
    if (t >= tiles) return;
    auto upper = [&](long long x) -> uint64_t {  // first i in [0, n_records + 1) with starts[i] > x
        uint64_t lo = 0, hi = n_records + 1;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if ((long long)starts[mid] <= x) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    };
    const long long front = (long long)(t * kTextTile) - 1;
    const uint64_t b = t == 0 ? 0 : upper(front);
    const uint64_t e = upper(front + kTextTile + l);
    tile_rec[2 * t] = b;
    tile_rec[2 * t + 1] = e > b ? e : b;
}

typedef uint32_t u32x4t __attribute__((ext_vector_type(4)));

template <int W, bool CANON, bool HASH_RC, int MODE, bool BATCH>
__global__ __launch_bounds__(kTextThreads) void text_walk_kernel(TextWalkParams p) {
    __shared__ uint2 s_in[256], s_out[256];
    __shared__ __attribute__((aligned(16))) uint8_t s_text[kTextBytes];
    __shared__ uint32_t s_key[kTextHashRun * kTextThreads];
    __shared__ uint32_t s_sel[kTextSelStride * kTextThreads];
    __shared__ uint32_t s_bid;
    __shared__ uint32_t s_wave_tot[kTextThreads / kWave];
    __shared__ unsigned long long s_excl;
    __shared__ uint16_t s_bnd[BATCH ? kTextBnd : 1];  // BATCH: the tile's record starts, tile-local (see bnd below)
    __shared__ uint32_t s_rs0;                         // BATCH: the start of the record in front of the list

    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t w = W > 0 ? (uint32_t)W : p.w;
    const uint32_t k = p.k;
    if (tid == 0) s_bid = atomicAdd(p.out.ticket, 1u);
    // the batch's size: kernel arguments, or (BATCH with p.counts) the device's own counts within those bounds
    uint64_t n = p.n, n_records = p.n_records, win_end = p.win_end;
    uint32_t last_bid = gridDim.x - 1;
    if constexpr (BATCH) {
        if (p.counts) {
            __syncthreads();
            const uint32_t b = s_bid;
            const TextCountsView v = text_counts_view(k + w - 1, p.n, p.n_records, p.counts[0], p.counts[1]);
            if (b >= v.tiles) return;  // (a surplus workgroup: no status word, no table, no output)
            if (!v.walk) {
                // counts beyond the bounds, or no record: ticket 0 alone, and nobody reads the starts
                if (tid == 0 && b == 0) {
                    *p.out.total = 0ull;
                    p.offsets[0] = 0ull;
                    if (v.refused) flag_error(p.out.error, 6u);
                }
                return;
            }
            n = v.n;
            n_records = v.n_records;
            win_end = v.win_end;
            last_bid = (uint32_t)v.tiles - 1u;
        }
    }
    s_in[tid] = p.tables[tid];
    s_out[tid] = p.tables[256 + tid];

    // ---- 1. stage the tile's bytes: global byte g0 + q at s_text[off0 + q], g0 = first window - 1
    __syncthreads();
    const uint32_t bid = s_bid;
    const uint64_t w0 = p.win_begin + (uint64_t)bid * kTextTile;
    const long long g0 = (long long)w0 - 1;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p.text);
    const uint32_t sh = (uint32_t)(addr & 15u);
    const long long a0 = g0 + (long long)sh;           // offset of byte g0 from the 16-byte boundary below the text
    const long long a0a = a0 >= 0 ? (a0 & ~15ll) : -16;  // (-1 only in the first tile: its byte g0 does not exist)
    const uint32_t off0 = (uint32_t)(a0 - a0a);
    const uint64_t tbase = a0a >= 0 ? (uint64_t)a0a : 0u;
    // the tile's own descriptor (offsets stay small for any n < 2^32), whole dwords up to the end of the text: the text's
    // last dword may hold bytes behind it - same dword, same page - that only k-mers past the last window see
    const uint64_t rem = ((n + sh + 3u) & ~3ull) - tbase;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void *>(addr - sh + tbase), 0, (int)(uint32_t)(rem < 0xfffffff0ull ? rem : 0xfffffff0ull), 0x00020000);
    const uint32_t span = kTextTile + 1 + w + k;       // bytes the tile reads (+1 spare)
    const uint32_t chunks = (off0 + span + 15) / 16;
    for (uint32_t c = tid; c < chunks; c += kTextThreads) {
        const long long o = a0a + 16ll * c - (long long)tbase;
        u32x4t v = {0u, 0u, 0u, 0u};
        if (o >= 0) v = __builtin_amdgcn_raw_buffer_load_b128(rs, (uint32_t)o, 0, 0);  // (past the end: zeros)
        *reinterpret_cast<u32x4t *>(s_text + 16 * c) = v;
    }
    // BATCH: record starts of the tile as offsets from its front window g0 (clamped: only an unordered list goes outside)
    // (n_records < 2^31, checked by the entry points: list indices and record numbers fit 32 bits)
    uint32_t rb = 0, nb = 0;
    auto local_of = [&](uint64_t x) -> uint32_t {
        const long long d = (long long)x - g0;
        return d < 0 ? 0u : (d > 0xffff ? 0xffffu : (uint32_t)d);
    };
    if constexpr (BATCH) {
        rb = (uint32_t)p.tile_rec[2 * bid];
        nb = (uint32_t)p.tile_rec[2 * bid + 1] - rb;
        if (nb <= kTextBnd)
            for (uint32_t i = tid; i < nb; i += kTextThreads) s_bnd[i] = (uint16_t)local_of(p.starts[rb + i]);
        if (tid == 0) s_rs0 = rb ? (uint32_t)p.starts[rb - 1] : 0u;
    }
    __syncthreads();

    // ---- 2. keys of k-mers u = 0 .. kTextTile + w - 1 (k-mer u starts at byte g0 + u)
    {
        const uint32_t R = p.rot;
        const uint32_t u0 = tid * kTextHashRun;
        const uint32_t n_keys = kTextTile + w;
        if (u0 < n_keys) {
            const uint8_t *s = s_text + off0 + u0;
            uint32_t fw = p.fw0, rc = p.rc0;
            for (uint32_t j = 0; j < k; ++j) {
                const uint2 t = s_in[s[j]];
                fw = rotl32(fw, R) ^ t.x;
                if (HASH_RC) rc = rotr32(rc, R) ^ t.y;
            }
#pragma unroll 4
            for (uint32_t j = 0; j < kTextHashRun; ++j) {
                const uint32_t h = HASH_RC ? fw + rc : fw;
                s_key[u0 + j] = (h & 0xffff0000u) | (u0 + j);
                const uint2 ti = s_in[s[j + k]], to = s_out[s[j]];
                fw = rotl32(fw, R) ^ ti.x ^ to.x;
                if (HASH_RC) rc = rotr32(rc, R) ^ ti.y ^ to.y;
            }
        }
    }
    __syncthreads();

    // ---- 3. window minima, windows u = 0 .. kTextTile round robin; offsets to s_sel (thread t's windows 32t+1 .. 32t+32
    // at dwords 17t .. : window u at half (u - 1) % 32 of thread (u - 1) / 32; window 0 at thread 255's spare dword)
    for (uint32_t u = tid; u <= kTextTile; u += kTextThreads) {
        uint32_t lo = s_key[u], hi = s_key[u] ^ 0xffff0000u;
        if (W > 0) {
#pragma unroll
            for (int j = 1; j < (W > 0 ? W : 1); ++j) {
                const uint32_t v = s_key[u + j];
                lo = min(lo, v);
                if (CANON) hi = max(hi, v ^ 0xffff0000u);
            }
        } else {
            for (uint32_t j = 1; j < w; ++j) {
                const uint32_t v = s_key[u + j];
                lo = min(lo, v);
                if (CANON) hi = max(hi, v ^ 0xffff0000u);
            }
        }
        const uint32_t sel = ((lo & 0xffffu) - u) | (CANON ? (((hi & 0xffffu) - u) << 8) : 0u);
        const uint32_t v = u == 0 ? kTextPerThread * kTextThreads : u - 1;
        const uint32_t t = v / kTextPerThread, e = v % kTextPerThread;
        uint16_t *q = reinterpret_cast<uint16_t *>(s_sel + (t < kTextThreads ? t * kTextSelStride : kTextThreads * kTextSelStride - 1));
        q[t < kTextThreads ? e : 0] = (uint16_t)sel;
    }
    __syncthreads();

    // ---- 4. collect: windows w0 + 32 tid + j, j < 32, with the window in front for the dedup
    const uint32_t l = k + w - 1;
    const uint16_t *mysel = reinterpret_cast<const uint16_t *>(s_sel + tid * kTextSelStride);
    const uint32_t u_first = tid * kTextPerThread + 1;  // tile-local index of the first window (window w0 + 32 tid)
    // strand vote of window u: bytes u .. u+l-1 of the tile (s_text[off0 + u ..])
    uint32_t odd = 0;
    const uint32_t u_prev = u_first - 1;
    if (CANON) {
        const uint8_t *s = s_text + off0 + u_prev;
        for (uint32_t q = 0; q < l; ++q) odd += (s[q] >> 1) & 1u;
    }
    auto pos_of = [&](uint32_t u, uint32_t sel, uint32_t odd_u) -> uint32_t {
        const uint32_t off = CANON ? ((2u * odd_u > l) ? (sel & 0xffu) : (sel >> 8)) : sel;
        return (uint32_t)(w0 - 1 + u + off);
    };
    uint32_t prev = 0;
    bool have_prev = false;
    if (w0 + u_prev >= 1 && w0 + u_prev - 1 < win_end) {  // (window w0 + u_prev - 1 exists)
        // (window u_prev: the spare slot for u_prev = 0, else the last offset of the previous thread)
        const uint16_t *q = u_prev == 0 ? reinterpret_cast<const uint16_t *>(s_sel + kTextThreads * kTextSelStride - 1)
                                        : reinterpret_cast<const uint16_t *>(s_sel + (tid - 1) * kTextSelStride) +
                                              (kTextPerThread - 1);
        prev = pos_of(u_prev, *q, odd);
        have_prev = true;
    }
    // BATCH: the record of window u is rb + i for the last list entry i with bnd(i) <= u (i = -1: the record in front
    // of the list, starting at s_rs0); cur = bnd(i) (0 for i = -1), nxt = bnd(i + 1) (~0: past the list)
    auto bnd = [&](uint32_t i) -> uint32_t { return nb <= kTextBnd ? (uint32_t)s_bnd[i] : local_of(p.starts[rb + i]); };
    int ri = -1;
    uint32_t cur = 0, nxt = ~0u;
    if constexpr (BATCH) {
        uint32_t lo = 0, hi = nb;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (bnd(mid) <= u_prev) lo = mid + 1;
            else hi = mid;
        }
        ri = (int)lo - 1;
        cur = ri >= 0 ? bnd((uint32_t)ri) : 0u;
        nxt = lo < nb ? bnd(lo) : ~0u;
    }
    const int ri0 = ri;
    // start of window u_prev's record in text coordinates; smask bit j: a record starts at window u_first + j
    const uint32_t rs0 = ri >= 0 ? (uint32_t)(g0 + cur) : s_rs0;
    uint32_t smask = 0;
    uint32_t flags = 0;
    uint32_t vals[kTextPerThread];
#pragma unroll
    for (uint32_t j = 0; j < kTextPerThread; ++j) {
        const uint32_t u = u_first + j;
        if (CANON) {
            const uint8_t *s = s_text + off0;
            odd += ((s[u + l - 1] >> 1) & 1u) - ((s[u - 1] >> 1) & 1u);
        }
        const uint64_t g = w0 + tid * kTextPerThread + j;
        const uint32_t pp = pos_of(u, mysel[j], odd);
        bool f = false;
        bool in_rec = true, first_of_rec = !have_prev;
        if constexpr (BATCH) {
            while (nxt <= u) {
                ++ri;
                cur = nxt;
                nxt = (uint32_t)(ri + 1) < nb ? bnd((uint32_t)(ri + 1)) : ~0u;
            }
            const int r = (int)rb + ri;
            in_rec = r >= 0 && (uint32_t)r < (uint32_t)n_records && u + l <= nxt;
            first_of_rec = u == cur;
            smask |= (uint32_t)first_of_rec << j;
        }
        if (g < win_end && in_rec) {
            if (MODE == 0) f = first_of_rec || pp != prev;
            else if (MODE == 1) f = (pp == (uint32_t)g) || (pp == (uint32_t)g + w - 1);
            else f = (pp == (uint32_t)g + w / 2);
        }
        vals[j] = MODE == 0 ? pp : (uint32_t)g;
        flags |= (uint32_t)f << j;
        prev = pp;
        have_prev = true;
    }
    const uint32_t cnt = __popc(flags);
    const uint32_t incl = wave_inclusive_sum(cnt);
    if (lane == kWave - 1) s_wave_tot[wave] = incl;
    __syncthreads();
    uint32_t wave_base = 0, block_total = 0;
#pragma unroll
    for (uint32_t v = 0; v < kTextThreads / kWave; ++v) {
        const uint32_t t = s_wave_tot[v];
        if (v < wave) wave_base += t;
        block_total += t;
    }
    if (wave == 0) {
        const unsigned long long carry = (bid == 0) ? *p.out.total : 0ull;
        const unsigned long long e = lookback_exclusive(p.out.status, bid, block_total, carry, p.out.error);
        if (lane == 0) s_excl = e;
    }
    __syncthreads();
    unsigned long long dst = s_excl + wave_base + (incl - cnt);
    if constexpr (BATCH) {
        // offsets of the records that start at this thread's windows: list entries ri0 + 1 .. ri, each at window bnd(i)
        for (int i = ri0 + 1; i <= ri; ++i) {
            const uint32_t j = bnd((uint32_t)i) - u_first;
            if (j < kTextPerThread) p.offsets[rb + (uint32_t)i] = dst + __popc(flags & ((1u << j) - 1u));
        }
    }
    uint32_t rec0 = rs0;  // (BATCH: the start of window j's record)
#pragma unroll
    for (uint32_t j = 0; j < kTextPerThread; ++j) {
        const uint32_t g = (uint32_t)(w0 + tid * kTextPerThread + j);
        if (BATCH && (smask & (1u << j))) rec0 = g;
        if (flags & (1u << j)) {
            if (dst < p.out.cap) {
                p.out.pos[dst] = BATCH ? vals[j] - rec0 : vals[j];
                if (p.out.sk) p.out.sk[dst] = BATCH ? g - rec0 : g;
            }
            ++dst;
        }
    }
    if (tid == 0 && bid == last_bid) {
        *p.out.total = s_excl + block_total;
        if (BATCH) p.offsets[n_records] = s_excl + block_total;
    }
}

}  // namespace mm
