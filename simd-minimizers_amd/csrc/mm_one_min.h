// mm_one_min.h — one minimizer per record (one_minimizer, src/minimizers.rs:22-28): the per-lane and per-tile logic of
// mm_one_min.hip.  mm_debug_one_minimizer_* and a host-only program run the same functions on the host.  Plain C++: a
// host-only program may include it without the HIP headers.
//
// The k-mer start positions of the records, laid back to back, are numbered from the first record's start and cut into
// tiles of kOneMinTile positions, one workgroup each.  A lane owns kOneMinPerLane consecutive positions: it builds its
// first hash from the definition (k table steps), rolls the others, and reports one 64-bit key per record it meets,
//   key = ((h & 0xffff0000) << 32) | record_local_position,
// whose minimum over a record is the LEFTMOST position of the minimal masked hash whatever the order of evaluation.
#pragma once
#include <stdint.h>

#include "mm_values_reads.h"

namespace mm {

constexpr uint32_t kOneMinThreads = 256;  // lanes of a workgroup
constexpr uint32_t kOneMinPerLane = 16;   // consecutive k-mer start positions of a lane
constexpr uint32_t kOneMinTile = kOneMinThreads * kOneMinPerLane;  // positions of a workgroup
constexpr uint32_t kOneMinSlots = 1024;    // records of a tile whose keys meet in LDS; later ones go to global memory
constexpr uint64_t kOneMinNoKey = ~0ull;  // no k-mer seen (a real key has zeros in bits 32 .. 47)

// (in, out) entries of the rolling tables: the layout of uint2, of HashTables::t_in and of TextTables::t_in / t_out
struct OneMinPair {
    uint32_t x, y;
};
// fw' = rotl(fw, rot) ^ t_in[in].x ^ t_out[out].x ; rc' = rotr(rc, rot) ^ t_in[in].y ^ t_out[out].y ; warm-up: t_in alone,
// from (fw0, rc0).  The hasher's XOR constants are folded into t_in (make_text_tables, mm_api.hip).
struct OneMinTables {
    const OneMinPair *t_in, *t_out;  // 4 entries (packed) or 256 (byte text)
    uint32_t fw0, rc0, rot, canonical;
};

MM_HOST_DEVICE inline uint32_t one_min_rotl(uint32_t x, uint32_t r) { return r ? (x << r) | (x >> (32u - r)) : x; }
MM_HOST_DEVICE inline uint32_t one_min_rotr(uint32_t x, uint32_t r) { return r ? (x >> r) | (x << (32u - r)) : x; }

// The symbols: symbol i of the run of records (i counts from base_offset of a packed buffer, from byte 0 of a text).
struct OneMinPacked {
    const uint8_t *p;
    uint64_t base0;
    MM_HOST_DEVICE uint32_t operator()(uint64_t i) const {
        const uint64_t b = base0 + i;
        return (p[b >> 2] >> (2u * (uint32_t)(b & 3u))) & 3u;
    }
};
struct OneMinText {
    const uint8_t *p;
    uint64_t origin;  // the symbol p[0] holds (0: the whole text; a tile's staged copy: its first symbol)
    MM_HOST_DEVICE uint32_t operator()(uint64_t i) const { return p[i - origin]; }
};

// The packed symbols with their ambiguity bits (the skip-ambiguous forms): symbol i is bit bit0 + i of `bits`, bit b being
// bit b % 8 of byte b / 8 (mm_run_packed_reads_skip_ambiguous_device_async's numbering).  A k-mer with a set bit among its
// k symbols does not exist: one_min_lane gives it no key.
struct OneMinPackedAmb {
    OneMinPacked sym;
    const uint8_t *bits;
    uint64_t bit0;
    MM_HOST_DEVICE uint32_t operator()(uint64_t i) const { return sym(i); }
    MM_HOST_DEVICE bool amb(uint64_t i) const {
        const uint64_t b = bit0 + i;
        return ((bits[b >> 3] >> (uint32_t)(b & 7u)) & 1u) != 0;
    }
};
// The compile-time switch of one_min_lane: only a symbol functor that answers amb(i) makes it count clean runs.
template <class Sym>
struct OneMinHasAmb {
    static constexpr bool value = false;
};
template <>
struct OneMinHasAmb<OneMinPackedAmb> {
    static constexpr bool value = true;
};

// The records: record r is the symbols [lay[r], lay.end(r)); lay[r] is non-decreasing over [0, n].
struct OneMinStarts {
    const uint64_t *s;  // [n + 1]
    MM_HOST_DEVICE uint64_t operator[](uint64_t r) const { return s[r]; }
    MM_HOST_DEVICE uint64_t end(uint64_t r) const { return s[r + 1]; }
};
struct OneMinStride {
    uint64_t stride, len;  // len <= stride
    MM_HOST_DEVICE uint64_t operator[](uint64_t r) const { return r * stride; }
    MM_HOST_DEVICE uint64_t end(uint64_t r) const { return r * stride + len; }
};

// What a tile covers: the positions [g_begin, g_end) and the records [r_lo, r_hi] that can own one of them.
struct OneMinTileRange {
    uint64_t g_begin, g_end, r_lo, r_hi;
};

// `limit`: symbols at or past it are never loaded (the end of the last record, clamped to the buffer).  n >= 1.
// Returns false for a tile without a position (g_begin >= g_end): nothing to do.
template <class Lay>
MM_HOST_DEVICE inline bool one_min_tile_range(const Lay &lay, uint64_t n, uint64_t limit, uint32_t k, uint64_t tile_index,
                                              uint32_t tile, OneMinTileRange *out) {
    const uint64_t s0 = lay[0];
    if (limit < s0 || limit - s0 < k) return false;
    const uint64_t n_pos = limit - s0 - k + 1;  // k-mers that lie inside the symbols
    const uint64_t first = tile_index * (uint64_t)tile;
    if (first >= n_pos) return false;
    out->g_begin = s0 + first;
    out->g_end = s0 + (n_pos - first < tile ? n_pos : first + tile);
    out->r_lo = values_read_of(lay, (uint64_t)0, n - 1, out->g_begin);
    // the record of the last position is usually near: gallop from r_lo before the search (lay[lo] <= last throughout)
    const uint64_t last = out->g_end - 1;
    uint64_t lo = out->r_lo, hi = n - 1, step = 32;
    while (hi - lo > step) {
        if (lay[lo + step] <= last) {
            lo += step;
            step *= 2;
        } else {
            hi = lo + step - 1;
            break;
        }
    }
    out->r_hi = values_read_of(lay, lo, hi, last);
    return true;
}

// One lane: the positions [g0, g1) of a tile (g0 < g1 <= range.g_end), every symbol it loads lies below g1 + k - 1.
// emit(r, key) is called once per record that owns one of them, with the minimum of that record's keys in the lane.
// With ambiguity bits (OneMinHasAmb<Sym>) the lane carries, beside its hash, the length of the clean run that ends at its
// newest symbol, saturated at k and built during the warm-up: a position has a key only when that run holds its k symbols.
template <class Sym, class Lay, class Emit>
MM_HOST_DEVICE inline void one_min_lane(const Sym &sym, const Lay &lay, const OneMinTileRange &range, const OneMinTables &t,
                                        uint32_t k, uint64_t g0, uint64_t g1, Emit &&emit) {
    constexpr bool AMB = OneMinHasAmb<Sym>::value;
    const uint32_t R = t.rot;
    const bool canon = t.canonical != 0;
    uint64_t r = values_read_of(lay, range.r_lo, range.r_hi, g0);
    uint64_t rs = lay[r], re = lay.end(r);
    // a k-mer belongs to the record it starts in and ends in: one that straddles two records belongs to none
    {
        // nothing to hash when no position of the lane can own a k-mer: the record at g0 is too short for one from here
        // and no other record starts in the lane
        const bool none_here = g0 < rs || g0 + k > re;
        if (none_here && (r >= range.r_hi || lay[r + 1] >= g1)) return;
    }
    uint32_t fw = t.fw0, rc = t.rc0;
    [[maybe_unused]] uint32_t clean = 0;  // (AMB) symbols of the clean run that ends at the newest symbol, at most k
    for (uint32_t j = 0; j < k; ++j) {
        const OneMinPair e = t.t_in[sym(g0 + j)];
        fw = one_min_rotl(fw, R) ^ e.x;
        if (canon) rc = one_min_rotr(rc, R) ^ e.y;
        if constexpr (AMB) clean = sym.amb(g0 + j) ? 0u : clean + 1u;
    }
    uint64_t best = kOneMinNoKey;
    for (uint64_t g = g0;;) {
        if (r < range.r_hi && g >= lay[r + 1]) {  // past this record: the LAST record that starts at or before g
            if (best != kOneMinNoKey) emit(r, best);
            best = kOneMinNoKey;
            r = values_read_of(lay, r + 1, range.r_hi, g);
            rs = lay[r];
            re = lay.end(r);
        }
        if (g >= rs && g + k <= re && (!AMB || clean >= k)) {
            const uint32_t h = canon ? fw + rc : fw;
            const uint64_t key = ((uint64_t)(h & 0xffff0000u) << 32) | (uint64_t)(uint32_t)(g - rs);
            if (key < best) best = key;
        }
        if (++g >= g1) break;
        const OneMinPair in = t.t_in[sym(g + k - 1)], out = t.t_out[sym(g - 1)];
        fw = one_min_rotl(fw, R) ^ in.x ^ out.x;
        if (canon) rc = one_min_rotr(rc, R) ^ in.y ^ out.y;
        if constexpr (AMB) clean = sym.amb(g + k - 1) ? 0u : (clean < k ? clean + 1u : k);
    }
    if (best != kOneMinNoKey) emit(r, best);
}

// One tile on the host, lane after lane: keys[r] = min(keys[r], key) for every record of the tile (keys: n words, preset
// to kOneMinNoKey).  `tile` overrides the tile size (tests); lanes keep kOneMinPerLane positions.
template <class Sym, class Lay>
inline void one_min_tile_host(const Sym &sym, const Lay &lay, uint64_t n, uint64_t limit, const OneMinTables &t, uint32_t k,
                              uint64_t tile_index, uint32_t tile, uint64_t *keys) {
    OneMinTileRange range;
    if (!one_min_tile_range(lay, n, limit, k, tile_index, tile, &range)) return;
    for (uint64_t g0 = range.g_begin; g0 < range.g_end; g0 += kOneMinPerLane) {
        const uint64_t g1 = range.g_end - g0 < kOneMinPerLane ? range.g_end : g0 + kOneMinPerLane;
        one_min_lane(sym, lay, range, t, k, g0, g1, [&](uint64_t r, uint64_t key) {
            if (key < keys[r]) keys[r] = key;
        });
    }
}

// Tiles that cover `n_pos` k-mer start positions.
inline uint64_t one_min_tiles(uint64_t n_pos, uint32_t tile) { return (n_pos + tile - 1) / tile; }

// Every tile on the host, the per-tile keys combined by minimum into keys[0 .. n) (preset to kOneMinNoKey): what the
// kernels compute for n >= 1 records over a buffer of `symbols` symbols.
template <class Sym, class Lay>
inline void one_min_host(const Sym &sym, const Lay &lay, uint64_t n, uint64_t symbols, const OneMinTables &t, uint32_t k,
                         uint32_t tile, uint64_t *keys) {
    uint64_t limit = lay.end(n - 1);
    if (limit > symbols) limit = symbols;
    const uint64_t s0 = lay[0];
    if (limit < s0 || limit - s0 < k) return;
    const uint64_t tiles = one_min_tiles(limit - s0 - k + 1, tile);
    for (uint64_t i = 0; i < tiles; ++i) one_min_tile_host(sym, lay, n, limit, t, k, i, tile, keys);
}

// The record count and the symbol count read on the DEVICE (mm_one_minimizer_*_counts_device_async; d_counts in the
// loaders' layout: symbols, records): the host sizes the launch from the bounds it was given, thread 0 of every workgroup
// turns {counts, bounds} into what the tile works on with the one function below (the pattern of text_counts_view,
// mm_text_counts.h).  The host runs the same function (mm_debug_one_minimizer_counts_view): no device needed.
struct OneMinCountsView {
    uint64_t n;        // records the kernels work on (0 when refused)
    uint64_t limit;    // symbols at or past it are never loaded: min(starts[n], n_sym) (0 when refused or n == 0)
    uint32_t refused;  // a count exceeds its bound: every output word is "none", the starts are not read
};
// max_sym <= the buffer's symbols (the entry points check it), so the limit never passes the buffer.  Counts within the
// bounds give what a host-n launch with n_reads = n computes on a buffer cut at n_sym symbols.
MM_HOST_DEVICE inline OneMinCountsView one_min_counts_view(const uint64_t *starts, uint64_t max_sym, uint64_t max_records,
                                                           uint64_t n_sym, uint64_t n) {
    OneMinCountsView v;
    v.refused = (n_sym > max_sym || n > max_records) ? 1u : 0u;
    v.n = v.refused ? 0 : n;
    v.limit = 0;
    if (v.n) {
        const uint64_t end = starts[v.n];
        v.limit = end < n_sym ? end : n_sym;
    }
    return v;
}

// A key as the caller sees it.
MM_HOST_DEVICE inline uint32_t one_min_position(uint64_t key) { return key == kOneMinNoKey ? 0xFFFFFFFFu : (uint32_t)key; }

}  // namespace mm
