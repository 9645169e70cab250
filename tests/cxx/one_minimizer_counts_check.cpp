// The counts form of the one-minimizer kernel (mm_one_min.h: one_min_counts_view, then the per-tile logic with the view's
// n and limit) in a stand-alone host program: every record against a loop written from the definition
// (src/minimizers.rs:22-28: the leftmost position that minimises hash & 0xffff0000), for counts at, below and beyond their
// bounds.  Built with -fsanitize=address,undefined by tests/test_one_minimizer_counts_cpu.py.  Every input lies in a heap
// block of exactly the size the contract lets the kernel touch - n + 1 starts (not max_records + 1), `limit` symbols, n
// keys, and NO starts at all for a refused view - so an index outside it is reported.  Needs nothing from HIP.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "mm_one_min.h"

namespace {

uint64_t g_x = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
    g_x ^= g_x << 13, g_x ^= g_x >> 7, g_x ^= g_x << 17;
    return g_x;
}
uint32_t rotl(uint32_t x, uint32_t r) {
    r &= 31u;
    return r ? (x << r) | (x >> (32u - r)) : x;
}

struct Hasher {
    std::vector<uint32_t> fw, rc;  // 4 or 256 entries
    uint32_t rot, canonical, fw_xor, rc_xor;
};

// h_fw(i) = fw_xor ^ XOR_j rotl(fw[s[i+j]], rot*(k-1-j)); h_rc(i) = rc_xor ^ XOR_j rotl(rc[s[i+j]], rot*j)
uint32_t hash_of(const Hasher &h, const uint8_t *s, uint32_t k) {
    uint32_t f = h.fw_xor, r = h.rc_xor;
    for (uint32_t j = 0; j < k; ++j) {
        f ^= rotl(h.fw[s[j]], (uint32_t)(((uint64_t)h.rot * (k - 1 - j)) & 31u));
        r ^= rotl(h.rc[s[j]], (uint32_t)(((uint64_t)h.rot * j) & 31u));
    }
    return h.canonical ? f + r : f;
}

struct Tables {
    std::vector<mm::OneMinPair> t_in, t_out;
    mm::OneMinTables view;
};
void make_tables(const Hasher &h, uint32_t k, Tables *t) {
    const uint32_t R = h.rot & 31u;
    const uint32_t df = rotl(h.fw_xor, R) ^ h.fw_xor, dr = rotl(h.rc_xor, 32u - R) ^ h.rc_xor;
    const size_t n = h.fw.size();
    t->t_in.resize(n);
    t->t_out.resize(n);
    for (size_t c = 0; c < n; ++c) {
        t->t_in[c] = {h.fw[c] ^ df, rotl(h.rc[c], (uint32_t)(((uint64_t)R * (k - 1)) & 31u)) ^ dr};
        t->t_out[c] = {rotl(h.fw[c], (uint32_t)(((uint64_t)R * k) & 31u)), rotl(h.rc[c], 32u - R)};
    }
    t->view = {t->t_in.data(), t->t_out.data(), h.fw_xor, h.rc_xor, R, h.canonical};
}

Hasher make_hasher(size_t size, uint32_t rot, uint32_t canonical, bool xors) {
    Hasher h;
    h.fw.resize(size);
    h.rc.resize(size);
    for (size_t c = 0; c < size; ++c) h.fw[c] = (uint32_t)rnd(), h.rc[c] = (uint32_t)rnd();
    h.rot = rot, h.canonical = canonical;
    h.fw_xor = xors ? (uint32_t)rnd() : 0, h.rc_xor = xors ? (uint32_t)rnd() : 0;
    return h;
}

int g_checked = 0, g_refused = 0;

int fail(const char *what, uint64_t a, uint64_t b) {
    printf("mismatch: %s: got %llu want %llu\n", what, (unsigned long long)a, (unsigned long long)b);
    return 1;
}

// `lens`: the records a loader found; the device counts say (n_sym, n) with n <= lens.size().  Bounds max_sym / max_records.
int check(const std::vector<uint64_t> &lens, uint64_t first, uint32_t base_offset, bool text, uint32_t k, uint32_t tile,
          const Hasher &h, uint64_t n, uint64_t n_sym, uint64_t max_sym, uint64_t max_records) {
    const bool refused = n_sym > max_sym || n > max_records;
    // the starts the view may read: [0 .. n] - none when it refuses
    std::unique_ptr<uint64_t[]> starts;
    if (!refused) {
        starts.reset(new uint64_t[n + 1]);
        starts[0] = first;
        for (uint64_t r = 0; r < n; ++r) starts[r + 1] = starts[r] + lens[r];
    }
    const mm::OneMinCountsView v = mm::one_min_counts_view(starts.get(), max_sym, max_records, n_sym, n);
    if (v.refused != (refused ? 1u : 0u)) return fail("refused", v.refused, refused);
    if (refused) {
        ++g_refused;
        if (v.n != 0) return fail("n of a refused view", v.n, 0);
        if (v.limit != 0) return fail("limit of a refused view", v.limit, 0);
        return 0;
    }
    if (v.n != n) return fail("n", v.n, n);
    const uint64_t limit = n == 0 ? 0 : (starts[n] < n_sym ? starts[n] : n_sym);
    if (v.limit != limit) return fail("limit", v.limit, limit);
    if (limit > max_sym) return fail("limit past the bound", limit, max_sym);
    if (n == 0) return 0;
    // exactly `limit` symbols
    std::vector<uint8_t> sym(base_offset + limit);
    for (auto &s : sym) s = (uint8_t)(rnd() % h.fw.size());
    const uint64_t bytes = text ? limit : (base_offset + limit + 3) / 4;
    std::unique_ptr<uint8_t[]> data(new uint8_t[bytes ? bytes : 1]);
    if (text) {
        if (limit) memcpy(data.get(), sym.data(), limit);
    } else {
        memset(data.get(), 0, bytes ? bytes : 1);
        for (uint64_t i = 0; i < sym.size(); ++i) data[i >> 2] |= (uint8_t)(sym[i] << (2 * (i & 3)));
    }
    Tables t;
    make_tables(h, k, &t);
    std::unique_ptr<uint64_t[]> keys(new uint64_t[n]);
    for (uint64_t r = 0; r < n; ++r) keys[r] = mm::kOneMinNoKey;
    // what the kernels do: every tile of the view's positions with the view's (n, limit)
    const mm::OneMinStarts lay{starts.get()};
    if (v.limit >= first && v.limit - first >= k) {
        const uint64_t tiles = mm::one_min_tiles(v.limit - first - k + 1, tile);
        for (uint64_t i = 0; i < tiles + 2; ++i) {  // (two workgroups past the real last tile: they find nothing)
            if (text) mm::one_min_tile_host(mm::OneMinText{data.get(), 0}, lay, v.n, v.limit, t.view, k, i, tile, keys.get());
            else mm::one_min_tile_host(mm::OneMinPacked{data.get(), base_offset}, lay, v.n, v.limit, t.view, k, i, tile, keys.get());
        }
    }
    const uint8_t *s = sym.data() + (text ? 0 : base_offset);
    for (uint64_t r = 0; r < n; ++r) {
        // a record cut by n_sym keeps the k-mers that end below the limit
        const uint64_t end = starts[r + 1] < limit ? starts[r + 1] : limit;
        const uint64_t len = end > starts[r] ? end - starts[r] : 0;
        uint32_t want = 0xFFFFFFFFu, best = 0;
        for (uint64_t p = 0; p + k <= len; ++p) {
            const uint32_t m = hash_of(h, s + starts[r] + p, k) & 0xffff0000u;
            if (want == 0xFFFFFFFFu || m < best) want = (uint32_t)p, best = m;
        }
        const uint32_t got = mm::one_min_position(keys[r]);
        ++g_checked;
        if (got != want) {
            printf("record %llu of %llu (len %llu) k %u tile %u base_offset %u text %d n_sym %llu: ", (unsigned long long)r,
                   (unsigned long long)n, (unsigned long long)lens[r], k, tile, base_offset, (int)text, (unsigned long long)n_sym);
            return fail("position", got, want);
        }
    }
    return 0;
}

}  // namespace

int main() {
    int round = 0;
    const uint32_t rots[] = {0, 1, 7, 16, 31};
    for (uint32_t tile : {16u, 64u}) {
        for (uint32_t k : {1u, 2u, 7u, 17u, 33u}) {
            const std::vector<uint64_t> lens = {3, tile - 1, 0, 0, tile + k, k - 1, k, 2ull * tile + 5, 1, 40};
            uint64_t total = 0;
            for (uint64_t l : lens) total += l;
            for (uint32_t bo = 0; bo < 4; ++bo) {
                const uint64_t first = bo + 1;
                const uint64_t all = first + total;  // the symbols a loader wrote
                const bool text = bo == 0;
                const Hasher h = make_hasher(text ? 256 : 4, rots[round % 5], round & 1, (round & 2) != 0);
                ++round;
                for (uint64_t n = 0; n <= lens.size(); ++n) {
                    // counts below and at the bounds, the record bound at and above the count
                    for (uint64_t max_records : {n, n + 1, n + 37})
                        for (uint64_t max_sym : {all, all + 9})
                            if (check(lens, first, bo, text, k, tile, h, n, all, max_sym, max_records)) return 1;
                    // n_sym below starts[n]: the last records lose their tails
                    for (uint64_t cut : {(uint64_t)1, (uint64_t)k, (uint64_t)tile, total / 2})
                        if (cut < all && check(lens, first, bo, text, k, tile, h, n, all - cut, all, lens.size())) return 1;
                    // n_sym of zero and below the first start
                    if (check(lens, first, bo, text, k, tile, h, n, 0, all, lens.size())) return 1;
                    if (check(lens, first, bo, text, k, tile, h, n, first - 1, all, lens.size())) return 1;
                    // beyond each bound, and both: refused, no start is read
                    if (check(lens, first, bo, text, k, tile, h, n, all + 1, all, lens.size())) return 1;
                    if (n && check(lens, first, bo, text, k, tile, h, n, all, all, n - 1)) return 1;
                    if (n && check(lens, first, bo, text, k, tile, h, n, ~0ull, all, n - 1)) return 1;
                }
            }
        }
    }
    // the kernel's own tile
    {
        const uint32_t T = mm::kOneMinTile, k = 21;
        const Hasher h4 = make_hasher(4, 7, 1, false);
        const std::vector<uint64_t> lens = {T - 1, T, T + 1, T + k - 1, T + k, k - 1, k, 0, 0, 0, 1, 2ull * T, 150, 150};
        uint64_t total = 0;
        for (uint64_t l : lens) total += l;
        for (uint64_t n : {(uint64_t)0, (uint64_t)5, (uint64_t)lens.size()}) {
            if (check(lens, 3, 1, false, k, T, h4, n, 3 + total, 3 + total, lens.size() + 37)) return 1;
            if (check(lens, 3, 1, false, k, T, h4, n, 3 + total - T / 2, 3 + total, lens.size() + 37)) return 1;
        }
    }
    if (g_refused == 0 || g_checked == 0) return fail("cases run", 0, 1);
    printf("one_minimizer_counts_check: %d records ok, %d refused views\n", g_checked, g_refused);
    return 0;
}
