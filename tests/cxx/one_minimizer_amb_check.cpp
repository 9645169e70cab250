// The ambiguity-aware lane of the one-minimizer kernel (mm_one_min.h: one_min_lane over OneMinPackedAmb, through
// one_min_host as the kernels and mm_debug_one_minimizer_reads_skip_ambiguous run it) in a stand-alone host program:
// every record against a loop written from the definition - the smallest position, among those whose k bases carry no
// ambiguity bit, that minimises hash & 0xffff0000; none when the record has no such position.  Built with
// -fsanitize=address,undefined by tests/test_one_minimizer_amb_cpu.py.  Packed bytes, ambiguity bytes, starts and keys
// each lie in a heap block of exactly the size the contract lets the kernel touch - the bytes that hold the symbols and
// the bits below the limit, n + 1 starts, n keys - so an index outside one is reported.  Needs nothing from HIP.
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
    uint32_t fw[4], rc[4];
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
    mm::OneMinPair t_in[4], t_out[4];
    mm::OneMinTables view;
};
void make_tables(const Hasher &h, uint32_t k, Tables *t) {
    const uint32_t R = h.rot & 31u;
    const uint32_t df = rotl(h.fw_xor, R) ^ h.fw_xor, dr = rotl(h.rc_xor, 32u - R) ^ h.rc_xor;
    for (int c = 0; c < 4; ++c) {
        t->t_in[c] = {h.fw[c] ^ df, rotl(h.rc[c], (uint32_t)(((uint64_t)R * (k - 1)) & 31u)) ^ dr};
        t->t_out[c] = {rotl(h.fw[c], (uint32_t)(((uint64_t)R * k) & 31u)), rotl(h.rc[c], 32u - R)};
    }
    t->view = {t->t_in, t->t_out, h.fw_xor, h.rc_xor, R, h.canonical};
}

Hasher make_hasher(uint32_t rot, uint32_t canonical, bool xors) {
    Hasher h;
    for (int c = 0; c < 4; ++c) h.fw[c] = (uint32_t)rnd(), h.rc[c] = (uint32_t)rnd();
    h.rot = rot, h.canonical = canonical;
    h.fw_xor = xors ? (uint32_t)rnd() : 0, h.rc_xor = xors ? (uint32_t)rnd() : 0;
    return h;
}

int g_checked = 0, g_none = 0, g_moved = 0;

int fail(const char *what, uint64_t a, uint64_t b) {
    printf("mismatch: %s: got %llu want %llu\n", what, (unsigned long long)a, (unsigned long long)b);
    return 1;
}

// Records `lens` from symbol `first` on; `density`: one base in `density` is ambiguous (0: none), plus the rules below.
// `short_amb`: the ambiguity buffer ends this many bits before the last record does - the k-mers beyond it do not exist.
// `stride`: 0 = the starts layout, else the fixed-stride layout with reads of lens[0] bases.
int check(const std::vector<uint64_t> &lens, uint64_t first, uint32_t base_offset, uint32_t amb_offset, uint32_t k, uint32_t tile,
          const Hasher &h, uint32_t density, uint64_t short_amb, uint64_t stride) {
    const uint64_t n = lens.size();
    std::unique_ptr<uint64_t[]> starts(new uint64_t[n + 1]);
    starts[0] = stride ? 0 : first;
    for (uint64_t r = 0; r < n; ++r) starts[r + 1] = stride ? (r + 1) * stride : starts[r] + lens[r];
    const uint64_t end = stride ? (n - 1) * stride + lens[0] : starts[n];
    const uint64_t amb_bits = end > short_amb ? end - short_amb : 0;  // the bits the buffer holds behind amb_offset
    const uint64_t limit = amb_bits < end ? amb_bits : end;
    // the symbols and the bits as values, then exactly the bytes that hold those below the limit
    std::vector<uint8_t> sym(limit), bit(limit);
    for (auto &s : sym) s = (uint8_t)(rnd() & 3u);
    for (auto &b : bit) b = density && rnd() % density == 0 ? 1 : 0;
    for (uint64_t r = 0; r < n; ++r) {
        const uint64_t s = starts[r], e = stride ? s + lens[0] : starts[r + 1];
        if (e > limit) continue;
        if (density && r % 5 == 1 && e > s) bit[e - 1] = 1;                      // the last base
        if (density && r % 5 == 2 && e > s) bit[s] = 1;                          // the first base
        if (density && r % 7 == 3) for (uint64_t i = s; i < e; ++i) bit[i] = 1;  // all N
        if (density && r % 7 == 4 && e - s > k + 2) {                            // the only clean run has k bases, or k - 1
            for (uint64_t i = s; i < e; ++i) bit[i] = 1;
            for (uint64_t i = s + 2; i < s + 2 + k - (r & 1); ++i) bit[i] = 0;
        }
    }
    for (uint64_t i = 0; i < first && i < limit; ++i) bit[i] = stride ? bit[i] : 1;  // junk in front of record 0
    const uint64_t pbytes = (base_offset + limit + 3) / 4, abytes = (amb_offset + limit + 7) / 8;
    std::unique_ptr<uint8_t[]> packed(new uint8_t[pbytes ? pbytes : 1]), amb(new uint8_t[abytes ? abytes : 1]);
    memset(packed.get(), 0xff, pbytes ? pbytes : 1);  // (junk in front: base_offset symbols, amb_offset SET bits)
    memset(amb.get(), 0xff, abytes ? abytes : 1);
    for (uint64_t i = 0; i < limit; ++i) {
        const uint64_t b = base_offset + i, a = amb_offset + i;
        packed[b >> 2] = (uint8_t)((packed[b >> 2] & ~(3u << (2 * (b & 3)))) | (uint32_t)(sym[i] << (2 * (b & 3))));
        if (!bit[i]) amb[a >> 3] = (uint8_t)(amb[a >> 3] & ~(1u << (a & 7)));
    }
    Tables t;
    make_tables(h, k, &t);
    std::unique_ptr<uint64_t[]> keys(new uint64_t[n]);
    for (uint64_t r = 0; r < n; ++r) keys[r] = mm::kOneMinNoKey;
    // what the entry points do: the symbols are what BOTH buffers hold (here the ambiguity buffer is the shorter one)
    const mm::OneMinPackedAmb s{mm::OneMinPacked{packed.get(), base_offset}, amb.get(), amb_offset};
    if (stride) {
        if (lens[0] >= k) mm::one_min_host(s, mm::OneMinStride{stride, lens[0]}, n, limit, t.view, k, tile, keys.get());
    } else {
        mm::one_min_host(s, mm::OneMinStarts{starts.get()}, n, limit, t.view, k, tile, keys.get());
    }
    for (uint64_t r = 0; r < n; ++r) {
        const uint64_t rs = starts[r], re = stride ? rs + lens[0] : starts[r + 1];
        const uint64_t e = re < limit ? re : limit;  // a record cut by the limit keeps the k-mers that end below it
        const uint64_t len = e > rs ? e - rs : 0;
        uint32_t want = 0xFFFFFFFFu, best = 0, plain = 0xFFFFFFFFu, plain_best = 0;
        for (uint64_t p = 0; p + k <= len; ++p) {
            const uint32_t m = hash_of(h, sym.data() + rs + p, k) & 0xffff0000u;
            if (plain == 0xFFFFFFFFu || m < plain_best) plain = (uint32_t)p, plain_best = m;
            bool clean = true;
            for (uint32_t j = 0; j < k; ++j) clean = clean && !bit[rs + p + j];
            if (clean && (want == 0xFFFFFFFFu || m < best)) want = (uint32_t)p, best = m;
        }
        const uint32_t got = mm::one_min_position(keys[r]);
        ++g_checked;
        g_none += want == 0xFFFFFFFFu && len >= k;
        g_moved += want != plain && want != 0xFFFFFFFFu;
        if (got != want) {
            printf("record %llu of %llu (len %llu) k %u tile %u base_offset %u amb_offset %u stride %llu: ", (unsigned long long)r,
                   (unsigned long long)n, (unsigned long long)len, k, tile, base_offset, amb_offset, (unsigned long long)stride);
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
        for (uint32_t k : {1u, 2u, 7u, 17u, 33u, 100u}) {
            std::vector<uint64_t> lens = {3, tile - 1, 0, 0, tile + k, k - 1, k, 2ull * tile + 5, 1, 40, k + 3, k + 4, 150, 150, 150};
            for (int i = 0; i < 12; ++i) lens.push_back(k + 1 + (uint64_t)(rnd() % 90));
            for (uint32_t bo = 0; bo < 4; ++bo) {
                for (uint32_t ao : {0u, 5u, 37u}) {
                    const Hasher h = make_hasher(rots[round % 5], round & 1, (round & 2) != 0);
                    ++round;
                    for (uint32_t density : {0u, 200u, 9u})
                        for (uint64_t short_amb : {(uint64_t)0, (uint64_t)1, (uint64_t)(k + 60)})
                            if (check(lens, bo + 1, bo, ao, k, tile, h, density, short_amb, 0)) return 1;
                    // fixed stride: reads of 100 at 128, reads of 150 back to back
                    if (check(std::vector<uint64_t>(40, 100), 0, bo, ao, k, tile, h, 50, 0, 128)) return 1;
                    if (check(std::vector<uint64_t>(40, 150), 0, bo, ao, k, tile, h, 50, 3, 150)) return 1;
                }
            }
        }
    }
    // the kernel's own tile, and more records in a tile than it has LDS slots
    {
        const uint32_t T = mm::kOneMinTile, k = 21;
        const Hasher h = make_hasher(7, 1, false);
        std::vector<uint64_t> lens = {T - 1, T, T + 1, T + k - 1, T + k, k - 1, k, 0, 0, 0, 1, 2ull * T, 150, 150, 150, 150};
        if (check(lens, 7, 3, 37, k, T, h, 200, 0, 0)) return 1;
        if (check(lens, 7, 1, 5, k, T, h, 200, T / 2, 0)) return 1;
        if (check(std::vector<uint64_t>(1500, 2), 7, 1, 5, 2, T, h, 50, 0, 0)) return 1;
    }
    if (g_checked == 0 || g_none == 0 || g_moved == 0) return fail("cases run", 0, 1);
    printf("one_minimizer_amb_check: %d records ok, %d without a clean k-mer, %d moved by a bit\n", g_checked, g_none, g_moved);
    return 0;
}
