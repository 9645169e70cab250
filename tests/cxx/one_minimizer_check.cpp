// The one-minimizer kernel's per-tile logic (mm_one_min.h) in a stand-alone host program: every record against a loop
// written from the definition (src/minimizers.rs:22-28: the leftmost position that minimises hash & 0xffff0000).
// Built with -fsanitize=address,undefined by tests/test_one_minimizer_cpu.py; every input lies in a heap block of
// exactly its size, so a symbol, start or key index outside its array is reported.  Needs nothing from HIP.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "mm_one_min.h"

namespace {

uint64_t g_x = 88172645463325252ull;
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

int g_checked = 0;

// Records of `lens` symbols behind `first` junk symbols (and `base_offset` more for packed input), checked for one k.
int check(const std::vector<uint64_t> &lens, uint64_t first, uint32_t base_offset, bool text, uint32_t k, uint32_t tile,
          const Hasher &h) {
    const uint64_t n = lens.size();
    std::unique_ptr<uint64_t[]> starts(new uint64_t[n + 1]);  // exactly n + 1 words
    starts[0] = first;
    for (uint64_t r = 0; r < n; ++r) starts[r + 1] = starts[r] + lens[r];
    const uint64_t symbols = starts[n];  // the buffer ends with the last record
    std::vector<uint8_t> sym(base_offset + symbols);
    for (auto &s : sym) s = (uint8_t)(rnd() % h.fw.size());
    const uint64_t bytes = text ? symbols : (base_offset + symbols + 3) / 4;
    std::unique_ptr<uint8_t[]> data(new uint8_t[bytes ? bytes : 1]);  // exactly the bytes the symbols need
    if (text) {
        if (symbols) memcpy(data.get(), sym.data(), symbols);
    } else {
        memset(data.get(), 0, bytes ? bytes : 1);
        for (uint64_t i = 0; i < sym.size(); ++i) data[i >> 2] |= (uint8_t)(sym[i] << (2 * (i & 3)));
    }
    Tables t;
    make_tables(h, k, &t);
    std::unique_ptr<uint64_t[]> keys(new uint64_t[n]);
    for (uint64_t r = 0; r < n; ++r) keys[r] = mm::kOneMinNoKey;
    const uint64_t avail = text ? bytes : 4 * bytes - base_offset;
    if (text)
        mm::one_min_host(mm::OneMinText{data.get(), 0}, mm::OneMinStarts{starts.get()}, n, avail, t.view, k, tile, keys.get());
    else
        mm::one_min_host(mm::OneMinPacked{data.get(), base_offset}, mm::OneMinStarts{starts.get()}, n, avail, t.view, k, tile,
                         keys.get());
    const uint8_t *s = sym.data() + (text ? 0 : base_offset);
    for (uint64_t r = 0; r < n; ++r) {
        uint32_t want = 0xFFFFFFFFu, best = 0;
        for (uint64_t p = 0; p + k <= lens[r]; ++p) {
            const uint32_t m = hash_of(h, s + starts[r] + p, k) & 0xffff0000u;
            if (want == 0xFFFFFFFFu || m < best) want = (uint32_t)p, best = m;
        }
        const uint32_t got = mm::one_min_position(keys[r]);
        ++g_checked;
        if (got != want) {
            printf("mismatch: record %llu of %llu (len %llu) k %u tile %u base_offset %u text %d: got %u want %u\n",
                   (unsigned long long)r, (unsigned long long)n, (unsigned long long)lens[r], k, tile, base_offset, (int)text,
                   got, want);
            return 1;
        }
    }
    return 0;
}

}  // namespace

int main() {
    const uint32_t tile = 8;
    const uint32_t rots[] = {0, 1, 7, 16, 31};
    int round = 0;
    for (uint32_t k : {1u, 2u, 5u, 9u, 17u, 33u}) {
        // one record of every length 0 .. 2 tile + k at every base offset, with neighbours of its own kind
        for (uint64_t len = 0; len <= 2 * tile + k; ++len)
            for (uint32_t bo = 0; bo < 4; ++bo) {
                const Hasher h4 = make_hasher(4, rots[round % 5], (round >> 1) & 1, (round & 4) != 0);
                ++round;
                if (check({len}, 0, bo, false, k, tile, h4)) return 1;
                if (check({3, len, 0, 0, len / 2, k, len}, bo + 1, bo, false, k, tile, h4)) return 1;
                if (bo == 0) {
                    const Hasher h256 = make_hasher(256, rots[round % 5], round & 1, (round & 2) != 0);
                    if (check({len}, 0, 0, true, k, tile, h256)) return 1;
                    if (check({0, len, 1, 0, len, k - 1}, 5, 0, true, k, tile, h256)) return 1;
                }
            }
    }
    // the kernel's own tile and one in between, records around their edges
    for (uint32_t T : {64u, mm::kOneMinTile}) {
        const Hasher h4 = make_hasher(4, 7, 1, false);
        for (uint32_t k : {1u, 21u, 33u})
            if (check({T - 1, T, T + 1, T + k - 1, T + k, k - 1, k, 0, 0, 0, 1, 2ull * T, 150, 150}, 3, 1, false, k, T, h4)) return 1;
    }
    printf("one_minimizer_check: %d records ok\n", g_checked);
    return 0;
}
