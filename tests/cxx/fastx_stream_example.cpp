/* A FASTQ streamed through the device in chunks (mm_fastx_stream_*: feed / next / finish through the C ABI, then the same
 * through Builder::stream_fastx of the C++ mirror), compared with the one-shot call on the same reads
 * (mm_run_packed_reads_host: Builder::run per read, src/lib.rs:378).  The reference reads a file of any size record by
 * record on the CPU (bench/src/lib.rs:51-82); the stream does it with chunks of 16 KB here, so that the 400 small reads
 * cross many chunk borders.  Exit code 0 = everything agrees; 77 = no GPU (the engine has no CPU fallback). */
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "simd_minimizers_amd.hpp"

namespace sm = simd_minimizers;

enum { N_READS = 400, K = 21, W = 11 };

struct Collected {
    std::vector<uint64_t> rec_text_pos, lens, offsets{0};
    std::vector<uint32_t> pos;
    uint64_t covered = 0;
    bool tiled = true;
    void add(const mm_fastx_batch_t &b) {
        if (b.text_begin != covered) tiled = false;
        covered = b.text_end;
        for (uint64_t r = 0; r < b.n_records; ++r) {
            rec_text_pos.push_back(b.rec_text_pos[r]);
            lens.push_back(b.rec_base[r + 1] - b.rec_base[r]);
            offsets.push_back(pos.size() + b.offsets[r + 1]);
        }
        pos.insert(pos.end(), b.pos, b.pos + b.n_positions);
    }
};

int main() {
    if (mm_device_count() <= 0) {
        printf("no GPU\n");
        return 77;
    }
    /* 400 reads of 0 .. 699 bases, one of 5 000 */
    std::string file;
    std::vector<uint64_t> want_text_pos, starts{0};
    std::vector<uint8_t> packed;
    uint64_t x = 0x9E3779B97F4A7C15ull, total = 0;
    for (int r = 0; r < N_READS; ++r) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        const uint64_t len = r == 7 ? 0 : (r == 200 ? 5000 : (x >> 40) % 700);
        want_text_pos.push_back(file.size());
        file += "@read" + std::to_string(r) + "\n";
        for (uint64_t j = 0; j < len; ++j) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            const char c = "ACGT"[(x >> 33) & 3];
            file.push_back(c);
            if ((total & 3) == 0) packed.push_back(0);
            packed[total >> 2] |= (uint8_t)((((uint8_t)c >> 1) & 3u) << (2 * (total & 3)));
            ++total;
        }
        file += "\n+\n" + std::string(len, 'I') + "\n";
        starts.push_back(total);
    }
    packed.resize(packed.size() + 16, 0);

    /* the one-shot call */
    mm_plan_t *plan = nullptr;
    mm_workspace_t *ws = nullptr;
    if (mm_plan_create(&plan, K, W, 1, MM_MINIMIZERS, nullptr) != MM_OK) return 2;
    if (mm_workspace_create(&ws, 0, nullptr) != MM_OK) return 3;
    std::vector<uint32_t> want_pos(total ? total : 1);
    std::vector<uint64_t> want_offsets(N_READS + 1);
    uint64_t want_n = 0;
    if (mm_run_packed_reads_host(plan, ws, packed.data(), N_READS, starts.data(), 0xffffffffu, want_pos.data(), nullptr,
                                 want_pos.size(), want_offsets.data(), &want_n) != MM_OK) {
        printf("one-shot: %s\n", mm_last_error());
        return 4;
    }
    want_pos.resize(want_n);

    /* the stream through the C ABI: pieces of 5 000 bytes, chunks of 16 KB */
    mm_fastx_stream_config_t cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.format = MM_FASTX_AUTO;
    cfg.chunk_bytes = 16384;
    cfg.max_records = 1000;
    mm_fastx_stream_t *st = nullptr;
    if (mm_fastx_stream_create(&st, plan, &cfg) != MM_OK) {
        printf("create: %s\n", mm_last_error());
        return 5;
    }
    Collected got;
    mm_fastx_batch_t batch;
    int r = MM_OK;
    for (uint64_t at = 0; at < file.size();) {
        const uint64_t piece = file.size() - at < 5000 ? file.size() - at : 5000;
        uint64_t took = 0;
        r = mm_fastx_stream_feed(st, (const uint8_t *)file.data() + at, piece, &took);
        if (r != MM_OK) return 6;
        at += took;
        if (took < piece) {
            r = mm_fastx_stream_next(st, &batch);
            if (r == MM_OK) got.add(batch);
            else if (r != MM_FASTX_NEED_INPUT) return 7;
        }
    }
    if (mm_fastx_stream_finish(st) != MM_OK) return 8;
    while ((r = mm_fastx_stream_next(st, &batch)) == MM_OK) got.add(batch);
    if (r != MM_FASTX_END) {
        printf("next: %d %s\n", r, mm_last_error());
        return 9;
    }
    mm_fastx_stream_destroy(st);
    if (!got.tiled || got.covered != file.size()) return 10;
    if (got.rec_text_pos != want_text_pos) return 11;
    for (int i = 0; i < N_READS; ++i)
        if (got.lens[i] != starts[i + 1] - starts[i]) return 12;
    if (got.offsets != want_offsets) return 13;
    if (got.pos != want_pos) return 14;

    /* the same through the C++ mirror */
    Collected got2;
    size_t at2 = 0;
    cfg.slots = 2;
    sm::canonical_minimizers(K, W).stream_fastx(
        [&](uint8_t *buf, size_t cap) {
            const size_t m = file.size() - at2 < cap ? file.size() - at2 : cap;
            memcpy(buf, file.data() + at2, m);
            at2 += m;
            return m;
        },
        [&](const mm_fastx_batch_t &b) { got2.add(b); }, cfg, 7000);
    if (!got2.tiled || got2.covered != file.size() || got2.rec_text_pos != want_text_pos || got2.offsets != want_offsets ||
        got2.pos != want_pos)
        return 20;

    mm_workspace_destroy(ws);
    mm_plan_destroy(plan);
    printf("fastx_stream_example: OK (%d reads, %llu bases, %llu positions)\n", (int)N_READS, (unsigned long long)total,
           (unsigned long long)want_n);
    return 0;
}
