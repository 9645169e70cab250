/* A FASTA record longer than a chunk streamed through the device (MM_FASTX_LONG_RECORDS): a record of 40 000 bases in lines
 * of 60 with chunks of 16 KB arrives in two pieces (the chunk that begins with its header, and the last one), which are joined here as the header describes it - record 0 of a batch
 * with first_continues goes on where the previous batch's last record stopped, its positions are record-global already -
 * and compared with the one-shot call on the whole record (mm_run_packed_reads_host: Builder::run, src/lib.rs:378).  First
 * through the C ABI, then through Builder::stream_fastx of the C++ mirror with an on_batch that takes the pieces.  A short
 * record stands in front of the long one and behind it.  Exit code 0 = everything agrees; 77 = no GPU. */
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "simd_minimizers_amd.hpp"

namespace sm = simd_minimizers;

enum { K = 21, W = 11, N_RECORDS = 3 };

struct Joined {
    std::vector<uint64_t> rec_text_pos, lens, counts;
    std::vector<uint32_t> pos;
    uint64_t covered = 0, pieces = 0;
    bool tiled = true, chained = true, open = false;
    void add(const mm_fastx_batch_t &b, const mm_fastx_pieces_t &p) {
        if (b.text_begin != covered) tiled = false;
        covered = b.text_end;
        if ((p.first_continues != 0) != open) chained = false;
        open = p.last_open != 0;
        for (uint64_t r = 0; r < b.n_records; ++r) {
            const uint64_t n = b.rec_base[r + 1] - b.rec_base[r], m = b.offsets[r + 1] - b.offsets[r];
            if (r == 0 && p.first_continues) {
                /* a piece of the record delivered last: the same '>', first_overlap of its bases were counted before */
                if (rec_text_pos.empty() || rec_text_pos.back() != b.rec_text_pos[0] || p.first_base + p.first_overlap != lens.back())
                    chained = false;
                lens.back() += n - p.first_overlap;
                counts.back() += m;
                ++pieces;
            } else {
                rec_text_pos.push_back(b.rec_text_pos[r]);
                lens.push_back(n);
                counts.push_back(m);
            }
        }
        pos.insert(pos.end(), b.pos, b.pos + b.n_positions);
    }
};

int main() {
    if (mm_device_count() <= 0) {
        printf("no GPU\n");
        return 77;
    }
    const uint64_t lens[N_RECORDS] = {150, 40000, 90};
    std::string file;
    std::vector<uint64_t> want_text_pos, starts{0};
    std::vector<uint8_t> packed;
    uint64_t x = 0x9E3779B97F4A7C15ull, total = 0;
    for (int r = 0; r < N_RECORDS; ++r) {
        want_text_pos.push_back(file.size());
        file += ">record" + std::to_string(r) + " of the example\n";
        for (uint64_t j = 0; j < lens[r]; ++j) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            const char c = "ACGT"[(x >> 33) & 3];
            file.push_back(c);
            if (j % 60 == 59) file.push_back('\n');
            if ((total & 3) == 0) packed.push_back(0);
            packed[total >> 2] |= (uint8_t)((((uint8_t)c >> 1) & 3u) << (2 * (total & 3)));
            ++total;
        }
        file.push_back('\n');
        starts.push_back(total);
    }
    packed.resize(packed.size() + 16, 0);

    /* the one-shot call on the whole records */
    mm_plan_t *plan = nullptr;
    mm_workspace_t *ws = nullptr;
    if (mm_plan_create(&plan, K, W, 1, MM_MINIMIZERS, nullptr) != MM_OK) return 2;
    if (mm_workspace_create(&ws, 0, nullptr) != MM_OK) return 3;
    std::vector<uint32_t> want_pos(total);
    std::vector<uint64_t> want_offsets(N_RECORDS + 1);
    uint64_t want_n = 0;
    if (mm_run_packed_reads_host(plan, ws, packed.data(), N_RECORDS, starts.data(), 0xffffffffu, want_pos.data(), nullptr, want_pos.size(),
                                 want_offsets.data(), &want_n) != MM_OK) {
        printf("one-shot: %s\n", mm_last_error());
        return 4;
    }
    want_pos.resize(want_n);

    /* the stream through the C ABI: pieces of 5 000 bytes, chunks of 16 KB */
    mm_fastx_stream_config_t cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.format = MM_FASTX_FASTA;
    cfg.flags = MM_FASTX_LONG_RECORDS;
    cfg.chunk_bytes = 16384;
    cfg.max_records = 100;
    mm_fastx_stream_t *st = nullptr;
    if (mm_fastx_stream_create(&st, plan, &cfg) != MM_OK) {
        printf("create: %s\n", mm_last_error());
        return 5;
    }
    Joined got;
    mm_fastx_batch_t batch;
    mm_fastx_pieces_t pieces;
    int r = MM_OK;
    for (uint64_t at = 0; at < file.size();) {
        const uint64_t piece = file.size() - at < 5000 ? file.size() - at : 5000;
        uint64_t took = 0;
        r = mm_fastx_stream_feed(st, (const uint8_t *)file.data() + at, piece, &took);
        if (r != MM_OK) return 6;
        at += took;
        if (took < piece) {
            r = mm_fastx_stream_next(st, &batch);
            if (r == MM_OK && mm_fastx_stream_pieces(st, &pieces) == MM_OK) got.add(batch, pieces);
            else if (r != MM_FASTX_NEED_INPUT) return 7;
        }
    }
    if (mm_fastx_stream_finish(st) != MM_OK) return 8;
    while ((r = mm_fastx_stream_next(st, &batch)) == MM_OK) {
        if (mm_fastx_stream_pieces(st, &pieces) != MM_OK) return 9;
        got.add(batch, pieces);
    }
    if (r != MM_FASTX_END) {
        printf("next: %d %s\n", r, mm_last_error());
        return 9;
    }
    mm_fastx_stream_destroy(st);

    auto agrees = [&](const Joined &g) {
        if (!g.tiled || !g.chained || g.open || g.covered != file.size()) return 10;
        if (g.pieces != 1) return 11;  /* the long record came in two pieces */
        if (g.rec_text_pos != want_text_pos) return 12;
        for (int i = 0; i < N_RECORDS; ++i)
            if (g.lens[i] != lens[i] || g.counts[i] != want_offsets[i + 1] - want_offsets[i]) return 13;
        if (g.pos != want_pos) return 14;
        return 0;
    };
    if (const int bad = agrees(got)) return bad;

    /* the same through the C++ mirror */
    Joined got2;
    size_t at2 = 0;
    cfg.slots = 2;
    sm::canonical_minimizers(K, W).stream_fastx(
        [&](uint8_t *buf, size_t cap) {
            const size_t m = file.size() - at2 < cap ? file.size() - at2 : cap;
            memcpy(buf, file.data() + at2, m);
            at2 += m;
            return m;
        },
        [&](const mm_fastx_batch_t &b, const mm_fastx_pieces_t &p) { got2.add(b, p); }, cfg, 7000);
    if (const int bad = agrees(got2)) return 20 + bad;

    mm_workspace_destroy(ws);
    mm_plan_destroy(plan);
    printf("fastx_long_example: OK (%llu bases, %llu positions, the long record in %llu pieces)\n", (unsigned long long)total,
           (unsigned long long)want_n, (unsigned long long)got.pieces + 1);
    return 0;
}
